#!/usr/bin/env python3
"""The one-wave-per-alignment kernels against the general kernels on the three entry points that reach them since the
wave family took every configuration: qcat_sg_align without statistics, qcat_scan_sequences of a kit with affine gap costs
and of the simple lists.  One session, the two paths ALTERNATING call by call (QCAT_HIP_NO_TINY=1 selects the general
kernels, byte for byte the code these entry points ran before), identical outputs asserted; ms per call (host clock around
the call, which ends in a stream synchronise): median and best of the repeats.

usage: bench_waves.py [--out FILE] [--quick]"""
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from qcat_amd import config, native, scanner  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def alternate(call, n):
    """call() under both paths in turn; -> (wave median, wave best, general median, general best) in ms"""
    times, outs = {True: [], False: []}, {}
    reps = 3 if n >= 10000 else 9
    for rep in range(reps + 1):                                   # (the first round warms both paths up)
        for waves in (True, False):
            native.set_option("NO_TINY", None if waves else 1)
            native.set_option("WAVE_MAX", (1 << 40) if waves else None)      # (every size on the waves, whatever the library's limits)
            t = time.perf_counter()
            got, tiny = call()
            dt = (time.perf_counter() - t) * 1e3
            assert (tiny > 0) == waves, (tiny, waves)
            outs[waves] = got.tobytes()
            if rep:
                times[waves].append(dt)
    native.set_option("NO_TINY", None)
    native.set_option("WAVE_MAX", None)
    assert outs[True] == outs[False]
    med = lambda v: sorted(v)[len(v) // 2]
    return med(times[True]), min(times[True]), med(times[False]), min(times[False])


def row(what, n, length, r):
    say("%-44s n %6d  L %5d   waves %10.3f (best %10.3f)   general %10.3f (best %10.3f)   x%.2f" %
        (what, n, length, r[0], r[1], r[2], r[3], r[2] / r[0]))


def main():
    ctx = native.NativeContext(0)
    lib = native.HipLibrary.get().lib
    tiny = lambda: lib.qcat_ctx_tiny_ends(ctx.handle)
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (no git checkout)"
    box = "unknown device"
    try:
        info = subprocess.check_output(["rocminfo"], stderr=subprocess.DEVNULL).decode("utf-8", "replace").splitlines()
        gpus = [i for i, line in enumerate(info) if "gfx" in line and "Name:" in line]
        names = [l.split(":", 1)[1].strip() for l in info[gpus[0]:gpus[0] + 6] if "Marketing Name" in l] if gpus else []
        box = "%s (%s)" % (names[0] if names else "?", info[gpus[0]].split(":", 1)[1].strip()) if gpus else box
    except (OSError, subprocess.CalledProcessError, IndexError):
        pass
    say("box: %s; commit the working tree sits on: %s" % (box, commit))
    say("ms per call, the two paths alternating; x = general / waves (above 1: the wave path is faster)")
    sizes = (1, 100) if QUICK else (1, 100, 10000, 100000)
    rng = random.Random(1)
    cfg = config.qcatConfig()

    # qcat_sg_align: 150 x 60
    det = scanner.factory(kit="NBD103/NBD104")
    target = det.layouts[0].get_adapter_sequences()[:60]
    windows = [r[:150] for r in synth.synth_batch(2000, 3, det.layouts, 1, 0, error_rate=0.1)]
    for gaps in ((2, 2), (3, 1)):
        for n in sizes:
            qs = [windows[i % 2000] for i in range(n)]
            ts = [target] * n
            row("sg_align 150 x 60, gaps %d/%d" % gaps, n, 150,
                alternate(lambda: (native.sg_align(ctx, qs, ts, gaps[0], gaps[1], cfg.matrix.table), tiny()), n))

    def sequences(layouts, n, length, seed):
        reads = synth.synth_batch(min(n, 500), seed, layouts, 1, 0, error_rate=0.1)
        out = []
        for r in reads:
            body = r
            while len(body) < length:
                body += "".join(rng.choice("ACGT") for _ in range(1000))
            out.append(body[:length])
        return native.pack_reads([out[i % len(out)] for i in range(n)])

    # qcat_scan_sequences, affine gap costs
    acfg = config.qcatConfig()
    acfg.gap_open, acfg.gap_extend = 3, 1
    kit = native.NativeKit(det.descriptor(qcat_config=acfg, ends=native.ENDS_5P))
    for length in (1000, 50000):
        for n in sizes:
            if length == 50000 and n > 100:
                continue
            b, o = sequences(det.layouts, n, length, 5)
            row("scan_sequences NBD103/NBD104, gaps 3/1", n, length, alternate(lambda: (ctx.scan_sequences(kit, b, o), tiny()), n))

    # qcat_scan_sequences, simple lists
    for which, lays_kit in (("standard", "PBK004/LWB001"), ("extended", "PBC096")):
        sdet = scanner.factory(mode="simple", kit=which)
        skit = native.NativeKit(sdet.descriptor(ends=native.ENDS_5P))
        lays = scanner.factory(kit=lays_kit).layouts
        for length in (1000, 50000):
            for n in sizes:
                if length == 50000 and n > 100:
                    continue
                b, o = sequences(lays, n, length, 7)
                row("scan_sequences simple %s (%d barcodes)" % (which, len(sdet.barcodes)), n, length,
                    alternate(lambda: (ctx.scan_sequences(skit, b, o), tiny()), n))
    if OUT:
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

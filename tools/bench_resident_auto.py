#!/usr/bin/env python
"""Time the reference driver's default run -- kit auto, batches of 4000 reads -- on reads resident in HBM.

The batch: `--reads` synthetic PBC096 reads (qcat_batch_synthesize on the 12-template auto kit).  Per round, alternating call
by call in one process (host clock around enqueue + synchronise):
  (a) qcat_scan_resident_batches with QCAT_RESIDENT_KIT_AUTO
  (b) the same with QCAT_RESIDENT_FILTER_BARCODES
  (c) the same reads through qcat_scan_batches_auto_ptrs in the file loop's chunks of 64 batches -- what a caller does today:
      the reads lie in host memory, every call uploads its windows and brings its records back
  (d) qcat_scan_resident with the fixed PBC096 kit
and, from a timed call of (b), the HIP-event marks filter_hist / filter_floor / filter_apply beside k_finalize of the same
scan.  With --chunks: (a) again under other values of QCAT_HIP_RESIDENT_AUTO_CHUNK.  Prints, and appends to --out, medians,
minima and maxima over the calls.  No GPU: fails."""
import argparse
import ctypes as C
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                               # noqa: E402

from qcat_amd import config, native, scanner     # noqa: E402


def _stats(v):
    return "median %8.3f ms   min %8.3f   max %8.3f   spread %5.1f %%" % (float(np.median(v)), min(v), max(v),
                                                                          100.0 * (max(v) - min(v)) / float(np.median(v)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--chunks", type=int, nargs="*", default=[], help="other values of QCAT_HIP_RESIDENT_AUTO_CHUNK to time (a) under")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = native.HipLibrary.get()
    lib = hip.lib
    if lib.qcat_device_count() <= 0:
        sys.exit("bench_resident_auto.py: no HIP device")
    ctx = native.NativeContext(0)
    cfg = config.qcatConfig()
    det = scanner.factory()                                            # kit auto: the 12 auto-detect templates
    full = det._native_kit(det.layouts, cfg, native.ENDS_BOTH)
    pbc_t = [i for i, l in enumerate(det.layouts) if l.kit == "PBC096"]
    fixed_det = scanner.factory(kit="PBC096")
    fixed = native.NativeKit(fixed_det.descriptor())
    sp = native.SynthParams(seed=a.seed, n_reads=a.reads, insert_len=600, lead_min=5, lead_max=40, error_rate=0.08,
                            no_adapter_fraction=0.05, tpl_5p=pbc_t[-1], tpl_3p=pbc_t[0])
    batch = native.ResidentBatch.synthesize(ctx, full, sp)
    n, n_bases = batch.info()
    # (c): the same reads in host memory, one pointer and one length each, cut into the file loop's calls of 64 batches
    bases, offsets = batch.download()
    ptrs = (bases.ctypes.data + offsets[:-1]).astype(np.uint64)
    lens = np.diff(offsets).astype(np.uint64)
    per_call = 64 * a.batch
    calls = [(r0, min(n, r0 + per_call), ptrs[r0:r0 + per_call].tobytes(), lens[r0:r0 + per_call].tobytes()) for r0 in range(0, n, per_call)]
    out = np.zeros(n, dtype=native.RESULT_DTYPE)
    slots = np.full((n + a.batch - 1) // a.batch, -1, dtype=np.int32)

    def sync():
        hip.check(lib.qcat_ctx_synchronize(ctx.handle))

    def leg_a():
        ctx.scan_resident_batches(full, batch, a.batch, kit_auto=True, fetch=False)
        sync()

    def leg_b():
        ctx.scan_resident_batches(full, batch, a.batch, kit_auto=True, filter_barcodes=True, fetch=False)
        sync()

    def leg_c():
        for r0, r1, p, l in calls:
            if r1 - r0 <= a.batch:                                     # (one batch: the plain call)
                slot = C.c_int32(-1)
                hip.check(lib.qcat_scan_batch_auto_ptrs(ctx.handle, full.handle, p, l, r1 - r0, out[r0:].ctypes.data, None, C.byref(slot), None, None))
            else:
                hip.check(lib.qcat_scan_batches_auto_ptrs(ctx.handle, full.handle, p, l, r1 - r0, a.batch, out[r0:].ctypes.data, None,
                                                          slots[r0 // a.batch:].ctypes.data))

    def leg_d():
        ctx.scan_resident(fixed, batch, fetch=False)
        sync()

    legs = [("(a) resident, kit auto", leg_a), ("(b) resident, kit auto + filter", leg_b),
            ("(c) host buffers, qcat_scan_batches_auto_ptrs x %d calls" % len(calls), leg_c), ("(d) resident, fixed PBC096 kit", leg_d)]
    times = {name: [] for name, _f in legs}
    for i in range(a.warmup + a.reps):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            if i >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    # (a) and (c) give the same records; (b) differs from (a) where the filter emptied a record
    leg_a()
    recs_a = np.zeros(n, dtype=native.RESULT_DTYPE)
    hip.check(lib.qcat_ctx_fetch_results(ctx.handle, recs_a.ctypes.data, n))
    leg_c()
    same = recs_a.tobytes() == out.tobytes()
    leg_b()
    recs_b = np.zeros(n, dtype=native.RESULT_DTYPE)
    hip.check(lib.qcat_ctx_fetch_results(ctx.handle, recs_b.ctypes.data, n))
    emptied = int(((recs_a["barcode_idx"] >= 0) & (recs_b["barcode_idx"] < 0)).sum())
    # the marks of a timed (b)
    names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()
    marks = {}
    for _ in range(a.reps):
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1))
        ctx.scan_resident_batches(full, batch, a.batch, kit_auto=True, filter_barcodes=True, fetch=False)
        k = lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)
        for j in range(k):
            marks.setdefault(names[j].decode(), []).append(float(ms[j]))
    hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
    lines = ["bench_resident_auto.py --reads %d --batch %d --reps %d --warmup %d --seed %d   box %s"
             % (a.reads, a.batch, a.reps, a.warmup, a.seed, socket.gethostname()),
             "batch: %d reads, %d bases, %d vote batches; %d timed calls per leg, alternating (a) (b) (c) (d)" % (n, n_bases, len(slots), a.reps)]
    for name, _f in legs:
        lines.append("  %-58s %s" % (name, _stats(times[name])))
    med = {name: float(np.median(v)) for name, v in times.items()}
    la, lb, lc, ld = [med[name] for name, _f in legs]
    lines.append("  (c) / (a) = %.2f    (b) - (a) = %.3f ms    (a) / (d) = %.2f    %.1f M reads/s under (a)" % (lc / la, lb - la, la / ld, n / la / 1e3))
    lines.append("  records of (a) equal those of (c): %s;  calls the filter of (b) emptied: %d of %d" % (same, emptied, n))
    lines.append("  marks of the last adapter pass of a timed (b) (HIP events, %d calls):" % a.reps)
    for name in marks:
        if name.startswith("filter_") or name in ("k_finalize", "k_count"):
            lines.append("    %-14s %s" % (name, _stats(marks[name])))
    for chunk in a.chunks:
        native.set_option("RESIDENT_AUTO_CHUNK", chunk)
        t = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            leg_a()
            if i >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        lines.append("  (a) with QCAT_HIP_RESIDENT_AUTO_CHUNK=%-8d %s" % (chunk, _stats(t)))
    native.set_option("RESIDENT_AUTO_CHUNK", None)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

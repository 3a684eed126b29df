#!/usr/bin/env python
"""Time FASTA text in device memory and the annotated single stream (qcat_batch_upload_text, qcat_batch_annot_text) on synthetic
PBC096 reads: the FASTQ file of tools/bench_fqtext.py and its two-line FASTA twin (the same titles and bases).

Two comparisons, each alternating call by call in one process, `--reps` timed calls (at least 12) after `--warmup`:
  parse    the device passes of qcat_batch_upload_text on the FASTA text against those of qcat_batch_upload_fastq_text on the
           FASTQ text (HIP events of the library: fq_count, fq_lines, fq_records, fq_bases) and against a hipMemcpyAsync
           device-to-device of each text's bytes
  stream   the phases of qcat_batch_annot_text (annot_segments, annot_copy) against a hipMemcpyAsync device-to-device of the
           stream's bytes, and against text_copy of qcat_batch_demux_text on the same batch, in ms and in bytes per second; the
           segments per 32 KiB chunk tell whether the copies' tables stay in the LDS
Prints, and writes to --out, medians and ranges.  No GPU: fails."""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                               # noqa: E402

from qcat_amd import native, scanner             # noqa: E402
from bench_partition import chk, hip_runtime     # noqa: E402
from bench_fqtext import _stats, make_file, timed_memcpy  # noqa: E402


def fasta_of(text):
    """the two-line FASTA of a plain four-line FASTQ text whose '+' lines are bare"""
    lines = text.split(b"\n")
    out = []
    for i in range(0, len(lines) - 3, 4):
        out += [b">", lines[i][1:], b"\n", lines[i + 1], b"\n"]
    return b"".join(out)


def _phases(lib, ctx, names, ms, into):
    for j in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)):
        into.setdefault(names[j].decode(), []).append(float(ms[j]))


def _median(v):
    return float(np.median(v)) if v else float("nan")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.reps = max(args.reps, 12)
    hip = native.HipLibrary.get()
    lib = hip.lib
    rt = hip_runtime()
    ctx = native.NativeContext(0)
    det = scanner.factory(kit="PBC096")
    stream = lib.qcat_ctx_stream(ctx.handle)
    work = tempfile.mkdtemp(prefix="bench_textstream_")
    lines = []
    try:
        path = os.path.join(work, "reads.fastq")
        n_bytes, n_bases = make_file(ctx, det, args.reads, args.seed, path)
        with open(path, "rb") as fh:
            fastq = fh.read()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    fasta = fasta_of(fastq)
    lines.append("reads: %d, %d bases (synthetic PBC096, seed %d); FASTQ text %d bytes, FASTA text %d bytes" %
                 (args.reads, n_bases, args.seed, len(fastq), len(fasta)))
    e0, e1 = C.c_void_p(), C.c_void_p()
    chk(rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
    chk(rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
    names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()

    # ---- parse: FASTA passes, FASTQ passes, a memcpy of each text, alternating -------------------------------------------------
    a, b = C.c_void_p(), C.c_void_p()
    chk(rt.hipMalloc(C.byref(a), len(fastq)), "hipMalloc")
    chk(rt.hipMalloc(C.byref(b), len(fastq)), "hipMalloc")
    chk(rt.hipMemsetAsync(a, 65, len(fastq), stream), "hipMemsetAsync")
    sides = {"fasta": (native.ResidentBatch.upload_text, fasta), "fastq": (native.ResidentBatch.upload_fastq_text, fastq)}
    phases = {k: {} for k in sides}
    memcpy_ms = {k: [] for k in sides}
    for i in range(args.warmup + args.reps):
        timed = i >= args.warmup
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
        for k, (upload, text) in sides.items():
            batch = upload(ctx, text)
            if timed:
                _phases(lib, ctx, names, ms, phases[k])
            batch.destroy()
            t = timed_memcpy(rt, stream, a, b, len(text), e0, e1)
            if timed:
                memcpy_ms[k].append(t)
    hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
    rt.hipFree(a); rt.hipFree(b)
    totals = {}
    for k, (_upload, text) in sides.items():
        lines.append("parse, %s: device passes by the context's events (the upload itself is in front of them)" % k.upper())
        total = 0.0
        for name in ("fq_count", "fq_lines", "fq_records", "fq_bases"):
            v = phases[k].get(name, [float("nan")])
            total += _median(v)
            lines.append("  %-12s %s" % (name, _stats(v)))
        totals[k] = total
        mc = _median(memcpy_ms[k])
        lines.append("  all passes   %9.3f ms   = %.1f GB/s of text" % (total, len(text) / total / 1e6))
        lines.append("  hipMemcpyAsync device-to-device of %d bytes: %s" % (len(text), _stats(memcpy_ms[k])))
        lines.append("  passes / memcpy = %.2f" % (total / mc))
    lines.append("parse, FASTA passes / FASTQ passes = %.2f in time, %.2f in bytes of text" % (totals["fasta"] / totals["fastq"], len(fasta) / len(fastq)))

    # ---- stream: annot_copy against a memcpy of its output and against text_copy of the same batch, alternating ---------------------
    tsv_names = det._tsv_names()
    for fmt, text in (("FASTQ", fastq), ("FASTA", fasta)):
        for trim, min_len in ((True, 100), (False, 0)):
            kit = native.NativeKit(det.descriptor(trim=trim, min_read_length=min_len))
            batch = native.ResidentBatch.upload_text(ctx, text)
            ctx.scan_resident(kit, batch, fetch=False)
            total_bytes = C.c_uint64()

            def annot():
                hip.check(lib.qcat_batch_annot_text(ctx.handle, kit.handle, batch.handle, None, C.byref(tsv_names.struct), 0, C.byref(total_bytes)))
                return int(total_bytes.value)

            def demux():
                hip.check(lib.qcat_batch_demux_text(ctx.handle, kit.handle, batch.handle, None, 0, C.byref(total_bytes)))
                return int(total_bytes.value)

            stream_bytes, files_bytes = annot(), demux()
            a, b = C.c_void_p(), C.c_void_p()
            chk(rt.hipMalloc(C.byref(a), max(stream_bytes, 1)), "hipMalloc")
            chk(rt.hipMalloc(C.byref(b), max(stream_bytes, 1)), "hipMalloc")
            chk(rt.hipMemsetAsync(a, 65, max(stream_bytes, 1), stream), "hipMemsetAsync")
            ph_annot, ph_demux, mc_ms, wall_ms = {}, {}, [], []
            for i in range(args.warmup + args.reps):
                timed = i >= args.warmup
                hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
                t0 = time.perf_counter()
                annot()
                wall = (time.perf_counter() - t0) * 1e3
                if timed:
                    wall_ms.append(wall)
                    _phases(lib, ctx, names, ms, ph_annot)
                demux()
                if timed:
                    _phases(lib, ctx, names, ms, ph_demux)
                t = timed_memcpy(rt, stream, a, b, stream_bytes, e0, e1)
                if timed:
                    mc_ms.append(t)
            hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
            rt.hipFree(a); rt.hipFree(b)
            batch.destroy()
            lines.append("stream, %s, trim=%s min_read_length=%d: qcat_batch_annot_text %d bytes out, %.1f segments per 32 KiB chunk; "
                         "qcat_batch_demux_text %d bytes out, %.1f segments per chunk (the copies' LDS tables hold 1024)" %
                         (fmt, trim, min_len, stream_bytes, 10.0 * args.reads / max(1.0, stream_bytes / 32768.0), files_bytes,
                          6.0 * args.reads / max(1.0, files_bytes / 32768.0)))
            for name in ("annot_segments", "annot_copy"):
                lines.append("  %-15s %s" % (name, _stats(ph_annot.get(name, [float("nan")]))))
            lines.append("  %-15s %s" % ("text_copy", _stats(ph_demux.get("text_copy", [float("nan")]))))
            lines.append("  hipMemcpyAsync device-to-device of %d bytes: %s" % (stream_bytes, _stats(mc_ms)))
            copy, other, mc = _median(ph_annot.get("annot_copy")), _median(ph_demux.get("text_copy")), _median(mc_ms)
            lines.append("  annot_copy / memcpy = %.2f   (%.1f GB/s read + written)" % (copy / mc, 2 * stream_bytes / copy / 1e6))
            spread = ph_demux.get("text_copy", [float("nan")])
            lines.append("  annot_copy %.3f ms = %.1f GB/s of output; text_copy %.3f ms = %.1f GB/s of output; per output byte annot_copy / text_copy = %.3f "
                         "(text_copy's own range in this job: %.3f .. %.3f of its median)" %
                         (copy, stream_bytes / copy / 1e6, other, files_bytes / other / 1e6, (copy / stream_bytes) / (other / files_bytes),
                          min(spread) / other, max(spread) / other))
            lines.append("  call, host clock (one wait): %s" % _stats(wall_ms))
    text_out = "\n".join(lines) + "\n"
    sys.stdout.write(text_out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()

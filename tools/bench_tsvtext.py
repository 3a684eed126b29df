#!/usr/bin/env python
"""Time the driver's TSV table formatted in device memory (qcat_batch_tsv_text, BarcodeScanner.tsv_fastq_text) on a FASTQ file of
synthetic PBC096 reads (the file of tools/bench_fqtext.py).

Three comparisons, each alternating call by call in one process, `--reps` timed calls (at least 12) after `--warmup`:
  kernels  the phases of qcat_batch_tsv_text (HIP events of the library: tsv_lengths, tsv_scan, tsv_write -- the tile table and
           the writer) against a hipMemcpyAsync device-to-device of the output's bytes
  host     the host writer's formatting of the same rows: write_s of qcat_fastq_demux with a TSV descriptor and nothing else
  whole    BarcodeScanner.tsv_fastq_text of the file's bytes as the host sees it against qcat_fastq_demux_stream with a TSV
           descriptor on the same file: text in, table out in both
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

from qcat_amd import config, native, scanner     # noqa: E402
from bench_partition import chk, hip_runtime     # noqa: E402
from bench_fqtext import _stats, make_file, timed_memcpy   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--whole-reps", type=int, default=5, help="timed calls of each whole-file path and of the host writer")
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.reps = max(args.reps, 12)
    hip = native.HipLibrary.get()
    lib = hip.lib
    rt = hip_runtime()
    ctx = native.NativeContext(0)
    det = scanner.factory(kit="PBC096")
    names_of = det._tsv_names()
    stream = lib.qcat_ctx_stream(ctx.handle)
    work = tempfile.mkdtemp(prefix="bench_tsvtext_")
    lines = []
    try:
        path = os.path.join(work, "reads.fastq")
        n_bytes, n_bases = make_file(ctx, det, args.reads, args.seed, path)
        with open(path, "rb") as fh:
            text = fh.read()
        lines.append("file: %d reads, %d bytes, %d bases (synthetic PBC096, seed %d)" % (args.reads, n_bytes, n_bases, args.seed))
        e0, e1 = C.c_void_p(), C.c_void_p()
        chk(rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
        chk(rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
        names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()

        # ---- kernels -------------------------------------------------------------------------------------------------------
        for trim, min_len in ((True, 100), (False, 0)):
            kit = native.NativeKit(det.descriptor(trim=trim, min_read_length=min_len))
            batch = native.ResidentBatch.upload_fastq_text(ctx, text)
            ctx.scan_resident(kit, batch, fetch=False)
            total_bytes = C.c_uint64()
            hip.check(lib.qcat_batch_tsv_text(ctx.handle, kit.handle, batch.handle, None, C.byref(names_of.struct), 0, C.byref(total_bytes)))
            out_bytes = int(total_bytes.value)
            a, b = C.c_void_p(), C.c_void_p()
            chk(rt.hipMalloc(C.byref(a), max(out_bytes, 1)), "hipMalloc")
            chk(rt.hipMalloc(C.byref(b), max(out_bytes, 1)), "hipMalloc")
            chk(rt.hipMemsetAsync(a, 65, max(out_bytes, 1), stream), "hipMemsetAsync")
            phases, memcpy_ms, wall_ms = {}, [], []
            for i in range(args.warmup + args.reps):
                timed = i >= args.warmup
                hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
                t0 = time.perf_counter()
                hip.check(lib.qcat_batch_tsv_text(ctx.handle, kit.handle, batch.handle, None, C.byref(names_of.struct), 0, C.byref(total_bytes)))
                wall = (time.perf_counter() - t0) * 1e3
                if timed:
                    wall_ms.append(wall)
                    for j in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)):
                        phases.setdefault(names[j].decode(), []).append(float(ms[j]))
                t = timed_memcpy(rt, stream, a, b, out_bytes, e0, e1)
                if timed:
                    memcpy_ms.append(t)
            hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
            rt.hipFree(a); rt.hipFree(b)
            batch.destroy()
            lines.append("kernels: qcat_batch_tsv_text, trim=%s min_read_length=%d: %d bytes of rows out (%.1f per read of the batch)"
                         % (trim, min_len, out_bytes, out_bytes / float(args.reads)))
            total = 0.0
            for name in ("tsv_lengths", "tsv_scan", "tsv_write"):
                v = phases.get(name, [float("nan")])
                total += float(np.median(v))
                lines.append("  %-12s %s" % (name, _stats(v)))
            write, mc = float(np.median(phases.get("tsv_write", [float("nan")]))), float(np.median(memcpy_ms))
            lines.append("  all passes   %9.3f ms" % total)
            lines.append("  hipMemcpyAsync device-to-device of %d bytes: %s" % (out_bytes, _stats(memcpy_ms)))
            lines.append("  tsv_write / memcpy = %.2f   all passes / memcpy = %.2f   (%.1f GB/s of rows written)"
                         % (write / mc, total / mc, out_bytes / write / 1e6))
            lines.append("  call, host clock (one wait): %s" % _stats(wall_ms))

        # ---- the host writer's formatting, and the whole calls --------------------------------------------------------------
        cfg = config.get_default_config()
        kit = native.NativeKit(det.descriptor())
        fq = native.FastqFile(path)
        fmt_ms, new_ms, old_ms, identical = [], [], [], True
        for i in range(1 + args.whole_reps):
            with open(os.path.join(work, "host.tsv"), "w+b") as out:
                _r, _s, st = fq.demux(ctx, kit, det.layouts, False, trim=True, min_read_length=100, tsv_fd=out.fileno())
                out.seek(0)
                host_rows = out.read()
            t0 = time.perf_counter()
            table = det.tsv_fastq_text(text, trim=True, min_read_length=100, qcat_config=cfg)
            t_new = time.perf_counter() - t0
            with open(os.path.join(work, "stream.tsv"), "w+b") as out:
                t0 = time.perf_counter()
                native.FastqFile.demux_stream(path, ctx, kit, det.layouts, False, trim=True, min_read_length=100, tsv_fd=out.fileno())
                t_old = time.perf_counter() - t0
                out.seek(0)
                stream_rows = out.read()
            if i:
                fmt_ms.append(st["write_s"] * 1e3); new_ms.append(t_new * 1e3); old_ms.append(t_old * 1e3)
            identical = identical and table[len(det.TSV_HEADER):] == host_rows == stream_rows
        lines.append("host writer, trim=True min_read_length=100 (the three tables are byte-identical: %s):" % identical)
        lines.append("  write_s of qcat_fastq_demux with a TSV descriptor only (formatting on the host threads and the write calls): %s" % _stats(fmt_ms))
        lines.append("whole calls, text in and table out:")
        lines.append("  tsv_fastq_text of the file's bytes      %s   %.2f M reads/s" % (_stats(new_ms), args.reads / np.median(new_ms) / 1e3))
        lines.append("  qcat_fastq_demux_stream with a TSV fd   %s   %.2f M reads/s" % (_stats(old_ms), args.reads / np.median(old_ms) / 1e3))
        lines.append("  tsv_fastq_text / demux_stream = %.2f" % (np.median(new_ms) / np.median(old_ms)))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text_out = "\n".join(lines) + "\n"
    sys.stdout.write(text_out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()

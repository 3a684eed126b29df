#!/usr/bin/env python
"""Time FASTQ text in device memory (qcat_batch_upload_fastq_text, qcat_batch_demux_text, BarcodeScanner.demux_fastq_text) on a
FASTQ file of synthetic PBC096 reads (BASELINE config 3's reads, written out with titles and qualities).

Three comparisons, each alternating call by call in one process, `--reps` timed calls (at least 12) after `--warmup`:
  parse    the device passes of qcat_batch_upload_fastq_text (HIP events of the library: fq_count, fq_lines, fq_records,
           fq_bases) against a hipMemcpyAsync device-to-device of the text's bytes
  egress   the phases of qcat_batch_demux_text (part_keys, part_order, text_segments, text_copy) against a hipMemcpyAsync
           device-to-device of the output's bytes; the segments per 32 KiB chunk tell whether the copy's table stays in the LDS
  whole    BarcodeScanner.demux_fastq_text of the file (read from page cache, files written to a directory) against
           qcat_fastq_demux_stream with out_dir on the same file: text in, files out in both
Prints, and writes to --out, medians and ranges.  No GPU: fails."""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                               # noqa: E402

from qcat_amd import config, native, scanner     # noqa: E402
from bench_partition import D2D, chk, hip_runtime  # noqa: E402


def _stats(v):
    return "median %9.3f ms   min %9.3f   max %9.3f   (%d timed calls)" % (float(np.median(v)), min(v), max(v), len(v))


def make_file(ctx, det, n_reads, seed, path):
    """n_reads synthetic reads as a FASTQ file; returns (bytes, bases)"""
    kit = native.NativeKit(det.descriptor())
    sp = native.SynthParams(seed=seed, n_reads=n_reads, insert_len=600, lead_min=5, lead_max=40, error_rate=0.08,
                            no_adapter_fraction=0.05, tpl_5p=1, tpl_3p=0)
    batch = native.ResidentBatch.synthesize(ctx, kit, sp)
    bases, offsets = batch.download()
    batch.destroy()
    raw, offs = bases.tobytes(), offsets.tolist()
    qual = bytes(0x21 + (i * 7) % 60 for i in range(4096)) * (int(max(np.diff(offsets.astype(np.int64)))) // 4096 + 2)
    with open(path, "wb") as fh:
        for r0 in range(0, n_reads, 20000):
            parts = []
            for r in range(r0, min(n_reads, r0 + 20000)):
                ln = offs[r + 1] - offs[r]
                parts += [b"@read%07d runid=bench ch=%d\n" % (r, 1 + r % 512), raw[offs[r]:offs[r + 1]], b"\n+\n", qual[r % 64:r % 64 + ln], b"\n"]
            fh.write(b"".join(parts))
    return os.path.getsize(path), int(offsets[-1])


def timed_memcpy(rt, stream, a, b, nbytes, e0, e1):
    chk(rt.hipEventRecord(e0, stream), "hipEventRecord")
    chk(rt.hipMemcpyAsync(b, a, nbytes, D2D, stream), "hipMemcpyAsync")
    chk(rt.hipEventRecord(e1, stream), "hipEventRecord")
    chk(rt.hipEventSynchronize(e1), "hipEventSynchronize")
    t = C.c_float()
    chk(rt.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
    return float(t.value)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--whole-reps", type=int, default=5, help="timed calls of each whole-file path")
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
    work = tempfile.mkdtemp(prefix="bench_fqtext_")
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

        # ---- parse ---------------------------------------------------------------------------------------------------------
        a, b = C.c_void_p(), C.c_void_p()
        chk(rt.hipMalloc(C.byref(a), n_bytes), "hipMalloc")
        chk(rt.hipMalloc(C.byref(b), n_bytes), "hipMalloc")
        chk(rt.hipMemsetAsync(a, 65, n_bytes, stream), "hipMemsetAsync")
        phases, memcpy_ms, wall_ms = {}, [], []
        for i in range(args.warmup + args.reps):
            timed = i >= args.warmup
            hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
            t0 = time.perf_counter()
            batch = native.ResidentBatch.upload_fastq_text(ctx, text)
            wall = (time.perf_counter() - t0) * 1e3
            if timed:
                wall_ms.append(wall)
                for j in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)):
                    phases.setdefault(names[j].decode(), []).append(float(ms[j]))
            batch.destroy()
            t = timed_memcpy(rt, stream, a, b, n_bytes, e0, e1)
            if timed:
                memcpy_ms.append(t)
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
        rt.hipFree(a); rt.hipFree(b)
        lines.append("parse: qcat_batch_upload_fastq_text, device passes by the context's events (the upload itself is in front of them)")
        total = 0.0
        for name in ("fq_count", "fq_lines", "fq_records", "fq_bases"):
            v = phases.get(name, [float("nan")])
            total += float(np.median(v))
            lines.append("  %-12s %s" % (name, _stats(v)))
        mc = float(np.median(memcpy_ms))
        lines.append("  all passes   %9.3f ms   = %.1f GB/s of text" % (total, n_bytes / total / 1e6))
        lines.append("  hipMemcpyAsync device-to-device of %d bytes: %s" % (n_bytes, _stats(memcpy_ms)))
        lines.append("  passes / memcpy = %.2f" % (total / mc))
        lines.append("  call, host clock (pageable upload over PCIe, allocations, three waits): %s" % _stats(wall_ms))

        # ---- egress --------------------------------------------------------------------------------------------------------
        for trim, min_len in ((True, 100), (False, 0)):
            kit = native.NativeKit(det.descriptor(trim=trim, min_read_length=min_len))
            batch = native.ResidentBatch.upload_fastq_text(ctx, text)
            ctx.scan_resident(kit, batch, fetch=False)
            total_bytes = C.c_uint64()
            hip.check(lib.qcat_batch_demux_text(ctx.handle, kit.handle, batch.handle, None, 0, C.byref(total_bytes)))
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
                hip.check(lib.qcat_batch_demux_text(ctx.handle, kit.handle, batch.handle, None, 0, C.byref(total_bytes)))
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
            lines.append("egress: qcat_batch_demux_text, trim=%s min_read_length=%d: %d bytes of text out, %.1f segments per 32 KiB chunk "
                         "(the copy's LDS table holds 1024)" % (trim, min_len, out_bytes, 6.0 * args.reads / max(1.0, out_bytes / 32768.0)))
            for name in ("part_keys", "part_order", "text_segments", "text_copy"):
                lines.append("  %-13s %s" % (name, _stats(phases.get(name, [float("nan")]))))
            copy, mc = float(np.median(phases.get("text_copy", [float("nan")]))), float(np.median(memcpy_ms))
            lines.append("  hipMemcpyAsync device-to-device of %d bytes: %s" % (out_bytes, _stats(memcpy_ms)))
            lines.append("  text_copy / memcpy = %.2f   (%.1f GB/s read + written)" % (copy / mc, 2 * out_bytes / copy / 1e6))
            lines.append("  call, host clock (one wait): %s" % _stats(wall_ms))

        # ---- whole file: text in, files out ----------------------------------------------------------------------------------------
        cfg = config.get_default_config()
        kit = native.NativeKit(det.descriptor(trim=True, min_read_length=100))
        new_s, old_s, identical = [], [], True
        for i in range(1 + args.whole_reps):
            out_new, out_old = os.path.join(work, "new%d" % i), os.path.join(work, "old%d" % i)
            os.makedirs(out_new); os.makedirs(out_old)
            t0 = time.perf_counter()
            with open(path, "rb") as fh:
                files = det.demux_fastq_text(fh.read(), trim=True, min_read_length=100, qcat_config=cfg)
            for name, data in files.items():
                with open(os.path.join(out_new, name), "wb") as fh:
                    fh.write(data)
            t_new = time.perf_counter() - t0
            t0 = time.perf_counter()
            native.FastqFile.demux_stream(path, ctx, kit, det.layouts, False, trim=True, min_read_length=100, out_dir=out_old)
            t_old = time.perf_counter() - t0
            if i:
                new_s.append(t_new * 1e3); old_s.append(t_old * 1e3)
            same = sorted(os.listdir(out_new)) == sorted(os.listdir(out_old)) and all(
                open(os.path.join(out_new, f), "rb").read() == open(os.path.join(out_old, f), "rb").read() for f in os.listdir(out_old))
            identical = identical and same
            shutil.rmtree(out_new); shutil.rmtree(out_old)
        lines.append("whole file, text in and files out, trim=True min_read_length=100 (the two paths' files are byte-identical: %s):" % identical)
        lines.append("  demux_fastq_text + writing its files   %s   %.2f M reads/s" % (_stats(new_s), args.reads / np.median(new_s) / 1e3))
        lines.append("  qcat_fastq_demux_stream with out_dir   %s   %.2f M reads/s" % (_stats(old_s), args.reads / np.median(old_s) / 1e3))
        lines.append("  demux_fastq_text / demux_stream = %.2f" % (np.median(new_s) / np.median(old_s)))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text_out = "\n".join(lines) + "\n"
    sys.stdout.write(text_out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time qcat_batch_partition on BASELINE config 3's batch (synthetic PBC096 reads resident in HBM), with and without trimming.

Per variant: the scan that the partition follows (host clock around enqueue + synchronise), then `--reps` rounds of
  partition (HIP events of the library around its four phases: keys, order, offsets, copy)
  hipMemcpyAsync device-to-device of exactly the bytes the partition copied (events around it)
alternating call by call in one process.  Prints, and writes to --out, the ms per phase, the copy's GB/s (bytes read plus
bytes written over the copy phase), the memcpy's, and their ratio.  With --qualities: the partition of the same batch carrying
a quality plane (both planes through one launch of the copy kernel) against the bases-only partition, two memcpys and one,
again alternating call by call.  No GPU: fails."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                               # noqa: E402

from qcat_amd import native, scanner             # noqa: E402

D2D = 3                                          # hipMemcpyDeviceToDevice


def hip_runtime():
    rt = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    rt.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    rt.hipFree.argtypes = [vp]
    rt.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    rt.hipEventCreate.argtypes = [C.POINTER(vp)]
    rt.hipEventRecord.argtypes = [vp, vp]
    rt.hipEventSynchronize.argtypes = [vp]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    rt.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]
    return rt


def chk(rc, what):
    if rc != 0:
        raise RuntimeError("%s: HIP error %d" % (what, rc))


def variant(lib, hip, rt, ctx, det, batch, trim, min_read_length, reps, warmup, lines):
    desc = det.descriptor(trim=trim, min_read_length=min_read_length)
    kit = native.NativeKit(desc)
    n, n_bases = batch.info()
    stream = lib.qcat_ctx_stream(ctx.handle)
    # the scan the partition follows
    for _ in range(2):
        ctx.scan_resident(kit, batch, fetch=False)
    hip.check(lib.qcat_ctx_synchronize(ctx.handle))
    t0 = time.perf_counter()
    for _ in range(3):
        ctx.scan_resident(kit, batch, fetch=False)
    hip.check(lib.qcat_ctx_synchronize(ctx.handle))
    scan_ms = (time.perf_counter() - t0) * 1e3 / 3
    # one partition for the size, then the memcpy's buffers of exactly that size
    part = ctx.partition(kit, batch)
    copied = part.batch.n_bases
    sizes = np.diff(part.bin_first.astype(np.int64))
    part.batch.destroy()
    a, b = C.c_void_p(), C.c_void_p()
    chk(rt.hipMalloc(C.byref(a), max(copied, 1)), "hipMalloc")
    chk(rt.hipMalloc(C.byref(b), max(copied, 1)), "hipMalloc")
    chk(rt.hipMemsetAsync(a, 65, max(copied, 1), stream), "hipMemsetAsync")
    e0, e1 = C.c_void_p(), C.c_void_p()
    chk(rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
    chk(rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
    names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()
    phases, memcpy_ms, wall_ms = {}, [], []
    for i in range(warmup + reps):
        timed = i >= warmup
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
        t0 = time.perf_counter()
        out = C.c_void_p()
        hip.check(lib.qcat_batch_partition(ctx.handle, kit.handle, batch.handle, None, 0, C.byref(out)))
        wall = (time.perf_counter() - t0) * 1e3
        lib.qcat_batch_destroy(out)
        if timed:
            wall_ms.append(wall)
            k = lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)
            for j in range(k):
                phases.setdefault(names[j].decode(), []).append(float(ms[j]))
        chk(rt.hipEventRecord(e0, stream), "hipEventRecord")
        chk(rt.hipMemcpyAsync(b, a, copied, D2D, stream), "hipMemcpyAsync")
        chk(rt.hipEventRecord(e1, stream), "hipEventRecord")
        chk(rt.hipEventSynchronize(e1), "hipEventSynchronize")
        t = C.c_float()
        chk(rt.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
        if timed:
            memcpy_ms.append(float(t.value))
    hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
    rt.hipFree(a)
    rt.hipFree(b)
    med = {k: float(np.median(v)) for k, v in phases.items()}
    total = sum(med.values())
    mc = float(np.median(memcpy_ms))
    copy = med.get("part_copy", float("nan"))
    lines.append("variant: trim=%s min_read_length=%d   reads %d, bases in %d, bases copied %d, bins %d (%d with reads, skipped %d)"
                 % (trim, min_read_length, n, n_bases, copied, len(sizes), int((sizes > 0).sum()), int(sizes[-1])))
    lines.append("  scan it follows (host clock, 3 steps)      %8.3f ms" % scan_ms)
    for name in ("part_keys", "part_order", "part_offsets", "part_copy"):
        v = phases.get(name, [float("nan")])
        lines.append("  %-12s median %8.3f ms   min %8.3f   max %8.3f   (%d timed calls)" % (name, np.median(v), min(v), max(v), len(v)))
    lines.append("  all four phases                            %8.3f ms   = %.2f of the scan" % (total, total / scan_ms))
    lines.append("  call, host clock (allocation of the output and the one synchronise included)  median %8.3f ms" % float(np.median(wall_ms)))
    lines.append("  copy: %.1f GB/s (read + written = 2 x %d bytes)" % (2 * copied / copy / 1e6, copied))
    lines.append("  hipMemcpyAsync device-to-device of %d bytes: median %8.3f ms  min %8.3f  max %8.3f   %.1f GB/s"
                 % (copied, mc, min(memcpy_ms), max(memcpy_ms), 2 * copied / mc / 1e6))
    lines.append("  copy / memcpy = %.2f" % (copy / mc))
    return total, scan_ms, copy / mc


def _stats(v):
    return "median %8.3f ms   min %8.3f   max %8.3f" % (float(np.median(v)), min(v), max(v))


def variant_qualities(lib, hip, rt, ctx, det, batch, trim, min_read_length, reps, warmup, lines):
    """the --qualities leg: in one process, alternating call by call, (a) the partition of the batch with a quality plane (both
    planes in one launch of the copy kernel), (b) the bases-only partition, (c) two hipMemcpyAsync device-to-device of the copied
    bytes, (d) one.  The quality plane is made with qcat_batch_from_device from the batch's own bases pointer (the content does
    not matter for time)."""
    desc = det.descriptor(trim=trim, min_read_length=min_read_length)
    kit = native.NativeKit(desc)
    n, n_bases = batch.info()
    stream = lib.qcat_ctx_stream(ctx.handle)
    p_bases, _none, p_offsets = batch.devptrs()
    qbatch = native.ResidentBatch.from_device(ctx, p_bases, p_offsets, n, qualities_ptr=p_bases)
    assert qbatch.has_qualities and qbatch.info() == (n, n_bases)
    for _ in range(2):
        ctx.scan_resident(kit, batch, fetch=False)
    hip.check(lib.qcat_ctx_synchronize(ctx.handle))
    part = ctx.partition(kit, batch)
    copied = part.batch.n_bases
    part.batch.destroy()
    bufs = [C.c_void_p() for _ in range(4)]
    for b in bufs:
        chk(rt.hipMalloc(C.byref(b), max(copied, 1)), "hipMalloc")
    chk(rt.hipMemsetAsync(bufs[0], 65, max(copied, 1), stream), "hipMemsetAsync")
    chk(rt.hipMemsetAsync(bufs[2], 66, max(copied, 1), stream), "hipMemsetAsync")
    e0, e1 = C.c_void_p(), C.c_void_p()
    chk(rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
    chk(rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
    names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()
    phases = {"two planes": {}, "bases only": {}}
    memcpy_ms = {1: [], 2: []}

    def timed_partition(which, handle, timed):
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
        out = C.c_void_p()
        hip.check(lib.qcat_batch_partition(ctx.handle, kit.handle, handle, None, 0, C.byref(out)))
        if timed:
            k = lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)
            for j in range(k):
                phases[which].setdefault(names[j].decode(), []).append(float(ms[j]))
        lib.qcat_batch_destroy(out)

    def timed_memcpy(count, timed):
        chk(rt.hipEventRecord(e0, stream), "hipEventRecord")
        for i in range(count):
            chk(rt.hipMemcpyAsync(bufs[2 * i + 1], bufs[2 * i], copied, D2D, stream), "hipMemcpyAsync")
        chk(rt.hipEventRecord(e1, stream), "hipEventRecord")
        chk(rt.hipEventSynchronize(e1), "hipEventSynchronize")
        t = C.c_float()
        chk(rt.hipEventElapsedTime(C.byref(t), e0, e1), "hipEventElapsedTime")
        if timed:
            memcpy_ms[count].append(float(t.value))

    for i in range(warmup + reps):
        timed = i >= warmup
        timed_partition("two planes", qbatch.handle, timed)                     # (a)
        timed_partition("bases only", batch.handle, timed)                      # (b)
        timed_memcpy(2, timed)                                                  # (c)
        timed_memcpy(1, timed)                                                  # (d)
    hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
    for b in bufs:
        rt.hipFree(b)
    qbatch.destroy()
    lines.append("variant: trim=%s min_read_length=%d   reads %d, bases in %d, bases copied %d per plane   (%d timed calls each, alternating)"
                 % (trim, min_read_length, n, n_bases, copied, reps))
    for which, tag in (("two planes", "(a)"), ("bases only", "(b)")):
        lines.append("  %s partition, %s:" % (tag, which))
        for name in ("part_keys", "part_order", "part_offsets", "part_copy"):
            lines.append("    %-12s %s" % (name, _stats(phases[which].get(name, [float("nan")]))))
        lines.append("    all four     median %8.3f ms" % sum(float(np.median(v)) for v in phases[which].values()))
    lines.append("  (c) two hipMemcpyAsync device-to-device of %d bytes each: %s" % (copied, _stats(memcpy_ms[2])))
    lines.append("  (d) one hipMemcpyAsync device-to-device of %d bytes:      %s" % (copied, _stats(memcpy_ms[1])))
    a, b = phases["two planes"]["part_copy"], phases["bases only"]["part_copy"]
    ma, mb, mc, md = (float(np.median(v)) for v in (a, b, memcpy_ms[2], memcpy_ms[1]))
    lines.append("  part_copy: (a) %.3f ms against 2 x (b) = %.3f ms: ratio %.3f   (spread of (b) over its calls: %.3f ms = %.1f %%; of (a): %.3f ms)"
                 % (ma, 2 * mb, ma / (2 * mb), max(b) - min(b), 100 * (max(b) - min(b)) / mb, max(a) - min(a)))
    lines.append("  part_copy (a) / (c) = %.2f     part_copy (b) / (d) = %.2f     (a): %.1f GB/s read + written, (b): %.1f GB/s"
                 % (ma / mc, mb / md, 4 * copied / ma / 1e6, 2 * copied / mb / 1e6))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--only", choices=["trim", "whole"], default=None, help="one variant only (counter runs)")
    ap.add_argument("--qualities", action="store_true",
                    help="time the partition of a batch WITH a quality plane against the bases-only partition and against one / two "
                         "device-to-device copies, alternating call by call (instead of the default legs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = native.HipLibrary.get()
    lib = hip.lib
    if lib.qcat_device_count() <= 0:
        sys.exit("bench_partition.py: no HIP device")
    rt = hip_runtime()
    ctx = native.NativeContext(0)
    det = scanner.factory(kit="PBC096")
    gen_kit = native.NativeKit(det.descriptor())
    lines = ["bench_partition.py%s --reads %d --reps %d --warmup %d --seed %d" % (" --qualities" if a.qualities else "", a.reads, a.reps, a.warmup, a.seed)]
    reads, batch = a.reads, None
    while batch is None:
        sp = native.SynthParams(seed=a.seed, n_reads=reads, insert_len=600, lead_min=5, lead_max=40, error_rate=0.08,
                                no_adapter_fraction=0.05, tpl_5p=1, tpl_3p=0)
        try:
            batch = native.ResidentBatch.synthesize(ctx, gen_kit, sp)
        except RuntimeError as e:
            if "error -4" not in str(e) or reads < 1000:
                raise
            lines.append("stepped down: %d reads could not be allocated (%s)" % (reads, e))
            reads //= 2
    for trim, mrl in ((True, 500), (False, 0)):
        if a.only and (a.only == "trim") != trim:
            continue
        (variant_qualities if a.qualities else variant)(lib, hip, rt, ctx, det, batch, trim, mrl, a.reps, a.warmup, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()

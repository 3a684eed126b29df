#!/usr/bin/env python
"""Time the evaluation of a text batch in device memory (qcat_batch_eval, BarcodeScanner.eval_fastx_text) on a FASTQ file of
synthetic PBC096 reads whose titles carry truebc= (the reads of tools/bench_fqtext.py under other titles).

Comparisons, each alternating call by call in one process, `--reps` timed calls (at least 12) after `--warmup`:
  kernels  the phases of qcat_batch_eval (HIP events of the library: eval_classify, eval_roc) against a hipMemcpyAsync
           device-to-device of the titles' bytes, and against tsv_lengths of qcat_batch_tsv_text on the same batch -- the pass
           that reads the same titles once, a byte at a time
           Both shapes of the classify pass are timed (option EVAL_SHAPE: one lane per read, a group of eight lanes per read).
  whole    BarcodeScanner.eval_fastx_text of the file's bytes against what a user does without it: tsv_fastx_text, then the
           reference's eval loop and its 1001 threshold loops in Python over the rows.  The Python side is timed on the first
           `--host-reads` rows (1001 loops over a million rows take minutes) and scaled by the number of rows; both figures
           are printed.
  bench    with --parent-tree DIR (a built checkout of the parent commit): the default `python bench.py` step there and here,
           alternating, every run recorded
Prints, and writes to --out, medians and ranges.  No GPU: fails."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                               # noqa: E402

from qcat_amd import config, native, scanner     # noqa: E402
from qcat_amd import eval as qeval               # noqa: E402
from bench_partition import chk, hip_runtime     # noqa: E402
from bench_fqtext import _stats, timed_memcpy    # noqa: E402


def make_text(ctx, det, n_reads, seed):
    """n_reads synthetic reads as FASTQ text with ONT-like titles that state a truebc; returns (text, bytes of the titles)"""
    kit = native.NativeKit(det.descriptor())
    sp = native.SynthParams(seed=seed, n_reads=n_reads, insert_len=600, lead_min=5, lead_max=40, error_rate=0.08,
                            no_adapter_fraction=0.05, tpl_5p=1, tpl_3p=0)
    batch = native.ResidentBatch.synthesize(ctx, kit, sp)
    bases, offsets = batch.download()
    batch.destroy()
    raw, offs = bases.tobytes(), offsets.tolist()
    qual = bytes(0x21 + (i * 7) % 60 for i in range(4096)) * (int(max(np.diff(offsets.astype(np.int64)))) // 4096 + 2)
    parts, title_bytes = [], 0
    for r in range(n_reads):
        ln = offs[r + 1] - offs[r]
        title = b"read%07d runid=2985a3f4bbb34dfee9aa3b33de40be8ec6afef7a read=%d ch=%d start_time=2018-08-01T13:31:17Z truebc=%s" % (
            r, r, 1 + r % 512, b"none" if r % 20 == 0 else b"%d" % (1 + r % 96))
        title_bytes += len(title)
        parts += [b"@", title, b"\n", raw[offs[r]:offs[r + 1]], b"\n+\n", qual[r % 64:r % 64 + ln], b"\n"]
    return b"".join(parts), title_bytes


def host_eval_and_roc(rows):
    """what qcat-eval --tsv and qcat-roc do with the rows of a table: the class of every row, then 1001 passes over the listing"""
    listing = []
    counts = {"CORRECT": 0, "INCORRECT": 0, "FN": 0, "FP": 0}
    for line in rows:
        cols = line.split("\t")
        value = qeval.parse_reads_info(cols[6])["truebc"]
        truebc, bc, score = value.split(","), cols[2], float(cols[3])
        result = "CORRECT" if bc in truebc else ("FN" if bc == "none" else ("FP" if truebc == ["none"] else "INCORRECT"))
        counts[result] += 1
        listing.append((value, bc, score))
    table = []
    for q in range(1001):
        min_score = q / 10.0
        c = [0, 0, 0, 0, 0, 0]
        for value, bc, score in listing:
            if score < min_score:
                bc = "none"
            if bc == "none":
                c[3 if value == "none" else 4] += 1
            elif value == "none":
                c[5] += 1
            elif bc == value:
                c[1] += 1
            else:
                c[2] += 1
            c[0] += 1
        table.append(c)
    return counts, table


def bench_against_parent(parent_tree, rounds):
    """the default `python bench.py` step of the parent's checkout and of this tree, alternating in one job, every run recorded;
    unchanged: this tree's median lies inside the parent's own run-to-run range"""
    import json
    import subprocess
    runs = {"parent": [], "change": []}
    for _r in range(rounds):
        for name, cwd in (("parent", parent_tree), ("change", ROOT)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=cwd, stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL, timeout=600, check=True).stdout.decode()
            runs[name].append(float(json.loads(out.strip().splitlines()[-1])["ms_per_step"]))
    lo, hi, med = min(runs["parent"]), max(runs["parent"]), float(np.median(runs["change"]))
    return ["python bench.py --gpus 1 --steps 20 --warmup 3, ms per step, %d alternating rounds (parent first):" % rounds,
            "  parent  %s   median %.3f" % ("  ".join("%.3f" % v for v in runs["parent"]), float(np.median(runs["parent"]))),
            "  change  %s   median %.3f" % ("  ".join("%.3f" % v for v in runs["change"]), med),
            "  the change's median is %s the parent's range %.3f..%.3f" % ("inside" if lo <= med <= hi else "OUTSIDE", lo, hi)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--whole-reps", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=20260928)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its default bench.py step and this tree's, alternating")
    ap.add_argument("--bench-rounds", type=int, default=5)
    args = ap.parse_args()
    args.reps = max(args.reps, 12)
    hip = native.HipLibrary.get()
    lib = hip.lib
    rt = hip_runtime()
    ctx = native.NativeContext(0)
    det = scanner.factory(kit="PBC096")
    names_of = det._tsv_names()
    stream = lib.qcat_ctx_stream(ctx.handle)
    lines = []
    text, title_bytes = make_text(ctx, det, args.reads, args.seed)
    lines.append("file: %d reads, %d bytes, %d bytes of titles (synthetic PBC096, seed %d)" % (args.reads, len(text), title_bytes, args.seed))
    e0, e1 = C.c_void_p(), C.c_void_p()
    chk(rt.hipEventCreate(C.byref(e0)), "hipEventCreate")
    chk(rt.hipEventCreate(C.byref(e1)), "hipEventCreate")
    names, ms = (C.c_char_p * 16)(), (C.c_float * 16)()

    # ---- kernels -----------------------------------------------------------------------------------------------------------
    kit = native.NativeKit(det.descriptor(trim=False, min_read_length=100))
    batch = native.ResidentBatch.upload_text(ctx, text)
    ctx.scan_resident(kit, batch, fetch=False)
    counts, total_bytes = native.EvalCounts(), C.c_uint64()
    a, b = C.c_void_p(), C.c_void_p()
    chk(rt.hipMalloc(C.byref(a), title_bytes), "hipMalloc")
    chk(rt.hipMalloc(C.byref(b), title_bytes), "hipMalloc")
    chk(rt.hipMemsetAsync(a, 65, title_bytes, stream), "hipMemsetAsync")
    phases, memcpy_ms, wall_ms = {}, [], {0: [], 1: []}
    for i in range(args.warmup + args.reps):
        timed = i >= args.warmup
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1 if timed else 0))
        for shape in (0, 1):                     # option EVAL_SHAPE: one lane per read, a group of eight lanes per read
            native.set_option("EVAL_SHAPE", shape)
            t0 = time.perf_counter()
            hip.check(lib.qcat_batch_eval(ctx.handle, kit.handle, batch.handle, None, C.byref(names_of.struct), 0, C.byref(counts)))
            wall = (time.perf_counter() - t0) * 1e3
            if timed:
                wall_ms[shape].append(wall)
                for j in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)):
                    phases.setdefault("%s shape %d" % (names[j].decode(), shape), []).append(float(ms[j]))
        native.set_option("EVAL_SHAPE", None)
        hip.check(lib.qcat_batch_tsv_text(ctx.handle, kit.handle, batch.handle, None, C.byref(names_of.struct), 0, C.byref(total_bytes)))
        if timed:
            for j in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)):
                phases.setdefault(names[j].decode(), []).append(float(ms[j]))
        t = timed_memcpy(rt, stream, a, b, title_bytes, e0, e1)
        if timed:
            memcpy_ms.append(t)
    hip.check(lib.qcat_ctx_set_timing(ctx.handle, 0))
    rt.hipFree(a); rt.hipFree(b)
    batch.destroy()
    lines.append("kernels: qcat_batch_eval, trim=False min_read_length=100: %d reads evaluated (%d correct, %d incorrect, %d fn, %d fp)"
                 % (counts.total, counts.correct, counts.incorrect, counts.fn, counts.fp))
    mc = float(np.median(memcpy_ms))
    for name in ("eval_classify shape 0", "eval_classify shape 1", "eval_roc shape 0", "tsv_lengths"):
        lines.append("  %-22s %s" % (name.replace("shape 0", "(one lane per read)").replace("shape 1", "(eight lanes per read)") if "classify" in name
                                     else name.replace(" shape 0", ""), _stats(phases.get(name, [float("nan")]))))
    tl = float(np.median(phases.get("tsv_lengths", [float("nan")])))
    lines.append("  hipMemcpyAsync device-to-device of the %d title bytes: %s" % (title_bytes, _stats(memcpy_ms)))
    for shape, what in ((0, "one lane per read"), (1, "eight lanes per read")):
        cl = float(np.median(phases.get("eval_classify shape %d" % shape, [float("nan")])))
        lines.append("  %s: eval_classify / memcpy = %.2f   eval_classify / tsv_lengths = %.2f   (%.1f GB/s of title bytes)   call, host clock: %s"
                     % (what, cl / mc, cl / tl, title_bytes / cl / 1e6, _stats(wall_ms[shape])))

    # ---- whole: text in, counts and table out ---------------------------------------------------------------------------------
    cfg = config.get_default_config()
    new_ms, tsv_ms = [], []
    for i in range(1 + args.whole_reps):
        t0 = time.perf_counter()
        out = det.eval_fastx_text(text, trim=False, min_read_length=100, qcat_config=cfg)
        t_new = time.perf_counter() - t0
        t0 = time.perf_counter()
        table = det.tsv_fastx_text(text, trim=False, min_read_length=100, qcat_config=cfg)
        t_tsv = time.perf_counter() - t0
        if i:
            new_ms.append(t_new * 1e3); tsv_ms.append(t_tsv * 1e3)
    rows = table.decode("latin-1").splitlines()[1:]
    sample = rows[:args.host_reads]
    t0 = time.perf_counter()
    host_counts, host_table = host_eval_and_roc(sample)
    host_s = time.perf_counter() - t0
    same = None
    if len(sample) == len(rows):
        same = (host_counts == {"CORRECT": out.counts["correct"], "INCORRECT": out.counts["incorrect"], "FN": out.counts["fn"], "FP": out.counts["fp"]}
                and host_table == out.roc.tolist())
    lines.append("whole calls, text in, counts and ROC table out:")
    lines.append("  eval_fastx_text of the file's bytes        %s   %.2f M reads/s" % (_stats(new_ms), args.reads / np.median(new_ms) / 1e3))
    lines.append("  tsv_fastx_text of the file's bytes         %s" % _stats(tsv_ms))
    lines.append("  eval and 1001 threshold loops in Python over %d of the %d rows: %.1f s; scaled to all rows: %.1f s%s"
                 % (len(sample), len(rows), host_s, host_s * len(rows) / max(1, len(sample)), "" if same is None else "   (same numbers as the device: %s)" % same))
    lines.append("  tsv_fastx_text + Python (scaled) / eval_fastx_text = %.0f"
                 % ((np.median(tsv_ms) + host_s * 1e3 * len(rows) / max(1, len(sample))) / np.median(new_ms)))
    if args.parent_tree:
        lines += bench_against_parent(args.parent_tree, args.bench_rounds)
    text_out = "\n".join(lines) + "\n"
    sys.stdout.write(text_out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()

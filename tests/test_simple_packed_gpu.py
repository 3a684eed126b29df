"""Simple mode on the packed end-tracking kernels (csrc/kernels_simple.inc: k_simple_packed -> k_simple_select ->
k_simple_redo, debug scans k_simple_select_rows) against the CPU oracle under both `r1_rule` values, against the general
kernel (QCAT_HIP_NO_SIMPLE_PACKED=1), and the native file loop in simple mode against the Python loop."""
import ctypes as C
import io
import logging
import os

import numpy as np
import pytest

import helpers
import oracle_lib
import simple_cases
import synth
from qcat_amd import cli, config, native, scanner

pytestmark = pytest.mark.gpu

RULES = ("striped", "scalar")
TRACE_FIELDS = ("window_len", "best_end", "bc_idx", "bc_raw", "adapter_end")


def _check_debug_scan(det, reads, ends, ctx=None):
    """records, counts, traces and per-barcode rows of one debug scan against the oracle's, and the plain scan's records
    (summary keys + redo list instead of the sequential loop over every barcode's score) against both"""
    d = det.descriptor(ends=ends, min_read_length=100, trim=True)
    kit = native.NativeKit(d)
    ctx = ctx or native.NativeContext(0)
    packed = native.pack_reads(reads)
    cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
    recs, traces, rows = ctx.scan(kit, *packed, counts=cnt, trace=True, rows=True)
    o_recs, o_cnt, o_traces, o_rows = oracle_lib.scan(d, reads, counts=True, trace=True, rows=True, threads=8)
    assert recs.tobytes() == o_recs.tobytes()
    assert np.array_equal(cnt, o_cnt)
    for name in TRACE_FIELDS:
        assert np.array_equal(traces[name], o_traces[name]), name
    assert np.array_equal(rows[:, 0, :], o_rows[:, 0, :])
    cnt2 = np.zeros(d.n_count_buckets, dtype=np.int64)
    plain = ctx.scan(kit, *packed, counts=cnt2)
    assert plain.tobytes() == o_recs.tobytes()
    assert np.array_equal(cnt2, o_cnt)
    return o_recs, o_traces


def _marks_of_a_resident_scan(kit, reads):
    hip = native.HipLibrary.get()
    lib = hip.lib
    ctx = native.NativeContext(0)
    bases, offsets = native.pack_reads(reads)
    batch = C.c_void_p()
    hip.check(lib.qcat_batch_upload(ctx.handle, bases.ctypes.data, offsets.ctypes.data, len(reads), C.byref(batch)))
    try:
        hip.check(lib.qcat_ctx_set_timing(ctx.handle, 1))
        hip.check(lib.qcat_scan_resident(ctx.handle, kit.handle, batch))
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        k = lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16)
        out = np.zeros(len(reads), dtype=native.RESULT_DTYPE)
        hip.check(lib.qcat_ctx_fetch_results(ctx.handle, out.ctypes.data, len(reads)))
        return [names[i].decode() for i in range(k)], out
    finally:
        lib.qcat_batch_destroy(batch)


# ---- 1. the path is taken -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["standard", "extended"])
def test_a_resident_scan_runs_the_packed_simple_kernels(which, hip_options):
    det = scanner.factory(mode="simple", kit=which)
    d = det.descriptor()
    kit = native.NativeKit(d)
    assert kit.describe()["packed"] == 1
    reads = synth.synth_batch(300, 11, scanner.factory(kit="PBK004/LWB001").layouts, 1, 0, error_rate=0.1)
    want = oracle_lib.scan(d, reads, threads=8)
    marks, got = _marks_of_a_resident_scan(kit, reads)
    assert "k_simple_packed" in marks and "k_scan_simple" not in marks, marks
    assert got.tobytes() == want.tobytes()
    hip_options(NO_SIMPLE_PACKED=1)
    marks, got = _marks_of_a_resident_scan(kit, reads)
    assert "k_scan_simple" in marks and "k_simple_packed" not in marks, marks
    assert got.tobytes() == want.tobytes()


def test_a_ragged_list_runs_the_general_kernel(tmp_path):
    det = simple_cases.detector(tmp_path, simple_cases.random_list(2, 3, 24) + simple_cases.random_list(3, 2, 20))
    kit = native.NativeKit(det.descriptor())
    assert kit.describe()["packed"] == 0
    marks, _ = _marks_of_a_resident_scan(kit, simple_cases.edge_reads(40, [b.sequence for b in det.barcodes], 5))
    assert "k_scan_simple" in marks and "k_simple_packed" not in marks, marks


# ---- 2. tile and chunk edges ----------------------------------------------------------------------------------------------------
def _list_of(name, tmp_path):
    if name in ("standard", "extended"):
        return scanner.factory(mode="simple", kit=name)
    std = [b.sequence for b in scanner.factory(mode="simple", kit="standard").barcodes]
    if name == "one":
        return simple_cases.detector(tmp_path, std[:1])
    if name == "two":
        return simple_cases.detector(tmp_path, std[:2])
    return simple_cases.detector(tmp_path, simple_cases.random_list(1024, 1024, 24))


@pytest.mark.parametrize("name", ["one", "two", "standard", "extended"])
def test_tile_and_chunk_edges(name, tmp_path):
    """batches of 1 .. 257 reads (one lane, a full half wave, one tile, one tile and a read ...), read lengths that differ
    between the two alignments of a lane and fall below the barcode length, lists of 1 / 2 / 24 / 120 barcodes"""
    det = _list_of(name, tmp_path)
    seqs = [b.sequence for b in det.barcodes]
    assert len(seqs) == {"one": 1, "two": 2, "standard": 24, "extended": 120}[name]
    ctx = native.NativeContext(0)
    for rule in RULES:
        with helpers.r1_rule(rule):
            for n in (1, 2, 127, 128, 129, 257):
                _check_debug_scan(det, simple_cases.edge_reads(n, seqs, 1000 + n), native.ENDS_5P, ctx)
            _check_debug_scan(det, simple_cases.edge_reads(300, seqs, 77), native.ENDS_BOTH, ctx)


def test_a_list_of_1024_barcodes(tmp_path):
    det = _list_of("synthetic", tmp_path)
    seqs = [b.sequence for b in det.barcodes]
    for rule in RULES:
        with helpers.r1_rule(rule):
            _check_debug_scan(det, simple_cases.edge_reads(129, seqs, 9), native.ENDS_5P)


# ---- 3. end positions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", simple_cases.CLASS_EDGES)
def test_end_positions_at_every_width_class_edge(length, tmp_path):
    """constructed windows (tests/simple_cases.py: end_windows; what they do in the oracle is pinned by
    tests/test_simple_packed_host.py): a copy on the window's last base, at offset 0, cut off by the window's end, two
    copies, a deletion, an insertion, ties of the two borders -- on both ends of a read"""
    seqs = simple_cases.random_list(100 + length, 3, length)
    det = simple_cases.detector(tmp_path, seqs, "l%d.fa" % length)
    windows = simple_cases.end_windows(seqs[1], 7 * length)
    reads = simple_cases.reads_of_windows(list(windows.values()), length)
    ctx = native.NativeContext(0)
    for rule in RULES:
        with helpers.r1_rule(rule):
            d = det.descriptor(trim=True)
            kit = native.NativeKit(d)
            assert kit.describe()["packed"] == 1
            o_recs, o_traces = oracle_lib.scan(d, reads, trace=True)
            recs, traces, _ = ctx.scan(kit, *native.pack_reads(reads), trace=True)
            plain = ctx.scan(kit, *native.pack_reads(reads))
            for got in (recs, plain):
                for f in ("adapter_end", "trim5p", "trim3p", "barcode_idx", "raw_score"):
                    assert np.array_equal(got[f], o_recs[f]), (rule, f)
                assert got.tobytes() == o_recs.tobytes()
            assert np.array_equal(traces["best_end"], o_traces["best_end"])
            assert (o_recs["barcode_idx"] == 1).sum() >= len(reads) // 2      # (the windows carry barcode 1)


# ---- 4. letters and R2 ----------------------------------------------------------------------------------------------------------
def test_letters_outside_the_alphabet_and_scores_of_zero(tmp_path):
    std = scanner.factory(mode="simple", kit="standard")
    seqs = [b.sequence for b in std.barcodes]
    base = synth.synth_batch(40, 3, scanner.factory(kit="PBK004/LWB001").layouts, 1, 0, error_rate=0.1)
    reads = [base[0].lower(), base[1][:60] + "N" * 5 + base[1][65:], base[2][:30] + "X" * 3 + base[2][33:], "ACGT*-RYKM" * 15,
             "N" * 150, "*" * 40, "N" * 150 + seqs[3], seqs[5][:10] + "NNNN" + seqs[5][14:] + "ACGT" * 50, "n" * 20, "X" * 200] + base[3:]
    for rule in RULES:
        with helpers.r1_rule(rule):
            for ends in (native.ENDS_BOTH, native.ENDS_5P):
                o_recs, o_traces = _check_debug_scan(std, reads, ends)
    # "*" * 40: every barcode scores exactly 0, the running best moves to the LAST index (R2) -- the redo list's case;
    # "N" * 150: every barcode scores -1, the first index keeps it
    assert o_traces["bc_raw"][5][0] == 0 and o_traces["bc_idx"][5][0] == len(seqs) - 1
    assert o_traces["bc_raw"][4][0] == -1 and o_traces["bc_idx"][4][0] == 0
    # the same barcode twice in a list: the first index wins
    twice = simple_cases.detector(tmp_path, [seqs[0], seqs[7], seqs[2], seqs[7], seqs[7]], "twice.fa")
    rd = [simple_cases.random_seq(__import__("random").Random(i), 20 + i) + seqs[7] + "ACGT" * 60 for i in range(6)]
    o_recs, o_traces = _check_debug_scan(twice, rd + reads[:8], native.ENDS_BOTH)
    assert (o_recs["barcode_idx"][:6] == 1).all()


def test_min_quality_on_either_side_of_14_and_15_of_24():
    """14 / 24 = 58.33 % and 15 / 24 = 62.5 %: thresholds of 58.0, 58.5, 62.0 and 63.0 put neither, the first, the first and
    both of these scores below min_quality"""
    lays = scanner.factory(kit="PBK004/LWB001").layouts
    reads = synth.synth_batch(600, 21, lays, 1, 0, error_rate=0.22)
    called = {}
    for q in (58.0, 58.5, 62.0, 63.0):
        det = scanner.factory(mode="simple", kit="standard", min_quality=q)
        o_recs, o_traces = _check_debug_scan(det, reads, native.ENDS_BOTH)
        assert (o_traces["bc_raw"] == 14).any() and (o_traces["bc_raw"] == 15).any()
        called[q] = int((o_recs["barcode_idx"] >= 0).sum())
    assert called[58.0] > called[58.5] == called[62.0] > called[63.0] > 0, called


# ---- 5. both device paths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,kit", [("standard", "PBK004/LWB001"), ("extended", "PBC096")])
def test_the_packed_and_the_general_kernel_give_the_same_bytes(which, kit, hip_options):
    det = scanner.factory(mode="simple", kit=which)
    lays = scanner.factory(kit=kit).layouts
    reads = synth.synth_batch(5000, 55, lays, 1, 0, error_rate=0.1)
    for i in range(0, 600, 3):
        reads[i] = reads[i][:(i * 7) % 400]
    reads += ["", "A", "N" * 300, reads[7].lower(), "ACGT*-RYKM" * 30]
    d = det.descriptor(min_read_length=300, trim=True)
    kit_h = native.NativeKit(d)
    packed = native.pack_reads(reads)
    want, want_cnt = oracle_lib.scan(d, reads, counts=True, threads=8)
    got = {}
    for off in (None, 1):
        hip_options(NO_SIMPLE_PACKED=off)
        cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
        got[off] = native.NativeContext(0).scan(kit_h, *packed, counts=cnt).tobytes()
        assert np.array_equal(cnt, want_cnt)
    assert got[None] == got[1] == want.tobytes()
    if which == "standard":
        hip_options(NO_SIMPLE_PACKED=None)
        many = (reads * 8)[:40000]                 # the pipelined host path
        d = det.descriptor()
        res = native.NativeContext(0).scan(native.NativeKit(d), *native.pack_reads(many))
        assert res.tobytes() == oracle_lib.scan(d, many, threads=8).tobytes()


# ---- 6. the file loop -----------------------------------------------------------------------------------------------------------
def _write_fastq(path, reads, fasta=False):
    with open(str(path), "w") as fh:
        for i, r in enumerate(reads):
            if fasta:
                fh.write(">r%d ch=%d\n%s\n" % (i, i % 512, r))
            else:
                fh.write("@r%d ch=%d\n%s\n+\n%s\n" % (i, i % 512, r, "I" * len(r)))
    return str(path)


def _file_reads(n, seed):
    lays = scanner.factory(kit="PBK004/LWB001").layouts
    reads = synth.synth_batch(n, seed, lays, 1, 0, error_rate=0.1)
    for i in range(0, n, 9):
        reads[i] = reads[i][:40 + (i * 13) % 300]      # short reads: the minimum-length filter and trimming have something to do
    # one rare barcode per batch of the driver's loop for --filter-barcodes to drop
    rare = scanner.factory(mode="simple", kit="standard").barcodes[23].sequence
    reads[5] = "ACGTTGCA" * 3 + rare + "GATTACA" * 50
    return [r if r else "A" for r in reads]


def test_demux_stream_takes_a_simple_kit(tmp_path):
    det = scanner.factory(mode="simple", kit="standard")
    reads = _file_reads(2500, 8)
    fq = _write_fastq(tmp_path / "reads.fastq", reads)
    cfg = config.qcatConfig()
    lays = [det._simple_layout]
    kit = det._native_kit(lays, cfg, native.ENDS_BOTH)
    with open(str(tmp_path / "out.tsv"), "wb") as fh:
        bc, ad, n_none, n_ad_none, stats = native.FastqFile.demux_stream(fq, det._context(), kit, lays, False, batch_size=1000,
                                                                         tsv_fd=fh.fileno())
    assert stats["segments"] > 0 and stats["n_reads"] == 2500 and not stats["incomplete"]
    want = oracle_lib.scan(det.descriptor(), reads, threads=8)
    assert ad.sum() == 0 and n_ad_none == 2500                      # no adapter in simple mode: every kept read under "none"
    assert n_none == int((want["barcode_idx"] < 0).sum())
    assert np.array_equal(bc[0, :, 0], np.bincount(want["barcode_idx"][want["barcode_idx"] >= 0], minlength=bc.shape[1]))
    rows = (tmp_path / "out.tsv").read_text().split("\n")[:-1]
    assert len(rows) == 2500
    for row, rec in zip(rows[:200], want[:200]):
        cols = row.split("\t")
        if rec["barcode_idx"] >= 0:
            assert cols[2] == str(det.barcodes[rec["barcode_idx"]].id) and cols[4] == "None" and cols[5] == str(int(rec["adapter_end"]))
        else:
            assert cols[2:6] == ["none", "-1", "none", "-1"]
    # the whole-file entry point as well
    f = native.FastqFile(fq)
    with open(str(tmp_path / "out2.tsv"), "wb") as fh:
        recs, skipped, st = f.demux(det._context(), kit, lays, False, batch_size=1000, tsv_fd=fh.fileno())
    f.close()
    assert recs.tobytes() == want.tobytes() and not skipped.any()
    assert (tmp_path / "out2.tsv").read_bytes() == (tmp_path / "out.tsv").read_bytes()


class _Capture(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _run_cli(reads_fq, which, variant, tmp, monkeypatch, native_loop):
    """one qcat_cli run in simple mode -> (TSV text, {file: bytes}, log lines, segments the native loop handled)"""
    segments = []
    orig = native.FastqFile.demux_stream

    def spy(*a, **kw):
        res = orig(*a, **kw)
        segments.append(res[4]["segments"])
        return res

    monkeypatch.setattr(native.FastqFile, "demux_stream", staticmethod(spy))
    if native_loop:
        monkeypatch.delenv("QCAT_AMD_NO_NATIVE_FASTQ", raising=False)
    else:
        monkeypatch.setenv("QCAT_AMD_NO_NATIVE_FASTQ", "1")
    os.makedirs(str(tmp))
    outdir = str(tmp / "bc") if variant == "dir" else None
    outfile = str(tmp / "out.fx")
    cap = _Capture()
    root = logging.getLogger()
    old_level = root.level
    root.addHandler(cap)
    root.setLevel(logging.INFO)
    buf = io.StringIO()
    try:
        cli.qcat_cli(reads_fq=reads_fq, kit=which, mode="simple", nobatch=False, out=outdir, min_qual=None, tsv=variant in ("tsv", "filter"),
                     output=None if outdir else outfile, threads=1, trim=variant == "dir", adapter_yaml=None, quiet=False,
                     filter_barcodes=variant == "filter", middle_adapter=False, min_read_length=100 if variant == "out" else 0,
                     qcat_config=config.get_default_config(), tsv_stream=buf)
    finally:
        root.removeHandler(cap)
        root.setLevel(old_level)
    files = {}
    if outdir:
        for f in sorted(os.listdir(outdir)):
            with open(os.path.join(outdir, f), "rb") as fh:
                files[f] = fh.read()
    elif os.path.exists(outfile):
        with open(outfile, "rb") as fh:
            files["out"] = fh.read()
    return buf.getvalue(), files, cap.lines, sum(segments)


@pytest.mark.parametrize("which", ["standard", "extended"])
@pytest.mark.parametrize("variant", ["tsv", "dir", "out", "filter"])
def test_cli_simple_mode_native_loop_equals_the_python_loop(which, variant, tmp_path, monkeypatch):
    """`--simple [--simple-barcodes extended]` with --tsv, -b dir --trim, -o file --min-read-length 100 and --filter-barcodes
    (batches of 4000: the file holds two, the second a short one): same TSV text, same files, same log lines as under
    QCAT_AMD_NO_NATIVE_FASTQ=1; the "out" variant reads a FASTA file."""
    reads = _file_reads(4300, 31)
    fq = _write_fastq(tmp_path / ("reads.fasta" if variant == "out" else "reads.fastq"), reads, fasta=variant == "out")
    got = _run_cli(fq, which, variant, tmp_path / "native", monkeypatch, True)
    want = _run_cli(fq, which, variant, tmp_path / "python", monkeypatch, False)
    assert got[3] > 0 and want[3] == 0            # the native loop really ran, and only where it should
    assert got[0] == want[0]
    assert sorted(got[1]) == sorted(want[1]) and all(got[1][k] == want[1][k] for k in want[1])
    assert got[2] == want[2]
    if variant in ("tsv", "filter"):
        assert got[0].count("\n") == 4300 + 1
    else:
        assert sum(len(v) for v in got[1].values()) > 100000

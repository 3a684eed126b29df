"""The evaluation of a text batch in device memory (qcat_batch_eval, NativeContext.eval_text, BarcodeScanner.eval_fastx_text,
python -m qcat_amd.eval): against the reference's own qcat-eval and qcat-roc over the reference driver's tables of the four
shipped files and over the crafted cases of tests/eval_cases.py (tests/golden/eval_golden.json), against a plain Python
restatement of both tools at sizes around a wave and a workgroup, with dropped reads, in comment mode on the annotated stream,
and the call's refusals and state."""
import json
import os

import numpy as np
import pytest

import eval_cases
import helpers
import synth
from qcat_amd import eval as qeval
from qcat_amd import native, scanner

pytestmark = pytest.mark.gpu

with open(os.path.join(helpers.GOLDEN, "eval_golden.json")) as _fh:
    _GOLD = {e["name"]: e for e in json.load(_fh)["inputs"]}
HEADER = b"name\tlength\tbarcode\tscore\tkit\tadapter_end\tcomment\n"


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


@pytest.fixture(params=["one lane per read", "a group of lanes per read"])
def shape(request):
    """both shapes of the classify pass (option EVAL_SHAPE; without it the library's default runs, as in every other test here)"""
    native.set_option("EVAL_SHAPE", 0 if request.param.startswith("one") else 1)
    yield request.param
    native.set_option("EVAL_SHAPE", None)


def _roc_of(changes):
    """the 1001 x 6 table of the golden's rows-at-which-a-count-changes"""
    roc = np.zeros((1001, 6), dtype=np.int64)
    for row in changes:
        roc[row[0]:] = row[1:]
    return roc


def _counts_of(summary):
    cols = summary.split("\t")
    return dict(zip(("total", "correct", "incorrect", "fn", "fp"), (int(c) for c in cols[2:7])))


# ---- 1. the reference's tools over the reference driver's tables of the shipped files ---------------------------------------------------
@pytest.mark.parametrize("tag", ["tsv-auto-batch", "tsv-dual"])
@pytest.mark.parametrize("name", ["nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq"])
def test_shipped_files_against_the_references_eval_and_roc(tag, name, capsys):
    gold = _GOLD["%s:%s" % (tag, name)]
    path = os.path.join(helpers.GOLDEN, "data", name)
    with open(path, "rb") as fh:
        text = fh.read()
    det = scanner.factory(kit="auto") if tag == "tsv-auto-batch" else scanner.factory(mode="dual")
    out = det.eval_fastx_text(text, trim=False, min_read_length=100)
    assert out.counts == _counts_of(gold["summary"]) and out.counts["total"] >= 5
    assert np.array_equal(out.roc, _roc_of(gold["roc"]))
    assert len(out.classes) == len(out.kinds) == len(out.buckets) == text.count(b"\n") // 4
    mode = ["--dual"] if tag == "tsv-dual" else []
    capsys.readouterr()
    qeval.main([path, "--scan", "-n", "prog", "-d", "data"] + mode)
    assert capsys.readouterr().out == gold["listing"]
    qeval.main([path, "--scan", "-s", "-n", "prog", "-d", "data"] + mode)
    assert capsys.readouterr().out == gold["summary"]
    qeval.main([path, "--scan", "--roc", "-n", "prog", "-d", "data"] + mode)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split("\t") == list(qeval.ROC_HEADER) and len(lines) == 1002
    assert lines[1 + 744].split("\t") == [str(c) for c in out.roc[744]] + ["74.4", "prog", "data"]


# ---- 2. the crafted cases ---------------------------------------------------------------------------------------------------------------
_CASES = eval_cases.cases()


@pytest.fixture(scope="module")
def case_scanners():
    return {"epi": eval_cases.epi_scanner(), "dual": eval_cases.dual_scanner()}


def _case_call(ctx, det, case):
    # (jit=False: the written kit is outside the built-in bundle, and no scan runs here -- a kit made with the default would start
    #  a background compile of kernels nobody uses, still at work when this short module's process ends)
    kit = native.NativeKit(det.descriptor(), jit=False)
    batch = native.ResidentBatch.upload_text(ctx, eval_cases.fastq_of(case))
    return kit, batch, eval_cases.records_of(case)


@pytest.mark.parametrize("case", [c for c in _CASES if "refused" not in c], ids=lambda c: c["name"])
def test_crafted_cases_against_the_references_eval_and_roc(ctx, case_scanners, case, shape):
    gold = _GOLD["case:" + case["name"]]
    det = case_scanners[case["kit"]]
    kit, batch, recs = _case_call(ctx, det, case)
    out = ctx.eval_text(kit, batch, det._tsv_names(), records=recs)
    table = ctx.tsv_text(kit, batch, det._tsv_names(), records=recs)
    batch.destroy()
    assert HEADER + table.text == gold["table"].encode("latin-1")               # the table the golden was made from
    assert out.counts == _counts_of(gold["summary"])
    assert np.array_equal(out.roc, _roc_of(gold["roc"]))
    rows = [(c[0], c[6], c[2], float(c[3])) for c in (line.split("\t") for line in table.text.decode("latin-1").splitlines())]
    listing = "\n".join(["\t".join(("program", "dataset", "read_id", "truebc", "bc", "result", "score"))] +
                        list(qeval.listing_lines("prog", "data", out.classes, rows))) + "\n"
    assert listing == gold["listing"]
    assert qeval.summary_line("prog", "data", out.counts) + "\n" == gold["summary"]
    assert (out.classes > 0).all() and set(out.kinds.tolist()) == {0, 1, 2} and len(set(out.buckets.tolist())) >= 4


# ---- 3. a plain restatement of both tools ---------------------------------------------------------------------------------------------------
def _restate(titles, calls, dropped=None, from_comment=False):
    """(classes, kinds, buckets, counts, roc) by qcat/eval.py:146-165 and qcat/eval_roc.py:41-64, read by read and threshold by
    threshold; calls: per read ``None`` or ``(call text, score as a float)``"""
    n = len(titles)
    classes, kinds, buckets = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    reads = []
    for i, title in enumerate(titles):
        if dropped is not None and dropped[i]:
            continue
        info = qeval.parse_reads_info(title.replace("\t", " ").partition(" ")[2])
        value = info["truebc"]
        truebc = value.split(",")
        if from_comment:
            bc, score = (info["barcode"] or "none"), -1
        else:
            bc, score = calls[i] if calls[i] is not None else ("none", -1.0)
        if bc in truebc:
            classes[i] = 1
        elif bc == "none":
            classes[i] = 3
        elif truebc == ["none"]:
            classes[i] = 4
        else:
            classes[i] = 2
        kinds[i] = 0 if value == "none" else (1 if bc == value else 2)
        if bc != "none":
            while buckets[i] <= 1000 and not score < buckets[i] / 10.0:
                buckets[i] += 1
        reads.append((value, bc, score))
    counts = {"correct": int((classes == 1).sum()), "incorrect": int((classes == 2).sum()), "fn": int((classes == 3).sum()), "fp": int((classes == 4).sum())}
    counts["total"] = sum(counts.values())
    roc = np.zeros((1001, 6), dtype=np.int64)
    values = np.array([0 if v == "none" else (1 if b == v else 2) for v, b, _s in reads], dtype=np.int64)
    scores = np.array([s if b != "none" else -np.inf for _v, b, s in reads], dtype=np.float64)
    for q in range(1001):
        called = ~(scores < q / 10.0)
        roc[q] = (len(reads), (called & (values == 1)).sum(), (called & (values == 2)).sum(), (~called & (values == 0)).sum(),
                  (~called & (values != 0)).sum(), (called & (values == 0)).sum())
    return classes, kinds, buckets, counts, roc


def _random_batch(n, seed, n_ids=96, den=42):
    """n titles with truebc in many forms and calls with scores all over the range: (titles, records, calls for _restate)"""
    rng = np.random.default_rng(seed)
    titles, calls = [], []
    recs = np.zeros(n, dtype=native.RESULT_DTYPE)
    for field in ("barcode_idx", "barcode2_idx", "adapter_idx", "adapter_end"):
        recs[field] = -1
    recs["score_den"] = den
    for i in range(n):
        bc = int(rng.integers(0, n_ids)) if rng.integers(0, 4) else -1
        raw = int(rng.integers(0, den + 1))
        truth = ("none", "1,12,3", "", str(bc + 2), "%d,%d" % (bc + 1, bc + 2))[int(rng.integers(0, 5))] if rng.integers(0, 3) == 0 else str(bc + 1)
        extra = (" ch=%d" % i, "", " read=%d  x" % i, " truebc=99", " a=b=c")[int(rng.integers(0, 5))]
        titles.append("r%d%s truebc=%s%s" % (i, extra, truth, (" start=%d" % i) if rng.integers(0, 2) else ""))
        if bc >= 0:
            recs["barcode_idx"][i], recs["adapter_idx"][i], recs["raw_score"][i], recs["adapter_end"][i] = bc, int(rng.integers(0, 2)), raw, 40
            calls.append((str(bc + 1), raw * 100.0 / (1.0 * den)))
        else:
            calls.append(None)
    return titles, recs, calls


def _fastq(titles, lengths=None):
    return "".join("@%s\n%s\n+\n%s\n" % (t, "A" * (lengths[i] if lengths else 120), "I" * (lengths[i] if lengths else 120))
                   for i, t in enumerate(titles)).encode("latin-1")


def _same(out, want):
    classes, kinds, buckets, counts, roc = want
    assert out.counts == counts
    assert np.array_equal(out.classes, classes) and np.array_equal(out.kinds, kinds) and np.array_equal(out.buckets, buckets)
    assert np.array_equal(out.roc, roc)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 63, 64, 65, 257, 4097])
def test_sizes_around_a_wave_and_a_workgroup_against_a_restatement(ctx, n, shape):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    titles, recs, calls = _random_batch(n, 100 + n)
    batch = native.ResidentBatch.upload_text(ctx, _fastq(titles))
    out = ctx.eval_text(kit, batch, pbc._tsv_names(), records=recs)
    again = ctx.eval_text(kit, batch, pbc._tsv_names(), records=recs)
    batch.destroy()
    _same(out, _restate(titles, calls))
    assert n < 257 or (len(set(out.classes.tolist())) == 4 and len(set(out.buckets.tolist())) >= 40)
    # two runs, the same bytes
    for a, b in ((out.classes, again.classes), (out.kinds, again.kinds), (out.buckets, again.buckets), (out.roc, again.roc)):
        assert a.tobytes() == b.tobytes()
    assert out.counts == again.counts


@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_dropped_reads_are_in_no_count(ctx, where, shape):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor(min_read_length=100))
    n = 70
    titles, recs, calls = _random_batch(n, 7)
    dropped = [where == "all" or i == {"first": 0, "middle": n // 2, "last": n - 1}[where] for i in range(n)]
    titles = [t if not d else "gone%d ch=1" % i for i, (t, d) in enumerate(zip(titles, dropped))]     # (a dropped read needs no truebc)
    batch = native.ResidentBatch.upload_text(ctx, _fastq(titles, [60 if d else 120 for d in dropped]))
    out = ctx.eval_text(kit, batch, pbc._tsv_names(), records=recs)
    rows = ctx.tsv_text(kit, batch, pbc._tsv_names(), records=recs)
    batch.destroy()
    _same(out, _restate(titles, calls, dropped=dropped))
    assert out.counts["total"] == n - sum(dropped) == rows.text.count(b"\n")           # the reads that have a TSV row
    assert (out.classes == 0).tolist() == dropped


# ---- 4. comment mode -----------------------------------------------------------------------------------------------------------------------
def test_comment_mode_on_the_annotated_stream_gives_the_scans_classes(ctx, capsys, tmp_path):
    pbc = scanner.factory(kit="PBC096")
    # adapter-free reads under truth none (CORRECT) and under a list (FN), forced barcodes under their own id, another id and none
    reads = [synth.synth_read(i, 11, pbc.layouts, 1, 0, error_rate=0.05, force_barcode=i % 96, force_bare=(i % 14 == 0 or i % 21 == 1))
             for i in range(300)]
    reads = [r[:60] if i % 50 == 7 else r for i, r in enumerate(reads)]
    truths = [("none", "1,2,3", str(i % 96 + 1), str(i % 96 + 1), str(i % 96 + 1), str((i + 5) % 96 + 1), "7,8")[i % 7] for i in range(len(reads))]
    text = "".join("@r%d ch=%d truebc=%s\n%s\n+\n%s\n" % (i, i, t, r, "I" * len(r)) for i, (r, t) in enumerate(zip(reads, truths))).encode()
    scanned = pbc.eval_fastx_text(text, trim=False, min_read_length=100)
    stream = pbc.annot_fastx_text(text, trim=False, min_read_length=100)
    kept = scanned.classes != 0
    assert 0 < (~kept).sum() < 20 and stream.count(b" barcode=") == kept.sum()
    batch = native.ResidentBatch.upload_text(ctx, stream)
    out = ctx.eval_text(None, batch, None, from_comment=True)
    batch.destroy()
    assert np.array_equal(out.classes, scanned.classes[kept]) and np.array_equal(out.kinds, scanned.kinds[kept])
    assert out.counts == scanned.counts and len(set(out.classes.tolist())) == 4
    assert not out.buckets.any() and np.array_equal(out.roc[0], out.roc[1000])          # the score is -1: no call at any threshold
    titles = [line[1:].decode() for line in stream.split(b"\n")[0::4] if line]
    _same(out, _restate(titles, None, from_comment=True))
    # the reference's usage: python -m qcat_amd.eval reads.fastq
    path = str(tmp_path / "annotated.fastq")
    with open(path, "wb") as fh:
        fh.write(stream)
    qeval.main([path, "-s", "-n", "p", "-d", "d"])
    assert capsys.readouterr().out == qeval.summary_line("p", "d", scanned.counts) + "\n"
    qeval.main([path])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 + kept.sum() and lines[1].split("\t")[:3] == ["-", "-", "r0"] and lines[1].endswith("\t-1")


# ---- 5. refusals and state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in _CASES if "refused" in c], ids=lambda c: c["name"])
def test_a_read_the_reference_cannot_read_is_refused_by_its_number(ctx, case_scanners, case, shape):
    assert _GOLD["case:" + case["name"]]["raises"] in ("KeyError", "IndexError", "TypeError")
    det = case_scanners[case["kit"]]
    good_case = [c for c in _CASES if c["name"] == "epi"][0]
    kit, good_batch, good_recs = _case_call(ctx, det, good_case)
    good = ctx.eval_text(kit, good_batch, det._tsv_names(), records=good_recs)
    rows = ctx.tsv_text(kit, good_batch, det._tsv_names(), records=good_recs)
    kit, batch, recs = _case_call(ctx, det, case)
    with pytest.raises(RuntimeError, match=r"error -1.*qcat_batch_eval: read %d cannot be evaluated" % case["refused"]):
        ctx.eval_text(kit, batch, det._tsv_names(), records=recs)
    batch.destroy()
    # no result is left behind, the other products of the context are, and the context goes on working
    with pytest.raises(RuntimeError, match="error -1.*qcat_ctx_fetch_eval: no evaluation on this context"):
        ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_eval(ctx.handle, None, None, None, None))
    buf = np.empty(len(rows.text), dtype=np.uint8)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_tsv_text(ctx.handle, buf.ctypes.data, len(buf), None))
    assert buf.tobytes() == rows.text
    again = ctx.eval_text(kit, good_batch, det._tsv_names(), records=good_recs)
    good_batch.destroy()
    assert again.counts == good.counts and again.classes.tobytes() == good.classes.tobytes() and again.roc.tobytes() == good.roc.tobytes()


def test_refusals_of_comment_mode_scores_and_arguments(ctx):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    names = pbc._tsv_names()
    titles, recs, _calls = _random_batch(40, 3)
    batch = native.ResidentBatch.upload_text(ctx, _fastq(titles))
    good = ctx.eval_text(kit, batch, names, records=recs)
    # comment mode: the first of two bad reads is named
    for lacking, bad_title, number, why in (((11, 30), "r%d truebc=1", 12, "barcode="), ((5, 6), "r%d barcode=2", 6, "truebc=")):
        stream = [bad_title % i if i in lacking else t + " barcode=1" for i, t in enumerate(titles)]
        other = native.ResidentBatch.upload_text(ctx, _fastq(stream))
        with pytest.raises(RuntimeError, match=r"error -1.*qcat_batch_eval: read %d cannot be evaluated.*%s" % (number, why)):
            ctx.eval_text(None, other, None, from_comment=True)
        other.destroy()
    # a called record without a score
    at = int(np.flatnonzero(recs["barcode_idx"] >= 0)[2])
    for field, value in (("score_den", 0), ("raw_score", -1)):
        bad = recs.copy()
        bad[field][at] = value
        with pytest.raises(RuntimeError, match=r"error -1.*qcat_batch_eval: read %d cannot be evaluated.*score_den" % (at + 1)):
            ctx.eval_text(kit, batch, names, records=bad)
    assert ctx.eval_text(kit, batch, names, records=recs).roc.tobytes() == good.roc.tobytes()
    # arguments: records == NULL without a matching scan, unknown flags, missing names, a batch without a text plane
    counts = native.EvalCounts()

    def call(k, b, r, nm, flags):
        rc = ctx.hip.lib.qcat_batch_eval(ctx.handle, k, b, r, nm, flags, native.C.byref(counts))
        return rc, ctx.hip.lib.qcat_last_error() or b""
    other = native.ResidentBatch.upload_text(ctx, _fastq(titles[:5]))
    rc, err = call(kit.handle, other.handle, None, native.C.byref(names.struct), 0)
    assert rc == -1 and b"records == NULL" in err
    other.destroy()
    rc, err = call(kit.handle, batch.handle, recs.ctypes.data, native.C.byref(names.struct), 2)
    assert rc == -1 and b"flags" in err
    rc, err = call(None, batch.handle, None, None, 3)
    assert rc == -1 and b"flags" in err
    rc, err = call(kit.handle, batch.handle, recs.ctypes.data, None, 0)
    assert rc == -1 and b"name tables" in err
    plain = native.ResidentBatch.upload(ctx, *native.pack_reads(["ACGT" * 30] * 4))
    for flags in (0, 1):
        rc, err = call(kit.handle, plain.handle, recs[:4].copy().ctypes.data, native.C.byref(names.struct), flags)
        assert rc == -1 and b"no text plane" in err
    plain.destroy()
    # records == NULL with the matching scan: the scan's own records
    ctx.scan_resident(kit, batch, fetch=False)
    assert ctx.eval_text(kit, batch, names).counts["total"] == len(titles)
    batch.destroy()

"""The one-wave-per-alignment kernels (qcat_amd/csrc/kernels_tiny.inc) on the configurations that used to bypass them:
qcat_sg_align without statistics (k_sg_wave), qcat_scan_sequences of kits with affine gap costs (k_tiny_adapter_affine) and of
simple kits (k_tiny_simple_barcode / k_tiny_simple_select).  Every answer against the CPU oracle or the independent DP's
recorded vectors, the path proven by qcat_ctx_tiny_ends, and the general kernels (QCAT_HIP_NO_TINY=1) as the cross-check."""
import json
import os
import random

import pytest

import helpers
import oracle_lib
import sg_cases
import simple_cases
import synth
from qcat_amd import config, native, scanner
from qcat_amd.utils import revcomp

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_path(_throughput_kernels_for_small_batches):
    """tests/conftest.py pins the general kernels (QCAT_HIP_NO_TINY=1) for GPU modules it does not list; this module tests the
    library's default routing, so the switch is cleared once that fixture has set it (and that fixture restores it afterwards)"""
    native.set_option("NO_TINY", None)
    before = native.get_option("WAVE_MAX")
    native.set_option("WAVE_MAX", 1 << 40)          # (whatever the default limits are: kernels_tiny.inc)
    yield
    native.set_option("WAVE_MAX", before)


def _tiny(ctx):
    return native.HipLibrary.get().lib.qcat_ctx_tiny_ends(ctx.handle)


class _no_tiny(object):
    def __enter__(self):
        native.set_option("NO_TINY", 1)

    def __exit__(self, *exc):
        native.set_option("NO_TINY", None)


def _triples(got):
    return [(int(r["score"]), int(r["end_query"]), int(r["end_ref"])) for r in got]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. qcat_sg_align: the DP pin
# ---------------------------------------------------------------------------------------------------------------------------
def test_sg_align_vectors_run_one_wave_each():
    with open(os.path.join(helpers.GOLDEN, "sg_vectors.json")) as fh:
        fx = json.load(fh)
    ctx = native.NativeContext(0)
    groups, singles = {}, []
    for i, want in enumerate(fx["results"]):
        s1, s2, go, ge, table = sg_cases.case(fx["seed"], i)
        if i % 8 == 5:
            singles.append((s1, s2, go, ge, table, tuple(want)))          # scores of its own: the n = 1 shape
        else:
            groups.setdefault((go, ge, table.tobytes()), []).append((s1, s2, table, tuple(want)))
    assert len(groups) <= 4 and len(singles) >= 1400
    for (go, ge, _t), cases in sorted(groups.items(), key=lambda kv: kv[0][:2]):
        qs, ts, table = [c[0] for c in cases], [c[1] for c in cases], cases[0][2]
        got = native.sg_align(ctx, qs, ts, go, ge, table)
        assert _tiny(ctx) == len(cases)
        assert _triples(got) == [c[3] for c in cases]
        assert not got["matches"].any() and not got["length"].any()
        with _no_tiny():
            general = native.sg_align(ctx, qs, ts, go, ge, table)
            assert _tiny(ctx) == 0
        assert general.tobytes() == got.tobytes()
        stats = native.sg_align(ctx, qs[:50], ts[:50], go, ge, table, with_stats=True)
        assert _tiny(ctx) == 0 and _triples(stats) == [c[3] for c in cases[:50]]
    for k, (s1, s2, go, ge, table, want) in enumerate(singles):
        got = native.sg_align(ctx, [s1], [s2], go, ge, table)
        assert _tiny(ctx) == 1
        assert _triples(got) == [want], (s1, s2, go, ge)
        if k % 100 == 0:
            with _no_tiny():
                assert native.sg_align(ctx, [s1], [s2], go, ge, table).tobytes() == got.tobytes()
                assert _tiny(ctx) == 0
    # rule R1 in plain parasail.sg's order: a sample of 400 over every family against the oracle
    rng = random.Random(400)
    sample = rng.sample(range(len(fx["results"])), 400)
    with helpers.r1_rule("scalar"):
        for i in sample:
            s1, s2, go, ge, table = sg_cases.case(fx["seed"], i)
            got = native.sg_align(ctx, [s1], [s2], go, ge, table)
            assert _tiny(ctx) == 1
            assert _triples(got) == [oracle_lib.sg(s1, s2, go, ge, table, rule=native.R1_SCALAR)], (i, s1, s2)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. qcat_sg_align: the lanes' edges
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_pairs():
    rng = random.Random(7)
    qlens, tlens = (0, 1, 63, 64, 65, 128, 129, 4500), (1, 63, 64, 65, 128)
    qs, ts = [], []
    for k in range(130):
        L, M = qlens[k % 8], tlens[(k // 8 + k) % 5]
        t = "".join(rng.choice("ACGT" if k % 3 else "ACGTNX") for _ in range(M))
        q = "".join(rng.choice("ACGT") for _ in range(L))
        if k % 2 and L > M:                                              # a noisy copy of the target inside the query
            p = rng.randrange(0, L - M + 1)
            q = q[:p] + "".join(c if rng.random() > 0.1 else rng.choice("ACGT") for c in t) + q[p + M:]
        if k % 5 == 1:
            q = "".join(c if rng.random() > 0.2 else rng.choice("NXnx*-Ry") for c in q)
        if k % 7 == 2:
            q = q.lower()
        if k % 11 == 3:
            t = t.lower()
        if k == 129:
            q, t = "*" * 40, "N" * 65
        qs.append(q)
        ts.append(t)
    return qs, ts


@pytest.mark.parametrize("gaps", [(2, 2), (3, 1)])
def test_sg_align_edges(gaps):
    cfg = config.qcatConfig()
    ctx = native.NativeContext(0)
    qs, ts = _edge_pairs()
    assert {len(q) for q in qs} >= {0, 1, 63, 64, 65, 128, 129, 4500} and {len(t) for t in ts} >= {1, 63, 64, 65, 128}
    want = [(0, -1, -1) if not q else oracle_lib.sg(q, t, gaps[0], gaps[1], cfg.matrix.table) for q, t in zip(qs, ts)]
    got = native.sg_align(ctx, qs, ts, gaps[0], gaps[1], cfg.matrix.table)               # n = 130
    assert _tiny(ctx) == 130
    assert _triples(got) == want
    k = 12                                                                               # n = 1: 65 letters against 65
    assert (len(qs[k]), len(ts[k])) == (65, 65)
    one = native.sg_align(ctx, [qs[k]], [ts[k]], gaps[0], gaps[1], cfg.matrix.table)
    assert _tiny(ctx) == 1 and _triples(one) == [want[k]]
    with _no_tiny():
        assert native.sg_align(ctx, qs, ts, gaps[0], gaps[1], cfg.matrix.table).tobytes() == got.tobytes()
        assert _tiny(ctx) == 0


def test_calls_beyond_the_limits_stay_on_the_general_kernels():
    """the size limit (option WAVE_MAX) and the gap costs beyond the biased cells' range (WAVE_GAP_MAX = 4096, wave_core.h):
    counter 0, the same answers"""
    cfg = config.qcatConfig()
    ctx = native.NativeContext(0)
    qs, ts = _edge_pairs()
    qs, ts = zip(*[(q, t) for q, t in zip(qs, ts) if q][:8])
    qs, ts = list(qs), list(ts)
    want = native.sg_align(ctx, qs, ts, 3, 1, cfg.matrix.table)
    assert _tiny(ctx) == 8
    native.set_option("WAVE_MAX", 7)
    assert native.sg_align(ctx, qs, ts, 3, 1, cfg.matrix.table).tobytes() == want.tobytes() and _tiny(ctx) == 0
    native.set_option("WAVE_MAX", 8)
    assert native.sg_align(ctx, qs, ts, 3, 1, cfg.matrix.table).tobytes() == want.tobytes() and _tiny(ctx) == 8
    for gaps in ((4096, 1), (4097, 1), (3, 4097)):
        got = native.sg_align(ctx, qs, ts, gaps[0], gaps[1], cfg.matrix.table)
        assert _tiny(ctx) == (8 if max(gaps) <= 4096 else 0)
        assert _triples(got) == [oracle_lib.sg(q, t, gaps[0], gaps[1], cfg.matrix.table) for q, t in zip(qs, ts)]
    native.set_option("WAVE_MAX", 1 << 40)
    det = scanner.factory(mode="epi2me", kit="NBD103/NBD104")
    seqs = _mixed_sequences(det.layouts, 1, 0)[:6]
    bases, offsets = native.pack_reads(seqs)
    for gaps in ((4096, 1), (4097, 1)):
        d = det.descriptor(qcat_config=_affine_cfg(gaps), ends=native.ENDS_5P)
        got = ctx.scan_sequences(native.NativeKit(d), bases, offsets)
        assert _tiny(ctx) == (len(seqs) if gaps[0] <= 4096 else 0)
        assert got.tobytes() == oracle_lib.scan_sequences(d, seqs).tobytes()
    d = det.descriptor(qcat_config=_affine_cfg((3, 1)), ends=native.ENDS_5P)
    native.set_option("WAVE_MAX", 5)                 # fewer than the call's waves
    assert ctx.scan_sequences(native.NativeKit(d), bases, offsets).tobytes() == oracle_lib.scan_sequences(d, seqs).tobytes()
    assert _tiny(ctx) == 0
    sdet = scanner.factory(mode="simple", kit="standard")
    d5 = sdet.descriptor(ends=native.ENDS_5P)
    assert ctx.scan_sequences(native.NativeKit(d5), bases, offsets).tobytes() == oracle_lib.scan_sequences(d5, seqs).tobytes()
    assert _tiny(ctx) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. / 4. kits with affine gap costs on whole sequences
# ---------------------------------------------------------------------------------------------------------------------------
def _affine_cfg(gaps):
    cfg = config.qcatConfig()
    cfg.gap_open, cfg.gap_extend = gaps
    return cfg


def _mixed_sequences(layouts, t5, t3):
    reads = synth.synth_batch(12, 31337, layouts, t5, t3, error_rate=0.1)
    seqs = []
    for i, r in enumerate(reads):
        if i % 4 == 0:
            seqs.append(r[: 100 + 37 * i])
        elif i % 4 == 1:
            seqs.append(r[150:-150])
        elif i % 4 == 2:
            seqs.append((r + reads[i - 1]).lower())
        else:
            seqs.append(r[:300] + "N" * 40 + "RYKM*-" + r[300:])
    return seqs + ["", "A", (reads[0] * 7)[:4000]]


@pytest.mark.parametrize("rule", ["striped", "scalar"])
@pytest.mark.parametrize("gaps", [(3, 1), (5, 2), (1, 3)])
@pytest.mark.parametrize("kit,t5,t3", [("NBD103/NBD104", 1, 0), ("VMK001", 0, -1)])
def test_affine_kits_scan_whole_sequences_on_waves(kit, t5, t3, gaps, rule):
    det = scanner.factory(mode="epi2me", kit=kit)
    assert (max(len(l.get_adapter_sequences()) for l in det.layouts) > 64) == (kit == "VMK001")
    seqs = _mixed_sequences(det.layouts, t5, t3)
    with helpers.r1_rule(rule):
        d = det.descriptor(qcat_config=_affine_cfg(gaps), ends=native.ENDS_5P)
        kit_h = native.NativeKit(d)
        want = oracle_lib.scan_sequences(d, seqs)
    assert (want["barcode_idx"] >= 0).sum() >= 3
    bases, offsets = native.pack_reads(seqs)
    ctx = native.NativeContext(0)
    got = ctx.scan_sequences(kit_h, bases, offsets)
    assert _tiny(ctx) == len(seqs)
    assert got.tobytes() == want.tobytes()
    with _no_tiny():
        general = ctx.scan_sequences(kit_h, bases, offsets)
        assert _tiny(ctx) == 0
    assert general.tobytes() == want.tobytes()


def test_scan_middle_under_an_affine_config():
    det = scanner.factory(kit="NBD103/NBD104")
    cfg = _affine_cfg((3, 1))
    reads = synth.synth_batch(4, 77, det.layouts, 1, 0, error_rate=0.05, no_adapter_fraction=0.0)
    n = cfg.max_align_length
    chimera = reads[0] + reads[1] + reads[2]
    rng = random.Random(5)
    clean = reads[3][:n] + "".join(rng.choice("ACGT") for _ in range(900)) + reads[3][-n:]
    kit_name = det.layouts[0].kit
    lays = det.get_adapters(kit_name)
    d = det.descriptor(layouts=lays, qcat_config=cfg, ends=native.ENDS_5P)
    answers = []
    for seq in (chimera, clean):
        middle = seq[n:-n]
        recs = oracle_lib.scan_sequences(d, [middle, revcomp(middle)])
        want = any(r["barcode_idx"] >= 0 and not int(r["raw_score"]) * 100.0 / (1.0 * int(r["score_den"])) < 50.0 for r in recs)
        assert det.scan_middle(seq, kit_name, cfg) == want
        assert _tiny(det._context()) == 2
        answers.append(want)
    assert answers == [True, False]


# ---------------------------------------------------------------------------------------------------------------------------
# 5. simple kits on whole sequences
# ---------------------------------------------------------------------------------------------------------------------------
def _simple_sequences(barcodes, seed, pick=None):
    rng = random.Random(seed)
    bl = len(barcodes[0])

    def noisy(b):
        return "".join(c if rng.random() > 0.08 else rng.choice("ACGT") for c in b)

    def rnd(k):
        return simple_cases.random_seq(rng, k)

    seqs = ["", rnd(1), rnd(max(bl - 3, 1)), rnd(63), rnd(64), rnd(65), rnd(151), rnd(4500)]
    for b in (barcodes[0], barcodes[-1], barcodes[len(barcodes) // 2]):
        seqs.append(noisy(b) + rnd(200))                                 # at offset 0
        seqs.append(rnd(90) + noisy(b) + rnd(140))                       # mid-sequence
        seqs.append(rnd(180) + noisy(b)[:len(b) - 5])                    # cut off at the end
    seqs += ["R" * 200, "*" * 40]
    return seqs if pick is None else [seqs[i] for i in pick]


def _check_simple(det, seqs, scans=4):
    d5 = det.descriptor(ends=native.ENDS_5P)
    kit_h = native.NativeKit(d5)
    want = oracle_lib.scan_sequences(d5, seqs)
    bases, offsets = native.pack_reads(seqs)
    ctx = native.NativeContext(0)
    got = ctx.scan_sequences(kit_h, bases, offsets)
    assert _tiny(ctx) == len(seqs)
    assert got.tobytes() == want.tobytes()
    with _no_tiny():
        general = ctx.scan_sequences(kit_h, bases, offsets)
        assert _tiny(ctx) == 0
    assert general.tobytes() == got.tobytes()
    cfg = config.qcatConfig()
    longs = [(q, r) for q, r in zip(seqs, got) if len(q) > cfg.max_align_length][:scans]
    assert len(longs) == min(scans, 4)
    for q, rec in longs:                                                  # BarcodeScannerSimple.scan() of a long sequence
        one = det.scan(q, None, [], [], qcat_config=cfg)
        assert one["adapter_end"] == int(rec["adapter_end"])
        assert (det.barcodes.index(one["barcode"]) if one["barcode"] else -1) == int(rec["barcode_idx"])
    return want


def test_simple_list_of_one_and_of_two(tmp_path):
    for n in (1, 2):
        bcs = simple_cases.random_list(10 + n, n, 24)
        det = simple_cases.detector(tmp_path, bcs, name="list%d.fa" % n)
        want = _check_simple(det, _simple_sequences(bcs, n))
        assert (want["barcode_idx"] >= 0).sum() >= 3


def test_simple_standard_list_and_the_list_order_chain():
    det = scanner.factory(mode="simple", kit="standard")
    bcs = [b.sequence for b in det.barcodes]
    seqs = _simple_sequences(bcs, 3)
    want = _check_simple(det, seqs)
    assert (want["barcode_idx"] >= 0).sum() >= 6
    # a winner whose raw score is exactly 0 is below every positive min_quality and leaves an empty record: with min_quality 0
    # the record names it.  Every barcode scores 0 against letters outside the alphabet, so rule R2's chain ends at the LAST
    # barcode of the list where the plain maximum would name the first.
    # (without the empty sequence: at min_quality 0 the oracle gives "no barcode, exit 0" for it where every device kernel,
    # the general one included, gives the empty record -- a corner of that setting, not of the path)
    det0 = scanner.factory(mode="simple", kit="standard", min_quality=0)
    seqs = [q for q in seqs if q]
    want0 = _check_simple(det0, seqs)
    zero = [i for i, r in enumerate(want0) if r["barcode_idx"] >= 0 and r["raw_score"] == 0]
    assert zero and all(want0[i]["barcode_idx"] == len(bcs) - 1 for i in zero if seqs[i] in ("R" * 200, "*" * 40))
    assert seqs.index("R" * 200) in zero


def test_simple_ragged_list(tmp_path):
    with open(os.path.join(helpers.GOLDEN, "simple_ragged.json")) as fh:
        entry = json.load(fh)[0]
    fa = tmp_path / "ragged.fasta"
    fa.write_text(entry["fasta"])
    det = scanner.factory(mode="simple", kit=str(fa))
    bcs = [b.sequence for b in det.barcodes]
    assert min(len(b) for b in bcs) <= 16 and max(len(b) for b in bcs) >= 29
    rng = random.Random(9)
    seqs = _simple_sequences(bcs, 4)
    for b in bcs[:8]:
        seqs.append(simple_cases.random_seq(rng, 60) + b + simple_cases.random_seq(rng, 120))
    want = _check_simple(det, seqs)
    lengths = {len(bcs[int(r["barcode_idx"])]) for r in want if r["barcode_idx"] >= 0}
    assert len(lengths) >= 2, lengths


def test_simple_longest_lists_the_library_takes(tmp_path):
    """Barcodes of 64 letters fill the wave's 64 lanes (a ragged list: 57 and 64).  Lists with longer barcodes -- two columns per
    lane -- do not exist: kit preparation and the oracle refuse targets beyond QCAT_MAX_TARGET_LEN = 64, as before."""
    bcs = simple_cases.random_list(21, 5, 64) + simple_cases.random_list(22, 3, 57)
    det = simple_cases.detector(tmp_path, bcs, name="wide.fa")
    want = _check_simple(det, _simple_sequences(bcs, 5))
    assert (want["barcode_idx"] >= 0).sum() >= 3
    longer = simple_cases.detector(tmp_path, simple_cases.random_list(23, 5, 70) + simple_cases.random_list(24, 3, 128), name="longer.fa")
    with pytest.raises(RuntimeError):
        native.NativeKit(longer.descriptor(ends=native.ENDS_5P))


def test_simple_list_of_1024_barcodes(tmp_path):
    bcs = simple_cases.random_list(31, 1024, 24)
    det = simple_cases.detector(tmp_path, bcs, name="big.fa")
    seqs = _simple_sequences([bcs[0], bcs[700], bcs[1023]], 6, pick=(8, 12, 16))   # offset 0, mid-sequence, cut off
    want = _check_simple(det, seqs, scans=3)
    assert sorted(set(int(i) for i in want["barcode_idx"]) - {-1})[-1] >= 700 and (want["barcode_idx"] >= 0).sum() >= 2

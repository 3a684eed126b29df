"""--detect-middle: the interior scan's scores and its boundary cases (builders, expected side and path runner:
tests/middle_cases.py).

The interior scan leaves the library as one bit per read (exit status 997), decided at `middle_min_score`; every other GPU
module sees it through that bit at 50.0, on reads whose interior adapter sits wherever chimeras put it.  Here the reads
are constructed -- the copy's end on either side of the binary16 kernel's 152-row blocks and across them, interiors at
the edges of the length classes, copies cut by the interior's borders, flanks damaged down to the whole-window path,
letters outside A, C, G, T, interiors at the end of the packed path -- and one batch is scanned under a ladder of
thresholds that holds every value a raw barcode score can produce, so that the rungs at which a read comes back 997 pin
its interior score to the raw unit.  Records and counts must equal the expected ones byte for byte at every rung, on every
interior path, and every path proves that it ran.

The CPU tests (no mark) assert from the oracle alone that every case is the case it claims to be and that the expected
staircases are the full oracle's; profiles/middle_boundary_sweep.txt holds the module's output on an MI355X."""
import numpy as np
import pytest

import geometry_cases as gc
import middle_cases as mc
from qcat_amd import native

gpu = pytest.mark.gpu
ALL = sorted(mc.PLANS) + ["LONG"]


def plan_of(name):
    return mc.plan(*(mc.LONG if name == "LONG" else mc.PLANS[name]))


@pytest.fixture(scope="module", autouse=True)
def _contexts_released_after_the_module():
    yield
    gc.release()
    import gc as collector
    collector.collect()


# ---- plan checks: the oracle alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_the_constructed_reads_are_called_and_sit_where_the_builder_aimed(name):
    p = plan_of(name)
    # error-free ends: the end scans call the kit, so the interior is scanned at all
    missed = ["%d [%s]" % (i, p.cases[i].label) for i in np.nonzero(~p.called)[0]]
    print("%s: %d reads, not called: %s; reads per family (0: decision filler) %s"
          % (p.name, len(p.reads), missed or "none", {int(f): int((p.family == f).sum()) for f in sorted(set(p.family))}))
    assert len(missed) <= 0.05 * len(p.reads), missed
    # a clean copy ends, by the oracle's own interior scan on the copy's strand, at the row the builder aimed at
    # (epi2me reports the end plus the template's trim offset, capped at the interior's length)
    clean = [i for i, c in enumerate(p.cases) if c.clean and p.called[i]]
    for f in {1, 2, 3, 6} & set(p.family):                                  # (every placement family has copies that can be checked so)
        assert sum(p.cases[i].family == f for i in clean) >= 12, (f, len(clean))
    for i in clean:
        c = p.cases[i]
        got = int((p.fwd if c.strand == "+" else p.rev)[i]["adapter_end"])
        want = min(c.row + (0 if p.mode == "dual" else int(p.layouts[c.tpl].trim_offset)), c.m)
        assert got == want, (p.name, c.label, c.m, c.row, got, want)
    # every family is there, on both strands
    fams = {(c.family, c.strand) for c in p.cases}
    want_fams = {6, 0} if name == "LONG" else ({0, 1, 2, 3, 4, 5} if name == "NBD" else {0, 3} if name == "NBD-scalar" else {0, 1, 3} if name == "NBD-ext0" else {0, 1, 2, 3})
    assert fams == {(f, s) for f in want_fams for s in "+-"}, sorted(fams)
    assert len(p.reads) <= 3000


@pytest.mark.parametrize("name", sorted(mc.PLANS))
def test_the_interior_scores_cover_the_decision(name):
    p = plan_of(name)
    real = p.called & (p.den > 1)                                           # (a score of 0 / 1: no barcode)
    dec = np.array([mc.decision_raw(d) for d in p.den])
    at, below = int((real & (p.raw == dec)).sum()), int((real & (p.raw == dec - 1)).sum())
    between = float((p.called & (p.score > p.ladder[0]) & (p.score < p.ladder[-2])).sum()) / len(p.reads)
    print("%s: %d reads at the smallest raw score that reaches 50.0, %d one below, %.3f strictly inside the ladder" % (p.name, at, below, between))
    print("%s: target lengths %s, %d rungs, %d next to a score; scores %s" % (p.name, p.tlens, len(p.ladder), len(p.adjacent()), p.histogram()))
    assert at >= 20 and below >= 20, (at, below)
    assert between >= 0.6, between
    assert (np.diff(p.ladder) > 0).all() and p.ladder[0] == 0.0 and p.ladder[-1] > 100.0
    for t in p.tlens:                                                       # equality is a rung: r * 100.0 / tlen itself
        assert all(r * 100.0 / (1.0 * t) in p.ladder for r in range(1, t + 1))


@pytest.mark.parametrize("name", ALL)
def test_the_derived_verdict_is_the_full_oracles_at_three_rungs(name):
    """997 <=> a called adapter and max over strands of scan_sequences' score >= threshold: at 50.0 and one rung below
    and above the median score the full oracle gives the same records and counts; its staircase is monotone"""
    p = plan_of(name)
    med = int(np.median(p.level[p.called])) - 1                             # the rung of the median score
    at50 = int(np.searchsorted(p.ladder, 50.0))
    assert p.ladder[at50] == 50.0 or 50.0 not in [r * 100.0 / t for t in p.tlens for r in range(t + 1)]
    n997 = []
    for i in sorted({at50, med - 1, med + 1}):
        recs, cnt = p.oracle_at(i)
        want, want_cnt = p.expected(i)
        bad = np.nonzero(recs != want)[0]
        assert recs.tobytes() == want.tobytes(), (p.name, i, [(p.cases[j].label, int(p.level[j])) for j in bad[:5]])
        assert np.array_equal(cnt, want_cnt), (p.name, i)
        n997.append(int((recs["exit_status"] == 997).sum()))
    assert n997 == sorted(n997, reverse=True) and n997[0] > n997[-1] > 0, n997
    assert 20 <= (p.expected(at50)[0]["exit_status"] == 997).sum() <= p.called.sum() - 20 or name == "LONG"     # (the product's threshold splits the batch)


def test_region_path_and_whole_window_path_are_both_taken():
    """family 4 holds reads on both sides of region_min_adapter_score by the oracle's adapter score; beyond the first
    window a copy with damaged flanks finds no good barcode, with whole flanks it does"""
    p = plan_of("NBD")
    rows = [(c, p.adapter_score(c), float(p.score[i])) for i, c in enumerate(p.cases) if c.family == 4 and p.called[i]]
    above = [r for r in rows if r[1] > 90.0]
    below = [r for r in rows if r[1] <= 90.0]
    print("family 4: %d reads above 90.0, %d at or below" % (len(above), len(below)))
    assert len(above) >= 10 and len(below) >= 10
    assert all(r[1] > 90.0 for r in rows if "0 flank" in r[0].label)
    beyond_low = [r[2] for r in below if "beyond" in r[0].label and " s0" in r[0].label]
    beyond_high = [r[2] for r in above if "beyond" in r[0].label and " s0" in r[0].label]
    inside_low = [r[2] for r in below if "inside" in r[0].label and " s0" in r[0].label]
    assert beyond_low and beyond_high and inside_low
    assert max(beyond_low) < 50.0 <= min(beyond_high) and min(inside_low) >= 50.0, (beyond_low, beyond_high, inside_low)


def test_special_letters_are_where_the_cases_say():
    p = plan_of("NBD")
    fam5 = [c for c in p.cases if c.family == 5]
    for c in fam5:
        special = not c.label.startswith(("neighbour", "lower"))
        assert c.special == special, c.label
    assert sum(c.special for c in fam5) >= 30 and not any(c.special for c in p.cases if c.family != 5)
    assert any(ch.islower() for c in fam5 for ch in c.interior(p.n))
    for name in sorted(mc.PLANS):
        if name != "NBD":
            assert not any(c.special for c in plan_of(name).cases)


def test_the_scoring_configurations_ask_the_library():
    """gap 1 keeps the binary16 adapter chains (and with them the packed interior scan), gap 3 does not; neither has the
    bit-sliced adapter plans, which are built on a gap of 2; a window of 100 letters and a barcode region without its
    extension keep everything"""
    from qcat_amd import config
    infos = {name: native.NativeKit(plan_of(name).descriptor(50.0)).describe() for name in ("NBD", "NBD-gap1", "NBD-n100", "NBD-ext0")}
    for name, info in infos.items():
        assert info["packed"] == 1 and info["adapter_f16"] == 1, (name, info)
    assert infos["NBD"]["bitslice_templates"] & 0xFF == 2 and infos["NBD-n100"]["bitslice_templates"] & 0xFF == 2 and infos["NBD-ext0"]["bitslice_templates"] & 0xFF == 2
    assert infos["NBD-gap1"]["bitslice_templates"] == 0
    cfg = config.qcatConfig()
    cfg.gap_open = cfg.gap_extend = 3
    cfg.update_matrix()
    p = plan_of("NBD")
    d3 = native.KitDescriptor(p.layouts, cfg, mode=p.mode, scan_middle=True)
    assert native.NativeKit(d3).describe()["adapter_f16"] == 0
    assert plan_of("NBD-n100").n == 100 and all(len(c.seq) == 200 + c.m for c in plan_of("NBD-n100").cases)


# ---- device runs ---------------------------------------------------------------------------------------------------------------
#: (plan, path) pairs that sweep the whole ladder; the others -- the general kernel, which walks every interior on one lane,
#: and the dual kit with its 128 rungs and two barcode sets -- sweep the rungs next to a score that occurs in the batch (each
#: occurring score's own rung and the next one above it: a read's verdict can only change there)
FULL_LADDER = {(name, path) for name in mc.PLANS for path in mc.PATHS if name != "DUAL" and path not in mc.ADJACENT_ONLY}


def path_params():
    """every interior path; the A/B switches that the library under test does not list are reported as skipped"""
    return [pytest.param(path, marks=() if mc.available(mc.PATHS[path]) else pytest.mark.skip(
        reason="%s: A/B switch of a -DQCAT_AB build, this library has no such path" % ", ".join(sorted(mc.PATHS[path]))))
        for path in sorted(mc.PATHS)]


def report(p, path, rungs, proofs, problems):
    rings = sorted({tuple(r) for _, r, _, _ in proofs})
    tiles = sorted({tuple(t) for _, _, t, _ in proofs})
    waves = sorted({w for _, _, _, w in proofs})
    print("%s path %s: %d of %d rungs (%s), marks %s, interior tiles [walked bit-sliced, big, handed back, of 128] %s, one-wave reads %s: %s"
          % (p.name, path, len(rungs), len(p.ladder), "whole ladder" if len(rungs) == len(p.ladder) else "rungs next to a score",
             [list(r) for r in rings], [list(t) for t in tiles], waves, "ok" if not problems else "%d problems" % len(problems)))


@gpu
@pytest.mark.parametrize("path", path_params())
@pytest.mark.parametrize("name", sorted(mc.PLANS))
def test_every_rung_on_every_interior_path(name, path, hip_options):
    p = plan_of(name)
    rungs = list(range(len(p.ladder))) if (name, path) in FULL_LADDER else p.adjacent()
    problems, proofs = mc.sweep(p, path, rungs, hip_options)
    report(p, path, rungs, proofs, problems)
    assert not problems, "%s, path %s:\n%s" % (p.name, path, "\n".join(problems))


@gpu
@pytest.mark.parametrize("path", sorted(mc.LONG_PATHS))
def test_the_end_of_the_packed_path(path, hip_options):
    """interiors of 16 383 and 16 384 letters stay on the packed interior scan, 16 385 goes to the one-wave kernels (the
    product's default) or, with those switched off, to the general kernel: the rungs next to an occurring score"""
    p = plan_of("LONG")
    ms = sorted({c.m for c in p.cases if c.family == 6})
    assert ms == [mc.MID_MAX - 1, mc.MID_MAX, mc.MID_MAX + 1] and p.called.all()
    rungs = p.adjacent()
    problems, proofs = mc.sweep(p, path, rungs, hip_options, paths=mc.LONG_PATHS)
    report(p, path, rungs, proofs, problems)
    assert not problems, "%s, path %s:\n%s" % (p.name, path, "\n".join(problems))
    if path == "default":
        assert {w for _, _, _, w in proofs} == {int(sum(c.m > mc.MID_MAX for c in p.cases))}, proofs[0]

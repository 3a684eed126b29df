#!/usr/bin/env python
"""Would the interior-scan boundary sweep (tests/test_middle_boundaries_gpu.py) notice a wrong expected side?  CPU only.

Perturbs the EXPECTED staircases of the NBD103/NBD104 plan and compares them with the full oracle, the way the suite
compares the device with them:

 a) the interior adapter end of the family-1 reads (block boundaries) moved by k rows on the copy's strand before the
    barcode region is cut (the package's extract_barcode_region, the barcodes scored with the oracle's DP), k = 0 (must reproduce the plan), 1 .. 6 and -1 .. -6;
 b) the raw score of the reads at the decision (the smallest raw score that reaches 50.0) raised by 1.

Prints what the comparison finds; the output is part of profiles/middle_boundary_sweep.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import middle_cases as mc                       # noqa: E402
import oracle_lib                               # noqa: E402
from qcat_amd import utils                      # noqa: E402
from qcat_amd.scanner_base import extract_barcode_region      # noqa: E402


def strand_raw(p, case, rec, shift):
    """raw barcode score of `case`'s interior on the copy's strand with the adapter end `shift` rows off (region path)"""
    kit_lays = [lay for lay in p.layouts if lay.kit == p.layouts[p.spec["t5"]].kit]
    lay = kit_lays[int(rec["adapter_idx"])]
    seq = case.interior(p.n)
    if case.strand == "-":
        seq = utils.revcomp(seq)
    ctx = int(p.cfg.barcode_context_length)
    stop = int(rec["adapter_end"]) - int(lay.trim_offset) + shift
    region = extract_barcode_region(seq, lay, 0, stop, p.cfg)
    up, dn = lay.get_upstream_context(ctx, 0), lay.get_downstream_context(ctx, 0)
    best = None
    for bc in lay.get_barcode_set(0):
        sc = oracle_lib.sg(region, up + bc.sequence + dn, 1, 1, p.cfg.matrix_barcode.table)[0] if region else None
        if sc is not None and (best is None or best == 0 or best < sc):
            best = sc
    return 0 if best is None else best


def compare(p, what):
    """the perturbed expected side against the full oracle at every rung next to an occurring score"""
    rungs, reads = [], set()
    for i in p.adjacent():
        recs, cnt = p.oracle_at(i)
        want, want_cnt = p.expected(i)
        bad = np.nonzero(recs != want)[0]
        if len(bad) or not np.array_equal(cnt, want_cnt):
            rungs.append(i)
            reads |= set(int(b) for b in bad)
    print("%s: the comparison %s (%d rungs differ, %d reads)" % (what, "FAILS" if rungs else "passes", len(rungs), len(reads)))
    return bool(rungs)


def main():
    p = mc.plan(*mc.PLANS[sys.argv[1] if len(sys.argv) > 1 else "NBD"])
    fam1 = [i for i, c in enumerate(p.cases) if c.family == 1 and c.clean and p.called[i]]
    print("plan %s: %d reads, %d clean family-1 reads" % (p.name, len(p.reads), len(fam1)))
    for shift in (0, 1, -1, 2, -2, 4, -4, 6, -6):
        bump = np.zeros(len(p.reads), dtype=np.int64)
        changed = 0
        for i in fam1:
            c = p.cases[i]
            rec = (p.fwd if c.strand == "+" else p.rev)[i]
            raw = strand_raw(p, c, rec, shift)
            if shift == 0:
                assert raw == int(rec["raw_score"]), (c.label, raw, int(rec["raw_score"]))
            # (both strands' raw scores take the bump: the copy's strand carries the maximum of these reads)
            bump[i] = raw - int(rec["raw_score"])
            changed += bump[i] != 0
        p.derive(raw_bump=bump)
        compare(p, "a) adapter end of the family-1 reads %+d rows: %d of %d raw scores change" % (shift, changed, len(fam1)))
    p.derive()
    dec = np.array([mc.decision_raw(d) for d in p.den])
    at = p.called & (p.den > 1) & (p.raw == dec)
    p.derive(raw_bump=at.astype(np.int64))
    compare(p, "b) raw score + 1 for the %d reads at the decision" % int(at.sum()))
    p.derive()
    assert not compare(p, "unperturbed")


if __name__ == "__main__":
    main()

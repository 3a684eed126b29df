"""The narrow N cell of the bit-sliced ADAPTER arithmetic on the CPU (no GPU needed).  qcat_amd/csrc/abs_core.h keeps TWO
planes of row state per N column of a template, on the ground that the difference b stays in 0..3 there.
tests/abs_ncell_check.cpp checks (a) the cell against the four-plane reference on every valid input, (b) that premise on a
scalar DP of its own and (c) plans that qcat_amd/abs_plan.py emits HERE for templates no shipped kit has -- an N run in
column 1, an N run last, two runs, a run of one N, nothing but N, and a fused pair that forks after its N run -- in the
two-stage, four-stage and front-padded forms against the oracle's DP, score and end_query."""
import os
import subprocess

import pytest

from qcat_amd import abs_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEMPLATES = {
    "lead": "N" * 24 + "TTAACCTACTTGCCTGTCGC",
    "tail": "GGTGCTGAAGAAAGTTGTCGG" + "N" * 24,
    "two": "CAGCACCT" + "N" * 10 + "GGTGCTG" + "N" * 12 + "TTAACC",
    "one": "ACGTTGCAGGTNCCATGACTTAGC",
    "alln": "N" * 30,
}
FUSED = ["CCGTGAC" + "N" * 24 + "TTTCTGTTGG", "CCGTGAC" + "N" * 24 + "ACTTGCCTGT"]
LONG = "AATGTACTTCGTTCAGTTACG" + "N" * 24 + "GTTTTCGCATTTATCGTGAAACGCT"          # four WIDE stages (k_adapter_mw's form)


def _sources():
    plans = ["#define ABS_COPY4(D, S) do { (D)[0] = (S)[0]; (D)[1] = (S)[1]; (D)[2] = (S)[2]; (D)[3] = (S)[3]; } while (0)\n",
             "namespace qabs {\n"]
    cases = []

    def strings(seqs):
        return "const std::string t[%d] = {%s};" % (len(seqs), ", ".join('"%s"' % q for q in seqs))

    for name, seq in TEMPLATES.items():
        cases.append('bad += check_premise("%s", "%s", 400);\n' % (name, seq))
        two = abs_plan.emit_plan("QN2_%s" % name, [seq], "test template %s" % name)
        four = abs_plan.emit_multi("QN4_%s" % name, [seq], "test template %s" % name)
        assert two and four, name
        assert "abs_cell_n2(" in two and "abs_cell_n(" not in two and "abs_cell_n2(" in four and "abs_cell_n(" not in four
        plans += [two, four]
        cases.append("{ %s\n" % strings([seq]))
        for L, rounds in ((150, "rounds"), (97, "rounds / 4 + 1"), (7, "rounds / 4 + 1"), (1, "2")):
            cases.append('  bad += check_plan<QN2_%s>("QN2_%s", t, %s, %d, false);\n' % (name, name, rounds, L))
        cases.append('  bad += check_plan<QN2_%s>("QN2_%s", t, rounds / 2 + 1, 211, true);\n' % (name, name))
        cases.append('  bad += check_multi<QN4_%s>("QN4_%s", t, rounds, 150); bad += check_multi<QN4_%s>("QN4_%s", t, rounds / 4 + 1, 97); }\n'
                     % (name, name, name, name))
    fused = abs_plan.emit_plan("QN2_fused", FUSED, "test pair: 31 shared columns")
    wide = abs_plan.emit_multi("QN4_long", [LONG], "test template (wide stages)", maxc=abs_plan.MW_MAX_COLUMNS)
    assert fused and wide and abs_plan.emit_multi("QN4_long_narrow", [LONG], "") is None
    plans += [fused, wide, "}  // namespace qabs\n#undef ABS_COPY4\n"]
    cases.append('{ %s\n  bad += check_plan<QN2_fused>("QN2_fused", t, rounds, 150, false); bad += check_plan<QN2_fused>("QN2_fused", t, rounds / 4 + 1, 97, false); }\n'
                 % strings(FUSED))
    cases.append('{ %s\n  bad += check_premise("long", t[0], 400);\n  bad += check_multi<QN4_long>("QN4_long", t, rounds, 150); }\n' % strings([LONG]))
    return "".join(plans), "".join(cases)


@pytest.fixture(scope="module")
def ncell_check(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    tmp = tmp_path_factory.mktemp("abs_ncell")
    plans, cases = _sources()
    (tmp / "abs_ncell_plans.inc").write_text(plans)
    (tmp / "abs_ncell_cases.inc").write_text(cases)
    exe = str(tmp / "abs_ncell_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", os.path.join(ROOT, "qcat_amd", "csrc"), "-I", str(tmp),
                           os.path.join(ROOT, "tests", "abs_ncell_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "oracle"), "-lqcat_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return exe


@pytest.mark.parametrize("seed", [1, 20261018])
def test_narrow_n_cell_premise_and_emitted_plans(ncell_check, seed):
    p = subprocess.run([ncell_check, str(seed), "12"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-2000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert all(l.endswith(": 0 mismatches") for l in lines), out[-3000:]
    assert lines[0].startswith("cell:")
    assert sum(l.startswith("premise") for l in lines) == len(TEMPLATES) + 1
    assert sum("front-padded" in l for l in lines) == len(TEMPLATES)
    assert sum(l.startswith("QN4_") for l in lines) == 2 * len(TEMPLATES) + 1
    # every premise case met N cells, and b = 3 occurs (the bound is tight, not vacuous)
    assert all(" 0 N cells" not in l for l in lines if l.startswith("premise"))
    assert any("largest b 3" in l for l in lines if l.startswith("premise"))


def test_plane_budget_and_n_tables():
    """a stage is limited by its planes (2 per N column), the plan's tables name its N columns, and the forms a template gets
    are those of the equal-cost split (so the shipped kits' plan list stays what it was)"""
    ops = abs_plan.program([TEMPLATES["lead"]])
    p = abs_plan.split_point(ops, max_planes=abs_plan.MAX_STAGE_PLANES)
    assert sum(abs_plan.op_planes(o) for o in ops[:p]) <= abs_plan.MAX_STAGE_PLANES
    assert abs_plan.split_point(ops, max_planes=8) is None
    text = abs_plan.emit_plan("X", [TEMPLATES["one"]], "")
    n0 = text.split("N0[")[1].split("{")[1].split("}")[0].replace(" ", "").split(",")
    n1 = text.split("N1[")[1].split("{")[1].split("}")[0].replace(" ", "").split(",")
    assert "".join(n0 + n1) == "".join("1" if c == "N" else "0" for c in TEMPLATES["one"])
    assert abs_plan.COST["N"] < abs_plan.COST["L"] and abs_plan.col_planes("N") == 2 and abs_plan.col_planes("A") == 4
    # 102 letter-cost columns do not get the two-stage form, though their planes would fit
    vmk = "AATGTACTTCGTTCAGTTACGTATTGCT" + "N" * 24 + "GTTTTCGCATTTATCGTGAAACGCTTTCGCGTTTTTCGTGCGCCGCTTCA"
    assert abs_plan.emit_plan("X", [vmk], "") is None and abs_plan.emit_multi("X", [vmk], "", maxc=abs_plan.MW_MAX_COLUMNS)

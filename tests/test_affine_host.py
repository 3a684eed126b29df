"""The lane arithmetic of an adapter alignment with affine gap costs on the CPU (no GPU needed).

qcat_amd/csrc/affine_core.h is a set of pure functions of 32-bit words (two signed 16-bit lanes each), so
tests/affine_host_check.cpp drives the packed Gotoh recurrence row by row the way a packed kernel would -- two alignments
per lane whose halves have different window lengths, so the freeze of the rows beyond a window is in play -- against the
independent DP's recorded answers (tests/golden/sg_vectors.json, family 5 of tests/sg_cases.py), against the oracle's DP
on random cases and exhaustively on small ones.  No kernel uses the header yet."""
import json
import os
import re
import subprocess
import sys

import pytest

import helpers
import sg_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    exe = str(tmp_path_factory.mktemp("affine") / "affine_host_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "qcat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "affine_host_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "oracle"), "-lqcat_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return exe


def golden_affine_lines():
    """family 5 of the DP pin: (open, extend, table, target, window, score, end_query) as the independent DP recorded them
    under the striped rule; under the scalar rule the independent DP runs here for every fifth case"""
    if helpers.GOLDEN not in sys.path:
        sys.path.insert(0, helpers.GOLDEN)
    import sg_independent
    with open(os.path.join(helpers.GOLDEN, "sg_vectors.json")) as fh:
        fx = json.load(fh)
    lines, n_scalar = [], 0
    for i, want in enumerate(fx["results"]):
        if i % 8 != 5:
            continue
        s1, s2, go, ge, table = sg_cases.case(fx["seed"], i)
        assert go >= ge and all(ch in "ACGTN" for ch in s1 + s2)
        eq_scalar = -9
        if (i // 8) % 5 == 0:
            sc, eq_scalar, _er = sg_independent.sg(s1, s2, go, ge, sg_independent.scorer_from_table7(table), rule="scalar")
            assert sc == want[0]
            n_scalar += 1
        lines.append("%d %d %s %s %s %d %d %d" % (go, ge, " ".join(str(int(v)) for v in table.reshape(-1)), s2, s1, want[0], want[1], eq_scalar))
    return lines, n_scalar


@pytest.mark.parametrize("seed", [1, 20261018])
def test_packed_affine_recurrence_equals_the_scalar_dps(host_check, tmp_path, seed):
    lines, n_scalar = golden_affine_lines()
    assert len(lines) >= 1400 and n_scalar >= 280
    path = tmp_path / "golden_affine.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([host_check, str(path), str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = dict(re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M))
    assert sorted(got) == ["exhaustive 6 x 4", "golden affine family", "random against the oracle"], out
    assert "without tables" not in out, out
    assert int(got["golden affine family"]) == len(lines) + n_scalar, out
    # 24 000 lanes of two windows under two rules (a window of length 0 does not exist: 1..150)
    assert int(got["random against the oracle"]) == 24000 * 4, out
    # (4 + 16 + ... + 4096) windows x (4 + ... + 256) templates x 4 configurations, two halves, two rules
    assert int(got["exhaustive 6 x 4"]) == 5460 * 340 * 4 * 4, out

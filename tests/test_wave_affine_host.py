"""The one-wave-per-alignment schedule under Gotoh's recurrences on the CPU (no GPU needed).

qcat_amd/csrc/wave_core.h holds the per-cell arithmetic of the one-wave kernels under affine gap costs (kernels_tiny.inc) as plain C++, so
tests/wave_affine_check.cpp emulates the 64-lane anti-diagonal schedule around it -- the hand-over from the left neighbour as
an array shift, the carry from column 64 to column 65 -- and compares with the independent DP's recorded answers
(tests/golden/sg_vectors.json, family 5 of tests/sg_cases.py, both R1 rules), with a plain Gotoh loop on every small case and
on targets of 64, 65 and 128 columns.  The same program runs once more under AddressSanitizer and UBSan."""
import json
import os
import re
import subprocess
import sys

import pytest

import helpers
import sg_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ["exhaustive 6 x 4", "golden affine family", "targets of 64, 65 and 128 columns"]


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "qcat_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "wave_affine_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wave_affine")
    return (_build(tmp, "wave_affine_check", ["-O2"]),
            _build(tmp, "wave_affine_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.fixture(scope="module")
def golden_file(tmp_path_factory):
    """family 5 of the DP pin: the independent DP's (score, end_query, end_ref) under the striped rule as recorded; under the
    scalar rule the independent DP runs here for every fifth case (as tests/test_affine_host.py derives them)"""
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
        eq_scalar, er_scalar = -9, -9
        if (i // 8) % 5 == 0:
            sc, eq_scalar, er_scalar = sg_independent.sg(s1, s2, go, ge, sg_independent.scorer_from_table7(table), rule="scalar")
            assert sc == want[0]
            n_scalar += 1
        lines.append("%d %d %s %s %s %d %d %d %d %d" % (go, ge, " ".join(str(int(v)) for v in table.reshape(-1)), s2, s1,
                                                        want[0], want[1], want[2], eq_scalar, er_scalar))
    assert len(lines) >= 1400 and n_scalar >= 280
    path = tmp_path_factory.mktemp("wave_golden") / "golden_affine.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), len(lines) + n_scalar


def _run(exe, golden_path):
    p = subprocess.run([exe, golden_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = dict(re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M))
    assert sorted(got) == SECTIONS, out
    return {k: int(v) for k, v in got.items()}


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan_ubsan"])
def test_the_wave_schedule_equals_the_scalar_dps(programs, golden_file, sanitized):
    path, n_golden = golden_file
    got = _run(programs[1 if sanitized else 0], path)
    assert got["golden affine family"] == n_golden
    # (4 + 16 + ... + 4096) queries x (4 + ... + 256) targets, two rules, five gap configurations
    assert got["exhaustive 6 x 4"] == 5460 * 340 * 2 * 5
    # 6 draws x 3 target lengths x 8 query lengths, two rules, the same five
    assert got["targets of 64, 65 and 128 columns"] == 6 * 3 * 8 * 2 * 5

"""The END of a bit-sliced barcode on the CPU (no GPU needed): after a barcode's row loops the device kernels
(kernels_bitslice.inc) turn the last row's codes and the deficit into the raw score with bs_last_row -- the row maximum
as a deficit, H(L,c) as one carry-save sum -- and hand the best (score, index) planes over as keys with bs_keys32 (both in
qcat_amd/csrc/bs_core.h, pure functions of 32-bit words).  tests/bs_epilogue_check.cpp runs them 32 alignments at a time
against what they replaced: bs_step / bs_max once per column, then bs_finish_split, bit for bit on the final planes; and
the bit-picking loop with kernels_packed.inc's key formula."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = ["exhaustive C=2", "exhaustive C=3", "exhaustive C=4", "exhaustive C=5", "exhaustive C=6",
            "random C=20", "random C=24", "random C=37", "random C=48", "extremes C=24", "extremes C=48", "keys"]


@pytest.fixture(scope="module")
def epilogue_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bs_epilogue") / "bs_epilogue_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "qcat_amd", "csrc"),
                           os.path.join(ROOT, "tests", "bs_epilogue_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 20261017])
def test_last_row_and_keys_equal_what_they_replace(epilogue_check, seed):
    p = subprocess.run([epilogue_check, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = dict(re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M))
    assert sorted(got) == sorted(SECTIONS), out
    # the exhaustive sections cover 4^C code sequences x 340 starting values (320 with shared columns, 20 without)
    for c in range(2, 7):
        assert int(got["exhaustive C=%d" % c]) >= 4 ** c * 340, out
    assert int(got["random C=24"]) >= 100000 and int(got["random C=48"]) >= 100000 and int(got["keys"]) == 64 * 64 * 32, out


def test_the_widest_kernel_the_check_covers_is_the_widest_instantiated():
    """bs_last_row's plane counts are stated for C <= 48 own columns (bs_core.h): the check's largest C is the kernels' largest"""
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "kernels_bitslice.inc")) as fh:
        cases = [int(c) for c in re.findall(r"QB_CASE\((\d+)\)", fh.read())]
    assert max(cases) == 48 and min(cases) == 20
    from qcat_amd import jit
    assert (jit.BS_C_MIN, jit.BS_C_MAX) == (20, 48)

"""The copy kernel of qcat_batch_partition on the CPU (no GPU needed): tests/partition_check.cpp runs the chunk and lane
schedule of k_part_chunks / k_part_copy (qcat_amd/csrc/kernels_partition.inc) on the host through the very functions the
kernels call (qcat_amd/csrc/partition_core.h) -- chunk search, vector ownership, the two aligned source vectors and their
shift -- over segment lists that cover every source and destination residue mod 16, lengths 0..70 at the start, middle
and end of a chunk, segments of several chunks, runs of empty segments beyond the LDS table, and three segments in the
vectors around a chunk boundary.  Buffers carry exactly the device batches' slack; the program is built a second time with
-fsanitize=address,undefined (the stand-alone program only: nothing loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = {"primitives": 16 + 136 + 4 * 8 * 8 * 2 + 9, "residues": 16 * 16 * 10, "lengths at chunk positions": 71 * 3 * 4,
            "long segments": 6, "runs of empty segments": 6 * 4 + 2, "three segments around a chunk boundary": 16 * 3, "random": 150}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "partition_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "qcat_amd", "csrc"), "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "partition_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def partition_check(tmp_path_factory):
    return _build(tmp_path_factory, "partition", [])


@pytest.fixture(scope="module")
def partition_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "partition_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261019])
def test_host_run_of_the_copy_schedule_equals_concatenation(partition_check, seed):
    _run(partition_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(partition_check_sanitized):
    _run(partition_check_sanitized, 7)


def test_the_check_and_the_kernel_share_their_constants():
    """the host run includes partition_core.h itself; the kernel file must take its schedule from there and not restate it"""
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "kernels_partition.inc")) as fh:
        text = fh.read()
    assert '#include "partition_core.h"' in text
    for name in ("qpart::gather_vector", "qpart::find_segment", "qpart::PART_CHUNK", "qpart::PART_LDS_SEGS", "qpart::slice_of"):
        assert name in text, name
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "batch.h")) as fh:
        batch = fh.read()
    assert "constexpr size_t BATCH_SLACK = 64;" in batch                     # = qpart::PART_SLACK, and the compiler holds them together
    assert '#include "partition_core.h"' in batch and "static_assert(BATCH_SLACK == qpart::PART_SLACK" in batch
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "partition_core.h")) as fh:
        assert "constexpr uint32_t PART_SLACK = 64;" in fh.read()

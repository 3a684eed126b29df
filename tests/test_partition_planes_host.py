"""The two-plane copy of qcat_batch_partition on the CPU (no GPU needed): tests/partition_planes_check.cpp runs the chunk and
lane schedule of k_part_copy<2> (qcat_amd/csrc/kernels_partition.inc: bases and qualities in one pass) on the host through
qpart::gather_vectors<P> of qcat_amd/csrc/partition_core.h, the function the kernel calls, for two planes with different
contents, over the families of segment lists of tests/test_partition_host.py; both outputs must equal plain concatenation,
and the one-plane form must equal gather_vector vector for vector.  Built a second time with -fsanitize=address,undefined
(the stand-alone program only: nothing loaded into Python is).  Plus the Python side of the quality plane that needs no
device: pack_qualities and the binding's table."""
import os
import re
import subprocess

import numpy as np
import pytest

from qcat_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = {"residues": 16 * 16 * 10, "lengths at chunk positions": 71 * 3 * 4, "long segments": 6, "runs of empty segments": 6 * 4 + 2,
            "three segments around a chunk boundary": 16 * 3, "random": 150}

NEW_SYMBOLS = ["qcat_batch_upload_fastq", "qcat_batch_has_qualities", "qcat_batch_download_qualities", "qcat_batch_from_device",
               "qcat_batch_devptrs"]


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "partition_planes_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "qcat_amd", "csrc"), "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "partition_planes_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def planes_check(tmp_path_factory):
    return _build(tmp_path_factory, "planes", [])


@pytest.fixture(scope="module")
def planes_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "planes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261020])
def test_host_run_of_the_two_plane_schedule_equals_concatenation_in_both_planes(planes_check, seed):
    _run(planes_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(planes_check_sanitized):
    _run(planes_check_sanitized, 7)


def test_the_kernel_takes_both_plane_counts_from_the_shared_gather():
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "kernels_partition.inc")) as fh:
        text = fh.read()
    assert "qpart::gather_vectors<P>" in text and "k_offsets_check" in text
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "batch_host.inc")) as fh:
        host = fh.read()
    # (the two launches share their argument list: one launcher over the plane count, called with 1 and with 2)
    assert "hipLaunchKernelGGL(k_part_copy<PLANES>" in host and "part_copy_launch<1>(" in host and "part_copy_launch<2>(" in host


def test_pack_qualities_follows_the_reads_offsets():
    reads = ["ACGT", "", "AC", None, "GGGTTT"]
    bases, offsets = native.pack_reads(reads)
    quals = native.pack_qualities(["!#%&", "", b"IJ", None, "abcdef"], offsets)
    assert quals.dtype == np.uint8 and quals.tobytes() == b"!#%&IJabcdef" and len(quals) == int(offsets[-1])
    with pytest.raises(ValueError, match="read 2 has 2 bases and 3 quality values"):
        native.pack_qualities(["!#%&", "", "IJK", None, "abcdef"], offsets)
    with pytest.raises(ValueError, match="read 1 has 0 bases and 1 quality values"):
        native.pack_qualities(["!#%&", "x", "IJ", None, "abcdef"], offsets)
    with pytest.raises(ValueError, match="4 quality strings for 5 reads"):
        native.pack_qualities(["!#%&", "", "IJ", None], offsets)
    assert len(native.pack_qualities([], native.pack_reads([])[1])) <= 1       # (no reads: a placeholder byte at most, like pack_reads)


def test_the_binding_lists_the_new_entry_points():
    hip = native.HipLibrary.get()
    for name in NEW_SYMBOLS:
        assert name in hip.symbols and hasattr(hip.lib, name), name
    text = open(os.path.join(ROOT, "include", "qcat_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "qcat/cli.py:521-526" in text and native.ABI_VERSION == 6
    # the quality plane in the Python layer
    assert callable(native.ResidentBatch.from_device) and callable(native.ResidentBatch.download_qualities)
    assert callable(native.ResidentBatch.devptrs) and callable(native.Partition.qualities)
    assert isinstance(native.ResidentBatch.has_qualities, property)

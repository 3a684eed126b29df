"""--filter-barcodes of the device on the CPU (no GPU needed): tests/filter_check.cpp runs the batch loop of k_filter_hist /
k_filter_floor / k_filter_apply (qcat_amd/csrc/kernels_filter.inc) on the host through the very functions the kernels call
(qcat_amd/csrc/filter_core.h) -- the key of a record, the floor, the emptied record -- against a std::map restatement of the
reference's get_valid(counts, 0.05) + filter_barcodes written in the test program on its own: random records of single, dual
and simple kits in batches of 1, 7, 64, 100 and 4000 with a short last batch, batches whose maximum is `none`, the floor's
edges (maxima 19, 20, 39, 40, 41 against rivals of 1, 2, 3), batches of one read, dual keys that share their first id.  The
program is built a second time with -fsanitize=address,undefined (the stand-alone program only: nothing loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = {"random, single kit": 28, "random, dual kit": 28, "random, simple kit": 28, "the maximum is none": 28,
            "the maximum is none, dual kit": 28, "floor edges": 60, "a batch of one read": 2, "dual keys that share the first id": 2}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "filter_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "qcat_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "filter_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def filter_check(tmp_path_factory):
    return _build(tmp_path_factory, "filter", [])


@pytest.fixture(scope="module")
def filter_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "filter_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261020])
def test_host_run_of_the_filter_equals_the_map_restatement(filter_check, seed):
    _run(filter_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(filter_check_sanitized):
    _run(filter_check_sanitized, 7)


def test_the_check_and_the_kernels_share_their_arithmetic():
    """the host run includes filter_core.h itself; the kernel file must take key, floor and rewrite from there and not restate them"""
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "kernels_filter.inc")) as fh:
        text = fh.read()
    assert '#include "filter_core.h"' in text
    for name in ("qfilt::key_of", "qfilt::floor_of", "qfilt::survives", "qfilt::make_empty", "qfilt::FILTER_LDS_BINS"):
        assert name in text, name
    assert "atomicAdd(&row" in text and "float" not in text and "double" not in text        # integer adds only; the factor lives in filter_core.h


def test_the_header_declares_the_entry_points_and_the_abi_version_stays():
    from qcat_amd import native
    assert native.ABI_VERSION == 6
    with open(os.path.join(ROOT, "include", "qcat_hip.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert "#define QCAT_ABI_VERSION 6" in header
    assert re.search(r"int\s+qcat_scan_resident_batches\(qcat_ctx\* ctx, const qcat_kit\* kit, const qcat_batch\* batch,\s*"
                     r"uint32_t batch_reads, uint32_t flags\);", header)
    assert re.search(r"int\s+qcat_ctx_fetch_kit_slots\(qcat_ctx\* ctx, int32_t\* slots, uint32_t n_batches\);", header)
    assert re.search(r"int\s+qcat_filter_barcodes\(qcat_ctx\* ctx, const qcat_kit\* kit, qcat_result\* records, uint32_t n_reads,\s*"
                     r"uint32_t batch_reads\);", header)
    assert "enum { QCAT_RESIDENT_KIT_AUTO = 1, QCAT_RESIDENT_FILTER_BARCODES = 2 };" in header
    assert (native.RESIDENT_KIT_AUTO, native.RESIDENT_FILTER_BARCODES) == (1, 2)

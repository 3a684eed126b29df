"""The passes of qcat_batch_upload_fastq_text and qcat_batch_demux_text on the CPU (no GPU needed): tests/fqtext_check.cpp runs
the block, wave and lane schedule of k_fq_count / k_fq_lines / k_fq_records and the segment table of k_fq_segments
(qcat_amd/csrc/kernels_fqtext.inc) on the host through the very functions the kernels call (qcat_amd/csrc/fqtext_core.h), and
the tables through the chunk and lane schedule of k_part_chunks / k_part_copy (partition_core.h) -- for a newline of every kind
of line at the last byte of a block, the first byte of the next and around wave, round and lane edges, lines longer than two
blocks, one record, no final newline, reads of length 1, every non-plain form at the first, a middle and the last record, and
random trims with empty kept slices and skipped reads.  Expected: a sequential parser and plain concatenation written in the
check.  The program is built a second time with -fsanitize=address,undefined (the stand-alone program only: nothing loaded into
Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcat_amd", "csrc")

SECTIONS = {"masks": 4000 * 5, "newlines at block edges": 4 * 4 * 4 * 2 * 2, "shapes": 2 * (3 + 6 * 7 + 40) + 1, "refusals": 17 * 3 * 2,
            "output text": 60 + 1}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "fqtext_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", CSRC, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "fqtext_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def fqtext_check(tmp_path_factory):
    return _build(tmp_path_factory, "fqtext", [])


@pytest.fixture(scope="module")
def fqtext_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "fqtext_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261020])
def test_host_run_of_the_text_passes_equals_a_sequential_parser_and_concatenation(fqtext_check, seed):
    _run(fqtext_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(fqtext_check_sanitized):
    _run(fqtext_check_sanitized, 7)


def test_the_check_and_the_kernels_share_their_arithmetic():
    """the host run includes fqtext_core.h itself; the kernel file must take its blocks, masks, ranks, record checks and
    segments from there and not restate them, and the host layer its sizes"""
    with open(os.path.join(CSRC, "kernels_fqtext.inc")) as fh:
        text = fh.read()
    assert '#include "fqtext_core.h"' in text
    for name in ("qfq::FQ_BLOCK", "qfq::FQ_ROUND", "qfq::FQ_ROUNDS", "qfq::FQ_VEC", "qfq::nl_mask16", "qfq::odd_title16", "qfq::odd_seq16",
                 "qfq::lines_bad", "qfq::wave_rank", "qfq::wave_total", "qfq::record_of", "qfq::record_segments", "qfq::FQ_SEGS"):
        assert name in text, name
    assert not re.search(r"0x0A0A0A0A|0x80808080", text)                      # (the SWAR constants live in the header)
    with open(os.path.join(CSRC, "fqtext_host.inc")) as fh:
        host = fh.read()
    for name in ("qfq::blocks_of", "qfq::lines_of", "qfq::records_of", "qfq::output_bound", "qfq::fq_constants", "qfq::FQ_CONST_BYTES",
                 "qfq::FQ_NO_LINE", "k_part_copy<1>", "k_part_chunks", "part_scan_launch<uint64_t>", "part_keys", "part_order"):
        assert name in host, name
    # the argument check, the tail and the read-out of the demultiplexed text are the text products' shared layer, which launches
    # nothing and keeps off the partition's scratch
    with open(os.path.join(CSRC, "text_out_host.inc")) as fh:
        shared = fh.read()
    for name in ("batch_call_check", "text_out_finish", "text_out_fetch_check", "text_out_fetch_copies", "text_out_devptr"):
        assert "static " in shared and name + "(" in shared and name + "(" in host, name
    assert "hipLaunchKernelGGL" not in shared and "part_keys" not in shared and "c->batch.part" not in shared
    with open(os.path.join(CSRC, "qcat_hip.hip")) as fh:
        unit = fh.read()
    assert '#include "kernels_fqtext.inc"' in unit and '#include "fqtext_host.inc"' in unit
    assert unit.index('#include "batch_host.inc"') < unit.index('#include "text_out_host.inc"') < unit.index('#include "fqtext_host.inc"')
    with open(os.path.join(CSRC, "fqtext_core.h")) as fh:
        core = fh.read()
    assert "constexpr uint32_t FQ_BLOCK = FQ_ROUND * FQ_ROUNDS;" in core and '#include "partition_core.h"' in core

"""The new passes of qcat_batch_upload_text and qcat_batch_annot_text on the CPU (no GPU needed): tests/textstream_check.cpp runs
the FASTA record pass (k_fa_records, qcat_amd/csrc/kernels_textstream.inc) through the very functions the kernel calls
(qcat_amd/csrc/fqtext_core.h) against a sequential restatement of fa_parse -- every non-plain form at the first, a middle and the
last record, with and without a final newline --, and the stream's segment tables (qcat_amd/csrc/textstream_core.h) through the
chunk and lane schedule of k_annot_copy against plain concatenation, with two planes: ids of 1 to 11 characters, dual ids, none,
titles with and without a blank and empty, empty kept slices, dropped reads at either end, records that end one byte either side
of a 32 KiB chunk edge, chunks with more segments than the LDS table holds, and tag-plane segments at every offset mod 16.  The
program is built a second time with -fsanitize=address,undefined (the stand-alone program only: nothing loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcat_amd", "csrc")

# 14 forms x 3 places x 2 x 2, less the texts that do not begin with '>' (a blank line or a FASTQ record in front of record 0)
SECTIONS = {"fasta shapes": 2 * (41 + 2), "fasta refusals": 14 * 3 * 2 * 2 - 2 * 4, "stream records": 3 * 2 * 2, "stream slices": 60,
            "stream chunk edges": 3 * 2 * 3 * 2, "stream beyond the LDS table": 6, "two planes at every alignment": 16 * 16, "bound": 6}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "textstream_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", CSRC, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "textstream_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def textstream_check(tmp_path_factory):
    return _build(tmp_path_factory, "textstream", [])


@pytest.fixture(scope="module")
def textstream_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "textstream_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261021])
def test_host_run_of_the_fasta_record_pass_and_the_two_plane_copy(textstream_check, seed):
    _run(textstream_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(textstream_check_sanitized):
    _run(textstream_check_sanitized, 7)


def test_the_check_and_the_kernels_share_their_arithmetic():
    """the host run includes fqtext_core.h and textstream_core.h themselves; the kernel file must take the record checks, the
    blame rule, the segments and the plane decoding from there and not restate them, and the host layer its sizes"""
    with open(os.path.join(CSRC, "kernels_textstream.inc")) as fh:
        text = fh.read()
    assert '#include "textstream_core.h"' in text
    for name in ("qfq::fa_record_of", "qfq::fa_blamed_line", "qfq::FA_OK", "qfq::fa_record_segments", "qfq::FQ_SEGS", "qann::ANNOT_SEGS",
                 "qann::record_segments", "qann::src_in_tag", "qann::src_plane_off", "qpart::gather_vectors<1>", "qpart::find_segment",
                 "qpart::PART_LDS_SEGS", "qpart::PART_CHUNK", "qpart::slice_of", "dev_skipped"):
        assert name in text, name
    assert not re.search(r"1ull << 6[23]|barcode=", text)                     # (the tag bit and the constants live in the header)
    with open(os.path.join(CSRC, "fqtext_host.inc")) as fh:
        host = fh.read()
    for name in ("qfq::fa_records_of", "qfq::fa_record_of_line", "k_fa_records", "k_fa_segments", "k_fq_records", "k_fq_segments"):
        assert name in host, name
    with open(os.path.join(CSRC, "textstream_host.inc")) as fh:
        host = fh.read()
    for name in ("qann::ANNOT_SEGS", "qann::output_bound", "qann::tag_const_off", "qann::tag_plane_bytes", "qann::annot_constants",
                 "k_annot_segments", "k_annot_firsts", "k_annot_copy", "k_part_chunks", "part_scan_launch<uint64_t>"):
        assert name in host, name
    assert "k_part_copy" not in host and "part_keys" not in host             # (scratch and copy of its own, no sort)
    # the id slots of the tag plane: the text products' shared layer builds them, this file calls it
    with open(os.path.join(CSRC, "text_out_host.inc")) as fh:
        shared = fh.read()
    for name, caller in (("qtsv::tables_build", "name_tables_build("), ("qtsv::TSV_MAX_DEN", "tables_at(")):
        assert name in shared and name not in host and caller in shared and caller in host, name
    assert "hipLaunchKernelGGL" not in shared and "part_keys" not in shared and "c->batch.part" not in shared and "k_part_copy" not in shared
    with open(os.path.join(CSRC, "kernels_partition.inc")) as fh:
        part = fh.read()
    assert "k_annot" not in part and "ANNOT_TAG" not in part                  # (k_part_copy<1> / <2> stay what they are)
    with open(os.path.join(CSRC, "qcat_hip.hip")) as fh:
        unit = fh.read()
    assert '#include "kernels_textstream.inc"' in unit and '#include "textstream_host.inc"' in unit

"""The passes of qcat_batch_tsv_text on the CPU (no GPU needed): tests/tsvtext_check.cpp runs the length pass, the scan, the tile
table and the tile, group and lane schedule of k_tsv_write (qcat_amd/csrc/kernels_tsvtext.inc) on the host through the very
functions the kernels call (qcat_amd/csrc/tsvtext_core.h), with the tables of the header's own builder -- decimal digits against
snprintf (0, every power of ten +-1, INT32_MIN / INT32_MAX, random values), the name / comment split of the six title forms,
rows that end one byte before, at and one byte behind a tile edge, rows longer than two tiles by their name and by their
comment, 1, 2, 63, 64, 65 and 257 reads, dropped reads at the first, a middle and the last position and all reads dropped.
Expected: plain sequential concatenation written in the check.  The score table of the builder is compared line by line with
Python's own repr.  The program is built a second time with -fsanitize=address,undefined (the stand-alone program only: nothing
loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcat_amd", "csrc")

SECTIONS = {"decimal": 2 + 9 * 3 * 3 + 5 + 2000 * 2, "titles": 3 * 6 * 2 * 2, "rows and tiles": 3 * (2 * 2 * 3 * 2 + 2 * 2 + 6 * 5 + 2) + 4}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "tsvtext_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", CSRC, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tsvtext_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def tsvtext_check(tmp_path_factory):
    return _build(tmp_path_factory, "tsvtext", [])


@pytest.fixture(scope="module")
def tsvtext_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "tsvtext_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261021])
def test_host_run_of_the_tsv_passes_equals_sequential_concatenation(tsvtext_check, seed):
    _run(tsvtext_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(tsvtext_check_sanitized):
    _run(tsvtext_check_sanitized, 7)


def test_the_score_table_holds_pythons_repr(tsvtext_check):
    """every entry of the table for denominators 1..200 and raw 0..den against repr(raw * 100.0 / (1.0 * den)) computed here, the
    reference's own formatter; an entry is a length byte and at most 23 characters.  What this holds to Python is the header's
    builder (denominator index, slot layout, lengths) and the std::to_chars recipe, which the check restates: the library's own
    fq_repr_double lives in fastq_host.inc, which no stand-alone program can include, and is held to the reference's score
    column by the golden and host-writer comparisons of tests/test_tsvtext_gpu.py."""
    p = subprocess.run([tsvtext_check, "--scores"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    want = ["{} {} {}".format(den, raw, repr(raw * 100.0 / (1.0 * den))) for den in range(1, 201) for raw in range(den + 1)]
    assert len(lines) == len(want) == sum(range(2, 202))
    bad = [(g, w) for g, w in zip(lines, want) if g != w]
    assert not bad, bad[:10]
    assert max(len(w.split(" ")[2]) for w in want) <= 23
    assert any(w.endswith(".0") for w in want) and any(len(w.split(" ")[2]) >= 17 for w in want)


def test_the_check_and_the_kernels_share_their_arithmetic():
    """the host run includes tsvtext_core.h itself; the kernel file must take its digits, names, predicate, fields, tiles and
    lane schedule from there and not restate them, and the host layer its tables, sizes and bounds"""
    with open(os.path.join(CSRC, "kernels_tsvtext.inc")) as fh:
        text = fh.read()
    assert '#include "tsvtext_core.h"' in text
    for name in ("qtsv::TSV_TILE", "qtsv::TSV_VEC", "qtsv::TSV_THREADS", "qtsv::TSV_GROUP", "qtsv::TSV_GROUPS", "qtsv::TSV_VECS_PER_LANE",
                 "qtsv::name_len", "qtsv::row_of", "qtsv::row_len", "qtsv::tile_rows", "qtsv::tile_put_row", "qtsv::vector_whole",
                 "qpart::slice_of", "dev_skipped", "qpart::find_segment"):
        assert name in text, name
    assert not re.search(r"'\\t'|'\\n'|/ ?10|% ?10|none|None", re.sub(r"//.*", "", text))     # (separators, digits and constants live in the header)
    with open(os.path.join(CSRC, "tsvtext_host.inc")) as fh:
        host = fh.read()
    for name in ("qtsv::score_table_build", "qtsv::output_bound", "qtsv::title_bound", "qtsv::tiles_of",
                 "qtsv::TSV_THREADS", "fq_repr_double", "part_scan_launch<uint64_t>", "k_tsv_lengths", "k_tsv_tiles",
                 "k_tsv_write"):
        assert name in host, name
    # the blob and its pointers on the device: the text products' shared layer builds them, this file calls it
    with open(os.path.join(CSRC, "text_out_host.inc")) as fh:
        shared = fh.read()
    for name, caller in (("qtsv::tables_build", "name_tables_build("), ("qtsv::TSV_MAX_DEN", "tables_at(")):
        assert name in shared and name not in host and "static " in shared and caller in shared and caller in host, name
    assert "hipLaunchKernelGGL" not in shared and "part_keys" not in shared and "c->batch.part" not in shared
    assert "part_keys" not in host and "c->batch.part" not in host                           # (scratch of its own, not the partition's)
    with open(os.path.join(CSRC, "qcat_hip.hip")) as fh:
        unit = fh.read()
    assert '#include "kernels_tsvtext.inc"' in unit and '#include "tsvtext_host.inc"' in unit
    assert unit.index('#include "fastq_host.inc"') < unit.index('#include "tsvtext_host.inc"')
    with open(os.path.join(CSRC, "tsvtext_core.h")) as fh:
        core = fh.read()
    for name in ("called(", "dec_len_u32", "dec_len_i32", "dec_char_u32", "dec_char_i32", "row_byte", "row_const", "score_slot"):
        assert name in core, name
    assert re.search(r"constexpr uint32_t TSV_TILE = \d+;", core) and '#include "partition_core.h"' in core

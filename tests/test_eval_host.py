"""The passes of qcat_batch_eval on the CPU (no GPU needed): tests/eval_check.cpp runs the classify pass's vector and lane schedule,
its workgroup histograms and the ROC kernel's rows (qcat_amd/csrc/kernels_eval.inc) on the host through the very functions the
kernels call (qcat_amd/csrc/eval_core.h) -- the tokenizer over aligned 16-byte vectors with titles at every alignment 0..15 of
the text plane, of one byte, ending at the plane's last byte, longer than 4096 bytes with the key at every position of a vector;
list membership for single and dual call texts; the integer bucket rule against ``score < q / 10.0`` in doubles for every
denominator 1..255; for both shapes of the pass (one lane per read, a group of eight) batches of 0, 1, 63, 64, 65, 257 reads and
of one read more than a full grid's first round with dropped reads at the first, a middle and the last
position and all reads dropped, and each refusal with its first read's number.  Expected: a byte-by-byte sequential restatement
of qcat/eval.py and qcat/eval_roc.py with strings and doubles, written in the check.  The program is built a second time with
-fsanitize=address,undefined (the stand-alone program only: nothing loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcat_amd", "csrc")

SECTIONS = {"tokenizer": 16 * 40 * 3 + 16, "membership": 19 * 8, "buckets": sum(den + den // 4 + 1 for den in range(1, 256)),
            "batches": 2 * (6 * 2 * (2 + 4 + 4) + 1)}


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "eval_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", CSRC, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "eval_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def eval_check(tmp_path_factory):
    return _build(tmp_path_factory, "eval", [])


@pytest.fixture(scope="module")
def eval_check_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "eval_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:] + p.stderr.decode()[-3000:]
    got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
    assert got == SECTIONS, out


@pytest.mark.parametrize("seed", [1, 20261021])
def test_host_run_of_the_eval_passes_equals_the_sequential_restatement(eval_check, seed):
    _run(eval_check, seed)


def test_the_same_under_address_and_undefined_behaviour_sanitizers(eval_check_sanitized):
    _run(eval_check_sanitized, 7)


def test_the_check_and_the_kernels_share_their_arithmetic():
    """the host run includes eval_core.h itself; the kernel file must take its masks, tokens, call texts, verdicts, slots and
    table rows from there and not restate them, and the host layer its sizes"""
    with open(os.path.join(CSRC, "kernels_eval.inc")) as fh:
        text = fh.read()
    assert '#include "eval_core.h"' in text
    for name in ("qev::read_verdict", "qev::read_verdict_group", "qev::suffix_sums", "qev::EVAL_GROUP", "__shfl", "qev::hist_slot", "qev::class_slot", "qev::roc_row", "qev::EVAL_THREADS", "qev::EVAL_HIST", "qev::EVAL_Q",
                 "qev::EVAL_ROC_COLS", "qev::CLS_BAD", "qev::CLS_DROPPED", "dev_skipped", "atomicMin", "__shared__"):
        assert name in text, name
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"truebc|barcode=|none|'='|' '|','|1000|1001|1002", code)     # (keys, separators and sizes live in the header)
    assert not re.search(r"\basm\b|__builtin_amdgcn", code)                             # plain HIP
    with open(os.path.join(CSRC, "eval_host.inc")) as fh:
        host = fh.read()
    for name in ("batch_call_check(", "name_tables_build(", "tables_at(", "records_on_device(", "mirror_upload(", "qev::classify_blocks", "qev::classify_group_blocks", "QO_EVAL_SHAPE",
                 "qev::EVAL_HIST", "qev::EVAL_NO_BAD", "qev::bad_text", "k_eval_classify", "k_eval_roc", "c->batch.eval"):
        assert name in host, name
    assert host.count("stream_done(") == 1                                               # one synchronisation
    for other in ("c->batch.tsv", "c->batch.annot", "c->batch.fqtext", "c->batch.part"):
        assert other not in host, other                                                  # scratch of its own
    with open(os.path.join(CSRC, "qcat_hip.hip")) as fh:
        unit = fh.read()
    assert '#include "kernels_eval.inc"' in unit and '#include "eval_host.inc"' in unit
    assert unit.index('#include "textstream_host.inc"') < unit.index('#include "eval_host.inc"')
    with open(os.path.join(CSRC, "eval_core.h")) as fh:
        core = fh.read()
    for name in ("byte_mask16", "blank_mask16", "scan_vector", "scan_title", "scan_title_group", "vector_masks", "suffix_sums", "token_end", "call_of(", "list_holds_call", "span_is_call", "bucket_of",
                 "verdict_of", "roc_row", "qtsv::called", "qfq::zero_bytes", "qfq::pack_high"):
        assert name in core, name
    with open(os.path.join(ROOT, "include", "qcat_hip.h")) as fh:
        header = fh.read()
    for name in ("QCAT_EVAL_FROM_COMMENT = 1", "qcat_eval_counts", "qcat_batch_eval(", "qcat_ctx_fetch_eval(", "#define QCAT_ABI_VERSION 6"):
        assert name in header, name

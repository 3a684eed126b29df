"""The device-free part of the chunked host-buffer scan on the CPU (no GPU needed): tests/pipeline_check.cpp includes
qcat_amd/csrc/pipeline_core.h alone -- the header scan_batch_pipelined (csrc/pipeline_host.inc) takes its pool, its chunk size and
cuts, the sizing rule of its stage slots, the length sums of a chunk's parts with their refusals, the compaction with its
prefetch and the split of a slot's records from -- and compares them with a naive restatement: 240 read counts up to 2^32 - 1
in both read forms with the default and six forced chunk sizes (forced 4096 at 2^32 - 1 must return), the slot sizes over the
calls of test_pipeline_stages_grow_between_calls and over growing file segments, a decreasing offset and a read over 2^32 - 1
in different parts of one chunk (the first in read order is reported, as the upload of a resident batch reports it), the staged
bytes, offsets and lengths of concatenated reads and of reads scattered through a file, 5' only and both ends, with read
lengths 0, 1, n-1, n, n+1, 2n-1, 2n, 2n+1, 3n for n = 150 and n = 4 at every border of a part, on pools of 0, 1, 2 and 7
workers, equal to what the upload of a resident batch stages, and the records of a slot copied exactly once each.  The program
is built three times -- plain, -fsanitize=address,undefined and -fsanitize=thread -- and each build runs as a program of its
own (nothing loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = {"cuts": 240 * 2 * 7, "stage sizing": 2 * (4 + 5 + 1), "length sums and refusals": 4 * 2 * 6,
            "compaction": 2 * 2 * 2 * 2 * 4 * 2, "record flush": 4 * 4}

BUILDS = {"plain": [],
          "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
          "thread": ["-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def pipeline_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pipeline_" + request.param) / "pipeline_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread"] + BUILDS[request.param] +
                          ["-I", os.path.join(ROOT, "qcat_amd", "csrc"), "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "pipeline_check.cpp"), "-o", exe])
    return request.param, exe


def test_pipeline_core_equals_the_naive_restatement(pipeline_check):
    build, exe = pipeline_check
    for seed in ((1, 20261020) if build == "plain" else (7,)):
        p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0, (build, seed, out[-3000:] + p.stderr.decode()[-3000:])
        assert not p.stderr, (build, seed, p.stderr.decode()[-3000:])                 # (a sanitizer's report)
        got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
        assert got == SECTIONS, out


def test_the_host_layer_takes_its_pipeline_steps_from_the_shared_header():
    """the check includes pipeline_core.h itself; scan_batch_pipelined must take its steps from there and not restate them"""
    csrc = os.path.join(ROOT, "qcat_amd", "csrc")
    with open(os.path.join(csrc, "pipeline_host.inc")) as fh:
        text = fh.read()
    for name in ("qpipe::chunk_reads", "qpipe::chunk_cuts", "qpipe::largest_chunk", "qpipe::stage_need", "qpipe::chunk_parts",
                 "qpipe::stage_lengths", "qpipe::stage_compact", "qpipe::copy_records", "qupload::keep_of"):
        assert name in text, name
    assert "memcpy(dst" not in text and "__builtin_prefetch" not in text and "std::thread" not in text
    with open(os.path.join(csrc, "pipeline.h")) as fh:
        assert '#include "pipeline_core.h"' in fh.read()
    with open(os.path.join(csrc, "pipeline_core.h")) as fh:
        core = fh.read()
    assert re.findall(r'#include "([^"]+)"', core) == ["upload_core.h"] and "hip/" not in core       # (no device: the standard library)
    with open(os.path.join(csrc, "upload_core.h")) as fh:
        assert "hip/" not in fh.read()

"""The device-free part of a host-buffer call's upload on the CPU (no GPU needed): tests/upload_check.cpp includes
qcat_amd/csrc/upload_core.h alone -- the header batch_upload_windows (csrc/batch_host.inc) takes its copy of a read, its length
pass, its slice bounds and its two thread schedules from -- and compares them with a naive restatement: both input forms, 5'
only / both ends / whole reads, read lengths 0, 1, n-1, n, n+1, 2n-1, 2n, 2n+1, 3n for n = 150 and n = 4, the three refusals,
and the sliced schedule (workers draw slices from a counter, the calling thread hands finished runs to a sender) with a sender
that copies each range the moment it gets it, on 1, 2, 3 and 8 threads, with reads longer than a slice, empty reads at slice
bounds, and thread factories that fail.  The program is built three times -- plain, -fsanitize=address,undefined and
-fsanitize=thread -- and each build runs as a program of its own (nothing loaded into Python is)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECTIONS = {"staged bytes, offsets and lengths": 2 * 4 * 8 + 2 * 3, "refusals": 3 * 4 + 1, "sliced schedule": 4 * 2 * 3 * 4 + 1,
            "sliced schedule without threads": 4 * 3, "even split without threads": 4 * 3}

BUILDS = {"plain": [],
          "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
          "thread": ["-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def upload_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upload_" + request.param) / "upload_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread"] + BUILDS[request.param] +
                          ["-I", os.path.join(ROOT, "qcat_amd", "csrc"), "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "upload_check.cpp"), "-o", exe])
    return request.param, exe


def test_upload_core_equals_the_naive_restatement(upload_check):
    build, exe = upload_check
    for seed in ((1, 20261020) if build == "plain" else (7,)):
        p = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        out = p.stdout.decode()
        assert p.returncode == 0, (build, seed, out[-3000:] + p.stderr.decode()[-3000:])
        assert not p.stderr, (build, seed, p.stderr.decode()[-3000:])                 # (a sanitizer's report)
        got = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases, 0 mismatches$", out, flags=re.M)}
        assert got == SECTIONS, out
        assert int(re.search(r"^slices run: (\d+)$", out, flags=re.M).group(1)) > 20000, out     # (thousands per schedule)


def test_the_host_layer_takes_its_upload_from_the_shared_header():
    """the check includes upload_core.h itself; batch_upload_windows must take its steps from there and not restate them"""
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "batch_host.inc")) as fh:
        text = fh.read()
    assert '#include "upload_core.h"' in text
    for name in ("qupload::length_pass", "qupload::compact", "qupload::slice_bounds", "qupload::run_sliced", "qupload::run_even"):
        assert name in text, name
    assert "memcpy(dst" not in text and "std::thread" not in text
    with open(os.path.join(ROOT, "qcat_amd", "csrc", "upload_core.h")) as fh:
        core = fh.read()
    assert '#include "' not in core and "hip/" not in core                          # (no device: the standard library alone)

"""FASTA text in device memory (qcat_batch_upload_text, qcat_batch_demux_text and qcat_batch_tsv_text on a FASTA batch,
BarcodeScanner.demux_fastx_text / tsv_fastx_text): the device's parse against qcat_fastq_open on the same bytes -- records, bases,
offsets, and the same verdict with the same record number on every non-plain form, where fa_parse blames the record IN FRONT of
a line that should begin with '>' --, the scan of a FASTA text batch against the scan of the host-parsed reads, and the two
products against the reference driver's own output for FASTA input (tests/golden/cli_golden.json)."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import helpers
import synth
from qcat_amd import config, native, scanner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "qcat_amd", "csrc", "fqtext_core.h")) as _fh:
    _CORE = _fh.read()
BLOCK = 1
for _name in ("FQ_THREADS", "FQ_VEC", "FQ_ROUNDS"):
    BLOCK *= int(re.search(r"constexpr uint32_t %s = (\d+);" % _name, _CORE).group(1))

# name only, comment, tabs, two blanks in a row, a trailing blank, empty
TITLES = ("r{i}", "r{i} ch=3", "r{i}\tch=3\tx=y", "r{i}  two", "r{i} ", "")
LENGTHS = (1, 2, 15, 16, 17, 40, 150, 1, 333, 1000)


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


def _title(i):
    return TITLES[i % len(TITLES)].format(i=i)


def _reads(n, seed, long_at=None):
    rng = np.random.default_rng(seed)
    return ["".join("ACGT"[b] for b in rng.integers(0, 4, 2 * BLOCK + 37 if i == long_at else LENGTHS[i % len(LENGTHS)])) for i in range(n)]


def _text(reads, final_newline=True, titles=None):
    text = "".join(">" + (titles[i] if titles else _title(i)) + "\n" + s + "\n" for i, s in enumerate(reads))
    return (text if final_newline else text[:-1]).encode("latin-1")


def _record_number(message):
    return int(re.search(r"\(record (\d+)\)", str(message)).group(1))


# ---- 1. parse parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 257, 3000])
def test_device_parse_equals_the_host_parse(ctx, n, tmp_path):
    if n == 0:                                                                  # an empty text is what an empty file is: no reads
        empty = native.ResidentBatch.upload_text(ctx, b"")
        assert empty.info() == (0, 0) and not empty.is_fasta
        return
    reads = _reads(n, 100 + n, long_at=1 if n in (2, 3000) else None)
    for final_newline in (True, False):
        text = _text(reads, final_newline)
        assert n < 257 or len(text) > 2 * BLOCK
        path = str(tmp_path / ("t%d.fasta" % final_newline))
        with open(path, "wb") as fh:
            fh.write(text)
        f = native.FastqFile(path)
        assert f.n_reads == n
        batch = native.ResidentBatch.upload_text(ctx, text)
        assert batch.n_reads == n and batch.is_fasta and not batch.has_qualities
        to, tl, so, sl = batch.text_records()
        want = [f.read_info(r) for r in range(n)]
        assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(to, tl, so, sl)] == want
        assert [int(x) for x in tl[:6]] == [len(_title(i).rstrip(" \t")) for i in range(min(n, 6))]
        parsed = [text[o:o + l].decode("latin-1") for _a, _b, o, l in want]
        assert parsed == reads
        host = native.ResidentBatch.upload(ctx, *native.pack_reads(parsed))
        bases, offsets = batch.download()
        want_bases, want_offsets = host.download()
        assert offsets.tobytes() == want_offsets.tobytes() and bases.tobytes() == want_bases.tobytes()
        assert batch.n_bases == host.n_bases and batch.devptrs()[1] is None
        batch.destroy(); host.destroy()


def test_the_dispatch_by_the_first_byte(ctx):
    """anything but '>' goes to exactly what upload_fastq_text does, which itself keeps refusing '>'"""
    reads = _reads(12, 5)
    fastq = "".join("@" + _title(i) + "\n" + s + "\n+\n" + "I" * len(s) + "\n" for i, s in enumerate(reads)).encode("latin-1")
    a, b = native.ResidentBatch.upload_text(ctx, fastq), native.ResidentBatch.upload_fastq_text(ctx, fastq)
    assert not a.is_fasta and not b.is_fasta
    assert [x.tolist() for x in a.text_records()] == [x.tolist() for x in b.text_records()]
    assert a.download()[0].tobytes() == b.download()[0].tobytes() == "".join(reads).encode()
    with pytest.raises(native.ResidentBatch.Unsupported, match="FASTA text is not supported.*record 1"):
        native.ResidentBatch.upload_fastq_text(ctx, _text(reads))
    with pytest.raises(native.ResidentBatch.Unsupported, match="qcat_batch_upload_fastq_text: not a plain four-line FASTQ file .record 3"):
        native.ResidentBatch.upload_text(ctx, fastq[:fastq.index(b"@r2")] + b"@x\n")
    plain = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    with pytest.raises(RuntimeError, match="error -1.*no text plane"):
        plain.is_fasta
    for x in (a, b, plain):
        x.destroy()


# ---- 2. the same verdict ---------------------------------------------------------------------------------------------------------------
FORMS = {
    "wrapped sequence": lambda t, s: ">" + t + "\n" + s[:len(s) // 2] + "\n" + s[len(s) // 2:] + "\n",
    "crlf": lambda t, s: ">" + t + "\r\n" + s + "\r\n",
    "blank line between records": lambda t, s: "\n>" + t + "\n" + s + "\n",
    "trailing blank line": lambda t, s: ">" + t + "\n" + s + "\n\n",
    "blank inside a sequence": lambda t, s: ">" + t + "\n" + s[:3] + " " + s[4:] + "\n",
    "byte 0x80 in a title": lambda t, s: ">a\x80" + t + "\n" + s + "\n",
    "control byte in a title": lambda t, s: ">a\x07" + t + "\n" + s + "\n",
    "empty sequence": lambda t, s: ">" + t + "\n\n",
    "title line without a sequence": lambda t, s: ">" + t + "\n",
    "four-line fastq record": lambda t, s: "@" + t + "\n" + s + "\n+\n" + "I" * len(s) + "\n",
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_non_plain_text_gets_the_verdict_of_the_host_parser(ctx, form, tmp_path):
    n = 9
    reads = [r if len(r) > 8 else r + "ACGTACGT" for r in _reads(n, 7)]
    named = []
    for at in (0, n // 2, n - 1):
        parts = [">" + _title(i) + "\n" + reads[i] + "\n" for i in range(n)]
        parts[at] = FORMS[form](_title(at), reads[at])
        text = "".join(parts).encode("latin-1")
        path = str(tmp_path / ("bad%d.fasta" % at))
        with open(path, "wb") as fh:
            fh.write(text)
        with pytest.raises(native.FastqFile.Unsupported) as host:
            native.FastqFile(path)
        with pytest.raises(native.ResidentBatch.Unsupported, match="error -2") as dev:
            native.ResidentBatch.upload_text(ctx, text)
        assert _record_number(dev.value) == _record_number(host.value), (form, at)
        fasta = text[:1] == b">"                                                # (a text that begins otherwise is refused as FASTQ)
        assert ("two-line FASTA" if fasta else "four-line FASTQ") in str(dev.value) and ("FASTA" if fasta else "FASTQ") in str(host.value)
        named.append(_record_number(dev.value) - 1 - at)
        # nothing is left behind and the context goes on: a plain upload
        good = native.ResidentBatch.upload_text(ctx, _text(reads))
        assert good.n_reads == n and good.is_fasta and good.download()[0].tobytes() == "".join(reads).encode()
        good.destroy()
    # who is blamed: the record in front where a line that should begin with '>' does not, the record itself otherwise
    if form == "blank line between records":
        assert named == [0, -1, -1]                                             # (at 0: the first record of a FASTQ text)
    elif form == "four-line fastq record":
        assert named == [1, -1, -1]                                             # (at 0: a FASTQ text whose second record begins with '>')
    elif form == "title line without a sequence":
        assert named[2] == 0
    else:
        assert named == [0, 0, 0]


# ---- 3. the scan is unchanged ----------------------------------------------------------------------------------------------------------
def _scan_cases():
    pbc = scanner.factory(kit="PBC096")
    yield "single kit", native.NativeKit(pbc.descriptor()), synth.synth_batch(300, 11, pbc.layouts, 1, 0, error_rate=0.08) + ["A", "N" * 200]
    dual = scanner.factory(mode="dual")
    yield "dual kit", native.NativeKit(dual.descriptor()), synth.synth_batch(300, 12, dual.layouts, 1, 0, error_rate=0.08)
    simple = scanner.factory(mode="simple", kit="standard")
    lays = scanner.factory(kit="PBK004/LWB001").layouts
    yield "simple kit", native.NativeKit(simple.descriptor()), synth.synth_batch(300, 13, lays, 1, 0, error_rate=0.05, insert_len=200)
    mid = scanner.factory(kit=synth.FLAGS["kit"], scan_middle_adapter=True)
    text = synth.flags_fastq(scanner.factory(kit=synth.FLAGS["kit"]).layouts)
    yield "detect-middle kit", native.NativeKit(mid.descriptor()), text.split("\n")[1::4]


@pytest.mark.parametrize("which", range(4))
def test_scan_of_a_fasta_text_batch_equals_the_scan_of_the_parsed_reads(ctx, which):
    name, kit, reads = list(_scan_cases())[which]
    assert kit.descriptor.scan_middle == (name == "detect-middle kit")
    host = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    want, want_counts = ctx.scan_resident(kit, host)
    batch = native.ResidentBatch.upload_text(ctx, _text(reads, final_newline=which % 2 == 0))
    assert batch.is_fasta
    got, got_counts = ctx.scan_resident(kit, batch)
    assert got.tobytes() == want.tobytes() and np.array_equal(got_counts, want_counts), name
    assert (got["barcode_idx"] >= 0).sum() > len(reads) // 3, name
    part, want_part = ctx.partition(kit, batch, got), ctx.partition(kit, host, want)
    assert np.array_equal(part.bin_first, want_part.bin_first) and np.array_equal(part.source, want_part.source)
    assert part.batch.download()[0].tobytes() == want_part.batch.download()[0].tobytes()


# ---- 4. the reference driver's output for FASTA input -----------------------------------------------------------------------------------
with open(os.path.join(helpers.GOLDEN, "cli_golden.json")) as _fh:
    _RUNS = json.load(_fh)["runs"]


def _run(tag):
    return [r for r in _RUNS if r["variant"]["tag"] == tag and r["file"] == "fasta_of_nbd103.fasta"][0]


def _fasta_of_nbd103():
    """as tests/golden/make_cli_golden.py (fasta_of_fastq) derives it"""
    with open(os.path.join(helpers.GOLDEN, "data", "nbd103.fastq")) as fh:
        lines = fh.read().split("\n")
    return "".join(">" + lines[i][1:] + "\n" + lines[i + 1] + "\n" for i in range(0, len(lines) - 3, 4))


def test_per_barcode_fasta_files_are_the_reference_drivers():
    run = _run("dir-auto-trim")
    v = run["variant"]
    assert v["trim"] and v["min_len"] == 100 and v["dir"] and run["kit"] == "auto"
    got = scanner.factory(kit="auto").demux_fastx_text(_fasta_of_nbd103(), trim=True, min_read_length=100, qcat_config=config.get_default_config())
    assert {name: hashlib.sha256(data).hexdigest() for name, data in got.items()} == run["files"]
    assert got and all(name.endswith(".fasta") and data.startswith(b">") and b"\n+\n" not in data for name, data in got.items())


def test_table_of_a_fasta_text_is_the_reference_drivers_stdout():
    run = _run("tsv-auto-batch")
    v = run["variant"]
    assert v["tsv"] and not v["trim"] and v["min_len"] == 100 and run["kit"] == "auto"
    got = scanner.factory(kit="auto").tsv_fastx_text(_fasta_of_nbd103(), trim=False, min_read_length=100)
    assert got == run["stdout"].encode("latin-1") and got.count(b"\n") >= 5


# ---- the two products at size: a FASTA text gives what its FASTQ twin gives, without the quality part (the table's bound must
# follow the format: a FASTA record holds its sequence once) ------------------------------------------------------------------------
def test_products_of_a_fasta_text_equal_those_of_its_fastq_twin():
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(400, 20261021, pbc.layouts, 1, 0, error_rate=0.08)
    reads = [r[:60] if i % 50 == 7 else (r[:150] if i % 9 == 4 else r) for i, r in enumerate(reads)]
    fastq = "".join("@" + _title(i) + "\n" + s + "\n+\n" + "I" * len(s) + "\n" for i, s in enumerate(reads)).encode("latin-1")
    for final_newline in (True, False):
        files, table = pbc.demux_fastx_text(_text(reads, final_newline), trim=True, min_read_length=100, tsv=True)
        want_files, want_table = pbc.demux_fastq_text(fastq, trim=True, min_read_length=100, tsv=True)
        assert table == want_table and table.count(b"\n") > 250
        assert sorted(files) == sorted(name.replace(".fastq", ".fasta") for name in want_files) and len(files) >= 20
        for name, data in want_files.items():
            lines = data.split(b"\n")
            want = b"".join(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 3, 4))
            assert files[name.replace(".fastq", ".fasta")] == want, name
        assert (files, table) == pbc.demux_fastx_text(_text(reads, final_newline), trim=True, min_read_length=100, tsv=True)
    assert pbc.demux_fastx_text(fastq, trim=True, min_read_length=100) == want_files       # FASTQ through the dispatch
    assert pbc.tsv_fastx_text(fastq, trim=True, min_read_length=100) == want_table


def test_table_of_a_fasta_text_with_titles_as_long_as_its_reads():
    """the table's bound counts the title bytes as text - sequences - a constant per record; a FASTA record holds its sequence
    once, so the bound of a FASTQ text would fall short here by the reads' bases"""
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(12, 4, pbc.layouts, 1, 0, error_rate=0.05)
    titles = ["t%d " % i + "c" * (len(r) + 40 * i) for i, r in enumerate(reads)]
    fastq = "".join("@" + t + "\n" + s + "\n+\n" + "I" * len(s) + "\n" for t, s in zip(titles, reads)).encode("latin-1")
    want = pbc.tsv_fastq_text(fastq)
    assert pbc.tsv_fastx_text(_text(reads, titles=titles)) == want and len(want) > sum(len(r) for r in reads)

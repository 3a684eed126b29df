"""FASTQ text in device memory (qcat_batch_upload_fastq_text, qcat_batch_demux_text, BarcodeScanner.demux_fastq_text): the
device's parse against qcat_fastq_open on the same bytes -- records, bases, offsets, and the same verdict with the same record
number on every non-plain form --, the scan of a text batch against the scan of the host-parsed reads, and the per-barcode FASTQ
text made on the device against the golden digests of the reference driver's own files, against text formatted here from the
oracle's records, and against the Python path's loop where one bin holds two file names."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import helpers
import oracle_lib
import simple_cases
import synth
from qcat_amd import config, native, scanner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "qcat_amd", "csrc", "fqtext_core.h")) as _fh:
    _CORE = _fh.read()
BLOCK = 1
for _name in ("FQ_THREADS", "FQ_VEC", "FQ_ROUNDS"):
    BLOCK *= int(re.search(r"constexpr uint32_t %s = (\d+);" % _name, _CORE).group(1))

TITLES = ("r{i}", "r{i} ch=3", "r{i}\tch=3\tx=y", "r{i}  two", "r{i} ", "")
LENGTHS = [n for n in simple_cases.READ_LENGTHS if n > 0]


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


def _title(i):
    return TITLES[i % len(TITLES)].format(i=i)


def _record(i, seq, qual):
    """one record; the '+' line alone, with blanks, with the title repeated"""
    title = _title(i)
    plus = ("", " \t ", title.rstrip(" \t"))[(i // 2) % 3]
    return "@" + title + "\n" + seq + "\n+" + plus + "\n" + qual + "\n"


def _reads(n, seed, long_at=None):
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for i in range(n):
        length = 2 * BLOCK + 37 if i == long_at else LENGTHS[i % len(LENGTHS)]
        reads.append("".join("ACGT"[b] for b in rng.integers(0, 4, length)))
        quals.append("".join(chr(c) for c in rng.integers(0x21, 0x7F, length)))
    return reads, quals


def _text(reads, quals, final_newline=True):
    text = "".join(_record(i, s, q) for i, (s, q) in enumerate(zip(reads, quals)))
    return (text if final_newline else text[:-1]).encode("latin-1")


def _upload_host_parsed(ctx, reads):
    return native.ResidentBatch.upload(ctx, *native.pack_reads(reads))


def _record_number(message):
    return int(re.search(r"\(record (\d+)\)", str(message)).group(1))


# ---- 1. parse parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 600])
def test_device_parse_equals_the_host_parse(ctx, n, tmp_path):
    reads, quals = _reads(n, 100 + n, long_at=1 if n in (65, 600) else None)
    for final_newline in (True, False):
        text = _text(reads, quals, final_newline)
        assert n < 600 or len(text) >= 3 * BLOCK
        path = str(tmp_path / ("t%d.fastq" % final_newline))
        with open(path, "wb") as fh:
            fh.write(text)
        f = native.FastqFile(path)
        assert f.n_reads == n
        batch = native.ResidentBatch.upload_fastq_text(ctx, text)
        assert batch.n_reads == n and not batch.has_qualities
        to, tl, so, sl = batch.text_records()
        want = [f.read_info(r) for r in range(n)]
        assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(to, tl, so, sl)] == want
        parsed = [text[o:o + l].decode("latin-1") for _a, _b, o, l in want]
        assert parsed == reads
        host = _upload_host_parsed(ctx, parsed)
        bases, offsets = batch.download()
        want_bases, want_offsets = host.download()
        assert offsets.tobytes() == want_offsets.tobytes() and bases.tobytes() == want_bases.tobytes()
        assert batch.n_bases == host.n_bases and batch.devptrs()[1] is None
        batch.destroy(); host.destroy()
    # an empty text is what an empty file is: no reads
    empty = native.ResidentBatch.upload_fastq_text(ctx, b"")
    assert empty.info() == (0, 0)


# ---- 2. the same verdict ---------------------------------------------------------------------------------------------------------------
def _wrapped(t, s, q, p):
    return "@" + t + "\n" + s[:len(s) // 2] + "\n" + s[len(s) // 2:] + "\n+\n" + q + "\n"


FORMS = {
    "wrapped sequence": _wrapped,
    "crlf": lambda t, s, q, p: ("@" + t + "\n" + s + "\n+" + p + "\n" + q + "\n").replace("\n", "\r\n"),
    "blank line between records": lambda t, s, q, p: "\n@" + t + "\n" + s + "\n+" + p + "\n" + q + "\n",
    "trailing blank line": lambda t, s, q, p: "@" + t + "\n" + s + "\n+" + p + "\n" + q + "\n\n",
    "blank inside a sequence": lambda t, s, q, p: "@" + t + "\n" + s[:3] + " " + s[4:] + "\n+" + p + "\n" + q + "\n",
    "byte 0x80 in a title": lambda t, s, q, p: "@a\x80" + t + "\n" + s + "\n+\n" + q + "\n",
    "control byte in a title": lambda t, s, q, p: "@a\x07" + t + "\n" + s + "\n+\n" + q + "\n",
    "quality shorter": lambda t, s, q, p: "@" + t + "\n" + s + "\n+" + p + "\n" + q[:-1] + "\n",
    "quality longer": lambda t, s, q, p: "@" + t + "\n" + s + "\n+" + p + "\n" + q + "I\n",
    "plus line with another title": lambda t, s, q, p: "@" + t + "\n" + s + "\n+other\n" + q + "\n",
    "truncated record": lambda t, s, q, p: "@" + t + "\n" + s + "\n+" + p + "\n",
    "empty sequence": lambda t, s, q, p: "@" + t + "\n\n+" + p + "\n\n",
    "first byte >": lambda t, s, q, p: ">" + t + "\n" + s + "\n+" + p + "\n" + q + "\n",
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_non_plain_text_gets_the_verdict_of_the_host_parser(ctx, form, tmp_path):
    n = 9
    reads, quals = _reads(n, 7)
    reads = [r if len(r) > 8 else r + "ACGTACGT" for r in reads]
    quals = [q if len(q) > 8 else q + "IIIIIIII" for q in quals]
    for at in (0, n // 2, n - 1):
        parts = []
        for i in range(n):
            rec = _record(i, reads[i], quals[i])
            if i == at:
                title, plus = rec.split("\n")[0][1:], rec.split("\n")[2][1:]
                rec = FORMS[form](title, reads[i], quals[i], plus)
            parts.append(rec)
        text = "".join(parts).encode("latin-1")
        path = str(tmp_path / ("bad%d.fastq" % at))
        with open(path, "wb") as fh:
            fh.write(text)
        with pytest.raises(native.FastqFile.Unsupported) as host:
            native.FastqFile(path)
        with pytest.raises(native.ResidentBatch.Unsupported, match="error -2") as dev:
            native.ResidentBatch.upload_fastq_text(ctx, text)
        # (a blank line behind a record is the start of the next one)
        assert _record_number(dev.value) == _record_number(host.value) == at + (2 if form == "trailing blank line" else 1), (form, at)
        # nothing is left behind and the context goes on: a plain upload
        good = native.ResidentBatch.upload_fastq_text(ctx, _text(reads, quals))
        assert good.n_reads == n and good.download()[0].tobytes() == "".join(reads).encode()
        good.destroy()


def test_refusals_of_the_text_calls(ctx):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    reads = synth.synth_batch(20, 3, pbc.layouts, 1, 0, error_rate=0.05)
    plain = _upload_host_parsed(ctx, reads)
    ctx.scan_resident(kit, plain, fetch=False)
    with pytest.raises(RuntimeError, match="error -1.*no text plane"):
        ctx.demux_text(kit, plain)
    with pytest.raises(RuntimeError, match="error -1.*no text plane"):
        plain.text_records()
    batch = native.ResidentBatch.upload_fastq_text(ctx, _text(reads, ["I" * len(r) for r in reads]))
    with pytest.raises(RuntimeError, match="error -1.*records == NULL"):
        ctx.demux_text(kit, native.ResidentBatch.upload_fastq_text(ctx, _text(reads[:5], ["I" * len(r) for r in reads[:5]])))
    total = native.C.c_uint64()
    rc = ctx.hip.lib.qcat_batch_demux_text(ctx.handle, kit.handle, batch.handle, None, 1, native.C.byref(total))
    assert rc == -1 and b"flags" in ctx.hip.lib.qcat_last_error()
    recs, _counts = ctx.scan_resident(kit, batch)
    out = ctx.demux_text(kit, batch)
    assert len(out.text) > 0 and ctx.hip.lib.qcat_ctx_demux_text_devptr(ctx.handle)
    assert ctx.demux_text(kit, batch, recs).text == out.text                    # records of the caller: the same text


# ---- 3. the scan is unchanged ----------------------------------------------------------------------------------------------------------
def _scan_cases():
    pbc = scanner.factory(kit="PBC096")
    yield "single kit", native.NativeKit(pbc.descriptor()), synth.synth_batch(300, 11, pbc.layouts, 1, 0, error_rate=0.08) + ["A", "N" * 200]
    dual = scanner.factory(mode="dual")
    lays = dual.layouts
    yield "dual kit", native.NativeKit(dual.descriptor()), synth.synth_batch(300, 12, lays, 1, 0, error_rate=0.08)
    simple = scanner.factory(mode="simple", kit="standard")
    lays = scanner.factory(kit="PBK004/LWB001").layouts
    yield "simple kit", native.NativeKit(simple.descriptor()), synth.synth_batch(300, 13, lays, 1, 0, error_rate=0.05, insert_len=200)
    mid = scanner.factory(kit=synth.FLAGS["kit"], scan_middle_adapter=True)
    text = synth.flags_fastq(scanner.factory(kit=synth.FLAGS["kit"]).layouts)
    yield "detect-middle kit", native.NativeKit(mid.descriptor()), text.split("\n")[1::4]


@pytest.mark.parametrize("which", range(4))
def test_scan_of_a_text_batch_equals_the_scan_of_the_parsed_reads(ctx, which):
    name, kit, reads = list(_scan_cases())[which]
    assert kit.descriptor.scan_middle == (name == "detect-middle kit")
    rng = np.random.default_rng(which)
    quals = ["".join(chr(c) for c in rng.integers(0x21, 0x7F, len(r))) for r in reads]
    host = _upload_host_parsed(ctx, reads)
    want, want_counts = ctx.scan_resident(kit, host)
    batch = native.ResidentBatch.upload_fastq_text(ctx, _text(reads, quals, final_newline=which % 2 == 0))
    got, got_counts = ctx.scan_resident(kit, batch)
    assert got.tobytes() == want.tobytes() and np.array_equal(got_counts, want_counts), name
    assert (got["barcode_idx"] >= 0).sum() > len(reads) // 3, name
    # the partition of a text batch is the partition of the parsed reads
    part, want_part = ctx.partition(kit, batch, got), ctx.partition(kit, host, want)
    assert np.array_equal(part.bin_first, want_part.bin_first) and np.array_equal(part.source, want_part.source)
    assert part.batch.download()[0].tobytes() == want_part.batch.download()[0].tobytes()


# ---- 4. the reference driver's files ---------------------------------------------------------------------------------------------------
with open(os.path.join(helpers.GOLDEN, "cli_golden.json")) as _fh:
    _RUNS = json.load(_fh)["runs"]
GOLDEN_FLAGS = [r for r in _RUNS if r["file"] == "flags_nbd104_150.fastq" and r["variant"]["tag"] == "dir-auto-middle-filter-trim"][0]
GOLDEN_TRIM = {r["file"]: r for r in _RUNS if r["variant"]["tag"] == "dir-auto-trim"}


def _digests(files):
    return {name: hashlib.sha256(data).hexdigest() for name, data in files.items()}


@pytest.mark.parametrize("name", ["nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq"])
def test_text_of_the_shipped_files_is_the_reference_drivers(name):
    run = GOLDEN_TRIM[name]
    v = run["variant"]
    assert v["trim"] and v["min_len"] == 100 and v["dir"] and run["kit"] == "auto"
    with open(os.path.join(helpers.GOLDEN, "data", name)) as fh:
        text = fh.read()
    got = scanner.factory(kit="auto").demux_fastq_text(text, trim=True, min_read_length=100, qcat_config=config.get_default_config())
    assert _digests(got) == run["files"]


def test_text_under_vote_filter_middle_and_trim_is_the_reference_drivers():
    v = GOLDEN_FLAGS["variant"]
    assert v["trim"] and v["min_len"] == 0 and v["middle"] and v["filter"] and GOLDEN_FLAGS["kit"] == "auto"
    text = synth.flags_fastq(scanner.factory(kit=synth.FLAGS["kit"]).layouts)
    det = scanner.factory(kit="auto", enable_filter_barcodes=True, scan_middle_adapter=True)
    got = det.demux_fastq_text(text, trim=True, min_read_length=0, qcat_config=config.get_default_config())
    assert _digests(got) == GOLDEN_FLAGS["files"]


# ---- 5. text at size, against the oracle -----------------------------------------------------------------------------------------------
def _format(title, seq, qual):
    """a record as the reference writer writes it (qcat/cli.py:327-342, the title split as extract_fastx_comment)"""
    cols = title.rstrip(" \t").replace("\t", " ").split(" ")
    name, comment = cols[0], (" ".join(cols[1:]) if len(cols) > 1 else "")
    return "@" + name + " " + comment + "\n" + seq + "\n+\n" + qual + "\n"


@pytest.fixture(scope="module")
def sized():
    """about 600 PBC096 reads, every ninth cut short, a few cut so that trimming leaves nothing: (scanner, reads, qualities, text)"""
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(603, 20261020, pbc.layouts, 1, 0, error_rate=0.08)
    reads = [r[:60] if i % 50 == 7 else (r[:150] if i % 9 == 4 else r) for i, r in enumerate(reads)]
    rng = np.random.default_rng(5)
    quals = ["".join(chr(c) for c in rng.integers(0x21, 0x7F, len(r))) for r in reads]
    return pbc, reads, quals, _text(reads, quals)


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("min_read_length", [0, 100])
def test_text_at_size_equals_text_formatted_from_the_oracles_records(ctx, sized, trim, min_read_length):
    pbc, reads, quals, text = sized
    cfg = config.qcatConfig()
    desc = pbc.descriptor(trim=trim, min_read_length=min_read_length)
    o = oracle_lib.scan(desc, reads, threads=8)
    want, lengths, skipped, empty = {}, {}, 0, 0
    per_read = {}
    for i, rec in enumerate(o):
        t5, t3 = (int(rec["trim5p"]), int(rec["trim3p"])) if trim else (0, len(reads[i]))
        seq, qual = reads[i][t5:t3], quals[i][t5:t3]
        empty += len(seq) == 0
        if len(seq) < min_read_length:
            skipped += 1
            continue
        called = rec["barcode_idx"] >= 0 and rec["adapter_idx"] >= 0
        barcode = pbc.layouts[int(rec["adapter_idx"])].barcode_set_1[int(rec["barcode_idx"])] if called else None
        name = (barcode.name.replace("/", "_") if barcode else "none") + ".fastq"
        per_read[i] = _format(_title(i), seq, qual).encode("latin-1")
        want[name] = want.get(name, b"") + per_read[i]
        b = desc.slot_ids.index(barcode.id) if barcode else desc.n_partition_bins - 2
        lengths[b] = lengths.get(b, 0) + len(per_read[i])
    # the data does what the test is about (the seed and the cuts were chosen on the CPU with the oracle)
    assert len(want) >= 21 and "none.fastq" in want
    assert skipped >= 1 or not min_read_length
    assert empty >= 1 or not trim
    got = pbc.demux_fastq_text(text, trim=trim, min_read_length=min_read_length, qcat_config=cfg)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    # the arrays of the device call
    kit = native.NativeKit(desc)
    batch = native.ResidentBatch.upload_fastq_text(ctx, text)
    recs, _counts = ctx.scan_resident(kit, batch)
    assert recs.tobytes() == o.tobytes()
    out = ctx.demux_text(kit, batch)
    sizes = np.diff(out.bin_first_bytes.astype(np.int64))
    assert out.bin_first_bytes[0] == 0 and int(out.bin_first_bytes[-1]) == len(out.text) == sum(lengths.values())
    assert {b: int(s) for b, s in enumerate(sizes) if s} == lengths and sizes[-1] == 0
    assert int(out.rec_first[-1]) == len(out.text) and sorted(out.source.tolist()) == list(range(len(reads)))
    for j, r in enumerate(out.source.tolist()):
        assert out.text[int(out.rec_first[j]):int(out.rec_first[j + 1])] == per_read.get(r, b""), (j, r)
    # the same bytes twice, and from a batch destroyed and made again on the same context
    again = ctx.demux_text(kit, batch)
    batch.destroy()
    batch = native.ResidentBatch.upload_fastq_text(ctx, text)
    ctx.scan_resident(kit, batch, fetch=False)
    anew = ctx.demux_text(kit, batch)
    for other in (again, anew):
        assert other.text == out.text and np.array_equal(other.bin_first_bytes, out.bin_first_bytes)
        assert np.array_equal(other.rec_first, out.rec_first) and np.array_equal(other.source, out.source)
    assert pbc.demux_fastq_text(text, trim=trim, min_read_length=min_read_length, qcat_config=cfg) == got


# ---- 6. two names in one bin -----------------------------------------------------------------------------------------------------------
def test_a_bin_with_two_file_names_is_split_record_by_record():
    det = scanner.factory(kit="auto")
    by_kit = {}
    for i, l in enumerate(det.layouts):
        by_kit.setdefault(l.kit, []).append(i)
    reads = []
    for q, kit_name in enumerate(["RAB204/RAB214", "PBC096", "PBC096", "RAB204/RAB214", "PBC096"]):
        idx = by_kit[kit_name]
        reads += [synth.synth_read(64 * q + i, 77, det.layouts, idx[-1], idx[0] if len(idx) > 1 else -1, error_rate=0.05,
                                   insert_len=200, force_barcode=(i + q) % 6) for i in range(64 if q < 4 else 40)]
    rng = np.random.default_rng(9)
    quals = ["".join(chr(c) for c in rng.integers(0x21, 0x7F, len(r))) for r in reads]
    cfg = config.get_default_config()
    got = det.demux_fastq_text(_text(reads, quals), batch_size=64, trim=True, min_read_length=100, qcat_config=cfg)
    # the Python path's loop over slices of 64, written as the reference writer writes
    want = {}
    for r0 in range(0, len(reads), 64):
        part = reads[r0:r0 + 64]
        for i, res in enumerate(det.detect_barcode_batch(part, [None] * len(part), cfg)):
            read, qual = reads[r0 + i], quals[r0 + i]
            seq, qual = read[res["trim5p"]:res["trim3p"]], qual[res["trim5p"]:res["trim3p"]]
            if len(seq) < 100:
                continue
            name = (res["barcode"].name.replace("/", "_") if res["barcode"] else "none") + ".fastq"
            want.setdefault(name, []).append(_format(_title(r0 + i), seq, qual).encode("latin-1"))
    want = {name: b"".join(parts) for name, parts in want.items()}              # (appended in read order: the order inside every file)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    both = [i for i in range(1, 7) if "BC%02d.fastq" % i in got and "barcode%02d.fastq" % i in got]
    assert len(both) >= 4, sorted(got)                                          # ids that one bin holds under two names

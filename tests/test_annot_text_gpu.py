"""The driver's annotated single stream assembled in device memory (qcat_batch_annot_text, NativeContext.annot_text,
BarcodeScanner.annot_fastx_text): against the reference driver's own out.fastq without -b and without --tsv
(tests/golden/cli_golden.json), against the product's host writer on the same bytes (qcat_fastq_demux with out_fd) for a FASTQ
and a FASTA file, against records formatted here from the oracle's records, with records so short that a chunk of the copy
leaves its LDS table, for a dual, a simple and a detect-middle kit, under a per-batch kit vote with the barcode filter, and the
call's refusals and state."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import helpers
import oracle_lib
import synth
from qcat_amd import cli, config, native, scanner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "qcat_amd", "csrc", "partition_core.h")) as _fh:
    _CORE = _fh.read()
CHUNK = 1
for _name in ("PART_THREADS", "PART_VEC", "PART_VECS_PER_LANE"):
    CHUNK *= int(re.search(r"constexpr uint32_t %s = (\d+);" % _name, _CORE).group(1))
LDS_SEGS = int(re.search(r"constexpr uint32_t PART_LDS_SEGS = (\d+);", _CORE).group(1))
with open(os.path.join(ROOT, "qcat_amd", "csrc", "textstream_core.h")) as _fh:
    SEGS = int(re.search(r"constexpr uint32_t ANNOT_SEGS = (\d+);", _fh.read()).group(1))

# name only, comment, several blanks (tabs), two blanks in a row, a trailing blank, empty -- and a leading blank: an empty name
TITLES = ("r{i}", "r{i} ch=3", "r{i}\tch=3\tx=y", "r{i}  two", "r{i} ", "", " lead{i}")


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


def _title(i):
    return TITLES[i % len(TITLES)].format(i=i)


def _quals(reads, seed):
    rng = np.random.default_rng(seed)
    return ["".join(chr(c) for c in rng.integers(0x21, 0x7F, len(r))) for r in reads]


def _text(reads, quals=None, final_newline=True):
    """FASTQ text with `quals`, FASTA text without"""
    if quals is None:
        text = "".join(">" + _title(i) + "\n" + s + "\n" for i, s in enumerate(reads))
    else:
        text = "".join("@" + _title(i) + "\n" + s + "\n+\n" + q + "\n" for i, (s, q) in enumerate(zip(reads, quals)))
    return (text if final_newline else text[:-1]).encode("latin-1")


def _host_writer(ctx, det, text, tmp_path, trim, min_read_length, batch_size=4000, kit_auto=False, filter_barcodes=False):
    """the stream qcat_fastq_demux writes to out_fd for the same bytes (the file loop's kit carries no trim and no minimum
    length: its options do)"""
    path = str(tmp_path / ("in.fasta" if text[:1] == b">" else "in.fastq"))
    with open(path, "wb") as fh:
        fh.write(text)
    simple = det._native_mode == "simple"
    layouts = [det._simple_layout] if simple else det.layouts
    kit = det._native_kit(layouts, config.qcatConfig(), native.ENDS_BOTH)
    with open(str(tmp_path / "out.fx"), "w+b") as out:
        native.FastqFile(path).demux(ctx, kit, layouts, det._native_mode == "dual", batch_size=batch_size, kit_auto=kit_auto, trim=trim,
                                     min_read_length=min_read_length, out_fd=out.fileno(), filter_barcodes=filter_barcodes)
        out.seek(0)
        return out.read()


def _records(text, rec_first):
    return [text[int(a):int(b)] for a, b in zip(rec_first[:-1], rec_first[1:])]


def _format(title, seq, qual, barcode_id):
    """a record as the reference writer writes it to the stream (qcat/cli.py:345-358, the title split as extract_fastx_comment)"""
    name, comment = cli.split_header(title.rstrip(" \t"))
    head = name + " " + "{} barcode={}".format(comment or "", barcode_id)
    return ("@" + head + "\n" + seq + "\n+\n" + qual + "\n") if qual is not None else (">" + head + "\n" + seq + "\n")


# ---- 1. the reference's own output -------------------------------------------------------------------------------------------------
with open(os.path.join(helpers.GOLDEN, "cli_golden.json")) as _fh:
    _RUNS = json.load(_fh)["runs"]


@pytest.mark.parametrize("name", ["nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq", "fasta_of_nbd103.fasta"])
def test_stream_of_the_shipped_files_is_the_reference_drivers(name):
    run = [r for r in _RUNS if r["variant"]["tag"] == "stream-kit-trim-minlen1000" and r["file"] == name][0]
    v = run["variant"]
    assert v["trim"] and v["min_len"] == 1000 and not v["dir"] and not v["tsv"] and not v["nobatch"] and v["mode"] == "epi2me"
    with open(os.path.join(helpers.GOLDEN, "data", name.replace("fasta_of_", "").replace(".fasta", ".fastq"))) as fh:
        text = fh.read()
    if name.startswith("fasta_of_"):                                            # as tests/golden/make_cli_golden.py derives it
        lines = text.split("\n")
        text = "".join(">" + lines[i][1:] + "\n" + lines[i + 1] + "\n" for i in range(0, len(lines) - 3, 4))
    got = scanner.factory(kit=run["kit"]).annot_fastx_text(text, trim=True, min_read_length=1000, qcat_config=config.get_default_config())
    assert hashlib.sha256(got).hexdigest() == run["files"]["out.fastq"]
    assert got[:1] == text[:1].encode() and b" barcode=" in got


# ---- 2. the product's host writer, 3. the oracle ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    """about 2000 PBC096 reads with the title forms above, every ninth cut to 150 bases, a few to 60 (trimming leaves nothing of
    those), every fortieth longer than 1000: (scanner, reads, qualities)"""
    pbc = scanner.factory(kit="PBC096")
    seed = 20261021
    reads = synth.synth_batch(2003, seed, pbc.layouts, 1, 0, error_rate=0.08)
    reads = [synth.synth_read(i, seed, pbc.layouts, 1, 0, error_rate=0.08, insert_len=1100 + i % 300) if i % 40 == 3 else r for i, r in enumerate(reads)]
    reads = [r[:60] if i % 50 == 7 else (r[:150] if i % 9 == 4 else r) for i, r in enumerate(reads)]
    return pbc, reads, _quals(reads, 5)


@pytest.fixture(scope="module")
def oracle_records(sized):
    """the oracle's records of the sized reads, computed once per (trim, min_read_length) and shared"""
    pbc, reads, _quals_ = sized
    cache = {}

    def get(trim, min_read_length):
        key = (trim, min_read_length)
        if key not in cache:
            desc = pbc.descriptor(trim=trim, min_read_length=min_read_length)
            cache[key] = (desc, oracle_lib.scan(desc, reads, threads=8))
        return cache[key]
    return get


@pytest.mark.parametrize("fasta", [False, True])
@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("min_read_length", [0, 100])
def test_stream_at_size_equals_the_host_writers_and_records_formatted_from_the_oracles(ctx, sized, oracle_records, fasta, trim, min_read_length, tmp_path):
    pbc, reads, quals = sized
    text = _text(reads, None if fasta else quals, final_newline=not (fasta and trim))
    desc, o = oracle_records(trim, min_read_length)
    dicts = pbc._records_to_dicts(o, pbc.layouts)
    want, seen = [], {"called": 0, "none": 0, "dropped": 0, "empty": 0}
    for i, d in enumerate(dicts):
        a, b = (d["trim5p"], d["trim3p"]) if trim else (0, len(reads[i]))
        seq = reads[i][a:b]
        seen["empty"] += len(seq) == 0
        if len(seq) < min_read_length:
            seen["dropped"] += 1
            want.append(b"")
            continue
        seen["called" if d["barcode"] else "none"] += 1
        want.append(_format(_title(i), seq, None if fasta else quals[i][a:b], d["barcode"].id if d["barcode"] else "none").encode("latin-1"))
    # the data does what the test is about
    assert seen["called"] >= 300 and seen["none"] >= 15
    assert seen["dropped"] >= 3 or not min_read_length
    assert seen["empty"] >= 1 or not trim
    assert sum(len(w) for w in want) > 20 * CHUNK
    # 2. the host writer's stream for the same bytes
    got = pbc.annot_fastx_text(text, trim=trim, min_read_length=min_read_length)
    assert got == _host_writer(ctx, pbc, text, tmp_path, trim, min_read_length)
    # 3. the oracle's records, record by record; the stream from the caller's records equals the stream from the scan
    kit = native.NativeKit(desc)
    batch = native.ResidentBatch.upload_text(ctx, text)
    assert batch.is_fasta == fasta
    recs, _counts = ctx.scan_resident(kit, batch)
    assert recs.tobytes() == o.tobytes()
    out = ctx.annot_text(kit, batch, pbc._tsv_names())
    assert out.rec_first[0] == 0 and int(out.rec_first[-1]) == len(out.text)
    for r, (g, w) in enumerate(zip(_records(out.text, out.rec_first), want)):
        assert g == w, r
    assert out.text == b"".join(want) == got
    assert ctx.hip.lib.qcat_ctx_annot_text_devptr(ctx.handle)
    again = ctx.annot_text(kit, batch, pbc._tsv_names())
    mine = ctx.annot_text(kit, batch, pbc._tsv_names(), records=recs)
    for other in (again, mine):
        assert other.text == out.text and np.array_equal(other.rec_first, out.rec_first)
    batch.destroy()


@pytest.mark.parametrize("fasta", [False, True])
def test_stream_of_a_file_equals_the_host_writers(ctx, fasta, tmp_path):
    """kit auto over batches of 64, trimming and a minimum length, with and without the final newline"""
    det = scanner.factory(kit="auto")
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(300, 31, pbc.layouts, 1, 0, error_rate=0.08)
    reads = [r[:150] if i % 9 == 4 else r for i, r in enumerate(reads)]
    cfg = config.get_default_config()
    for final_newline in (True, False):
        text = _text(reads, None if fasta else _quals(reads, 3), final_newline)
        want = _host_writer(ctx, det, text, tmp_path, True, 100, batch_size=64, kit_auto=True)
        got = det.annot_fastx_text(text, batch_size=64, trim=True, min_read_length=100, qcat_config=cfg)
        assert got == want and want.count(b" barcode=") > 200 and want.count(b"barcode=none\n") >= 5


# ---- 4. short records: a chunk of the copy holds more segments than its LDS table ----------------------------------------------------
@pytest.mark.parametrize("fasta", [False, True])
def test_records_so_short_that_the_copy_leaves_its_lds_table(ctx, fasta):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    rng = np.random.default_rng(8)
    n = 2500
    reads = ["".join("ACGT"[b] for b in rng.integers(0, 4, 1 + i % 40)) for i in range(n)]
    quals = None if fasta else _quals(reads, 9)
    recs = np.zeros(n, dtype=native.RESULT_DTYPE)
    for field in ("barcode_idx", "barcode2_idx", "adapter_idx"):
        recs[field] = -1
    called = np.arange(n) % 3 == 0                                              # a third of the reads with an id of the kit
    recs["adapter_idx"][called] = 0
    recs["barcode_idx"][called] = (np.arange(n) % 96)[called]
    recs["score_den"] = 1
    recs["trim3p"] = [len(r) for r in reads]
    ids = [b.id for b in pbc.layouts[0].barcode_set_1]
    want = [_format(_title(i), reads[i], None if fasta else quals[i], ids[int(recs["barcode_idx"][i])] if called[i] else "none").encode("latin-1")
            for i in range(n)]
    assert max(len(w) for w in want) < 300 and sum(len(w) for w in want) > 2 * CHUNK
    assert CHUNK // 300 * SEGS > LDS_SEGS                                       # every whole chunk holds more segments than the table
    batch = native.ResidentBatch.upload_text(ctx, _text(reads, quals))
    out = ctx.annot_text(kit, batch, pbc._tsv_names(), records=recs)
    assert _records(out.text, out.rec_first) == want and out.text == b"".join(want)
    assert ctx.annot_text(kit, batch, pbc._tsv_names(), records=recs).text == out.text
    batch.destroy()


def test_an_empty_text_and_a_text_whose_reads_are_all_dropped(ctx):
    pbc = scanner.factory(kit="PBC096")
    assert pbc.annot_fastx_text(b"") == b""
    reads = synth.synth_batch(20, 3, pbc.layouts, 1, 0, error_rate=0.05)
    assert pbc.annot_fastx_text(_text(reads), min_read_length=100000) == b""


# ---- 5. kits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dual", "simple", "middle"])
def test_dual_simple_and_detect_middle_kits(ctx, mode, tmp_path):
    if mode == "dual":
        det = scanner.factory(mode="dual")
        reads = synth.synth_batch(300, 12, det.layouts, 1, 0, error_rate=0.08)
    elif mode == "simple":
        det = scanner.factory(mode="simple", kit="standard")
        reads = synth.synth_batch(300, 13, scanner.factory(kit="PBK004/LWB001").layouts, 1, 0, error_rate=0.05, insert_len=200)
    else:
        det = scanner.factory(kit=synth.FLAGS["kit"], scan_middle_adapter=True)
        reads = synth.flags_fastq(scanner.factory(kit=synth.FLAGS["kit"]).layouts).split("\n")[1::4]
    for fasta in (False, True):
        text = _text(reads, None if fasta else _quals(reads, 8))
        want = _host_writer(ctx, det, text, tmp_path, True, 100)
        got = det.annot_fastx_text(text, trim=True, min_read_length=100, qcat_config=config.get_default_config() if mode == "middle" else None)
        assert got == want
        ids = re.findall(rb" barcode=(\S+)\n", want)
        called = [i for i in ids if i != b"none"]
        assert len(ids) == want.count(b"\n") // (2 if fasta else 4) and len(called) < len(ids)
        assert len(called) > (10 if mode == "middle" else len(reads) // 4)
        if mode == "dual":
            assert all(re.match(rb"^\d+/\d+$", i) for i in called)
        else:
            assert all(re.match(rb"^\d+$", i) for i in called)


def test_two_kits_in_one_run_under_the_vote_with_the_barcode_filter(ctx, tmp_path):
    det = scanner.factory(kit="auto", enable_filter_barcodes=True)
    by_kit = {}
    for i, l in enumerate(det.layouts):
        by_kit.setdefault(l.kit, []).append(i)
    reads = []
    for q, kit_name in enumerate(["RAB204/RAB214", "PBC096", "PBC096", "RAB204/RAB214", "PBC096"]):
        idx = by_kit[kit_name]
        reads += [synth.synth_read(64 * q + i, 77, det.layouts, idx[-1], idx[0] if len(idx) > 1 else -1, error_rate=0.05,
                                   insert_len=200, force_barcode=(i + q) % 6) for i in range(64 if q < 4 else 40)]
    quals = _quals(reads, 9)
    cfg = config.get_default_config()
    got = det.annot_fastx_text(_text(reads, quals), batch_size=64, trim=True, min_read_length=100, qcat_config=cfg)
    # the Python path's loop over slices of 64, written as the reference writer writes
    want = []
    for r0 in range(0, len(reads), 64):
        part = reads[r0:r0 + 64]
        for i, res in enumerate(det.detect_barcode_batch(part, [None] * len(part), cfg)):
            a, b = res["trim5p"], res["trim3p"]
            if len(reads[r0 + i][a:b]) < 100:
                continue
            want.append(_format(_title(r0 + i), reads[r0 + i][a:b], quals[r0 + i][a:b], res["barcode"].id if res["barcode"] else "none").encode("latin-1"))
    assert got == b"".join(want) and len(want) > 200
    assert got == _host_writer(ctx, det, _text(reads, quals), tmp_path, True, 100, batch_size=64, kit_auto=True, filter_barcodes=True)


# ---- 6. refusals and state ---------------------------------------------------------------------------------------------------------
def _call(ctx, kit, batch, records, names, flags=0):
    total = native.C.c_uint64()
    rc = ctx.hip.lib.qcat_batch_annot_text(ctx.handle, kit.handle, batch.handle, records.ctypes.data if records is not None else None,
                                           native.C.byref(names) if names is not None else None, flags, native.C.byref(total))
    return rc, ctx.hip.lib.qcat_last_error() or b""


def test_refusals_and_state(ctx):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    names = pbc._tsv_names()
    reads = synth.synth_batch(40, 3, pbc.layouts, 1, 0, error_rate=0.05)
    quals = ["I" * len(r) for r in reads]
    fresh = native.NativeContext(0)
    with pytest.raises(RuntimeError, match="error -1.*no annotated text"):
        fresh.hip.check(fresh.hip.lib.qcat_ctx_fetch_annot_text(fresh.handle, None, 0, None))
    assert not fresh.hip.lib.qcat_ctx_annot_text_devptr(fresh.handle)
    plain = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    ctx.scan_resident(kit, plain, fetch=False)
    with pytest.raises(RuntimeError, match="error -1.*no text plane"):
        ctx.annot_text(kit, plain, names)
    batch = native.ResidentBatch.upload_text(ctx, _text(reads, quals))
    recs, _counts = ctx.scan_resident(kit, batch)
    good = ctx.annot_text(kit, batch, names)
    assert good.text.count(b" barcode=") == len(reads)
    rc, err = _call(ctx, kit, batch, None, names.struct, flags=1)
    assert rc == -1 and b"flags" in err
    rc, err = _call(ctx, kit, batch, None, None)
    assert rc == -1 and b"name tables" in err
    no_ids = native.TsvNamesStruct(kit_name=names.struct.kit_name, bc_id=None, bc2_id=None)
    rc, err = _call(ctx, kit, batch, None, no_ids)
    assert rc == -1 and b"name tables" in err
    other = native.ResidentBatch.upload_text(ctx, _text(reads[:5], quals[:5]))
    with pytest.raises(RuntimeError, match="error -1.*records == NULL"):
        ctx.annot_text(kit, other, names)
    other.destroy()
    # every refusal leaves the latest stream fetchable and the context usable
    buf = np.empty(len(good.text), dtype=np.uint8)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_annot_text(ctx.handle, buf.ctypes.data, len(buf), None))
    assert buf.tobytes() == good.text
    with pytest.raises(RuntimeError, match="error -1.*shorter than the text"):
        ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_annot_text(ctx.handle, buf.ctypes.data, len(buf) - 1, None))
    assert ctx.annot_text(kit, batch, names, records=recs).text == good.text
    # a record that indexes outside the name tables counts as "not called", as in the TSV rows
    loose = recs.copy()
    at = int(np.flatnonzero(loose["barcode_idx"] >= 0)[0])
    loose["barcode_idx"][at] = 4000
    lines = ctx.annot_text(kit, batch, names, records=loose).text.split(b"\n")
    assert lines[4 * at].endswith(b" barcode=none") and lines[4 * at + 1] == reads[at].encode()
    # the demultiplexed text, the TSV text and the stream of one context coexist
    ctx.scan_resident(kit, batch, fetch=False)
    first = ctx.annot_text(kit, batch, names)
    files = ctx.demux_text(kit, batch)
    rows = ctx.tsv_text(kit, batch, names)
    second = ctx.annot_text(kit, batch, names)
    assert first.text == second.text == good.text and np.array_equal(first.rec_first, second.rec_first)
    for fetch, want in ((ctx.hip.lib.qcat_ctx_fetch_annot_text, first.text), (ctx.hip.lib.qcat_ctx_fetch_tsv_text, rows.text)):
        buf = np.empty(len(want), dtype=np.uint8)
        ctx.hip.check(fetch(ctx.handle, buf.ctypes.data, len(buf), None))
        assert buf.tobytes() == want and len(want) > 0
    fbuf = np.empty(len(files.text), dtype=np.uint8)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_demux_text(ctx.handle, fbuf.ctypes.data, len(fbuf), None, 0, None, None))
    assert fbuf.tobytes() == bytes(files.text) and len(fbuf) > 0
    # another kit's names on the same context: the tag plane follows
    dual = scanner.factory(mode="dual")
    dkit = native.NativeKit(dual.descriptor())
    ctx.scan_resident(dkit, batch, fetch=False)
    assert ctx.annot_text(dkit, batch, dual._tsv_names()).text.count(b" barcode=") == len(reads)
    ctx.scan_resident(kit, batch, fetch=False)
    assert ctx.annot_text(kit, batch, names).text == good.text
    batch.destroy(); plain.destroy()

"""The driver's TSV table formatted in device memory (qcat_batch_tsv_text, NativeContext.tsv_text, BarcodeScanner.tsv_fastq_text,
demux_fastq_text(tsv=True)): against the reference driver's own stdout under --tsv (tests/golden/cli_golden.json), against the
product's host writer on the same bytes (qcat_fastq_demux with a TSV descriptor), against rows formatted here from the oracle's
records with cli.tsv_row, at the writer's tile edges, for a dual and a simple kit, under a per-batch kit vote, and the call's
refusals and state."""
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
with open(os.path.join(ROOT, "qcat_amd", "csrc", "tsvtext_core.h")) as _fh:
    TILE = int(re.search(r"constexpr uint32_t TSV_TILE = (\d+);", _fh.read()).group(1))

HEADER = b"name\tlength\tbarcode\tscore\tkit\tadapter_end\tcomment\n"
# name only, comment, several blanks (tabs), two blanks in a row, a trailing blank, empty -- and a leading blank: an empty name
TITLES = ("r{i}", "r{i} ch=3", "r{i}\tch=3\tx=y", "r{i}  two", "r{i} ", "", " lead{i}")


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


def _title(i):
    return TITLES[i % len(TITLES)].format(i=i)


def _text(reads, quals, titles=None, final_newline=True):
    text = "".join("@" + (titles[i] if titles else _title(i)) + "\n" + s + "\n+\n" + q + "\n" for i, (s, q) in enumerate(zip(reads, quals)))
    return (text if final_newline else text[:-1]).encode("latin-1")


def _quals(reads, seed):
    rng = np.random.default_rng(seed)
    return ["".join(chr(c) for c in rng.integers(0x21, 0x7F, len(r))) for r in reads]


def _host_writer(ctx, det, text, tmp_path, trim, min_read_length, batch_size=4000, kit_auto=False):
    """the rows qcat_fastq_demux writes to a TSV descriptor for the same bytes (the file loop's kit carries no trim and no
    minimum length: its options do)"""
    path = str(tmp_path / "in.fastq")
    with open(path, "wb") as fh:
        fh.write(text)
    simple = det._native_mode == "simple"
    layouts = [det._simple_layout] if simple else det.layouts
    kit = det._native_kit(layouts, config.qcatConfig(), native.ENDS_BOTH)
    with open(str(tmp_path / "out.tsv"), "w+b") as out:
        native.FastqFile(path).demux(ctx, kit, layouts, det._native_mode == "dual", batch_size=batch_size, kit_auto=kit_auto, trim=trim,
                                     min_read_length=min_read_length, tsv_fd=out.fileno())
        out.seek(0)
        return out.read()


def _rows(text, row_first):
    return [text[int(a):int(b)] for a, b in zip(row_first[:-1], row_first[1:])]


# ---- 1. the reference's own output -------------------------------------------------------------------------------------------------
with open(os.path.join(helpers.GOLDEN, "cli_golden.json")) as _fh:
    _RUNS = json.load(_fh)["runs"]


def _run(tag, name):
    return [r for r in _RUNS if r["variant"]["tag"] == tag and r["file"] == name][0]


@pytest.mark.parametrize("tag", ["tsv-auto-batch", "tsv-dual"])
@pytest.mark.parametrize("name", ["nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq"])
def test_table_of_the_shipped_files_is_the_reference_drivers_stdout(tag, name):
    run = _run(tag, name)
    v = run["variant"]
    assert v["tsv"] and not v["trim"] and v["min_len"] == 100 and not v["nobatch"] and run["kit"] == "auto"
    with open(os.path.join(helpers.GOLDEN, "data", name)) as fh:
        text = fh.read()
    det = scanner.factory(kit="auto") if tag == "tsv-auto-batch" else scanner.factory(mode="dual")
    assert v["mode"] == ("dual" if tag == "tsv-dual" else "epi2me")
    got = det.tsv_fastq_text(text, trim=False, min_read_length=100)
    assert got == run["stdout"].encode("latin-1")
    assert got.startswith(HEADER) and got.count(b"\n") >= 5


@pytest.mark.parametrize("tag", ["tsv-kit-middle", "tsv-auto-filter-trim"])
def test_table_under_detect_middle_and_under_vote_filter_and_trim_is_the_reference_drivers(tag):
    run = _run(tag, "flags_nbd104_150.fastq")
    v = run["variant"]
    text = synth.flags_fastq(scanner.factory(kit=synth.FLAGS["kit"]).layouts)
    if tag == "tsv-kit-middle":
        assert v["middle"] and not v["filter"] and not v["trim"] and v["min_len"] == 100 and run["kit"] == synth.FLAGS["kit"]
        det = scanner.factory(kit=synth.FLAGS["kit"], scan_middle_adapter=True)
    else:
        assert v["filter"] and not v["middle"] and v["trim"] and v["min_len"] == 100 and run["kit"] == "auto"
        det = scanner.factory(kit="auto", enable_filter_barcodes=True)
    got = det.tsv_fastq_text(text, trim=v["trim"], min_read_length=100, qcat_config=config.get_default_config())
    assert got == run["stdout"].encode("latin-1")


# ---- 2. the product's host writer, 3. the oracle ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    """about 600 PBC096 reads with the title forms above, every ninth cut to 150 bases, a few to 60 (trimming leaves nothing of
    those), every fortieth longer than 1000: (scanner, reads, text).  Seed and cuts were chosen on the CPU with the oracle."""
    pbc = scanner.factory(kit="PBC096")
    seed = 20261021
    reads = synth.synth_batch(603, seed, pbc.layouts, 1, 0, error_rate=0.08)
    reads = [synth.synth_read(i, seed, pbc.layouts, 1, 0, error_rate=0.08, insert_len=1100 + i) if i % 40 == 3 else r for i, r in enumerate(reads)]
    reads = [r[:60] if i % 50 == 7 else (r[:150] if i % 9 == 4 else r) for i, r in enumerate(reads)]
    return pbc, reads, _text(reads, _quals(reads, 5))


def _oracle_rows(det, desc, reads, titles, trim, min_read_length):
    """one row per read (b"" for a dropped one) from the oracle's records with cli.tsv_row, and what the data holds"""
    o = oracle_lib.scan(desc, reads, threads=8)
    dicts = det._records_to_dicts(o, det.layouts)
    rows, seen = [], {"called": 0, "none": 0, "dropped": 0, "empty": 0, "digits": set(), "scores": set()}
    for i, d in enumerate(dicts):
        seq = reads[i][d["trim5p"]:d["trim3p"]] if trim else reads[i]
        seen["empty"] += len(seq) == 0
        if len(seq) < min_read_length:
            seen["dropped"] += 1
            rows.append(b"")
            continue
        name, comment = cli.split_header(titles[i].rstrip(" \t"))
        rows.append((cli.tsv_row(d, comment, name, seq) + "\n").encode("latin-1"))
        seen["called" if d["barcode"] else "none"] += 1
        seen["digits"].add(min(len(str(len(seq))), 4))
        if d["barcode"]:
            seen["scores"].add(str(d["barcode_score"]))
    return o, rows, seen


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("min_read_length", [0, 100])
def test_table_at_size_equals_the_host_writers_and_rows_formatted_from_the_oracles_records(ctx, sized, trim, min_read_length, tmp_path):
    pbc, reads, text = sized
    titles = [_title(i) for i in range(len(reads))]
    desc = pbc.descriptor(trim=trim, min_read_length=min_read_length)
    o, rows, seen = _oracle_rows(pbc, desc, reads, titles, trim, min_read_length)
    # the data does what the test is about
    assert seen["called"] >= 100 and seen["none"] >= 5
    assert seen["dropped"] >= 1 or not min_read_length
    assert seen["empty"] >= 1 or not trim
    assert seen["digits"] == {3, 4} | ({2} if not min_read_length else set()) | ({1} if trim and not min_read_length else set())
    assert len(seen["scores"]) >= 10 and any(s.endswith(".0") for s in seen["scores"]) and max(len(s) for s in seen["scores"]) >= 17
    # 2. the host writer's rows for the same bytes
    got = pbc.tsv_fastq_text(text, trim=trim, min_read_length=min_read_length)
    assert got.startswith(HEADER)
    assert got[len(HEADER):] == _host_writer(ctx, pbc, text, tmp_path, trim, min_read_length)
    # 3. the oracle's records, row by row
    kit = native.NativeKit(desc)
    batch = native.ResidentBatch.upload_fastq_text(ctx, text)
    recs, _counts = ctx.scan_resident(kit, batch)
    assert recs.tobytes() == o.tobytes()
    out = ctx.tsv_text(kit, batch, pbc._tsv_names())
    assert out.row_first[0] == 0 and int(out.row_first[-1]) == len(out.text)
    for r, (g, w) in enumerate(zip(_rows(out.text, out.row_first), rows)):
        assert g == w, r
    assert out.text == b"".join(rows) == got[len(HEADER):]
    assert ctx.hip.lib.qcat_ctx_tsv_text_devptr(ctx.handle)
    # the same bytes twice, from the caller's records, and from a batch destroyed and made again
    again = ctx.tsv_text(kit, batch, pbc._tsv_names())
    mine = ctx.tsv_text(kit, batch, pbc._tsv_names(), records=recs)
    batch.destroy()
    batch = native.ResidentBatch.upload_fastq_text(ctx, text)
    ctx.scan_resident(kit, batch, fetch=False)
    anew = ctx.tsv_text(kit, batch, pbc._tsv_names())
    for other in (again, mine, anew):
        assert other.text == out.text and np.array_equal(other.row_first, out.row_first)
    batch.destroy()


# ---- 4. shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_sizes_around_a_wave_with_and_without_a_final_newline(ctx, n, tmp_path):
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(n, 300 + n, pbc.layouts, 1, 0, error_rate=0.05, insert_len=150)
    quals = _quals(reads, n)
    want = _host_writer(ctx, pbc, _text(reads, quals), tmp_path, False, 0)
    assert want.count(b"\n") == n
    for final_newline in (True, False):
        assert pbc.tsv_fastq_text(_text(reads, quals, final_newline=final_newline)) == HEADER + want


def test_an_empty_text_gives_no_rows():
    assert scanner.factory(kit="PBC096").tsv_fastq_text(b"") == HEADER


def _nocall_rows(titles, reads):
    rows = []
    for t, r in zip(titles, reads):
        name, comment = cli.split_header(t)
        rows.append("{}\t{}\tnone\t-1\tnone\t-1\t{}\n".format(name, len(r), comment).encode("latin-1"))
    return rows


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("by_comment", [False, True])
def test_a_row_that_ends_around_the_writers_tile_edge(ctx, delta, by_comment):
    """records without a call have rows of known length: the fourth row ends one byte before, at, and one byte behind the first
    tile edge, stretched by its name or by its comment; rows of ordinary size lie around it"""
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    reads = ["ACGT" * (5 + i) for i in range(9)]
    titles = [_title(i).replace("\t", " ").rstrip(" ") for i in range(9)]
    titles[3] = "n c"
    front = sum(len(r) for r in _nocall_rows(titles[:4], reads[:4]))
    pad = "x" * (TILE + delta - front)
    titles[3] = ("n c" + pad) if by_comment else ("n" + pad + " c")
    rows = _nocall_rows(titles, reads)
    assert sum(len(r) for r in rows[:4]) == TILE + delta
    batch = native.ResidentBatch.upload_fastq_text(ctx, _text(reads, ["I" * len(r) for r in reads], titles=titles))
    recs = np.zeros(len(reads), dtype=native.RESULT_DTYPE)
    for field in ("barcode_idx", "barcode2_idx", "adapter_idx"):
        recs[field] = -1
    recs["score_den"] = 1
    out = ctx.tsv_text(kit, batch, pbc._tsv_names(), records=recs)
    assert _rows(out.text, out.row_first) == rows and out.text == b"".join(rows)
    batch.destroy()


@pytest.mark.parametrize("by_comment", [False, True])
def test_a_title_longer_than_two_tiles(ctx, by_comment, tmp_path):
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(70, 41, pbc.layouts, 1, 0, error_rate=0.05, insert_len=150)
    titles = [_title(i) for i in range(len(reads))]
    big = "".join("abcdefghij"[(7 * i) % 10] for i in range(2 * TILE + 1234))
    titles[33] = ("name " + big) if by_comment else (big + " comment")
    text = _text(reads, _quals(reads, 3), titles=titles)
    want = _host_writer(ctx, pbc, text, tmp_path, False, 0)
    got = pbc.tsv_fastq_text(text)
    assert got == HEADER + want and len(want) > 2 * TILE and want.count(big.encode()) == 1


# ---- 5. dual kit and simple kit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dual", "simple"])
def test_dual_and_simple_kits(ctx, mode, tmp_path):
    if mode == "dual":
        det = scanner.factory(mode="dual")
        reads = synth.synth_batch(300, 12, det.layouts, 1, 0, error_rate=0.08)
        layouts = det.layouts
    else:
        det = scanner.factory(mode="simple", kit="standard")
        reads = synth.synth_batch(300, 13, scanner.factory(kit="PBK004/LWB001").layouts, 1, 0, error_rate=0.05, insert_len=200)
        layouts = [det._simple_layout]
    text = _text(reads, _quals(reads, 8))
    want = _host_writer(ctx, det, text, tmp_path, True, 100)
    got = det.tsv_fastq_text(text, trim=True, min_read_length=100)
    assert got == HEADER + want
    cols = [row.split(b"\t") for row in want.splitlines()]
    called = [c for c in cols if c[2] != b"none"]
    assert len(called) > len(reads) // 3 and len(called) < len(cols)
    if mode == "dual":
        assert all(re.match(rb"^\d+/\d+$", c[2]) for c in called)
    else:
        assert all(c[4] == b"None" for c in called)                             # the simple kit's kit column
    # records passed by the caller give the same bytes as records=None
    kit = det._native_kit(layouts, config.qcatConfig(), native.ENDS_BOTH, min_read_length=100, trim=True)
    batch = native.ResidentBatch.upload_fastq_text(ctx, text)
    recs, _counts = ctx.scan_resident(kit, batch)
    out = ctx.tsv_text(kit, batch, det._tsv_names())
    mine = ctx.tsv_text(kit, batch, det._tsv_names(), records=recs)
    assert out.text == want == mine.text and np.array_equal(out.row_first, mine.row_first)
    batch.destroy()


# ---- 6. two kits in one run under the vote -------------------------------------------------------------------------------------------
def test_two_kits_in_one_run_under_the_vote():
    det = scanner.factory(kit="auto")
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
    files, table = det.demux_fastq_text(_text(reads, quals), batch_size=64, trim=True, min_read_length=100, qcat_config=cfg, tsv=True)
    # the Python path's loop over slices of 64 with cli.tsv_row
    want = [HEADER]
    for r0 in range(0, len(reads), 64):
        part = reads[r0:r0 + 64]
        for i, res in enumerate(det.detect_barcode_batch(part, [None] * len(part), cfg)):
            seq = reads[r0 + i][res["trim5p"]:res["trim3p"]]
            if len(seq) < 100:
                continue
            name, comment = cli.split_header(_title(r0 + i).rstrip(" \t"))
            want.append((cli.tsv_row(res, comment, name, seq) + "\n").encode("latin-1"))
    assert table == b"".join(want)
    kits = set(row.split(b"\t")[4] for row in table.splitlines()[1:])
    assert {b"RAB204/RAB214", b"PBC096"} <= kits
    assert files == det.demux_fastq_text(_text(reads, quals), batch_size=64, trim=True, min_read_length=100, qcat_config=cfg)
    assert table == det.tsv_fastq_text(_text(reads, quals), batch_size=64, trim=True, min_read_length=100, qcat_config=cfg)


# ---- 7. refusals and state ---------------------------------------------------------------------------------------------------------
def _call(ctx, kit, batch, records, names, flags=0):
    total = native.C.c_uint64()
    rc = ctx.hip.lib.qcat_batch_tsv_text(ctx.handle, kit.handle, batch.handle, records.ctypes.data if records is not None else None,
                                         native.C.byref(names) if names is not None else None, flags, native.C.byref(total))
    return rc, ctx.hip.lib.qcat_last_error() or b""


def test_refusals_and_state(ctx):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor())
    names = pbc._tsv_names()
    reads = synth.synth_batch(40, 3, pbc.layouts, 1, 0, error_rate=0.05)
    text = _text(reads, ["I" * len(r) for r in reads])
    plain = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    ctx.scan_resident(kit, plain, fetch=False)
    with pytest.raises(RuntimeError, match="error -1.*no text plane"):
        ctx.tsv_text(kit, plain, names)
    batch = native.ResidentBatch.upload_fastq_text(ctx, text)
    recs, _counts = ctx.scan_resident(kit, batch)
    rc, err = _call(ctx, kit, batch, None, names.struct, flags=1)
    assert rc == -1 and b"flags" in err
    rc, err = _call(ctx, kit, batch, None, None)
    assert rc == -1 and b"name tables" in err
    no_ids = native.TsvNamesStruct(kit_name=names.struct.kit_name, bc_id=None, bc2_id=None)
    rc, err = _call(ctx, kit, batch, None, no_ids)
    assert rc == -1 and b"name tables" in err
    other = native.ResidentBatch.upload_fastq_text(ctx, _text(reads[:5], ["I" * len(r) for r in reads[:5]]))
    with pytest.raises(RuntimeError, match="error -1.*records == NULL"):
        ctx.tsv_text(kit, other, names)
    other.destroy()
    # a called record outside the score table: refused by the device's flag, and a good call succeeds afterwards
    assert (recs["barcode_idx"] >= 0).sum() >= 10
    good = ctx.tsv_text(kit, batch, names, records=recs)
    for field, value in (("score_den", 41), ("raw_score", 4000), ("raw_score", -1)):
        bad = recs.copy()
        at = int(np.flatnonzero((bad["barcode_idx"] >= 0) & (bad["adapter_idx"] >= 0))[3])
        bad[field][at] = value
        with pytest.raises(RuntimeError, match="error -1.*score table"):
            ctx.tsv_text(kit, batch, names, records=bad)
        with pytest.raises(RuntimeError, match="error -1.*no TSV text"):
            ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_tsv_text(ctx.handle, None, 0, None))
        assert ctx.tsv_text(kit, batch, names, records=recs).text == good.text
    # a record without a call may hold any score: it is not looked up
    loose = recs.copy()
    at = int(np.flatnonzero(loose["barcode_idx"] < 0)[0]) if (loose["barcode_idx"] < 0).any() else 0
    loose["barcode_idx"][at] = -1
    loose["score_den"][at] = 77
    assert ctx.tsv_text(kit, batch, names, records=loose).text.count(b"\n") == len(reads)
    # tsv_text, demux_text, tsv_text: the same bytes, and both results stay fetchable
    ctx.scan_resident(kit, batch, fetch=False)
    first = ctx.tsv_text(kit, batch, names)
    files = ctx.demux_text(kit, batch)
    second = ctx.tsv_text(kit, batch, names)
    assert first.text == second.text == good.text and np.array_equal(first.row_first, second.row_first)
    buf = np.empty(len(first.text), dtype=np.uint8)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_tsv_text(ctx.handle, buf.ctypes.data, len(buf), None))
    assert buf.tobytes() == first.text
    fbuf = np.empty(len(files.text), dtype=np.uint8)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_demux_text(ctx.handle, fbuf.ctypes.data, len(fbuf), None, 0, None, None))
    assert fbuf.tobytes() == bytes(files.text) and len(fbuf) > 0
    assert ctx.demux_text(kit, batch).text == files.text
    batch.destroy(); plain.destroy()


def test_demux_fastq_text_without_tsv_returns_what_it_did(ctx):
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(120, 21, pbc.layouts, 1, 0, error_rate=0.08)
    text = _text(reads, _quals(reads, 2))
    plain = pbc.demux_fastq_text(text, trim=True, min_read_length=100)
    assert isinstance(plain, dict) and plain and all(isinstance(v, bytes) for v in plain.values())
    files, table = pbc.demux_fastq_text(text, trim=True, min_read_length=100, tsv=True)
    assert files == plain and table == pbc.tsv_fastq_text(text, trim=True, min_read_length=100)
    # the files' records and the table's rows are the same reads
    assert sum(v.count(b"\n") for v in files.values()) == 4 * (table.count(b"\n") - 1)

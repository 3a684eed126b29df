"""The reference driver's per-batch semantics on reads that stay in device memory (qcat_scan_resident_batches,
qcat_ctx_fetch_kit_slots, qcat_filter_barcodes, BarcodeScanner.demux_batches): a kit voted per batch of a resident batch
(qcat/scanner_base.py:662-678, :714-733) and --filter-barcodes per batch (:690-712, :730-731) as device code, against the
host-buffer kit-auto calls, the oracle, a Python restatement of get_valid / filter_barcodes, the Python path's
detect_barcode_batch and the golden digests of the reference driver's own per-barcode files."""
import hashlib
import json
import os

import numpy as np
import pytest

import custom_kits
import helpers
import oracle_lib
import synth
from qcat_amd import config, native, scanner

pytestmark = pytest.mark.gpu

EMPTY = dict(barcode_idx=-1, barcode2_idx=-1, adapter_idx=-1, exit_status=1, adapter_end=0, trim5p=0, trim3p=0, raw_score=0, score_den=1)


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


@pytest.fixture(scope="module")
def auto():
    return scanner.factory()                                   # kit auto: the 12 auto-detect templates


def _upload(ctx, reads, quals=None):
    bases, offsets = native.pack_reads(reads)
    return native.ResidentBatch.upload(ctx, bases, offsets, None if quals is None else native.pack_qualities(quals, offsets))


def _mixed_batch(det, majority, n, seed):
    """reads of three kits, `majority` most frequent, in random order (tests/test_batch_auto_gpu.py)"""
    by_kit = {}
    for i, l in enumerate(det.layouts):
        by_kit.setdefault(l.kit, []).append(i)
    reads = []
    for k, frac in zip([majority] + [k for k in by_kit if k != majority][:2], [0.6, 0.25, 0.15]):
        idx = by_kit[k]
        reads += synth.synth_batch(int(n * frac), seed + len(reads), det.layouts, idx[-1], idx[0] if len(idx) > 1 else -1, error_rate=0.08)
    order = np.random.default_rng(seed).permutation(len(reads))
    return [reads[i] for i in order]


# ---- 1. the vote ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voted(auto):
    """two full batches of 1500 reads with different majority kits and a short third with the degenerate reads in it"""
    reads = _mixed_batch(auto, "PBC096", 1500, 31)[:1500] + _mixed_batch(auto, "RBK004", 1500, 32)[:1500]
    reads += _mixed_batch(auto, "NBD104/NBD114", 600, 33)[:597] + ["", "A", "N" * 200]
    assert len(reads) == 3600
    return reads


def _host_auto(ctx, kit, reads, per):
    """the host-buffer kit-auto call over the same reads: (records, voted kit slot per batch)"""
    views = native.read_views(reads)
    if views is not None and per < len(reads):
        return ctx.scan_batches_auto_views(kit, views, len(reads), per)
    recs, slots = [], []
    for r0 in range(0, len(reads), per):                                       # (without the C helper: one call per batch)
        one, slot = ctx.scan_auto(kit, *native.pack_reads(reads[r0:r0 + per]))
        recs.append(one); slots.append(slot)
    return np.concatenate(recs), np.array(slots, dtype=np.int32)


def test_resident_vote_equals_the_host_buffer_call_and_the_oracle(ctx, auto, voted, hip_options):
    cfg = config.qcatConfig()
    kit = auto._native_kit(auto.layouts, cfg, native.ENDS_BOTH)
    batch = _upload(ctx, voted)
    recs, counts, slots = ctx.scan_resident_batches(kit, batch, 1500, kit_auto=True)
    want, want_slots = _host_auto(ctx, kit, voted, 1500)
    assert slots.tolist() == want_slots.tolist() and len(slots) == 3 and len(set(slots.tolist())) == 3
    assert recs.tobytes() == want.tobytes()
    assert [kit.descriptor.kit_names[s] for s in slots] == ["PBC096", "RBK004", "NBD104/NBD114"]
    for q, slot in enumerate(slots.tolist()):
        part = voted[q * 1500:(q + 1) * 1500]
        sub = auto.get_adapters(kit.descriptor.kit_names[slot])
        o = oracle_lib.scan(auto.descriptor(layouts=sub, qcat_config=cfg), part, threads=8)
        full_index = np.array([auto.layouts.index(l) for l in sub] + [-1])
        mine = recs[q * 1500:q * 1500 + len(part)]
        assert np.array_equal(full_index[o["adapter_idx"]], mine["adapter_idx"]), q
        for name in ("barcode_idx", "barcode2_idx", "exit_status", "adapter_end", "trim5p", "trim3p", "raw_score", "score_den"):
            assert np.array_equal(o[name], mine[name]), (q, name)
    assert counts.sum() == 2 * len(voted) and np.array_equal(counts, helpers.driver_histogram(kit.descriptor, auto.layouts, recs,
                                                                                              [len(r) for r in voted], 0, False))
    # the adapter passes in chunks of one and of two whole vote batches: the same records, slots and counts
    for chunk in (1500, 3000, 1):
        hip_options(RESIDENT_AUTO_CHUNK=chunk)
        r2, c2, s2 = ctx.scan_resident_batches(kit, batch, 1500, kit_auto=True)
        assert r2.tobytes() == recs.tobytes() and np.array_equal(c2, counts) and s2.tolist() == slots.tolist(), chunk
    hip_options(RESIDENT_AUTO_CHUNK=None)
    # one batch: batch_reads 0 and batch_reads > n
    one, one_slot = ctx.scan_auto(kit, *native.pack_reads(voted))
    for per in (0, 4000):
        r1, c1, s1 = ctx.scan_resident_batches(kit, batch, per, kit_auto=True)
        assert s1.tolist() == [one_slot] and r1.tobytes() == one.tobytes(), per
    # an empty resident batch: no batch, no slot, no record
    empty = _upload(ctx, [])
    r0, c0, s0 = ctx.scan_resident_batches(kit, empty, 1500, kit_auto=True)
    assert len(r0) == 0 and len(s0) == 0 and c0.sum() == 0


# ---- 2. the filter on constructed records ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filter_kits(tmp_path_factory):
    """name -> (scanner, layouts, kit, calls): `calls` are (template, barcode, barcode2) triples with pairwise different keys"""
    out = {}
    det = scanner.factory(kit="PBC096")
    out["PBC096"] = (det, det.layouts, native.NativeKit(det.descriptor()), [(1, i, -1) for i in range(96)])
    folder = str(tmp_path_factory.mktemp("k1024"))
    rng = __import__("random").Random(1024)
    custom_kits.write_kit(folder, "K1024", "K1024", "GGTGCTG" + "N" * 24 + "TTAACCTTTCTGTTGGTGCTGATATTGC", custom_kits.random_barcodes(rng, 1024))
    det = scanner.factory(kit="K1024", kit_folder=folder)
    assert len(det.layouts) == 1 and len(det.layouts[0].barcode_set_1) == 1024
    out["1024 barcodes"] = (det, det.layouts, native.NativeKit(det.descriptor(), jit=False), [(0, 1023 - 7 * i, -1) for i in range(100)])
    det = scanner.factory(mode="dual")
    # pairs that share their first id, and one pair with the ids the other way round
    out["dual"] = (det, det.layouts, native.NativeKit(det.descriptor()), [(0, 5, i) for i in range(60)] + [(1, i, 5) for i in range(6, 24)])
    det = scanner.factory(mode="simple", kit="standard")
    n_simple = len(det._simple_layout.barcode_set_1)
    out["simple"] = (det, [det._simple_layout], native.NativeKit(det.descriptor()), [(-1, i, -1) for i in range(n_simple)])
    return out


def _records(calls):
    """RESULT_DTYPE records: a (template, barcode, barcode2) call, or None for a record without one"""
    recs = np.zeros(len(calls), dtype=native.RESULT_DTYPE)
    for i, call in enumerate(calls):
        if call is None:
            recs[i] = (-1, -1, 0 if i % 3 == 0 else -1, 1002 if i % 2 else 1, i % 50, i % 90, 400 + i % 90, 0, 1)
        else:
            recs[i] = (call[1], call[2], call[0], 0, 20 + i % 60, i % 90, 400 + i % 90, 50 + i % 40, 99)
    return recs


def _python_filter(det, layouts, recs, batch_reads, simple=False):
    """get_valid(counts, 0.05) + filter_barcodes (qcat/scanner_base.py:690-712) per batch, restated over the dicts of the records;
    returns the filtered records"""
    if simple:                                   # (simple mode: no adapter to look the Barcode up under; the list is the kit's one set)
        ids = [layouts[0].barcode_set_1[int(b)].id if b >= 0 else None for b in recs["barcode_idx"]]
    else:
        ids = [d["barcode"].id if d["barcode"] and d["adapter"] else None for d in det._records_to_dicts(recs, layouts)]
    out = recs.copy()
    per = batch_reads if batch_reads else len(recs)
    for r0 in range(0, len(recs), per):
        counts = {}
        for key in ids[r0:r0 + per]:
            counts["0" if key is None else key] = counts.get("0" if key is None else key, 0) + 1
        top = max(list(counts.values()) + [0])
        valid = [bc for bc, c in counts.items() if c > int(top * 0.05)]
        for r in range(r0, min(len(recs), r0 + per)):
            if ids[r] is not None and ids[r] not in valid:
                for name, v in EMPTY.items():
                    out[name][r] = v
    return out


def _edge_batches(calls, per):
    """one batch of `per` records per (maximum, rival): `maximum` records of one call -- or without a call: `none` is counted
    and can be the maximum --, `rival` of another call, filled up with fewer than `maximum` records of the other of the two
    kinds and with calls seen once"""
    rows = []
    for with_none in (False, True):
        for m in (19, 20, 39, 40, 41):
            for rival in (1, 2, 3):
                row = [None if with_none else calls[0]] * m + [calls[1]] * rival
                fill = per - len(row)
                second = min(m - 1, fill)
                row += [calls[0] if with_none else None] * second + [calls[2 + i] for i in range(fill - second)]
                assert len(row) == per and max(row.count(c) for c in set(row)) == m
                rows.append(row)
    return rows


@pytest.mark.parametrize("name", ["PBC096", "1024 barcodes", "dual", "simple"])
def test_filter_floor_edges_on_the_device(ctx, filter_kits, name, hip_options):
    det, layouts, kit, calls = filter_kits[name]
    per = 44                                     # = 41 + 3: the largest maximum and its largest rival fill a batch
    simple = name == "simple"
    rows = _edge_batches(calls, per)
    rng = np.random.default_rng(7)
    flat = []
    for row in rows:
        assert len(row) == per
        flat += [row[i] for i in rng.permutation(per)]
    recs = _records(flat)
    want = _python_filter(det, layouts, recs, per, simple)
    got = ctx.filter_barcodes(kit, recs, per)
    assert got.tobytes() == want.tobytes()
    changed = got.tobytes() != recs.tobytes()
    survived = ((got["barcode_idx"] >= 0) & (got["barcode_idx"] == recs["barcode_idx"])).sum()
    rewritten = ((recs["barcode_idx"] >= 0) & (got["barcode_idx"] < 0)).sum()
    assert changed and survived > 0 and rewritten > 0, (survived, rewritten)
    # strictly greater survives: a rival of r records stays exactly when r > int(max * 0.05)
    rival = (recs["barcode_idx"] == calls[1][1]) & (recs["adapter_idx"] == calls[1][0]) & (recs["barcode2_idx"] == calls[1][2])
    for q, row in enumerate(rows):
        m = max(row.count(calls[0]), row.count(None))
        r = row.count(calls[1])
        left = (got["barcode_idx"][q * per:(q + 1) * per][rival[q * per:(q + 1) * per]] >= 0).sum()
        assert left == (r if r > int(m * 0.05) else 0), (q, m, r)
    assert ctx.filter_barcodes(kit, recs, per).tobytes() == got.tobytes()                    # run after run: the same bytes
    if name == "dual":
        # the table in rounds: one batch's row per round, then three
        n_bins = kit.descriptor.n_partition_bins - 1
        for budget in (n_bins * 4, 3 * n_bins * 4 + 5, 1):
            hip_options(FILTER_TABLE_BYTES=budget)
            assert ctx.filter_barcodes(kit, recs, per).tobytes() == got.tobytes(), budget


@pytest.mark.parametrize("name", ["PBC096", "1024 barcodes", "dual", "simple"])
@pytest.mark.parametrize("per", [1, 7, 100])
def test_filter_equals_the_python_restatement(ctx, filter_kits, name, per, hip_options):
    det, layouts, kit, calls = filter_kits[name]
    n = 2 * per + 3
    rng = np.random.default_rng(100 * per + len(calls))
    hot = calls[:2]
    flat = []
    for i in range(n):
        u = rng.random()
        flat.append(None if u < 0.12 else (hot[int(rng.integers(2))] if u < 0.8 else calls[int(rng.integers(len(calls)))]))
    recs = _records(flat)
    want = _python_filter(det, layouts, recs, per, name == "simple")
    got = ctx.filter_barcodes(kit, recs, per)
    assert got.tobytes() == want.tobytes()
    if per == 100:                                                              # (7 reads: the floor is 0 and every call stays)
        assert ((recs["barcode_idx"] >= 0) & (got["barcode_idx"] < 0)).any() and (got["barcode_idx"] >= 0).any()
    else:
        assert got.tobytes() == recs.tobytes()
    assert ctx.filter_barcodes(kit, recs, per).tobytes() == got.tobytes()
    if name == "dual":                                                           # three batches in three rounds
        hip_options(FILTER_TABLE_BYTES=(kit.descriptor.n_partition_bins - 1) * 4)
        assert ctx.filter_barcodes(kit, recs, per).tobytes() == got.tobytes()
    # one batch (0, and more than there are records) is one filter over everything
    whole = _python_filter(det, layouts, recs, 0, name == "simple")
    assert ctx.filter_barcodes(kit, recs, 0).tobytes() == whole.tobytes() == ctx.filter_barcodes(kit, recs, n + 5).tobytes()


# ---- 3. filter + vote + middle, pinned by the reference driver -------------------------------------------------------------------------
with open(os.path.join(helpers.GOLDEN, "cli_golden.json")) as _fh:
    _RUNS = json.load(_fh)["runs"]
GOLDEN_FLAGS = [r for r in _RUNS if r["file"] == "flags_nbd104_150.fastq" and r["variant"]["tag"] == "dir-auto-middle-filter-trim"][0]
GOLDEN_TRIM = {r["file"]: r for r in _RUNS if r["variant"]["tag"] == "dir-auto-trim"}


def _parse_fastq(text):
    lines = text.split("\n")
    titles, reads, quals = [], [], []
    for i in range(0, len(lines) - 3, 4):
        assert lines[i].startswith("@") and lines[i + 2].startswith("+")
        titles.append(lines[i][1:]); reads.append(lines[i + 1]); quals.append(lines[i + 3])
    return titles, reads, quals


def _latest_records(det, n):
    """the records of the scan behind the scanner's latest demux_batches: they stay with its context"""
    ctx = det._context()
    recs = np.zeros(n, dtype=native.RESULT_DTYPE)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_results(ctx.handle, recs.ctypes.data, n))
    return recs


def _driver_files(det, bins, titles):
    """every bin written as the reference writer writes it (qcat/cli.py:327-342, the title split as extract_fastx_comment):
    file name -> sha256 of its text; the driver writes nothing for skipped reads.  A file is named after the Barcode the
    records call (kits name the same id differently: barcode12 / barcode12a), a bin is labelled with its id."""
    recs = _latest_records(det, len(titles))
    names = {}
    for label, entries in bins.items():
        if label in ("none", "skipped"):
            continue
        r = recs[entries[0][0]]
        barcode = det.layouts[int(r["adapter_idx"])].barcode_set_1[int(r["barcode_idx"])]
        assert barcode.id == label
        names[label] = (barcode.name or "").replace("/", "_") if barcode.name else barcode.name
    files = {}
    for label, entries in bins.items():
        if label == "skipped":
            continue
        text = ""
        for i, seq, qual in entries:
            cols = titles[i].replace("\t", " ").split(" ")
            title, comment = cols[0], (" ".join(cols[1:]) if len(cols) > 1 else "")
            text += "@" + title + " " + comment + "\n" + seq + "\n+\n" + qual + "\n"
        files[("none" if label == "none" else names[label]) + ".fastq"] = hashlib.sha256(text.encode()).hexdigest()
    return files


def _python_bins(det, reads, quals, batch_size, cfg, trim, min_read_length):
    """the driver's loop on the Python path: detect_barcode_batch over slices, trimmed and binned here"""
    want = {}
    for r0 in range(0, len(reads), batch_size):
        part = reads[r0:r0 + batch_size]
        for i, res in enumerate(det.detect_barcode_batch(part, [None] * len(part), cfg)):
            read, qual = reads[r0 + i], quals[r0 + i]
            t5, t3 = (res["trim5p"], res["trim3p"]) if trim else (0, len(read))
            key = "skipped" if len(read[t5:t3]) < min_read_length else (res["barcode"].id if res["barcode"] else "none")
            want.setdefault(key, []).append((r0 + i, read[t5:t3], qual[t5:t3]))
    return want


def test_vote_filter_and_middle_give_the_reference_drivers_files():
    v = GOLDEN_FLAGS["variant"]
    assert v["trim"] and v["min_len"] == 0 and v["middle"] and v["filter"] and GOLDEN_FLAGS["kit"] == "auto"
    titles, reads, quals = _parse_fastq(synth.flags_fastq(scanner.factory(kit=synth.FLAGS["kit"]).layouts))
    assert len(reads) == 150
    det = scanner.factory(kit="auto", enable_filter_barcodes=True, scan_middle_adapter=True)
    cfg = config.get_default_config()
    got = det.demux_batches(reads, trim=True, min_read_length=0, qcat_config=cfg, read_qualities=quals)
    assert _driver_files(det, got, titles) == GOLDEN_FLAGS["files"]
    # the filter and the interior scan did something on this file: without either, other files
    plain = scanner.factory(kit="auto").demux_batches(reads, trim=True, min_read_length=0, qcat_config=cfg, read_qualities=quals)
    assert len(plain) > len(got)
    # batches of 40: each votes and is filtered on its own -- the Python path over slices of 40
    got40 = det.demux_batches(reads, batch_size=40, trim=True, min_read_length=0, qcat_config=cfg, read_qualities=quals)
    want40 = _python_bins(det, reads, quals, 40, cfg, True, 0)
    assert {k: sorted(e) for k, e in got40.items()} == {k: sorted(e) for k, e in want40.items()}
    assert all(e == sorted(e) for e in got40.values())                          # file order inside every bin


# ---- 4. the four shipped FASTQ files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq"])
def test_demux_batches_gives_the_reference_drivers_trimmed_fastq_files(name):
    run = GOLDEN_TRIM[name]
    v = run["variant"]
    assert v["trim"] and v["min_len"] == 100 and v["dir"] and run["kit"] == "auto"
    with open(os.path.join(helpers.GOLDEN, "data", name)) as fh:
        titles, reads, quals = _parse_fastq(fh.read())
    assert 7 <= len(reads) <= 11
    det = scanner.factory(kit="auto")
    got = det.demux_batches(reads, trim=True, min_read_length=100, qcat_config=config.get_default_config(), read_qualities=quals)
    assert _driver_files(det, got, titles) == run["files"]


# ---- 5. counts and bins ------------------------------------------------------------------------------------------------------------------
def test_counts_and_bins_follow_the_filtered_records(ctx, auto, voted):
    cfg = config.qcatConfig()
    desc = auto.descriptor(auto.layouts, cfg, native.ENDS_BOTH, min_read_length=100, trim=True)
    kit = native.NativeKit(desc)
    reads = voted[:1500] + ["ACGT" * 20] + voted[1500:]                           # (a read the minimum-length filter drops whatever its trims)
    batch = _upload(ctx, reads)
    recs, counts, slots = ctx.scan_resident_batches(kit, batch, 1000, kit_auto=True, filter_barcodes=True)
    assert len(slots) == 4
    unfiltered, _c, slots_u = ctx.scan_resident_batches(kit, batch, 1000, kit_auto=True)
    assert slots.tolist() == slots_u.tolist()
    assert recs.tobytes() == _python_filter(auto, auto.layouts, unfiltered, 1000).tobytes() != unfiltered.tobytes()
    ctx.scan_resident_batches(kit, batch, 1000, kit_auto=True, filter_barcodes=True, fetch=False)
    nb = desc.n_count_buckets
    fetched = np.zeros(nb, dtype=np.int64)
    ctx.hip.check(ctx.hip.lib.qcat_ctx_fetch_counts(ctx.handle, fetched.ctypes.data, nb))
    want = helpers.driver_histogram(desc, auto.layouts, recs, [len(r) for r in reads], 100, True)
    assert np.array_equal(fetched, want) and np.array_equal(counts, want) and want[-1] >= 4
    part = ctx.partition(kit, batch)
    sizes = np.diff(part.bin_first.astype(np.int64))
    n_bins = desc.n_partition_bins
    assert np.array_equal(sizes[:n_bins - 1], counts[:n_bins - 1]) and sizes[n_bins - 1] == counts[-1]
    again = ctx.partition(kit, batch, recs)
    assert np.array_equal(again.bin_first, part.bin_first) and np.array_equal(again.source, part.source)
    assert again.batch.download()[0].tobytes() == part.batch.download()[0].tobytes()


# ---- 6. refusals leave the context usable ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(auto, tmp_path):
    ctx = native.NativeContext(0)
    cfg = config.qcatConfig()
    pbc = scanner.factory(kit="PBC096")
    reads = synth.synth_batch(400, 61, pbc.layouts, 1, 0, error_rate=0.08) + ["", "A", "N" * 200]
    batch = _upload(ctx, reads)
    with pytest.raises(RuntimeError, match="error -1.*ENDS_BOTH"):
        ctx.scan_resident_batches(native.NativeKit(auto.descriptor(ends=native.ENDS_5P)), batch, 100, kit_auto=True)
    simple = scanner.factory(mode="simple", kit="standard")
    with pytest.raises(RuntimeError, match="error -1.*simple"):
        ctx.scan_resident_batches(native.NativeKit(simple.descriptor()), batch, 100, kit_auto=True)
    # templates outside the generated kernels share adapter slices: their adapter pass cannot be resumed per kit
    rng = __import__("random").Random(3)
    folder = str(tmp_path)
    for name, seq in (("KA", "GGTGCTG" + "N" * 24 + "TTAACCTTTCTGTTGGTGCTGATATTGC"), ("KB", "CCGTGAC" + "N" * 24 + "AGAGTTTGATCATGGCTCAGGATTACC")):
        custom_kits.write_kit(folder, name, name, seq, custom_kits.random_barcodes(rng, 8))
    import yaml
    for f in os.listdir(folder):
        d = yaml.safe_load(open(os.path.join(folder, f)))
        d["auto_detect"] = True
        yaml.safe_dump(d, open(os.path.join(folder, f), "w"))
    custom = scanner.factory(kit_folder=folder)
    assert len(custom.layouts) == 2
    with pytest.raises(RuntimeError, match="error -2"):
        ctx.scan_resident_batches(native.NativeKit(custom.descriptor(qcat_config=cfg), jit=False), batch, 100, kit_auto=True)
    with pytest.raises(RuntimeError, match="error -1.*unknown flag"):
        ctx.hip.check(ctx.hip.lib.qcat_scan_resident_batches(ctx.handle, native.NativeKit(pbc.descriptor()).handle, batch.handle, 100, 4))
    # nothing of the refused scans is left: no slots, no records to partition
    kit = native.NativeKit(pbc.descriptor())
    with pytest.raises(RuntimeError, match="error -1"):
        ctx.fetch_kit_slots(len(reads), 100)
    # a plain scan afterwards gives the oracle's records
    recs, _counts = ctx.scan_resident(kit, batch)
    assert recs.tobytes() == oracle_lib.scan(pbc.descriptor(), reads, threads=8).tobytes()
    # the slots of a scan that did not vote; the records of a scan of another batch
    filtered, _c, none = ctx.scan_resident_batches(kit, batch, 100, filter_barcodes=True)
    assert none is None and filtered.tobytes() == _python_filter(pbc, pbc.layouts, recs, 100).tobytes()
    with pytest.raises(RuntimeError, match="QCAT_RESIDENT_KIT_AUTO"):
        ctx.fetch_kit_slots(len(reads), 100)
    other = _upload(ctx, reads[:50])
    with pytest.raises(RuntimeError, match="records == NULL"):
        ctx.partition(kit, other)
    full = auto._native_kit(auto.layouts, cfg, native.ENDS_BOTH)
    ctx.scan_resident_batches(full, batch, 100, kit_auto=True, fetch=False)
    with pytest.raises(RuntimeError, match="n_batches"):
        ctx.fetch_kit_slots(len(reads), 50)
    assert len(ctx.fetch_kit_slots(len(reads), 100)) == 5
    with pytest.raises(ValueError, match="kit auto.*demux_batches"):
        auto.demux_batch(reads)


# ---- 7. no flags ----------------------------------------------------------------------------------------------------------------------------
def test_without_flags_it_is_scan_resident(ctx):
    pbc = scanner.factory(kit="PBC096")
    kit = native.NativeKit(pbc.descriptor(trim=True, min_read_length=100))
    reads = synth.synth_batch(5000, 71, pbc.layouts, 1, 0, error_rate=0.08) + ["", "A", "N" * 200]
    batch = _upload(ctx, reads)
    recs, counts = ctx.scan_resident(kit, batch)
    got, got_counts, slots = ctx.scan_resident_batches(kit, batch, 4000)
    assert slots is None and got.tobytes() == recs.tobytes() and np.array_equal(got_counts, counts)
    part = ctx.partition(kit, batch)
    assert np.array_equal(np.diff(part.bin_first.astype(np.int64))[:-1], counts[:len(part.bin_first) - 2])

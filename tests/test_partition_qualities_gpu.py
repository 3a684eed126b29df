"""The quality plane of a resident batch and the device-pointer calls on the GPU: qcat_batch_upload_fastq / _has_qualities /
_download_qualities, qcat_batch_partition moving both planes in one pass (k_part_copy<2>, csrc/kernels_partition.inc),
qcat_batch_from_device / _devptrs, and BarcodeScanner.demux_batch(read_qualities=...).  The expectations are the numpy
restatement of tests/partition_cases.py: ``pc.expected`` applied to the quality strings in place of the reads gives the
expected quality plane, because the bins and the slices depend on the records and the lengths only."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import helpers
import partition_cases as pc
import synth
from qcat_amd import config, native, scanner

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    return native.NativeContext(0)


@pytest.fixture(scope="module")
def pbc096():
    return scanner.factory(kit="PBC096")


@pytest.fixture(scope="module")
def edge_reads():
    return pc.edge_reads()


def _quals_for(reads, seed):
    """seeded random quality bytes 33..126 of the reads' lengths: list of bytes"""
    rng = np.random.RandomState(seed)
    return [rng.randint(33, 127, size=len(r)).astype(np.uint8).tobytes() for r in reads]


def _upload(ctx, reads, quals=None):
    bases, offsets = native.pack_reads(reads)
    return native.ResidentBatch.upload(ctx, bases, offsets, None if quals is None else native.pack_qualities(quals, offsets))


def _split(raw, offsets):
    o = [int(x) for x in offsets]
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _check(part, want, want_q):
    """bases, qualities, offsets, bin_first and source of a partition against the restatement"""
    assert np.array_equal(want_q["offsets"], want["offsets"]) and np.array_equal(want_q["source"], want["source"])
    got_bases, got_offsets = part.batch.download()
    assert part.batch.info() == (len(want["source"]), len(want["bases"]))
    assert np.array_equal(got_offsets, want["offsets"])
    assert np.array_equal(part.bin_first, want["bin_first"])
    assert np.array_equal(part.source, want["source"])
    assert got_bases.tobytes() == want["bases"]
    assert part.batch.has_qualities
    got_q = part.batch.download_qualities()
    assert len(got_q) == len(want_q["bases"]) and got_q.tobytes() == want_q["bases"]


# ---- 1. edges, with records the test supplies ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(trim=True, min_read_length=500), dict(trim=False), dict(ends=native.ENDS_5P, trim=True, min_read_length=300)],
                         ids=["trim-min500", "whole", "5p-trim"])
def test_edge_lengths_and_trims_move_both_planes(ctx, pbc096, edge_reads, kw):
    desc = pbc096.descriptor(**kw)
    kit = native.NativeKit(desc)
    reads = edge_reads
    quals = _quals_for(reads, 31)
    assert len(reads) >= 300 and pc.EDGE_LONG in set(len(r) for r in reads)
    recs = pc.edge_records(desc, pbc096.layouts, reads)
    want = pc.expected(desc, pbc096.layouts, reads, recs)
    want_q = pc.expected(desc, pbc096.layouts, quals, recs)
    batch = _upload(ctx, reads, quals)
    assert batch.has_qualities and batch.download_qualities().tobytes() == b"".join(quals)
    part = ctx.partition(kit, batch, recs)
    _check(part, want, want_q)
    assert part.qualities(96) == [want_q["bases"][int(want["offsets"][i]):int(want["offsets"][i + 1])]
                                  for i in range(int(want["bin_first"][96]), int(want["bin_first"][97]))]
    assert [len(q) for q in part.qualities(0)] == [len(r) for r in part.reads(0)]
    # the bases are the bytes of the partition of the same reads WITHOUT qualities
    plain = _upload(ctx, reads)
    assert not plain.has_qualities
    plain_part = ctx.partition(kit, plain, recs)
    assert not plain_part.batch.has_qualities
    assert plain_part.batch.download()[0].tobytes() == part.batch.download()[0].tobytes()
    assert np.array_equal(plain_part.source, part.source) and np.array_equal(plain_part.bin_first, part.bin_first)


# ---- 2. after a real scan, records = NULL ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic(pbc096):
    reads = [r.encode() for r in synth.synth_batch(2000, 21, pbc096.layouts, 1, 0, error_rate=0.08)]
    return reads, _quals_for(reads, 32)


def test_partition_of_the_latest_resident_scan_of_a_fastq_batch(ctx, pbc096, synthetic):
    reads, quals = synthetic
    desc = pbc096.descriptor(trim=True, min_read_length=500)
    kit = native.NativeKit(desc)
    bases, offsets = native.pack_reads(reads)
    lib = native.HipLibrary.get().lib
    h = C.c_void_p()
    q = native.pack_qualities(quals, offsets)
    assert lib.qcat_batch_upload_fastq(ctx.handle, bases.ctypes.data, q.ctypes.data, offsets.ctypes.data, len(reads), C.byref(h)) == 0
    batch = native.ResidentBatch(ctx, h)
    assert lib.qcat_batch_has_qualities(batch.handle) == 1
    plain = _upload(ctx, reads)
    recs_plain, counts_plain = ctx.scan_resident(kit, plain)
    recs, counts = ctx.scan_resident(kit, batch)
    assert recs.tobytes() == recs_plain.tobytes() and np.array_equal(counts, counts_plain)      # the scans never look at the plane
    ctx.scan_resident(kit, batch, fetch=False)
    part = ctx.partition(kit, batch)                                            # records = NULL
    want = pc.expected(desc, pbc096.layouts, reads, recs)
    want_q = pc.expected(desc, pbc096.layouts, quals, recs)
    _check(part, want, want_q)
    sizes = np.diff(part.bin_first.astype(np.int64))
    assert (sizes[:96] > 0).sum() >= 90 and sizes[96] > 0 and 0 < len(want["bases"]) < int(offsets[-1])
    again = ctx.partition(kit, batch)
    assert again.batch.download()[0].tobytes() == part.batch.download()[0].tobytes()
    assert again.batch.download_qualities().tobytes() == part.batch.download_qualities().tobytes()
    assert np.array_equal(again.source, part.source) and np.array_equal(again.bin_first, part.bin_first)


# ---- 3. degenerate sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no reads", "one read", "one bin", "all skipped"])
def test_degenerate_sizes(ctx, pbc096, case):
    desc = pbc096.descriptor(trim=True, min_read_length=100000 if case == "all skipped" else 0)
    kit = native.NativeKit(desc)
    rng = np.random.RandomState(5)
    n = {"no reads": 0, "one read": 1}.get(case, 700)
    reads = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=rng.randint(0, 900))].tobytes() for _ in range(n)]
    quals = _quals_for(reads, 33)
    recs = np.zeros(n, dtype=native.RESULT_DTYPE)
    recs["adapter_idx"], recs["barcode_idx"], recs["barcode2_idx"] = 1, 33, -1
    recs["trim5p"] = 2
    recs["trim3p"] = np.array([max(0, len(r) - 3) for r in reads], dtype=np.int32)
    batch = _upload(ctx, reads, quals)
    assert batch.has_qualities and len(batch.download_qualities()) == sum(len(r) for r in reads)
    part = ctx.partition(kit, batch, recs)
    _check(part, pc.expected(desc, pbc096.layouts, reads, recs), pc.expected(desc, pbc096.layouts, quals, recs))
    sizes = np.diff(part.bin_first.astype(np.int64))
    assert sizes.sum() == n and (sizes > 0).sum() == (1 if n else 0)


# ---- 4. the output is a batch --------------------------------------------------------------------------------------------------------
def test_the_qualities_follow_through_a_second_partition(ctx, pbc096, synthetic):
    reads, quals = synthetic
    desc0 = pbc096.descriptor()                                                 # no trimming: the reads come out whole
    kit0 = native.NativeKit(desc0)
    batch = _upload(ctx, reads, quals)
    recs0, _ = ctx.scan_resident(kit0, batch)
    part0 = ctx.partition(kit0, batch)
    want0 = pc.expected(desc0, pbc096.layouts, reads, recs0)
    want0_q = pc.expected(desc0, pbc096.layouts, quals, recs0)
    _check(part0, want0, want0_q)
    assert part0.batch.info() == batch.info()
    reads1, quals1 = _split(want0["bases"], want0["offsets"]), _split(want0_q["bases"], want0["offsets"])
    desc1 = pbc096.descriptor(trim=True, min_read_length=500)
    kit1 = native.NativeKit(desc1)
    recs1, _ = ctx.scan_resident(kit1, part0.batch)
    part1 = ctx.partition(kit1, part0.batch)
    want1 = pc.expected(desc1, pbc096.layouts, reads1, recs1)
    _check(part1, want1, pc.expected(desc1, pbc096.layouts, quals1, recs1))
    assert 0 < len(want1["bases"]) < len(want0["bases"])


# ---- 5. from_device / devptrs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_quals", [True, False], ids=["bases+qualities", "bases only"])
def test_a_batch_made_from_another_batchs_device_pointers(ctx, pbc096, synthetic, with_quals):
    reads, quals = synthetic[0][:300], synthetic[1][:300]
    desc = pbc096.descriptor(trim=True, min_read_length=500)
    kit = native.NativeKit(desc)
    a = _upload(ctx, reads, quals)
    a_bases, a_offsets = a.download()
    a_quals = a.download_qualities()
    recs_a, _ = ctx.scan_resident(kit, a)
    part_a = ctx.partition(kit, a)
    pa_bases, pa_quals = part_a.batch.download()[0].tobytes(), part_a.batch.download_qualities().tobytes()
    p_bases, p_quals, p_offsets = a.devptrs()
    assert p_bases and p_quals and p_offsets and p_bases % 16 == 0 and p_quals % 16 == 0
    b = native.ResidentBatch.from_device(ctx, p_bases, p_offsets, len(reads), p_quals if with_quals else None)
    assert b.has_qualities == with_quals and b.info() == a.info()
    pb = b.devptrs()
    assert pb[0] != p_bases and pb[2] != p_offsets and (pb[1] is None) == (not with_quals)       # a copy, not a view
    a.destroy()
    got_bases, got_offsets = b.download()
    assert got_bases.tobytes() == a_bases.tobytes() and np.array_equal(got_offsets, a_offsets)
    if with_quals:
        assert b.download_qualities().tobytes() == a_quals.tobytes()
    recs_b, _ = ctx.scan_resident(kit, b)
    assert recs_b.tobytes() == recs_a.tobytes()
    part_b = ctx.partition(kit, b)
    assert part_b.batch.download()[0].tobytes() == pa_bases
    assert np.array_equal(part_b.source, part_a.source) and np.array_equal(part_b.bin_first, part_a.bin_first)
    assert part_b.batch.has_qualities == with_quals
    if with_quals:
        assert part_b.batch.download_qualities().tobytes() == pa_quals


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(pbc096, edge_reads):
    lib = native.HipLibrary.get().lib
    ctx = native.NativeContext(0)
    desc = pbc096.descriptor(trim=True, min_read_length=500)
    kit = native.NativeKit(desc)
    reads = edge_reads[:120]
    quals = _quals_for(reads, 34)
    recs = pc.edge_records(desc, pbc096.layouts, reads)
    batch = _upload(ctx, reads, quals)
    plain = _upload(ctx, reads)
    p_bases, p_quals, p_offsets = batch.devptrs()
    vp = C.c_void_p

    def refused(rc):
        assert rc == ERR_ARG and lib.qcat_last_error()

    def from_device(bases, quals_ptr, offsets, n, out=True):
        h = vp()
        rc = lib.qcat_batch_from_device(ctx.handle, vp(bases), vp(quals_ptr), vp(offsets), n, C.byref(h) if out else None)
        assert rc != 0 or h.value
        if rc == 0:
            lib.qcat_batch_destroy(h)
        return rc

    # null pointers
    refused(from_device(None, p_quals, p_offsets, len(reads)))
    refused(from_device(p_bases, p_quals, None, len(reads)))
    refused(from_device(p_bases, p_quals, p_offsets, len(reads), out=False))
    h = vp()
    refused(lib.qcat_batch_from_device(None, vp(p_bases), vp(p_quals), vp(p_offsets), len(reads), C.byref(h)))
    bases, offsets = native.pack_reads(reads)
    refused(lib.qcat_batch_upload_fastq(ctx.handle, bases.ctypes.data, None, offsets.ctypes.data, len(reads), C.byref(h)))
    # the quality plane of a batch that has none; the pointers of nothing
    out = np.zeros(plain.n_bases, dtype=np.uint8)
    refused(lib.qcat_batch_download_qualities(ctx.handle, plain.handle, out.ctypes.data))
    with pytest.raises(RuntimeError, match="no quality plane"):
        plain.download_qualities()
    a, b, c = vp(), vp(), vp()
    refused(lib.qcat_batch_devptrs(None, C.byref(a), C.byref(b), C.byref(c)))
    assert lib.qcat_batch_has_qualities(None) < 0
    assert plain.devptrs()[1] is None and plain.devptrs()[0]
    # wrong offsets: the offset array lives on the device as the BASES of a small uploaded batch (valid memory, which the check
    # kernel may read in full); its bases pointer goes in as d_offsets.  The reads pointer is `batch`'s, far longer than 8 bytes.
    def offsets_batch(values):
        raw = np.array(values, dtype=np.uint64).view(np.uint8)
        return native.ResidentBatch.upload(ctx, raw, np.array([0, len(raw)], dtype=np.uint64))

    assert batch.n_bases >= 8
    good, decreasing, nonzero = offsets_batch([0, 3, 5, 8]), offsets_batch([0, 5, 3, 8]), offsets_batch([2, 5, 6, 8])
    assert from_device(p_bases, p_quals, good.devptrs()[0], 3) == 0                             # (the set-up itself is accepted)
    refused(from_device(p_bases, p_quals, decreasing.devptrs()[0], 3))
    assert b"non-decreasing" in lib.qcat_last_error()
    refused(from_device(p_bases, None, decreasing.devptrs()[0], 3))
    refused(from_device(p_bases, p_quals, nonzero.devptrs()[0], 3))
    refused(from_device(p_bases, p_quals, good.devptrs()[0] + 4, 2))                            # offsets not aligned to 8 bytes
    # the context works as before
    part = ctx.partition(kit, batch, recs)
    _check(part, pc.expected(desc, pbc096.layouts, reads, recs), pc.expected(desc, pbc096.layouts, quals, recs))
    again = native.ResidentBatch.from_device(ctx, p_bases, p_offsets, len(reads), p_quals)
    assert again.download_qualities().tobytes() == b"".join(quals)


# ---- 7. demux_batch ------------------------------------------------------------------------------------------------------------------
def test_demux_batch_cuts_the_qualities_with_the_reads(pbc096):
    reads = synth.synth_batch(200, 14, pbc096.layouts, 1, 0, error_rate=0.08) + ["", "ACGT"]
    quals = [q.decode() for q in _quals_for(reads, 35)]
    results = pbc096.detect_barcode_batch(reads, [None] * len(reads))
    got = pbc096.demux_batch(reads, trim=True, min_read_length=100, read_qualities=quals)
    want, want_plain = {}, {}
    for i, (read, qual, res) in enumerate(zip(reads, quals, results)):
        t5, t3 = res["trim5p"], res["trim3p"]
        key = "skipped" if len(read[t5:t3]) < 100 else (res["barcode"].id if res["barcode"] else "none")
        want.setdefault(key, []).append((i, read[t5:t3], qual[t5:t3]))
        want_plain.setdefault(key, []).append((i, read[t5:t3]))
    assert got == want and len(got["skipped"]) == 2 and len(got) > 20
    slot = pbc096.descriptor().id_slots
    order = [k for k in got if k not in ("none", "skipped")]
    assert order == sorted(order, key=lambda k: slot[k]) and list(got)[-1] == "skipped"          # bin order, as without qualities
    assert pbc096.demux_batch(reads, trim=True, min_read_length=100) == want_plain                # without: what it returns today
    untrimmed = pbc096.demux_batch(reads, read_qualities=quals)
    assert sorted(e for v in untrimmed.values() for e in v) == [(i, r, q) for i, (r, q) in enumerate(zip(reads, quals))]
    with pytest.raises(ValueError, match="quality values"):
        pbc096.demux_batch(reads, read_qualities=quals[:-1] + ["!"])
    with pytest.raises(ValueError, match="kit auto"):
        scanner.factory(kit="auto").demux_batch(reads, read_qualities=quals)


# ---- 8. the reference driver's own per-barcode FASTQ files ------------------------------------------------------------------------------
with open(os.path.join(helpers.GOLDEN, "cli_golden.json")) as _fh:
    GOLDEN_RUNS = {r["file"]: r for r in json.load(_fh)["runs"] if r["variant"]["tag"] == "dir-auto-trim"}


@pytest.mark.parametrize("name", ["nbd103.fastq", "pbk004.fastq", "rab204.fastq", "rbk004.fastq"])
def test_partitioned_planes_give_the_reference_drivers_trimmed_fastq_files(ctx, name):
    """records of the kit-auto batch call (the call the driver makes), bases and qualities partitioned in HBM under
    trim=True, min_read_length=100, every barcode bin written as the reference writer writes it (qcat/cli.py:327-342, the
    title split as extract_fastx_comment): the sha256 of each text is the golden digest of the reference driver's file"""
    run = GOLDEN_RUNS[name]
    v = run["variant"]
    assert v["trim"] and v["min_len"] == 100 and v["dir"] and run["kit"] == "auto"
    with open(os.path.join(helpers.GOLDEN, "data", name)) as fh:
        lines = fh.read().split("\n")
    titles, reads, quals = [], [], []
    for i in range(0, len(lines) - 3, 4):
        assert lines[i].startswith("@") and lines[i + 2].startswith("+")
        titles.append(lines[i][1:]); reads.append(lines[i + 1]); quals.append(lines[i + 3])
    assert 7 <= len(reads) <= 11
    det = scanner.factory(kit="auto")
    cfg = config.get_default_config()
    bases, offsets = native.pack_reads(reads)
    got = ctx.scan_auto(det._native_kit(det.layouts, cfg, native.ENDS_BOTH), bases, offsets)
    assert got is not None
    recs = got[0]
    desc = det.descriptor(det.layouts, cfg, native.ENDS_BOTH, min_read_length=100, trim=True)
    kit = native.NativeKit(desc)
    batch = native.ResidentBatch.upload(ctx, bases, offsets, native.pack_qualities(quals, offsets))
    part = ctx.partition(kit, batch, recs)
    n_bins = part.n_bins
    files = {}
    for b in np.flatnonzero(np.diff(part.bin_first.astype(np.int64)) > 0).tolist():
        if b == n_bins - 1:
            continue                                                            # skipped: the driver writes nothing
        first = int(part.bin_first[b])
        src = [int(part.source[first + i]) for i in range(len(part.reads(b)))]
        bc_id = "none"
        if b < n_bins - 2:
            r = recs[src[0]]
            barcode = det.layouts[int(r["adapter_idx"])].barcode_set_1[int(r["barcode_idx"])]
            assert desc.partition_label(b) == barcode.id                        # the bin's label is the barcode the records call
            bc_id = (barcode.name or "").replace("/", "_") if barcode.name else barcode.name
        text = ""
        for i, seq, qual in zip(src, part.reads(b), part.qualities(b)):
            cols = titles[i].replace("\t", " ").split(" ")
            title, comment = cols[0], (" ".join(cols[1:]) if len(cols) > 1 else "")
            text += "@" + title + " " + comment + "\n" + seq.decode() + "\n+\n" + qual.decode() + "\n"
        files[bc_id + ".fastq"] = hashlib.sha256(text.encode()).hexdigest()
    assert files == run["files"]

"""qcat_batch_partition on the GPU: the stable partition of a resident batch by barcode (csrc/kernels_partition.inc) against the
numpy restatement of tests/partition_cases.py, byte for byte -- bases, offsets, bin_first and source."""
import ctypes as C

import numpy as np
import pytest

import partition_cases as pc
import synth
from qcat_amd import native, scanner

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


def _host_reads(batch):
    bases, offsets = batch.download()
    raw, o = bases.tobytes(), offsets.tolist()
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _check(part, want):
    got_bases, got_offsets = part.batch.download()
    assert part.batch.info() == (len(want["source"]), len(want["bases"]))
    assert np.array_equal(got_offsets, want["offsets"])
    assert np.array_equal(part.bin_first, want["bin_first"])
    assert np.array_equal(part.source, want["source"])
    assert got_bases.tobytes() == want["bases"]


def _partition_raw(ctx, kit, batch, records, flags=0):
    """the C call itself: (status, batch handle)"""
    lib = native.HipLibrary.get().lib
    out = C.c_void_p()
    rc = lib.qcat_batch_partition(ctx.handle, kit.handle, batch.handle, records.ctypes.data if records is not None else None, flags, C.byref(out))
    return rc, out


# ---- 1. edges, with records the test supplies ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(trim=True, min_read_length=500), dict(trim=False), dict(ends=native.ENDS_5P, trim=True, min_read_length=300)],
                         ids=["trim-min500", "whole", "5p-trim"])
def test_edge_lengths_and_trims_with_supplied_records(ctx, pbc096, edge_reads, kw):
    desc = pbc096.descriptor(**kw)
    kit = native.NativeKit(desc)
    reads = edge_reads
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    assert set(pc.EDGE_LENGTHS + [pc.EDGE_LONG]) <= set(lens.tolist()) and len(reads) >= 300
    recs = pc.edge_records(desc, pbc096.layouts, reads)
    assert (recs["trim5p"] >= 0).all() and (recs["trim3p"] >= 0).all()
    want = pc.expected(desc, pbc096.layouts, reads, recs)
    # every residue mod 16 of the slices' source offsets and of their destination offsets (non-empty slices)
    trimming = bool(kw.get("trim")) and kw.get("ends", native.ENDS_BOTH) == native.ENDS_BOTH
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1] + (np.minimum(recs["trim5p"], lens) if trimming else 0)
    keep = np.diff(want["offsets"].astype(np.int64))
    assert set((starts[want["source"]][keep > 0] % 16).tolist()) == set(range(16))
    assert set((want["offsets"][:-1][keep > 0].astype(np.int64) % 16).tolist()) == set(range(16))
    assert (keep == 0).sum() >= 14 and ((keep > 0) & (keep < 16)).sum() > 20    # empty slices and slices shorter than a vector
    sizes = np.diff(want["bin_first"].astype(np.int64))
    assert (sizes[:96] == 0).sum() > 80 and sizes[96] > 0                       # most barcode bins stay empty; `none` does not
    batch = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    part = ctx.partition(kit, batch, recs)
    _check(part, want)
    assert [part.reads(b) for b in (0, 96)] == [[want["bases"][int(want["offsets"][i]):int(want["offsets"][i + 1])]
                                                  for i in range(int(want["bin_first"][b]), int(want["bin_first"][b + 1]))] for b in (0, 96)]


# ---- 2. after a real scan, records = NULL ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scanned(ctx, pbc096):
    desc = pbc096.descriptor(trim=True, min_read_length=500)
    kit = native.NativeKit(desc)
    sp = native.SynthParams(seed=11, n_reads=20000, insert_len=600, lead_min=5, lead_max=40, error_rate=0.08, no_adapter_fraction=0.05,
                            tpl_5p=1, tpl_3p=0)
    batch = native.ResidentBatch.synthesize(ctx, kit, sp)
    recs, counts = ctx.scan_resident(kit, batch)
    return desc, kit, batch, recs, counts


def test_partition_of_the_latest_resident_scan(ctx, pbc096, scanned):
    desc, kit, batch, recs, counts = scanned
    ctx.scan_resident(kit, batch, fetch=False)
    part = ctx.partition(kit, batch)                                            # records = NULL
    want = pc.expected(desc, pbc096.layouts, _host_reads(batch), recs)
    _check(part, want)
    n_bins = desc.n_partition_bins
    assert n_bins == 98 and len(part.bin_first) == n_bins + 1
    sizes = np.diff(part.bin_first.astype(np.int64))
    assert np.array_equal(sizes[:n_bins - 1], counts[:n_bins - 1]) and sizes[n_bins - 1] == counts[-1]      # barcodes, none | skipped
    assert sizes[n_bins - 1] > 0 and (sizes[:96] > 0).sum() >= 90
    assert np.array_equal(np.sort(part.source), np.arange(20000))
    again = ctx.partition(kit, batch)
    assert again.batch.download()[0].tobytes() == part.batch.download()[0].tobytes()
    assert np.array_equal(again.source, part.source) and np.array_equal(again.bin_first, part.bin_first)
    # the same vectors in device memory
    lib = native.HipLibrary.get().lib
    assert lib.qcat_ctx_partition_bins_devptr(ctx.handle) and lib.qcat_ctx_partition_source_devptr(ctx.handle)


# ---- 3. many bins ------------------------------------------------------------------------------------------------------------------
def test_dual_kit_needs_more_than_one_digit(ctx):
    det = scanner.factory(mode="dual")
    desc = det.descriptor(trim=True, min_read_length=300)
    kit = native.NativeKit(desc)
    assert desc.n_partition_bins == 96 * 96 + 2                                 # the shipped 24 x 96 dual kit: 96 distinct ids, two digits
    sp = native.SynthParams(seed=12, n_reads=5000, insert_len=600, lead_min=5, lead_max=40, error_rate=0.08, no_adapter_fraction=0.05,
                            tpl_5p=1, tpl_3p=0)
    batch = native.ResidentBatch.synthesize(ctx, kit, sp)
    recs, counts = ctx.scan_resident(kit, batch)
    part = ctx.partition(kit, batch)
    want = pc.expected(desc, det.layouts, _host_reads(batch), recs)
    _check(part, want)
    sizes = np.diff(part.bin_first.astype(np.int64))
    n_bins = desc.n_partition_bins
    assert np.array_equal(sizes[:n_bins - 1], counts[:n_bins - 1]) and sizes[n_bins - 1] == counts[-1]
    assert (np.flatnonzero(sizes[:n_bins - 2]) >= 256).any()                    # calls beyond the first digit


def test_simple_mode(ctx):
    det = scanner.factory(mode="simple", kit="standard")
    desc = det.descriptor(trim=False, min_read_length=300)
    kit = native.NativeKit(desc)
    lays = scanner.factory(kit="PBK004/LWB001").layouts
    reads = [r.encode() for r in synth.synth_batch(2000, 13, lays, 1, 0, error_rate=0.05, insert_len=200)]
    batch = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    recs, counts = ctx.scan_resident(kit, batch)
    part = ctx.partition(kit, batch)
    want = pc.expected(desc, [det._simple_layout], reads, recs)
    _check(part, want)
    sizes = np.diff(part.bin_first.astype(np.int64))
    n_bins = desc.n_partition_bins
    assert np.array_equal(sizes[:n_bins - 1], counts[:n_bins - 1]) and sizes[n_bins - 1] == counts[-1]
    assert (sizes[:n_bins - 2] > 0).sum() >= 6 and sizes[n_bins - 1] > 0


# ---- 4. degenerate sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no reads", "one read", "one bin", "all skipped"])
def test_degenerate_sizes(ctx, pbc096, case):
    desc = pbc096.descriptor(trim=True, min_read_length=100000 if case == "all skipped" else 0)
    kit = native.NativeKit(desc)
    rng = np.random.RandomState(5)
    n = {"no reads": 0, "one read": 1}.get(case, 700)
    reads = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=rng.randint(0, 900))].tobytes() for _ in range(n)]
    recs = np.zeros(n, dtype=native.RESULT_DTYPE)
    recs["adapter_idx"], recs["barcode_idx"], recs["barcode2_idx"] = 1, 33, -1
    recs["trim5p"] = 2
    recs["trim3p"] = np.array([max(0, len(r) - 3) for r in reads], dtype=np.int32)
    batch = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    part = ctx.partition(kit, batch, recs)
    want = pc.expected(desc, pbc096.layouts, reads, recs)
    _check(part, want)
    sizes = np.diff(part.bin_first.astype(np.int64))
    assert sizes.sum() == n and (sizes > 0).sum() == (1 if n else 0)
    if case == "all skipped":
        assert sizes[-1] == n


# ---- 5. the output is a batch --------------------------------------------------------------------------------------------------------
def test_the_output_scans_like_any_batch(ctx, pbc096, scanned):
    _desc, _kit, batch, _recs, _counts = scanned
    desc = pbc096.descriptor()                                                  # no trimming: the reads come out whole
    kit = native.NativeKit(desc)
    recs, _ = ctx.scan_resident(kit, batch)
    part = ctx.partition(kit, batch)
    assert part.batch.info() == batch.info()
    recs_out, _ = ctx.scan_resident(kit, part.batch)
    assert recs_out.tobytes() == recs[part.source].tobytes()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(pbc096, edge_reads):
    lib = native.HipLibrary.get().lib
    ctx = native.NativeContext(0)                                               # a context without a resident scan
    desc = pbc096.descriptor(trim=True, min_read_length=500)
    kit = native.NativeKit(desc)
    reads = edge_reads[:120]
    recs = pc.edge_records(desc, pbc096.layouts, reads)
    batch = native.ResidentBatch.upload(ctx, *native.pack_reads(reads))
    other = native.ResidentBatch.upload(ctx, *native.pack_reads(reads[:50]))

    def refused(rc):
        assert rc == ERR_ARG and lib.qcat_last_error()

    refused(_partition_raw(ctx, kit, batch, None)[0])                           # records = NULL, no resident scan before it
    ctx.scan_resident(kit, other, fetch=False)
    refused(_partition_raw(ctx, kit, batch, None)[0])                           # the latest scan was of another number of reads
    refused(_partition_raw(ctx, kit, batch, recs, flags=1)[0])
    bad = recs.copy()
    bad["barcode_idx"][7] = 96                                                  # outside the set
    refused(_partition_raw(ctx, kit, batch, bad)[0])
    _check(ctx.partition(kit, batch, recs), pc.expected(desc, pbc096.layouts, reads, recs))


# ---- 7. demux_batch ------------------------------------------------------------------------------------------------------------------
def test_demux_batch_groups_like_detect_barcode_batch(pbc096):
    reads = synth.synth_batch(200, 14, pbc096.layouts, 1, 0, error_rate=0.08) + ["", "ACGT"]
    got = pbc096.demux_batch(reads)
    results = pbc096.detect_barcode_batch(reads, [None] * len(reads))
    want = {}
    for i, (read, res) in enumerate(zip(reads, results)):
        want.setdefault(res["barcode"].id if res["barcode"] else "none", []).append((i, read))
    assert got == want and len(got) > 20
    slot = pbc096.descriptor().id_slots
    order = [k for k in got if k != "none"]
    assert order == sorted(order, key=lambda k: slot[k]) and list(got)[-1] == "none"         # bin order
    # trimmed, with the minimum-length filter
    got = pbc096.demux_batch(reads, trim=True, min_read_length=100)
    want = {}
    for i, (read, res) in enumerate(zip(reads, results)):
        kept = read[res["trim5p"]:res["trim3p"]]
        key = "skipped" if len(kept) < 100 else (res["barcode"].id if res["barcode"] else "none")
        want.setdefault(key, []).append((i, kept))
    assert got == want and len(got["skipped"]) == 2
    with pytest.raises(ValueError, match="kit auto"):
        scanner.factory(kit="auto").demux_batch(reads)

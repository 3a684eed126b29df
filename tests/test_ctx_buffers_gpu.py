"""The scratch buffers of a context (csrc/dev_buf.h: DevBuf / PinBuf in qcat_ctx, PackedScratch and PipeStage) across scans
that grow them, leave them bigger than needed, and move them: one context is walked through every buffer family, a
reallocation must drop a captured graph, and the pipeline's stage staging must grow between two calls.  Everything is compared
with the CPU oracle, records byte for byte and count vectors; a scan on a used context must also return what a fresh context
returns for the same input (a lost slack term, a capacity attached to the wrong buffer or a dangling group member shows there).

The Python read generator and the oracle are what costs time here, so reads are generated once per kit (module cache) and the
larger batches repeat them: a read's record does not depend on its neighbours, so the oracle's records repeat the same way and
its count vectors add up."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import synth
from qcat_amd import config, native, scanner

pytestmark = pytest.mark.gpu

_cache = {}


def _resident_scan(ctx, kit, reads):
    """qcat_batch_upload + qcat_scan_resident on `ctx`: (records, count vector)"""
    hip = native.HipLibrary.get()
    lib = hip.lib
    bases, offsets = native.pack_reads(reads)
    batch = C.c_void_p()
    hip.check(lib.qcat_batch_upload(ctx.handle, bases.ctypes.data, offsets.ctypes.data, len(reads), C.byref(batch)))
    try:
        hip.check(lib.qcat_scan_resident(ctx.handle, kit.handle, batch))
        recs = np.zeros(len(reads), dtype=native.RESULT_DTYPE)
        cnt = np.zeros(kit.descriptor.n_count_buckets, dtype=np.int64)
        hip.check(lib.qcat_ctx_fetch_results(ctx.handle, recs.ctypes.data, len(reads)))
        hip.check(lib.qcat_ctx_fetch_counts(ctx.handle, cnt.ctypes.data, len(cnt)))
        return recs, cnt
    finally:
        lib.qcat_batch_destroy(batch)


def _families():
    """name -> (descriptor, reads, oracle records, oracle counts, options of the scan)"""
    if "families" in _cache:
        return _cache["families"]
    pbc = scanner.factory(mode="epi2me", kit="PBC096")
    nbd = scanner.factory(mode="epi2me", kit="NBD103/NBD104")
    dual = scanner.factory(mode="dual")
    simple = scanner.factory(mode="simple", kit="standard")
    middle = scanner.factory(mode="epi2me", kit="NBD103/NBD104", scan_middle_adapter=True)
    pbc_reads = synth.synth_batch(6000, 20261101, pbc.layouts, 1, 0, error_rate=0.08)
    pbc_reads[5], pbc_reads[6], pbc_reads[7] = "", "A", pbc_reads[7][:33] + "N" + pbc_reads[7][34:]
    for i, cut in enumerate((1, 149, 150, 151, 299, 300, 301, 302, 449, 450, 451)):      # (ragged reads around one and two windows)
        pbc_reads[10 + i] = pbc_reads[10 + i][:cut]
    half = synth.synth_batch(2500, 20261102, nbd.layouts, len(nbd.layouts) - 1, 0, error_rate=0.08, no_adapter_fraction=0.2)
    half[5], half[6], half[7] = "", "N" * 180, half[7][:120]
    nbd_reads = half + half[::-1]
    dual_reads = synth.synth_batch(150, 20261103, dual.layouts, 1, 0, error_rate=0.08) + synth.synth_batch(150, 20261104, dual.layouts, 0, 1, error_rate=0.08)
    middle_reads = [half[i % 2500] + half[(i + 1250) % 2500] if i % 3 == 0 else half[i % 2500] for i in range(3000)]   # (every third read a chimera)
    plan = {
        "tiny3": (pbc.descriptor(ends=native.ENDS_BOTH), pbc_reads[100:103], {}),
        "packed5000": (nbd.descriptor(ends=native.ENDS_5P), nbd_reads, {}),
        "dual300": (dual.descriptor(ends=native.ENDS_BOTH), dual_reads, {}),
        "simple2000": (simple.descriptor(), pbc_reads[:2000], {}),
        "middle3000": (middle.descriptor(), middle_reads, {"MIDDLE_ABS_MIN": 1}),
        "bitslice6000": (pbc.descriptor(ends=native.ENDS_BOTH), pbc_reads, {"ADAPTER_BITSLICE_MIN": 1}),
        "tiny40": (pbc.descriptor(ends=native.ENDS_BOTH), pbc_reads[200:240], {}),
    }
    out = {}
    for name, (d, reads, opts) in plan.items():
        o_recs, o_cnt = oracle_lib.scan(d, reads, counts=True, threads=16)
        out[name] = (d, reads, o_recs, o_cnt, opts)
    assert plan["middle3000"][0].scan_middle
    assert np.count_nonzero(out["middle3000"][2]["exit_status"] == 997) > 0          # (interior adapters were found: that scan had work)
    assert np.count_nonzero(out["simple2000"][2]["barcode_idx"] >= 0) > 100          # (the list holds some of these reads' barcodes)
    _cache["families"] = out
    return out


def test_one_context_through_every_buffer_family(hip_options):
    """3 reads on the one-wave kernels, 5000 on the packed path (5' only), the dual kit, a simple list on the packed simple
    kernels, --detect-middle with the bit-sliced interior scan, a batch on the bit-sliced adapter kernels, then 40 reads and
    the 5000 again in buffers that are now larger than they need: each scan equals the oracle, the last two also a fresh context"""
    fam = _families()
    hip_options(NO_TINY=None)                                   # (the product's default: a handful of reads takes the one-wave kernels)
    lib = native.HipLibrary.get().lib
    ctx = native.NativeContext(0)
    kits = {}
    order = ["tiny3", "packed5000", "dual300", "simple2000", "middle3000", "bitslice6000", "tiny40", "packed5000"]
    for step, name in enumerate(order):
        d, reads, o_recs, o_cnt, opts = fam[name]
        kit = kits.setdefault(name, native.NativeKit(d))
        hip_options(MIDDLE_ABS_MIN=opts.get("MIDDLE_ABS_MIN"), ADAPTER_BITSLICE_MIN=opts.get("ADAPTER_BITSLICE_MIN"))
        recs, cnt = _resident_scan(ctx, kit, reads)
        bad = np.nonzero(recs != o_recs)[0]
        assert len(bad) == 0, (step, name, bad[:10], recs[bad[:3]], o_recs[bad[:3]])
        assert np.array_equal(cnt, o_cnt), (step, name)
        # the scans ran where they were meant to
        if name.startswith("tiny"):
            assert lib.qcat_ctx_tiny_ends(ctx.handle) == 2 * len(reads), (step, name)
        if name == "middle3000":
            tiles = (C.c_uint32 * 4)()
            assert lib.qcat_ctx_middle_bitslice_tiles(ctx.handle, tiles) == 0 and tiles[0] >= 1, list(tiles)
        if name == "bitslice6000":
            front = (C.c_uint32 * 2)()
            assert lib.qcat_ctx_fused_front(ctx.handle, front) == 0 and front[0] == 2 * len(reads), list(front)
        if step >= 6:
            f_recs, f_cnt = _resident_scan(native.NativeContext(0), kit, reads)
            assert recs.tobytes() == f_recs.tobytes() and np.array_equal(cnt, f_cnt), (step, name)


def _mixed(det, n, seed):
    """reads of three kits, PBC096 most frequent, and the degenerate reads"""
    by_kit = {}
    for i, l in enumerate(det.layouts):
        by_kit.setdefault(l.kit, []).append(i)
    kits = ["PBC096"] + [k for k in by_kit if k != "PBC096"][:2]
    reads = ["", "A", "N" * 200]
    for k, share in zip(kits, (n - 3 - (n - 3) * 2 // 5, (n - 3) // 4, (n - 3) * 2 // 5 - (n - 3) // 4)):     # 60 %, 25 %, 15 %
        idx = by_kit[k]
        reads += synth.synth_batch(share, seed + len(reads), det.layouts, idx[-1], idx[0] if len(idx) > 1 else -1, error_rate=0.08)
    order = np.random.default_rng(seed).permutation(len(reads))
    return [reads[i] for i in order]


def test_a_reallocation_drops_a_captured_graph():
    """kit-auto host-buffer calls of one shape replay a captured graph, which holds buffer addresses; a bigger call in between
    moves the staging and the scratch, so the next call of the old shape must launch kernel by kernel (the replay counter
    stands still across it) and replays come back only after a new capture -- every call's records against the oracle"""
    det = scanner.factory()
    cfg = config.qcatConfig()
    lib = native.HipLibrary.get().lib
    ctx = native.NativeContext(0)
    kit = det._native_kit(det.layouts, cfg, native.ENDS_BOTH)
    sub = det.get_adapters("PBC096")
    full_index = np.array([det.layouts.index(l) for l in sub] + [-1])
    reads = _mixed(det, 500, 31)
    assert len(reads) == 500
    o = oracle_lib.scan(det.descriptor(layouts=sub, qcat_config=cfg), reads, threads=16)
    want = {500: (native.pack_reads(reads), o), 9000: (native.pack_reads(reads * 18), np.tile(o, 18))}     # (the same vote, eighteen times)

    def call(n):
        (bases, offsets), o = want[n]
        got = ctx.scan_auto(kit, bases, offsets)
        assert got is not None
        recs, slot = got
        assert kit.descriptor.kit_names[slot] == "PBC096"
        assert np.array_equal(full_index[o["adapter_idx"]], recs["adapter_idx"])
        for name in ("barcode_idx", "barcode2_idx", "exit_status", "adapter_end", "trim5p", "trim3p", "raw_score", "score_den"):
            assert np.array_equal(o[name], recs[name]), (n, name)
        return lib.qcat_ctx_graph_replays(ctx.handle)

    def until_a_replay(start):
        for calls in range(1, 6):                               # (plain, capture, replay: the third call at the latest)
            if call(500) > start:
                return calls
        raise AssertionError("calls of one shape never replayed a graph")

    start = lib.qcat_ctx_graph_replays(ctx.handle)
    until_a_replay(start)
    before_big = lib.qcat_ctx_graph_replays(ctx.handle)
    assert call(9000) == before_big                             # (another shape: launched kernel by kernel)
    assert call(500) == before_big, "a call replayed a graph captured before its buffers were reallocated"
    assert until_a_replay(before_big) >= 1


def test_pipeline_stages_grow_between_calls(hip_options):
    """chunks of 4096 reads: a 33 000-read call sizes the two stage slots, a 70 000-read call on the same context reuses them (a
    slot is sized by the largest chunk, not by the batch); the same 70 000 reads in chunks of 8192 then grow the slots by the
    capped factor (pipeline_core.h: stage_need), and chunks of 4096 run once more in the slots that are now too big -- every call against
    the oracle.  The batches repeat the 6000 PBC096 reads of the first test (ragged reads among them, which land at other
    places of a chunk in every repetition)."""
    d, uniq, o_recs, o_cnt, _ = _families()["bitslice6000"]
    parts = [oracle_lib.scan(d, uniq[a:b], counts=True, threads=16) for a, b in ((0, 3000), (3000, 4000), (4000, 6000))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == o_recs.tobytes() and np.array_equal(sum(p[1] for p in parts), o_cnt)
    cnt_to = {3000: parts[0][1], 4000: parts[0][1] + parts[1][1]}
    kit = native.NativeKit(d)
    ctx = native.NativeContext(0)
    for n, chunk in ((33000, 4096), (70000, 4096), (70000, 8192), (33000, 4096)):
        hip_options(PIPELINE_CHUNK=chunk)
        whole, rest = divmod(n, len(uniq))
        reads = uniq * whole + uniq[:rest]
        want, want_cnt = np.concatenate([o_recs] * whole + [o_recs[:rest]]), o_cnt * whole + cnt_to[rest]
        cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
        recs = ctx.scan(kit, *native.pack_reads(reads), counts=cnt)
        bad = np.nonzero(recs != want)[0]
        assert len(bad) == 0, (n, chunk, bad[:10], recs[bad[:3]], want[bad[:3]])
        assert np.array_equal(cnt, want_cnt), (n, chunk)

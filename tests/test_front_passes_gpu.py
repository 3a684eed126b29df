"""The front end of a big batch in one kernel: k_pack_planes (csrc/kernels_abs.inc) packs the windows as k_pack_windows does
and builds the letter planes, keep masks and tile flags of the bit-sliced adapter scan from the windows it holds in the LDS,
where k_abs_planes read them back from memory.  A workgroup takes `wg` consecutive read ends (qcat_ctx_fused_front reports the
number), four workgroups a plane tile of 2048.  Everything is compared with the oracle, record for record and, in a debug scan,
per template (score and end of every template: a wrong plane word moves these); every test asserts through
qcat_ctx_fused_front that the kernel took the batch, since small batches are forced onto the big-batch path by options.

The batches are prefixes of one seeded batch per kit (a read's record does not depend on its neighbours), the oracle runs once."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import synth
from qcat_amd import config, native, scanner

TILE = 2048
_cache = {}
_KITS = {"both": ("PBC096", native.ENDS_BOTH), "5p": ("NBD103/NBD104", native.ENDS_5P)}


def _front(ctx):
    """(read ends of the latest scan that k_pack_planes took, read ends per workgroup of that kernel)"""
    lib = native.HipLibrary.get()
    out = (C.c_uint32 * 2)()
    lib.check(lib.lib.qcat_ctx_fused_front(ctx.handle, out))
    return int(out[0]), int(out[1])


def _ran(ctx):
    lib = native.HipLibrary.get().lib
    names = (C.c_char_p * 16)()
    ms = (C.c_float * 16)()
    return [names[i].decode() for i in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16))]


def _wg():
    if "wg" not in _cache:
        _cache["wg"] = _front(native.NativeContext(0))[1]
        assert 64 <= _cache["wg"] <= TILE and TILE % _cache["wg"] == 0
    return _cache["wg"]


def _batch(which):
    """3 * 2048 + 1 reads of the kit and their oracle records, counts left to the tests.  Off the bit-sliced path, NOT a multiple of
    128 apart so that flagged and unflagged 128-end tiles alternate: every 97th read is short (20 .. 159 bases, so some are
    still full windows) or holds an N; reads of 0 and 1 bases; the ends at the tile and workgroup edges."""
    if which not in _cache:
        kit, ends = _KITS[which]
        det = scanner.factory(mode="epi2me", kit=kit)
        n = 3 * TILE + 1
        reads = synth.synth_batch(n, 20261019 + len(kit), det.layouts, 1, 0, error_rate=0.08)
        for i in range(5, n, 97):
            reads[i] = reads[i][:20 + i % 140] if i % 2 else reads[i][:33] + "N" + reads[i][34:]
        reads[7] = ""
        reads[300] = "A"
        wg = _wg()
        reads[wg - 2] = reads[wg - 2][:149]                               # one code short, in front of a workgroup edge
        reads[wg] = reads[wg][:149] + "N" + reads[wg][150:]               # the first end of a workgroup: N in the window's last code
        reads[TILE - 2] = reads[TILE - 2][:149]
        reads[TILE] = reads[TILE][:149] + "N" + reads[TILE][150:]
        d = det.descriptor(ends=ends)
        o_recs, o_traces = oracle_lib.scan(d, reads, trace=True, threads=16)
        _cache[which] = (reads, d, o_recs, o_traces, 2 if ends == native.ENDS_BOTH else 1)
    return _cache[which]


def _check_prefix(which, n_reads, hip_options, debug_too=True):
    reads, d, o_recs, o_traces, per = _batch(which)
    hip_options(ADAPTER_BITSLICE_MIN=1, ABS_STAGES=2, BITSLICE_MIN=2048)
    bases, offsets = native.pack_reads(reads[:n_reads])
    kit = native.NativeKit(d)
    lib = native.HipLibrary.get()
    for debug in (False, True) if debug_too else (False,):
        ctx = native.NativeContext(0)
        lib.check(lib.lib.qcat_ctx_set_timing(ctx.handle, 1))
        got = ctx.scan(kit, bases, offsets, trace=True) if debug else ctx.scan(kit, bases, offsets)
        ran = _ran(ctx)
        assert _front(ctx)[0] == n_reads * per and "k_adapter_bitslice" in ran, (_front(ctx), ran)
        recs = got[0] if debug else got
        bad = np.nonzero(recs != o_recs[:n_reads])[0]
        assert len(bad) == 0, (debug, bad[:10], recs[bad[:3]], o_recs[bad[:3]])
        if debug:
            for name in ("window_len", "tpl_raw", "tpl_end", "best_tpl", "best_end"):
                assert np.array_equal(got[1][name], o_traces[name][:n_reads * per]), name


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["both", "5p"])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_tile_edges(which, n, hip_options):
    """one below, at and one above a plane tile, and three tiles and one: with one window per read (NBD103/NBD104, 5' only) these
    are the read-end counts; with two (PBC096) the read counts -- 4094, 4096, 4098 and 12 290 read ends, the same edges two
    ends at a time (a workgroup past the last read end only clears its keep masks; a tile that holds one or two ends)"""
    _check_prefix(which, n, hip_options)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["both", "5p"])
@pytest.mark.parametrize("side", [-1, 1])
def test_workgroup_edges(which, side, hip_options):
    """one read end below and above a workgroup of the kernel (5' only), one read -- two ends -- below and above (both ends)"""
    wg = _wg()
    per = 2 if which == "both" else 1
    _check_prefix(which, wg // per + side, hip_options)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["both", "5p"])
def test_flagged_ends_between_plain_ones(which, hip_options):
    """a tile and a half in which 128-end tiles with a short window or an N alternate with plain ones: the flagged tiles are
    the binary16 kernel's, the rest the bit-sliced kernel's, and the keep masks say which -- records, per-template scores
    and (oracle on this prefix) the count histogram, whose total is one barcode and one kit bucket per read"""
    reads, d, o_recs, o_traces, per = _batch(which)
    n = TILE + TILE // 2 + 3
    flagged = set()
    for i, r in enumerate(reads[:n]):
        if len(r) < 150 or "N" in r[:150] or (per == 2 and "N" in r[-150:]):
            flagged.add(i * per // 128)
    n_tiles128 = (n * per + 127) // 128
    plain = set(range(n_tiles128)) - flagged
    assert len(flagged) >= 8 and len(plain) >= 2 and min(plain) < max(flagged) and min(flagged) < max(plain)
    assert any(len(r) == 0 for r in reads[:n]) and any(len(r) == 1 for r in reads[:n])
    _check_prefix(which, n, hip_options)
    hip_options(ADAPTER_BITSLICE_MIN=1, ABS_STAGES=2, BITSLICE_MIN=2048)
    o_cnt = oracle_lib.scan(d, reads[:n], counts=True, threads=16)[1]
    cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
    ctx = native.NativeContext(0)
    recs = ctx.scan(native.NativeKit(d), *native.pack_reads(reads[:n]), counts=cnt)
    assert _front(ctx)[0] == n * per
    assert np.array_equal(cnt, o_cnt) and int(cnt.sum()) == 2 * n and recs.tobytes() == o_recs[:n].tobytes()


@pytest.mark.gpu
def test_dual_kit(hip_options):
    """the shipped dual kit: two templates per end with two barcode sets each, both ends"""
    det = scanner.factory(mode="dual")
    d = det.descriptor(ends=native.ENDS_BOTH)
    reads = synth.synth_batch(1500, 4005, det.layouts, 1, 0, error_rate=0.08)
    reads += synth.synth_batch(1500, 4006, det.layouts, 0, 1, error_rate=0.08)
    for i in range(3, len(reads), 61):
        reads[i] = reads[i][:100 + i % 60] if i % 2 else reads[i][:70] + "N" + reads[i][71:]
    o_recs, o_cnt = oracle_lib.scan(d, reads, counts=True, threads=16)
    hip_options(ADAPTER_BITSLICE_MIN=1, ABS_STAGES=2, BITSLICE_MIN=2048)
    lib = native.HipLibrary.get()
    ctx = native.NativeContext(0)
    lib.check(lib.lib.qcat_ctx_set_timing(ctx.handle, 1))
    cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
    recs = ctx.scan(native.NativeKit(d), *native.pack_reads(reads), counts=cnt)
    assert _front(ctx)[0] == 2 * len(reads) and "k_adapter_bitslice" in _ran(ctx)
    assert {int(t) for t in recs["adapter_idx"]} >= {0, 1}                  # both templates' paths
    bad = np.nonzero(recs != o_recs)[0]
    assert len(bad) == 0, (bad[:10], recs[bad[:3]], o_recs[bad[:3]])
    assert np.array_equal(cnt, o_cnt)


@pytest.mark.gpu
def test_small_batches_and_kit_auto_keep_the_two_kernels(hip_options):
    """outside the big batches of one kit the windows are packed alone: a batch below the switch (default options), and the
    vote pass of a kit-auto batch even where its adapter scan is bit-sliced"""
    reads, d, o_recs, _t, per = _batch("both")
    ctx = native.NativeContext(0)
    recs = ctx.scan(native.NativeKit(d), *native.pack_reads(reads[:3000]))
    assert _front(ctx)[0] == 0
    assert recs.tobytes() == o_recs[:3000].tobytes()
    hip_options(ADAPTER_BITSLICE_MIN=1, ABS_STAGES=2)
    det = scanner.factory()
    cfg = config.qcatConfig()
    kit = det._native_kit(det.layouts, cfg, native.ENDS_BOTH)
    got = det._context().scan_auto(kit, *native.pack_reads(reads[:3000]))
    assert got is not None and _front(det._context())[0] == 0
    arecs, slot = got
    assert kit.descriptor.kit_names[slot] == "PBC096"
    for name in ("barcode_idx", "exit_status", "adapter_end", "trim5p", "trim3p", "raw_score", "score_den"):
        assert np.array_equal(arecs[name], o_recs[name][:3000]), name


@pytest.mark.gpu
def test_detect_middle_batch(hip_options):
    """--detect-middle: the scan of the read ends is an ordinary big-batch scan and takes the kernel; the interior scan behind it
    packs its own windows and keeps k_abs_planes -- records against the oracle"""
    det = scanner.factory(kit="PBC096", scan_middle_adapter=True)
    d = det.descriptor(ends=native.ENDS_BOTH)
    assert d.scan_middle
    reads = _batch("both")[0][:2500]
    o_recs = oracle_lib.scan(d, reads, threads=16)
    hip_options(ADAPTER_BITSLICE_MIN=1, ABS_STAGES=2, BITSLICE_MIN=2048)
    ctx = native.NativeContext(0)
    recs = ctx.scan(native.NativeKit(d), *native.pack_reads(reads))
    assert _front(ctx)[0] == 2 * len(reads)
    bad = np.nonzero(recs != o_recs)[0]
    assert len(bad) == 0, (bad[:10], recs[bad[:3]], o_recs[bad[:3]])

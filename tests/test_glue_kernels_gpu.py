"""The two memory-side kernels in front of the adapter scan, at the shapes where they can go wrong: k_pack_windows
(csrc/kernels_common.inc: one thread per 32 codes, one workgroup per 64 windows, both sides in one instruction stream)
and k_abs_planes (csrc/kernels_abs.inc: tiles of 2048 read ends, slices of 64).  Everything is compared with the oracle,
record for record; the scans are ordinary ones (lazy byte windows, slim records), the way the benchmark runs them, plus a
debug scan for the per-template scores where the plane kernel is the subject.

Behind the scans, the hand-over of the barcode keys into read order (csrc/kernels_bitslice.inc: k_bs_select_ordered folds the
keys of a super-tile's barcode chunks; the binary16 kernels write the keys of the jobs outside the super-tiles): a PBC096
batch just above the switch to the bit-sliced kernels, where both kinds of kernel write keys, and a dual-kit batch whose
super-tiles are cut into several barcode chunks."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle_lib
import synth
from qcat_amd import native, scanner

_cache = {}


def _pbc096():
    if "det" not in _cache:
        _cache["det"] = scanner.factory(mode="epi2me", kit="PBC096")
    return _cache["det"]


def _ran(ctx):
    lib = native.HipLibrary.get().lib
    names = (C.c_char_p * 16)()
    ms = (C.c_float * 16)()
    return [names[i].decode() for i in range(lib.qcat_ctx_last_timing(ctx.handle, names, ms, 16))]


def _tile_batch():
    """3 * 2048 + 1 reads for 5'-only scans (one read end each) and their oracle records, computed once: a read's record
    does not depend on its neighbours, so every shorter batch is a prefix.  Some windows stay off the bit-sliced path
    (short, an N, lower case is fine), among them the last read end of every batch size tested."""
    if "tiles" not in _cache:
        det = _pbc096()
        n = 3 * 2048 + 1
        reads = synth.synth_batch(n, 20261019, det.layouts, 1, 0, error_rate=0.08)
        for i in range(5, n, 97):
            reads[i] = reads[i][:20 + i % 140] if i % 2 else reads[i][:33] + "N" + reads[i][34:]
        reads[2046] = reads[2046][:149]                                   # the last end of a batch of 2047: one code short
        reads[2048] = reads[2048][:149] + "N" + reads[2048][150:]         # the first end of the second tile: N in the window's last code
        d = det.descriptor(ends=native.ENDS_5P)
        o_recs, o_traces = oracle_lib.scan(d, reads, trace=True, threads=16)
        _cache["tiles"] = (reads, d, o_recs, o_traces)
    return _cache["tiles"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_ends", [2047, 2048, 2049, 3 * 2048 + 1])
def test_plane_kernel_at_tile_edges(n_ends, monkeypatch):
    """read-end counts one below, at and one above a tile of 2048, and three tiles and one end: a tile short of one end, a
    tile that holds a single read end"""
    reads, d, o_recs, o_traces = _tile_batch()
    bases, offsets = native.pack_reads(reads[:n_ends])
    monkeypatch.setenv("QCAT_HIP_ADAPTER_BITSLICE_MIN", "1")
    monkeypatch.setenv("QCAT_HIP_ABS_STAGES", "2")
    kit = native.NativeKit(d)
    lib = native.HipLibrary.get()
    for debug in (False, True):
        ctx = native.NativeContext(0)
        lib.check(lib.lib.qcat_ctx_set_timing(ctx.handle, 1))
        got = ctx.scan(kit, bases, offsets, trace=True) if debug else ctx.scan(kit, bases, offsets)
        assert "k_adapter_bitslice" in _ran(ctx)
        recs = got[0] if debug else got
        bad = np.nonzero(recs != o_recs[:n_ends])[0]
        assert len(bad) == 0, (debug, bad[:10], recs[bad[:3]], o_recs[bad[:3]])
        if debug:
            for name in ("window_len", "tpl_raw", "tpl_end", "best_tpl", "best_end"):
                assert np.array_equal(got[1][name], o_traces[name][:n_ends]), name


def _edge_reads():
    """reads of the lengths at which a window is shorter than, equal to or overlapping its partner, an N in the last code of
    either window, and between them reads trimmed so that the read starts fall on every byte alignment 0 .. 15"""
    det = _pbc096()
    base = synth.synth_batch(96, 77, det.layouts, 1, 0, error_rate=0.05)
    reads = []
    for i, n in enumerate((0, 1, 15, 16, 17, 149, 150, 151, 301)):
        reads.append(base[i][:n])
        reads.append(base[20 + i][-n:] if n else "")
    r = base[40][:400]
    reads.append(r[:149] + "N" + r[150:])                   # 5' window: the only other letter is its last code
    reads.append(r[:-150] + "N" + r[-149:])                 # 3' window (reverse complement of the last 150): the same
    reads.append(r[:149] + "n" + r[150:301])
    for i in range(48):
        reads.append(base[41 + i][:len(base[41 + i]) - (i * 7) % 16 - (1 if i % 5 == 0 else 0)])
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["one wave per alignment", "throughput kernels", "throughput kernels, eager byte windows",
                                  "bit-sliced adapter kernel"])
def test_pack_kernel_lengths_alignments_and_last_code(path, monkeypatch):
    """the readers of what k_pack_windows writes: the one-wave kernels (byte windows of every end), the binary16 kernels
    (win2, and byte windows of the flagged ends only -- the default for this kit -- or, with EAGER_BYTES, of every end: the
    kernel's other store path) and the bit-sliced adapter kernel (win2 and wspec through k_abs_planes)"""
    det = _pbc096()
    reads = _edge_reads()
    bases, offsets = native.pack_reads(reads)
    assert set(int(o) % 16 for o in offsets[:-1]) == set(range(16))
    for ends in (native.ENDS_BOTH, native.ENDS_5P):
        d = det.descriptor(ends=ends)
        key = ("edge", ends)
        if key not in _cache:
            _cache[key] = oracle_lib.scan(d, reads, counts=True, trace=True, threads=8)
        o_recs, o_cnt, o_traces = _cache[key][:3]
        if path == "bit-sliced adapter kernel":
            monkeypatch.setenv("QCAT_HIP_ADAPTER_BITSLICE_MIN", "1")
        if path == "throughput kernels, eager byte windows":
            monkeypatch.setenv("QCAT_HIP_EAGER_BYTES", "1")
        native.set_option("NO_TINY", None if path == "one wave per alignment" else 1)
        lib = native.HipLibrary.get()
        try:
            ctx = native.NativeContext(0)
            lib.check(lib.lib.qcat_ctx_set_timing(ctx.handle, 1))
            cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
            recs = ctx.scan(native.NativeKit(d), bases, offsets, counts=cnt)
            ran = _ran(ctx)
            tiny = lib.lib.qcat_ctx_tiny_ends(ctx.handle)
            ctx2 = native.NativeContext(0)
            lib.check(lib.lib.qcat_ctx_set_timing(ctx2.handle, 1))
            _r2, traces = ctx2.scan(native.NativeKit(d), bases, offsets, trace=True)[:2]
            ran2 = _ran(ctx2)
        finally:
            native.set_option("NO_TINY", None)
        # the path the label names is the one that ran: the one-wave kernels take every end or none, and only the third
        # path has the bit-sliced adapter kernel (which reads win2 and wspec; its ordinary scan keeps no byte windows)
        n_ends = len(reads) * (2 if ends == native.ENDS_BOTH else 1)
        assert tiny == (n_ends if path == "one wave per alignment" else 0), (path, tiny)
        for r in (ran, ran2):
            assert ("k_adapter_bitslice" in r) == (path == "bit-sliced adapter kernel"), (path, r)
        # the windows themselves, not only what the records keep of them: lengths, and every template's score and end
        # (a wrong last code, or an N the flags missed, moves these for the two reads that hold one there)
        for name in ("window_len", "tpl_raw", "tpl_end", "best_tpl", "best_end"):
            assert np.array_equal(traces[name], o_traces[name]), (path, ends, name)
        bad = np.nonzero(recs != o_recs)[0]
        assert len(bad) == 0, (path, ends, bad[:10], [len(reads[i]) for i in bad[:10]], recs[bad[:3]], o_recs[bad[:3]])
        assert _r2.tobytes() == o_recs.tobytes() and np.array_equal(cnt, o_cnt)


def _bitslice_tiles(ctx):
    lib = native.HipLibrary.get()
    tiles = (C.c_uint32 * 3)()
    lib.check(lib.lib.qcat_ctx_barcode_bitslice_tiles(ctx.handle, tiles))
    return sum(tiles)


@pytest.mark.gpu
def test_pbc096_batch_just_above_the_bit_sliced_switch(hip_options):
    """29 896 reads, 5' + 3': 59 792 jobs, the first batch size at or above 40 000 + 1 900 000 / 96 = 59 791.
    The default path takes the bit-sliced barcode kernels for the full super-tiles and the binary16 kernels for what those
    leave, so both write keys that end up in read order.  Records and counts against the oracle, and against the same batch
    with the bit-sliced kernels switched off (every key through the binary16 kernels and the existing select)."""
    det = _pbc096()
    n = (40000 + 1900000 // 96) // 2 + 1
    reads = synth.synth_batch(n, 59792, det.layouts, 1, 0, error_rate=0.08)
    d = det.descriptor(ends=native.ENDS_BOTH)
    o_recs, o_cnt = oracle_lib.scan(d, reads, counts=True, threads=16)
    bases, offsets = native.pack_reads(reads)
    kit = native.NativeKit(d)
    lib = native.HipLibrary.get()
    got = {}
    for bitslice in (True, False):
        hip_options(NO_BITSLICE=None if bitslice else 1)
        ctx = native.NativeContext(0)
        lib.check(lib.lib.qcat_ctx_set_timing(ctx.handle, 1))
        cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
        recs = ctx.scan(kit, bases, offsets, counts=cnt)
        ran = _ran(ctx)
        assert ("k_barcode_bitslice" in ran) == bitslice and "k_barcode_static" in ran, (bitslice, ran)
        assert (_bitslice_tiles(ctx) > 0) == bitslice
        got[bitslice] = (recs, cnt)
        bad = np.nonzero(recs != o_recs)[0]
        assert len(bad) == 0, (bitslice, bad[:10], recs[bad[:3]], o_recs[bad[:3]])
        assert np.array_equal(cnt, o_cnt)
    assert got[True][0].tobytes() == got[False][0].tobytes()


@pytest.mark.gpu
def test_dual_kit_batch_with_several_barcode_chunks_per_super_tile(hip_options, capfd):
    """the shipped dual kit, 3 000 reads forced onto the bit-sliced kernels: so few super-tiles that those of the 96-barcode
    second set are cut into barcode chunks, whose keys k_bs_select_ordered folds (maximum key: best raw, lowest index).  The
    unit log proves that units of more than one chunk ran; the records and counts are the oracle's."""
    det = scanner.factory(mode="dual")
    d = det.descriptor(ends=native.ENDS_BOTH)
    reads = synth.synth_batch(3000, 4004, det.layouts, 1, 0, error_rate=0.08)
    o_recs, o_cnt = oracle_lib.scan(d, reads, counts=True, threads=16)
    bases, offsets = native.pack_reads(reads)
    kit = native.NativeKit(d)
    assert kit.describe()["bitslice_groups"] == 0x40004
    lib = native.HipLibrary.get()
    hip_options(BITSLICE_MIN=2048, BITSLICE_PAD=128, BS_TRACE=1)
    ctx = native.NativeContext(0)
    lib.check(lib.lib.qcat_ctx_set_timing(ctx.handle, 1))
    cnt = np.zeros(d.n_count_buckets, dtype=np.int64)
    capfd.readouterr()
    recs = ctx.scan(kit, bases, offsets, counts=cnt)
    log = capfd.readouterr().err
    assert "k_barcode_bitslice" in _ran(ctx) and _bitslice_tiles(ctx) > 0
    chunks = sorted(set(int(m) for m in re.findall(r"bs units: launch +\d+ bin +\d+ chunks (\d+):", log)))
    assert chunks and chunks[-1] >= 2, (chunks, log[-2000:])
    bad = np.nonzero(recs != o_recs)[0]
    assert len(bad) == 0, (bad[:10], recs[bad[:3]], o_recs[bad[:3]])
    assert np.array_equal(cnt, o_cnt)

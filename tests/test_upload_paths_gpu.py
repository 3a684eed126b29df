"""The upload of a host-buffer call (csrc/batch_host.inc: batch_upload_windows) on every path it can take: the zero-copy view of
the pinned staging for up to 64 reads and the device view behind it, ragged reads around one and two windows in both input
forms (concatenated, and one pointer and one length per read), whole reads (FULL_UPLOAD, --detect-middle) compacted by the even
split and by the sliced schedule whose finished runs this thread sends on while the workers still copy, its refusals, and one
context whose staging grows and is then too big.  A characterisation: every case compares records and count vectors byte for
byte with the CPU oracle and with qcat_batch_upload + qcat_scan_resident of the same whole reads.

FULL_UPLOAD and NO_ZERO_COPY are A/B switches (csrc/options.h): a default build has neither -- their branches fold away at
compile time -- so the cases that set one run against a library built with -DQCAT_AB and skip, saying so, on a default build.
There the whole-read paths are reached through the --detect-middle kit, and the zero-copy boundary is run as it is.

Reads are generated once per kit; the big batches repeat them (a read's record does not depend on its neighbours, so the
oracle's records repeat the same way and its count vectors add up).  The fallback for more than a gigabyte of whole reads is
not run: it would take minutes and gigabytes."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
import synth
from qcat_amd import config, native, scanner

pytestmark = pytest.mark.gpu

N = 150                                                       # max_align_length of the shipped configuration
RAGGED = (0, 1, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 3 * N)
ERR_ARG = -1

_cache = {}


def _kits():
    """name -> (descriptor, distinct reads, oracle records, oracle counts)"""
    if "kits" in _cache:
        return _cache["kits"]
    assert config.qcatConfig().max_align_length == N
    pbc = scanner.factory(mode="epi2me", kit="PBC096")
    nbd = scanner.factory(mode="epi2me", kit="NBD103/NBD104")
    middle = scanner.factory(mode="epi2me", kit="NBD103/NBD104", scan_middle_adapter=True)
    pbc_reads = synth.synth_batch(300, 20261201, pbc.layouts, 1, 0, error_rate=0.08)
    pbc_reads[5], pbc_reads[6], pbc_reads[7] = "", "A", "N" * 200
    nbd_reads = synth.synth_batch(300, 20261202, nbd.layouts, len(nbd.layouts) - 1, 0, error_rate=0.08, no_adapter_fraction=0.2)
    # about 1050 bases per read (the sliced schedule is reached through volume); every third read of the --detect-middle kit a chimera
    long_pbc = synth.synth_batch(300, 20261203, pbc.layouts, 1, 0, error_rate=0.08, insert_len=950)
    long_pbc[5], long_pbc[6] = "", "A"
    half = synth.synth_batch(300, 20261204, nbd.layouts, len(nbd.layouts) - 1, 0, error_rate=0.08, no_adapter_fraction=0.2, insert_len=620)
    half[5], half[6] = "", "N" * 180
    chimeras = [half[i] + half[(i + 150) % 300] if i % 3 == 0 else half[i] for i in range(300)]
    long_half = synth.synth_batch(300, 20261205, nbd.layouts, len(nbd.layouts) - 1, 0, error_rate=0.08, no_adapter_fraction=0.2, insert_len=680)
    long_chimeras = [long_half[i] + long_half[(i + 150) % 300] if i % 3 == 0 else long_half[i] for i in range(300)]
    plan = {
        "pbc": (pbc.descriptor(ends=native.ENDS_BOTH), pbc_reads),
        "pbc_ragged": (pbc.descriptor(ends=native.ENDS_BOTH), _ragged(pbc_reads[10:])),
        "nbd5p_ragged": (nbd.descriptor(ends=native.ENDS_5P), _ragged(nbd_reads[10:])),
        "pbc_long": (pbc.descriptor(ends=native.ENDS_BOTH), long_pbc),
        "middle": (middle.descriptor(), chimeras),
        "middle_long": (middle.descriptor(), long_chimeras),
    }
    out = {}
    for name, (d, reads) in plan.items():
        o_recs, o_cnt = oracle_lib.scan(d, reads, counts=True, threads=16)
        out[name] = (d, reads, o_recs, o_cnt)
    assert out["middle"][0].scan_middle and np.count_nonzero(out["middle"][2]["exit_status"] == 997) > 0     # (interior adapters were found)
    assert np.count_nonzero(out["middle_long"][2]["exit_status"] == 997) > 0
    _cache["kits"] = out
    return out


def _ragged(reads):
    """ten reads of every length of RAGGED, the lengths interleaved (reads of at least 3 N bases cut short)"""
    src = [r for r in reads if len(r) >= 3 * N]
    assert len(src) >= 10 * len(RAGGED)
    return [src[i][:RAGGED[i % len(RAGGED)]] for i in range(10 * len(RAGGED))]


def _resident_scan(ctx, kit, reads):
    """qcat_batch_upload + qcat_scan_resident of the whole reads: (records, count vector)"""
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


def _host_scan(ctx, kit, reads):
    """qcat_scan_batch of the concatenated reads: (records, count vector)"""
    cnt = np.zeros(kit.descriptor.n_count_buckets, dtype=np.int64)
    recs = ctx.scan(kit, *native.pack_reads(reads), counts=cnt)
    return recs, cnt


def _equal(got, want, what):
    recs, cnt = got
    w_recs, w_cnt = want
    bad = np.nonzero(recs != w_recs)[0]
    assert len(bad) == 0, (what, bad[:10], recs[bad[:3]], w_recs[bad[:3]])
    assert recs.tobytes() == w_recs.tobytes(), what
    assert np.array_equal(cnt, w_cnt), what


def _switch(hip_options, **switches):
    """set A/B switches; a default build has none of them (csrc/options.h: build with -DQCAT_AB)"""
    missing = [name for name in switches if name not in native.options()]
    if missing:
        pytest.skip("this build of the library has no %s switch (A/B builds only: -DQCAT_AB)" % " / ".join(missing))
    hip_options(**switches)


def _zero_copy_case(n, hip_options, no_zero_copy):
    d, reads, o_recs, o_cnt = _kits()["pbc"]
    reads = reads[10:10 + n]
    kit = native.NativeKit(d)
    if no_zero_copy:
        _switch(hip_options, NO_ZERO_COPY=1)
    ctx = native.NativeContext(0)
    got = _host_scan(ctx, kit, reads)
    _equal(got, oracle_lib.scan(d, reads, counts=True), (n, no_zero_copy, "oracle"))
    _equal(got, _resident_scan(ctx, kit, reads), (n, no_zero_copy, "resident"))
    return got


@pytest.mark.parametrize("n", [1, 64, 65])
def test_zero_copy_boundary(n, hip_options):
    """up to 64 reads the kernels read the pinned staging in place, 65 reads go through the device staging"""
    _zero_copy_case(n, hip_options, None)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_zero_copy_boundary_against_copied_staging(n, hip_options):
    """NO_ZERO_COPY=1 sends the small batches through the device staging as well: the same bytes either way"""
    copied = _zero_copy_case(n, hip_options, 1)
    hip_options(NO_ZERO_COPY=None)
    in_place = _zero_copy_case(n, hip_options, None)
    assert in_place[0].tobytes() == copied[0].tobytes() and in_place[1].tobytes() == copied[1].tobytes()


@pytest.mark.parametrize("name", ["pbc_ragged", "nbd5p_ragged"])
def test_ragged_lengths_concatenated(name):
    """reads of 0, 1, n-1, n, n+1, 2n-1, 2n, 2n+1 and 3n bases: whole up to the kept length, head (and tail) beyond it"""
    d, reads, o_recs, o_cnt = _kits()[name]
    kit = native.NativeKit(d)
    ctx = native.NativeContext(0)
    got = _host_scan(ctx, kit, reads)
    _equal(got, (o_recs, o_cnt), (name, "oracle"))
    _equal(got, _resident_scan(ctx, kit, reads), (name, "resident"))


def _views(reads):
    """one pointer and one length per read (the pointers into one array that is returned with them and must stay alive)"""
    bases, offsets = native.pack_reads(reads)
    ptrs = (np.uint64(bases.ctypes.data) + offsets[:-1]).astype(np.uint64)
    lens = np.diff(offsets).astype(np.uint64)
    return bases, ptrs, lens


def _auto_ptrs(ctx, kit, ptrs, lens, n):
    """qcat_scan_batch_auto_ptrs: (return code, records, counts, voted kit slot)"""
    lib = native.HipLibrary.get().lib
    out = np.zeros(n, dtype=native.RESULT_DTYPE)
    cnt = np.zeros(kit.descriptor.n_count_buckets, dtype=np.int64)
    slot = C.c_int32(-1)
    rc = lib.qcat_scan_batch_auto_ptrs(ctx.handle, kit.handle, ptrs.tobytes(), lens.tobytes(), n, out.ctypes.data, cnt.ctypes.data,
                                       C.byref(slot), None, None)
    return rc, out, cnt, int(slot.value)


def _counts_in(full, sub, sub_cnt):
    """a count vector of descriptor `sub` (some of the kits of `full`) in the buckets of `full`:
    [barcode slots.., none][kit slots.., none][skipped]"""
    out = np.zeros(full.n_count_buckets, dtype=np.int64)
    nb_f, nb_s = len(full.slot_ids), len(sub.slot_ids)
    for i, sid in enumerate(sub.slot_ids):
        out[full.slot_ids.index(sid)] = sub_cnt[i]
    out[nb_f] = sub_cnt[nb_s]
    for i, name in enumerate(sub.kit_names):
        out[nb_f + 1 + full.kit_names.index(name)] = sub_cnt[nb_s + 1 + i]
    out[nb_f + 1 + len(full.kit_names)] = sub_cnt[nb_s + 1 + len(sub.kit_names)]
    out[-1] = sub_cnt[-1]
    return out


def _auto_case():
    """the kit-auto kit, the PBC096 ragged reads, their oracle records under the voted kit's templates, and what maps those
    onto the full template list"""
    if "auto" not in _cache:
        det = scanner.factory()
        cfg = config.qcatConfig()
        kit = det._native_kit(det.layouts, cfg, native.ENDS_BOTH)
        sub = det.get_adapters("PBC096")
        sub_desc = det.descriptor(layouts=sub, qcat_config=cfg)
        reads = _kits()["pbc_ragged"][1]
        o_recs, o_cnt = oracle_lib.scan(sub_desc, reads, counts=True, threads=16)
        full_index = np.array([det.layouts.index(l) for l in sub] + [-1])
        _cache["auto"] = (det, kit, sub_desc, reads, o_recs, o_cnt, full_index)
    return _cache["auto"]


def _auto_equal(recs, want, full_index, what):
    assert np.array_equal(full_index[want["adapter_idx"]], recs["adapter_idx"]), what
    for name in native.RESULT_DTYPE.names:
        if name != "adapter_idx":
            assert np.array_equal(want[name], recs[name]), (what, name)


def test_ragged_lengths_pointer_form():
    """the same ragged reads as one pointer and one length per read (qcat_scan_batch_auto_ptrs on the kit-auto kit: the reads
    vote for PBC096, the oracle and the resident scan use that kit's templates).  A kit that scans the 5' end only has no
    pointer form on the device: every entry point that takes pointers -- the two kit-auto calls and the file loops -- refuses
    a kit that was not made with ENDS_BOTH (the first assertion below holds that); tests/upload_check.cpp runs that
    combination on the host"""
    lib = native.HipLibrary.get().lib
    d5, reads5, _, _ = _kits()["nbd5p_ragged"]
    keep5, ptrs5, lens5 = _views(reads5)
    rc5, _, _, _ = _auto_ptrs(native.NativeContext(0), native.NativeKit(d5), ptrs5, lens5, len(reads5))
    assert rc5 == ERR_ARG and b"QCAT_ENDS_BOTH" in lib.qcat_last_error()
    det, kit, sub_desc, reads, o_recs, o_cnt, full_index = _auto_case()
    keep, ptrs, lens = _views(reads)
    ctx = native.NativeContext(0)
    rc, recs, cnt, slot = _auto_ptrs(ctx, kit, ptrs, lens, len(reads))
    assert rc == 0 and kit.descriptor.kit_names[slot] == "PBC096"
    _auto_equal(recs, o_recs, full_index, "oracle")
    assert np.array_equal(cnt, _counts_in(kit.descriptor, sub_desc, o_cnt))
    r_recs, r_cnt = _resident_scan(ctx, native.NativeKit(sub_desc), reads)
    _auto_equal(recs, r_recs, full_index, "resident")
    assert np.array_equal(cnt, _counts_in(kit.descriptor, sub_desc, r_cnt))
    # ... and the concatenated form of the same call
    got = ctx.scan_auto(kit, *native.pack_reads(reads))
    assert got is not None and got[1] == slot and got[0].tobytes() == recs.tobytes()
    del keep


@pytest.mark.parametrize("name,options", [("pbc", {"FULL_UPLOAD": 1}), ("middle", {"MIDDLE_ABS_MIN": 1})])
def test_whole_reads_even_split(name, options, hip_options):
    """about 300 whole reads: FULL_UPLOAD=1, and a --detect-middle kit on reads with chimeras"""
    d, reads, o_recs, o_cnt = _kits()[name]
    _switch(hip_options, **{k: v for k, v in options.items() if k == "FULL_UPLOAD"})
    hip_options(**{k: v for k, v in options.items() if k != "FULL_UPLOAD"})
    kit = native.NativeKit(d)
    ctx = native.NativeContext(0)
    got = _host_scan(ctx, kit, reads)
    _equal(got, (o_recs, o_cnt), (name, "oracle"))
    _equal(got, _resident_scan(ctx, kit, reads), (name, "resident"))


@pytest.mark.parametrize("name,options", [("pbc_long", {"FULL_UPLOAD": 1}), ("middle_long", {})])
def test_whole_reads_sliced_schedule(name, options, hip_options):
    """at least 36 MiB of whole reads: slices of 8 MiB that host threads draw from a counter while the calling thread sends every
    finished run of slices to the device"""
    if len(os.sched_getaffinity(0)) < 2:
        pytest.skip("the sliced schedule needs 2 host threads")
    _switch(hip_options, **options)
    d, uniq, o_recs, o_cnt = _kits()[name]
    per = sum(len(r) for r in uniq)
    times = (36 << 20) // per + 1
    reads = uniq * times
    assert sum(len(r) for r in uniq) * times >= 36 << 20 and len(reads) < 60000
    want = (np.concatenate([o_recs] * times), o_cnt * times)
    kit = native.NativeKit(d)
    ctx = native.NativeContext(0)
    got = _host_scan(ctx, kit, reads)
    _equal(got, want, (name, "oracle"))
    _equal(got, _resident_scan(ctx, kit, reads), (name, "resident"))


def test_refusals_leave_the_context_usable():
    """decreasing offsets, offsets[0] != 0 and a null pointer with a length: QCAT_ERR_ARG, and the next call on the same
    context returns what a fresh context returns"""
    lib = native.HipLibrary.get().lib
    d, reads, o_recs, o_cnt = _kits()["pbc"]
    reads = reads[:200]
    kit = native.NativeKit(d)
    fresh = _host_scan(native.NativeContext(0), kit, reads)
    _equal(fresh, oracle_lib.scan(d, reads, counts=True, threads=16), "oracle")
    bases, offsets = native.pack_reads(reads)
    out = np.zeros(len(reads), dtype=native.RESULT_DTYPE)
    ctx = native.NativeContext(0)
    _equal(_host_scan(ctx, kit, reads), fresh, "before")

    decreasing = offsets.copy()
    decreasing[100], decreasing[101] = decreasing[101], decreasing[100]
    assert decreasing[101] < decreasing[100]
    assert lib.qcat_scan_batch(ctx.handle, kit.handle, bases.ctypes.data, decreasing.ctypes.data, len(reads), out.ctypes.data, None) == ERR_ARG
    assert b"non-decreasing" in lib.qcat_last_error()
    _equal(_host_scan(ctx, kit, reads), fresh, "after decreasing offsets")

    shifted = offsets.copy()
    shifted[0] = 1
    assert lib.qcat_scan_batch(ctx.handle, kit.handle, bases.ctypes.data, shifted.ctypes.data, len(reads), out.ctypes.data, None) == ERR_ARG
    assert b"offsets[0] must be 0" in lib.qcat_last_error()
    _equal(_host_scan(ctx, kit, reads), fresh, "after offsets[0] != 0")

    # the pointer form on the kit-auto kit
    det, akit, sub_desc, areads, a_recs, a_cnt, full_index = _auto_case()
    keep, ptrs, lens = _views(areads)
    actx = native.NativeContext(0)
    rc, first, first_cnt, slot = _auto_ptrs(actx, akit, ptrs, lens, len(areads))
    assert rc == 0
    broken = ptrs.copy()
    at = int(np.nonzero(lens)[0][3])
    broken[at] = 0
    rc, _, _, _ = _auto_ptrs(actx, akit, broken, lens, len(areads))
    assert rc == ERR_ARG and b"null read pointer" in lib.qcat_last_error()
    rc, again, again_cnt, slot2 = _auto_ptrs(actx, akit, ptrs, lens, len(areads))
    assert rc == 0 and slot2 == slot and again.tobytes() == first.tobytes() and np.array_equal(again_cnt, first_cnt)
    rc, other, other_cnt, slot3 = _auto_ptrs(native.NativeContext(0), akit, ptrs, lens, len(areads))
    assert rc == 0 and slot3 == slot and again.tobytes() == other.tobytes() and np.array_equal(again_cnt, other_cnt)
    del keep


def test_growing_calls_on_one_context():
    """50 reads (the zero-copy view), 5000 (the device staging grows), 50 again (the zero-copy view after the device view, in a
    staging that is now too big)"""
    d, uniq, o_recs, o_cnt = _kits()["pbc"]
    kit = native.NativeKit(d)
    ctx = native.NativeContext(0)
    small = uniq[20:70]
    want_small = oracle_lib.scan(d, small, counts=True)
    whole, rest = divmod(5000, len(uniq))
    part = oracle_lib.scan(d, uniq[:rest], counts=True, threads=16)
    big = uniq * whole + uniq[:rest]
    want_big = (np.concatenate([o_recs] * whole + [part[0]]), o_cnt * whole + part[1])
    for step, (reads, want) in enumerate(((small, want_small), (big, want_big), (small, want_small))):
        _equal(_host_scan(ctx, kit, reads), want, step)

"""The end of a bit-sliced barcode on the device: after a barcode's row loops k_bs_barcode (kernels_bitslice.inc) takes the
raw score from the last row's codes and the deficit (bs_core.h: bs_last_row) and hands the best (score, index) planes over
as keys (bs_keys32).  tests/test_bs_epilogue_host.py checks that arithmetic against what it replaced; here whole batches
run through the kernels -- the generated ones and the letters-from-memory ones -- against the oracle, with the reads the
last row decides mixed into an ordinary batch:
  * regions that START inside the upstream context or the barcode (extra bases behind the barcode: the region is cut from the
    adapter's end) and regions that END inside the downstream context or the barcode (bases missing behind the barcode; the
    adapter only survives the bigger gap in dual mode, which cuts regions whatever the adapter scores) -- one of the two is
    the leading context of the walk, the other one its end, where the best path ends in the last row;
  * hybrid reads that tie two barcodes at a positive score (the smallest index must win through the keys);
  * full 150-base windows without an adapter that hold a target at the window's very end, whole and cut off up to 15
    bases before its end (beyond the trailing context: the best path ends in the last row inside the barcode's own columns);
  * low-complexity ends, where the best raw score is 0 or close to it.
Batches of 2 048 - 6 000 reads are forced onto the bit-sliced path (BITSLICE_MIN=2048, BITSLICE_PAD=128: the smallest
super-tile, as tests/geometry_cases.py does), records -- and on the debug scan every trace field and per-barcode row --
compared exactly."""
import random

import numpy as np
import pytest

import geometry_cases as gc
import synth
from qcat_amd import config, jit, native, scanner

gpu = pytest.mark.gpu
needs_compiler = pytest.mark.skipif(jit.compiler() is None, reason="neither libhiprtc nor hipcc available")

EXT = config.qcatConfig().extracted_barcode_extension
WINDOW = config.qcatConfig().max_align_length


@pytest.fixture(scope="module", autouse=True)
def _contexts_released_after_the_module():
    yield
    gc.release()
    import gc as collector
    collector.collect()


def _acgt(rng, n):
    return "".join(synth._BASES[rng.below(4)] for _ in range(n))


def shifted_reads(layouts, tpl, n, seed, shift):
    """error-free reads whose adapter has `shift` bases too many (> 0: random ones) or too few (< 0) right behind the barcode:
    the barcode region is cut from the adapter's end, so it lies `shift` bases off the barcode -- behind it (the region starts
    inside the leading context or the barcode) or in front of it (the region ends inside the barcode).  Returns (reads, where
    the barcode starts in each read)"""
    lay = layouts[tpl]
    e = lay.barcode_pos_1.end
    out, starts = [], []
    for i in range(n):
        rng = synth.SplitMix64(seed, i)
        seq = synth.fill(lay, rng.below(1 << 16), 0)
        lead = 14 + rng.below(20)                     # (room for the extension in front: the region keeps its nominal length)
        mid = _acgt(rng, shift) if shift > 0 else ""
        rest = seq[e + 1:] if shift > 0 else seq[e + 1 - shift:]
        out.append(_acgt(rng, lead) + seq[:e + 1] + mid + rest + _acgt(rng, 220))
        starts.append(lead + lay.barcode_pos_1.start)
    return out, starts


def window_end_reads(layouts, tpl, n, seed, context=11):
    """reads without an adapter whose first WINDOW bases END with a target (context + barcode + context) -- whole, or cut off
    up to 15 bases before its end: the whole window is the barcode region and the best path ends in its last row"""
    lay = layouts[tpl]
    s, e = lay.barcode_pos_1.start, lay.barcode_pos_1.end
    out = []
    for i in range(n):
        rng = synth.SplitMix64(seed, i)
        seq = synth.fill(lay, rng.below(1 << 16), 0)
        target = seq[max(0, s - context):e + 1 + context]
        cut = (i % 4) * (1 + rng.below(5))
        out.append(_acgt(rng, WINDOW - len(target) + cut) + target + _acgt(rng, 250))
    return out


def low_complexity_reads(n, seed):
    """ends of one, two or three repeated letters: every barcode scores next to nothing"""
    out = []
    for i in range(n):
        rng = synth.SplitMix64(seed, i)
        unit = _acgt(rng, 1 + i % 3)
        out.append((unit * 400)[:300 + rng.below(100)])
    return out


def epilogue_batch(layouts, tpl, n, seed, hybrid=True):
    """an ordinary batch of n reads at 8 % errors plus the reads the last row decides; returns (reads, {kind: slice},
    {kind of shifted reads: where the barcode starts in each})"""
    reads = gc.batch(layouts, n, seed, t5=tpl, t3=tpl)
    kinds, bstart = {}, {}

    def add(kind, more):
        kinds[kind] = slice(len(reads), len(reads) + len(more))
        reads.extend(more)
    for q, (kind, shift) in enumerate((("ends_in_context", -6), ("ends_in_barcode", -(EXT + 3)), ("starts_in_context", 6), ("starts_in_barcode", EXT + 2))):
        more, where = shifted_reads(layouts, tpl, 160, seed + 10 + q, shift)
        add(kind, more)
        bstart[kind] = np.array(where)
    if hybrid:
        add("hybrid", gc.hybrid_reads(layouts, tpl, 400, seed + 4))
    add("window_end", window_end_reads(layouts, tpl, 200, seed + 5))
    add("low_complexity", low_complexity_reads(200, seed + 6))
    return reads, kinds, bstart


def expect_kinds(want, kinds, bstart, ends, in_barcode=25):
    """the conditions that keep the special reads from passing empty, from the ORACLE's traces of the 5' ends"""
    tr = want.traces[::ends]
    start, length, raw = tr["region_start"][:, 0], tr["region_len"][:, 0], tr["bc_raw"][:, 0]
    stats = {}
    for kind, sl in kinds.items():
        stats[kind] = (int((length[sl] == WINDOW).sum()), int((raw[sl] <= 0).sum()), int(np.median(length[sl])), sl.stop - sl.start)
    print("kind: (full windows, best raw <= 0, median region length, reads) %s" % stats)
    n_full = stats["window_end"][0]
    assert n_full >= 0.9 * stats["window_end"][3], stats                  # no adapter found: the whole window is the region
    assert (raw[kinds["window_end"]] >= 20).sum() >= 0.5 * n_full, stats   # ... and the target at its end is found there
    assert stats["low_complexity"][1] >= 20, stats
    # regions cut behind the barcode's start / the context's start, from the oracle's region and the read's construction
    regional = length < WINDOW
    sl, at = kinds["starts_in_context"], bstart["starts_in_context"]
    assert (regional[sl] & (start[sl] > at - 11) & (start[sl] <= at)).sum() >= 150, stats
    sl, at = kinds["starts_in_barcode"], bstart["starts_in_barcode"]
    assert (regional[sl] & (start[sl] > at)).sum() >= in_barcode, stats      # (13 extra bases: not every adapter survives them)
    return stats


def run(kit, want, hip_options, static=True):
    paths = [("bs_memory", None), ("raw", None)] + ([("bs_static", None)] if static else [])
    results = gc.check(kit, want, paths=paths, setter=hip_options)
    bad = gc.failures(results)
    assert not bad, "\n".join("%s: %s" % (p, "; ".join(v)) for (p, _), v in bad.items())


@gpu
def test_pbc096_ends_the_last_row_decides(hip_options):
    layouts = scanner.factory(kit="PBC096").layouts
    d = gc.descriptor(layouts)
    reads, kinds, bstart = epilogue_batch(layouts, 0, 2400, 96)
    want = gc.Want(d, reads, threads=16)
    expect_kinds(want, kinds, bstart, 2)
    assert gc.tie_stats(gc.Want(d, reads[kinds["hybrid"]], threads=16))[2] >= 20       # ends tied at a positive score
    kit = native.NativeKit(d)
    assert kit.describe()["bitslice_groups"] == 0x20002
    run(kit, want, hip_options)


@gpu
def test_a_twelve_barcode_kit(hip_options):
    """twelve barcodes: a unit has idle waves, so the two contexts' columns come from producer waves beside the row loops
    and the tail (what bs_last_row starts from) is published last"""
    layouts = scanner.factory(kit="RBK004").layouts
    d = gc.descriptor(layouts)
    reads, kinds, bstart = epilogue_batch(layouts, 0, 2400, 12)
    want = gc.Want(d, reads, threads=16)
    expect_kinds(want, kinds, bstart, 2)
    kit = native.NativeKit(d)
    assert kit.describe()["bitslice_groups"] == 0x10001
    run(kit, want, hip_options)


@gpu
def test_the_dual_kit(hip_options):
    layouts = scanner.factory(mode="dual").layouts
    d = gc.descriptor(layouts, mode="dual")
    reads, kinds, bstart = epilogue_batch(layouts, 1, 2400, 2, hybrid=False)
    want = gc.Want(d, reads, threads=16)
    # dual mode cuts the region whatever the adapter scores: the regions of the reads with bases missing behind the barcode
    # end inside the barcode, at the nominal length
    tr = want.traces[::2]
    sl = kinds["ends_in_barcode"]
    end = tr["region_start"][sl, 0] + tr["region_len"][sl, 0]
    nominal = 2 * EXT + layouts[1].get_barcode_length(0) + 1
    assert ((end < bstart["ends_in_barcode"] + layouts[1].get_barcode_length(0)) & (tr["region_len"][sl, 0] == nominal)).sum() >= 100
    kit = native.NativeKit(d)
    info = kit.describe()
    assert info["n_static_groups"] == info["n_groups"] == 4 and info["bitslice_groups"] == 0x40004, info
    run(kit, want, hip_options)


@gpu
@needs_compiler
def test_a_generated_kit_with_targets_of_63_columns(tmp_path_factory, hip_options):
    """11 + 41 + 11 columns, the longest target the score planes hold: error-free reads score 63 = raw + 64 of 127"""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("QCAT_AMD_JIT_CACHE", str(tmp_path_factory.mktemp("jit_cache")))
        layouts = gc.single_kit(random.Random(63), 6, blen=41, up=25, dn=30)
        d = gc.descriptor(layouts)
        assert gc.bs_shapes(d) == [(False, 11, 41, 11)]
        reads, kinds, bstart = epilogue_batch(layouts, 0, 1400, 63)
        expect_kinds(gc.Want(d, reads, threads=16), kinds, bstart, 2, in_barcode=0)
        reads += gc.batch(layouts, 1000, 64, error_rate=0.0, no_adapter_fraction=0.0)
        want = gc.Want(d, reads, threads=16)
        assert (want.traces["bc_raw"][:, 0] == 63).sum() >= 1000
        gc.compile_kits([(d, ("NO_ABS",))])
        kit = gc.generated_kit(d, ("NO_ABS",))
        info = kit.describe()
        assert info["n_static_groups"] == 1 and info["bitslice_groups"] == 0x10001, info
        run(kit, want, hip_options)
    finally:
        mp.undo()

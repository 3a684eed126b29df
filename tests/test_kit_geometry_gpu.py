"""Parity over KIT geometry and barcode ties on every kernel family (cases and path runner: tests/geometry_cases.py).

The other GPU modules vary the reads; here the kit varies: partial, permuted and reversed sets of a built-in barcode
family (built-in chains bound by hash in case order, keys carry the kit's index; four-target chains with pairs and half
pairs left over), set sizes around the host's thresholds up to the 1024 of the key's index field, sets that name one
sequence twice (the arg-max rule -- first index wins unless the maximum is exactly 0 -- rides in the low bits of a key
through every merge step), reads that put two different barcodes on one positive score, and seven small custom kits on run-time
generated kernels (doubled sets, heterogeneous set sizes, barcode and flank lengths over the bit-sliced kernels' shapes).  Every (kit, reads) pair has ONE oracle result; each device path is compared with it -- records byte
for byte, counts, and on debug scans every trace field and per-barcode row -- and proves that it ran.  Every tie case
asserts its tie share from the oracle's rows before the device runs.

The geometries that need a compile EACH (every set size 1 .. 130, every own-column count, target and template length, the
templates' bit-sliced adapter plans at 13 s of compile time per template) are tools/fuzz_geometry.py's; its output is
profiles/kit_geometry_sweep.txt."""
import importlib.util
import os
import random

import pytest

import geometry_cases as gc
from qcat_amd import config, jit, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
needs_compiler = pytest.mark.skipif(jit.compiler() is None, reason="neither libhiprtc nor hipcc available")


@pytest.fixture(scope="module", autouse=True)
def _contexts_released_after_the_module():
    yield
    gc.release()
    import gc as collector
    collector.collect()


def expect_clean(results):
    assert results, "no path ran"
    bad = gc.failures(results)
    assert not bad, "\n".join("%s chunk %s: %s" % (p, c, "; ".join(v)) for (p, c), v in bad.items())


def paths_of(results):
    return {p for p, _ in results}


# ---- tier A: the built-in kernels, no compile --------------------------------------------------------------------------------
SUBSETS = gc.pbc096_subsets()


def test_one_barcode_less_leaves_whole_quads_a_pair_and_a_half_pair():
    """what the 95-barcode cases rest on, from the generator's own lists: all 48 pairs of the PBC096 family sit inside
    four-target chains, so any one barcode removed leaves 23 whole quads, one whole pair and one half pair"""
    spec = importlib.util.spec_from_file_location("gen_static_kernels", os.path.join(ROOT, "tools", "gen_static_kernels.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    import collections
    fams, _, _, members = gen.collect()
    lay = gc.subset_layouts(range(96))[0]
    n = config.qcatConfig().barcode_context_length
    up, dn = lay.get_upstream_context(n, 0), lay.get_downstream_context(n, 0)
    targets = fams[(up, dn, len(up) + 24 + len(dn))]
    assert sorted(targets) == sorted(up + b.sequence + dn for b in lay.get_barcode_set(0))
    groups = collections.OrderedDict()
    for t in targets:
        groups.setdefault(frozenset(members[t]), []).append(t)
    pairs, in_quads = [], 0
    for grp in groups.values():
        first = len(pairs)
        pairs.extend(gen.pair_up(grp, len(up)))
        in_quads += 2 * len([i for i in range(first, len(pairs) - 1, 2) if pairs[i][0] != pairs[i][1] and pairs[i + 1][0] != pairs[i + 1][1]])
    assert len(targets) >= gen.QUAD_MIN_TARGETS and len(pairs) == 48 and in_quads == 48
    assert all(a != b for a, b, _ in pairs)


@pytest.fixture(scope="module")
def family_reads():
    """3000 reads of the WHOLE family (made once: the generator is pure Python): to a partial set most of them carry a barcode
    the kit does not hold, so the arg-max runs over middling scores where indices tie"""
    return gc.batch(gc.subset_layouts(range(96)), 3000, 1000)


@gpu
@pytest.mark.parametrize("name", sorted(SUBSETS))
def test_subsets_and_permutations_of_a_builtin_family(name, family_reads, hip_options):
    picks = SUBSETS[name]
    d = gc.descriptor(gc.subset_layouts(picks))
    kit = native.NativeKit(d)
    info = kit.describe()
    assert info["n_static_groups"] == info["n_groups"] == 1 and info["bitslice_groups"] == 0x10001 and info["packed"] == 1, info
    ends = sorted({0, len(picks) // 2, len(picks) - 1})
    reads = family_reads + gc.forced_reads(d.layouts, 0, ends, 7, per=8)
    want = gc.Want(d, reads, threads=16)
    assert set(ends) <= set(int(b) for b in want.recs["barcode_idx"])             # the set's first, middle and last index are called
    results = gc.check(kit, want, setter=hip_options)
    assert {"raw", "key", "table", "bs_static", "bs_memory", "tiny", "generic", "default"} <= paths_of(results)
    expect_clean(results)

@gpu
@pytest.mark.parametrize("n2", [49, 95])
def test_partial_second_set_of_the_dual_kit(n2, hip_options):
    d = gc.descriptor(gc.dual_subset_layouts(n2), mode="dual")
    kit = native.NativeKit(d)
    info = kit.describe()
    assert info["n_static_groups"] == info["n_groups"] == 4 and info["bitslice_groups"] == 0x40004, info
    want = gc.Want(d, gc.batch(d.layouts, 3000, 2000 + n2, t5=1, t3=0))
    results = gc.check(kit, want, setter=hip_options)
    assert {"raw", "key", "bs_static", "bs_memory", "tiny", "default"} <= paths_of(results)
    expect_clean(results)
    # the merged small-batch launch (k_barcode_multi: two or more bound groups, a few hundred tiles at most)
    small = gc.Want(d, want.reads[:600] + want.reads[-5:])
    expect_clean(gc.check(kit, small, paths=[("default", None), ("key", None), ("key", 2), ("key", 6), ("raw", None)], setter=hip_options))


TIE_SETS = gc.tie_sets()


def expect_ties(want, share, share_pos):
    """the conditions that keep a tie case from passing empty, from the ORACLE's rows"""
    n, tied, tied_pos, wrong = gc.tie_stats(want)
    assert n >= 0.9 * len(want.reads) * want.ends - 12, (n, len(want.reads))      # (nearly every end has barcode scores at all)
    assert tied >= share * n and tied_pos >= share_pos * n, (n, tied, tied_pos)
    assert wrong == 0, "the oracle does not call the smallest tied index on %d tied ends" % wrong


@gpu
@pytest.mark.parametrize("name", sorted(TIE_SETS))
def test_sets_that_name_a_barcode_twice(name, hip_options):
    """a built-in family's barcodes with repeats: the registry binds no chain to such a set, so the table kernels, the
    one-wave kernels and the int32 fallback decide the ties (the bit-sliced kernels need bound chains: tier B)"""
    seq, _ = gc.pbc096()
    d = gc.descriptor([gc.layout("REPEATS", seq, TIE_SETS[name])])
    kit = native.NativeKit(d, jit=False)
    info = kit.describe()
    assert info["n_static_groups"] == 0 and info["bitslice_groups"] == 0x1 and info["packed"] == 1, info
    want = gc.Want(d, gc.batch(d.layouts, 800, 3000, no_adapter_fraction=0.0))
    if name == "triple20":
        expect_ties(want, 0.1, 0.1)                   # (three of 20 indices hold the repeated barcode: the share of reads that carry it, 3 / 20)
    else:
        expect_ties(want, 0.9, 0.8)
    results = gc.check(kit, want, setter=hip_options)
    assert {"raw", "default", "tiny", "generic"} <= paths_of(results)
    expect_clean(results)


@gpu
@pytest.mark.parametrize("error_rate", [0.0, 0.08])
def test_hybrid_reads_tie_two_barcodes_at_a_positive_score(error_rate, hip_options):
    """the barcode region is the first half of one barcode joined to the second half of another: two different targets
    reach one positive score on the 5' end (measured with the oracle: 12.7 % of such reads tie, against none of 1000 plain
    reads; the 3' end of a read without an adapter there ties at low scores in both batches and is left out)"""
    d = gc.descriptor(gc.subset_layouts(range(96)), ends=native.ENDS_5P)
    kit = native.NativeKit(d)
    assert kit.describe()["n_static_groups"] == 1
    plain = gc.Want(d, gc.batch(d.layouts, 1000, 41, t3=-1, error_rate=error_rate, no_adapter_fraction=0.0))
    hybrid = gc.Want(d, gc.hybrid_reads(d.layouts, 0, 5000, 42, error_rate=error_rate) + gc.edge_reads(d.layouts, 0))
    (p_share, _), (h_share, h_pos) = gc.tie_share(plain), gc.tie_share(hybrid)
    print("tie share: plain %.4f, hybrid %.4f (%.4f at a positive maximum)" % (p_share, h_share, h_pos))
    assert h_share >= 5 * p_share, (p_share, h_share)
    assert h_pos * len(hybrid.reads) >= 100, h_pos                                   # (... and enough tied ends at a positive score to bite)
    assert gc.tie_stats(hybrid)[3] == 0
    results = gc.check(kit, hybrid, setter=hip_options)
    assert {"raw", "key", "table", "bs_static", "bs_memory", "tiny", "generic"} <= paths_of(results)
    expect_clean(results)


# ---- the ends of the range -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [129, 1024])
def test_sets_beyond_the_bit_sliced_range(n, hip_options):
    """129: one more than the bit-sliced kernels take; 1024: the last index the key's ten bits hold (1023 - b must not wrap)"""
    d = gc.descriptor(gc.single_kit(random.Random(n), n))
    kit = native.NativeKit(d, jit=False)
    info = kit.describe()
    assert info["packed"] == 1 and info["bitslice_groups"] == 0 and info["n_static_groups"] == 0, info
    reads = gc.forced_reads(d.layouts, 0, [0, n // 2, n - 1], 17, per=20) + gc.batch(d.layouts, 100 if n > 200 else 300, n)
    want = gc.Want(d, reads)
    called = set(int(b) for b in want.recs["barcode_idx"])
    assert {0, n // 2, n - 1} <= called, sorted(called)[:5]
    results = gc.check(kit, want, setter=hip_options)
    assert {"raw", "default", "tiny", "generic"} <= paths_of(results)
    expect_clean(results)


def test_what_the_device_path_refuses_stays_refused():
    rng = random.Random(5)
    with pytest.raises(RuntimeError, match="error -2: barcode set too large"):
        native.NativeKit(gc.descriptor(gc.single_kit(rng, 1025)), jit=False)
    with pytest.raises(RuntimeError, match="error -2: barcode target length 65"):
        native.NativeKit(gc.descriptor(gc.shape_kit(rng, 11, 43, 11)), jit=False)
    assert native.NativeKit(gc.descriptor(gc.shape_kit(rng, 11, 42, 11)), jit=False).describe()["n_groups"] == 1     # (64: the last that fits)
    with pytest.raises(RuntimeError, match="error -1: template 0: length must be in 1..128"):
        native.NativeKit(gc.descriptor(gc.single_kit(rng, 6, tlen=129)), jit=False)
    assert native.NativeKit(gc.descriptor(gc.single_kit(rng, 6, tlen=128)), jit=False).describe()["packed"] == 1


def test_a_64_column_target_stays_off_the_bit_sliced_kernels():
    """their score counters hold up to 63 and a 64-column target read without an error scores 64 (kit.h BS_MAX_TARGET)"""
    d64 = gc.descriptor(gc.full_width_kit())
    assert gc.bs_shapes(d64) == [None]
    assert native.NativeKit(d64, jit=False).describe()["bitslice_groups"] == 0
    d63 = gc.descriptor(gc.single_kit(random.Random(63), 12, blen=41, up=25, dn=30))
    assert gc.bs_shapes(d63) == [(False, 11, 41, 11)] and native.NativeKit(d63, jit=False).describe()["bitslice_groups"] == 1


@gpu
@needs_compiler
def test_reads_without_an_error_of_a_64_column_target(generated_kits, hip_options):
    """the reduced case of what the sweep found: on the bit-sliced kernels every read that matched a 64-column target letter
    for letter came back with a wrapped score (59, 46 ... for 64) and so with another barcode or none.  Error-free reads, a big
    batch with the bit-sliced path forced: the set now runs its generated binary16 chains there"""
    d, switches = generated_kits["WIDTH64"]
    want = gc.Want(d, gc.batch(d.layouts, 3000, 64, error_rate=0.0, no_adapter_fraction=0.0))
    assert (want.traces["bc_raw"][:, 0] == 64).sum() >= 0.8 * len(want.traces)
    kit = gc.generated_kit(d, switches)
    info = kit.describe()
    assert info["n_static_groups"] == 1 and info["bitslice_groups"] == 0, info
    for opts in ({"BITSLICE_MIN": 2048, "BITSLICE_PAD": 128}, {"BITSLICE_MIN": 2048, "BITSLICE_PAD": 128, "NO_BS_STATIC": 1}):
        hip_options(**opts)
        expect_clean(gc.check(kit, want, paths=[("key", None), ("default", None), ("raw", None)], setter=hip_options))
        hip_options(**{k: None for k in opts})


def classless_kits():
    """(name, descriptor) of kits one of whose lengths has no width class: the whole kit runs on the general kernel"""
    out = []
    for tlen in (65, 75, 93):
        out.append(("template%d" % tlen, gc.descriptor(gc.single_kit(random.Random(tlen), 6, tlen=tlen))))
    cfg = config.qcatConfig()
    cfg.barcode_context_length = 3
    out.append(("target31", gc.descriptor(gc.single_kit(random.Random(31), 6, blen=25), cfg=cfg)))
    return out


def test_lengths_without_a_width_class_leave_the_packed_path():
    for name, d in classless_kits():
        assert native.NativeKit(d, jit=False).describe()["packed"] == 0, name


@gpu
def test_lengths_without_a_width_class_match_the_oracle_on_the_general_kernel(hip_options):
    for name, d in classless_kits():
        kit = native.NativeKit(d, jit=False)
        assert kit.describe()["packed"] == 0, name
        want = gc.Want(d, gc.batch(d.layouts, 300, 65))
        results = gc.check(kit, want, setter=hip_options)
        assert paths_of(results) == {"generic", "default"}
        expect_clean(results)


# ---- tier B: run-time generated kernels ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated_kits(tmp_path_factory):
    """the custom kits' sources generated up front and compiled side by side (one child process per kit) into one code-object
    cache that the module's CPU and GPU tests share: the wall time is the longest compile, not the sum"""
    mp = pytest.MonkeyPatch()
    if not os.environ.get("QCAT_AMD_JIT_CACHE"):
        mp.setenv("QCAT_AMD_JIT_CACHE", str(tmp_path_factory.mktemp("jit_cache")))
    kits = {name: (gc.descriptor(make()), switches) for name, (make, switches) in list(gc.GENERATED.items()) + list(gc.EXTRA.items())}
    seconds = gc.compile_kits(list(kits.values()))
    print("compiled %d kits in %.1f s (%s)" % (len(kits), seconds, jit.compiler()))
    yield kits
    mp.undo()


@needs_compiler
def test_generated_kernels_bind_every_group_of_the_custom_kits(generated_kits):
    for name in sorted(gc.GENERATED):
        d, switches = generated_kits[name]
        no_bs = "NO_BS" in switches
        plain = native.NativeKit(d, jit=False).describe()
        ng = len(d.layouts)
        assert plain["packed"] == 1 and plain["n_static_groups"] == 0 and plain["bitslice_groups"] == ng, (name, plain)
        _, _, _, entries, quads = gc.generate(d, switches)
        info = gc.generated_kit(d, switches).describe()
        assert info["n_static_groups"] == info["n_groups"] == ng and info["n_static_templates"] == ng, (name, info)
        assert info["bitslice_groups"] == ng * (0x1 if no_bs else 0x10001), (name, info)
        for g, lay in enumerate(d.layouts):
            bcs = [b.sequence for b in lay.get_barcode_set(0)]
            if len(bcs) >= jit.QUAD_MIN_TARGETS:
                assert quads[2 * g] and entries[2 * g], (name, g)                    # four-target chains AND pairs left over
            else:
                assert not quads[2 * g]
            # no chain runs a barcode beside its copy (two equal targets would share every column and one score register)
            for _, a, b in entries[2 * g]:
                assert b < 0 or bcs[a] != bcs[b], (name, a, b)
            for _, a1, a2, b1, b2 in quads[2 * g]:
                assert bcs[a1] != bcs[a2] and bcs[b1] != bcs[b2], (name, a1, a2, b1, b2)
            covered = sorted([x for e in entries[2 * g] for x in e[1:] if x >= 0] + [x for q in quads[2 * g] for x in q[1:]])
            assert covered == list(range(len(bcs))), (name, g)
    assert sum(1 for d, _ in generated_kits.values() for lay in d.layouts if len(lay.get_barcode_set(0)) >= jit.QUAD_MIN_TARGETS) >= 3
    # the LENGTHS kits hold every own-column count and target length they were made for, all with a bit-sliced form
    shapes = [sh for name in sorted(gc.GENERATED) if name.startswith("LENGTHS") for sh in gc.bs_shapes(generated_kits[name][0])]
    assert None not in shapes and {(sh[2], sh[0]) for sh in shapes} >= {(c, r) for c in gc.LENGTHS_OWN for r in (False, True)}
    lengths = {sum(sh[1:]) for sh in shapes}
    assert lengths >= set(gc.LENGTHS_TARGETS), sorted(lengths)


@gpu
@needs_compiler
@pytest.mark.parametrize("name", sorted(gc.GENERATED))
def test_custom_kits_on_generated_and_table_kernels(name, generated_kits, hip_options):
    d, switches = generated_kits[name]
    no_bs = "NO_BS" in switches
    nt = len(d.layouts)
    reads = []
    for t in range(nt):
        reads += gc.batch(d.layouts, 3000 // nt + 300, 500 + t, t5=t, t3=t, no_adapter_fraction=0.0)
    want = gc.Want(d, reads, threads=16)
    used = want.traces["used_tpl"]
    for t in range(nt):                             # every template is used by >= 10 % of the read ends
        assert (used == t).sum() >= 0.1 * len(used), (t, (used == t).sum())
    if name.startswith("TIES"):
        expect_ties(want, 0.9, 0.8)
    kit = gc.generated_kit(d, switches)
    info = kit.describe()
    assert info["n_static_groups"] == info["n_groups"] == nt and info["bitslice_groups"] == nt * (0x1 if no_bs else 0x10001), info
    results = gc.check(kit, want, setter=hip_options)
    assert {"raw", "key", "table", "bs_memory", "tiny", "generic", "default"} <= paths_of(results)
    assert ("bs_static" in paths_of(results)) == (not no_bs)
    expect_clean(results)
    # a small batch (the merged launch k_barcode_multi is for built-in chains only -- packed_host.inc asks for static_kernel <
    # QCAT_JIT_BASE -- so a generated kit's groups run as launches of their own here, side by side)
    small = gc.Want(d, [r for t in range(nt) for r in reads[t * (len(reads) // nt):][:600 // nt]] + reads[-5:])
    expect_clean(gc.check(kit, small, paths=[("default", None), ("key", None), ("key", 2), ("key", 6), ("raw", None)], setter=hip_options))
    table = native.NativeKit(d, jit=False)
    assert table.describe()["n_static_groups"] == 0
    expect_clean(gc.check(table, want, paths=[("raw", None), ("raw", 2), ("raw", 6), ("default", None)], setter=hip_options))

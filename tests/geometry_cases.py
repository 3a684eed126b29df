"""Kits, read batches and the path runner of the kit-geometry parity sweep (tests/test_kit_geometry_gpu.py in the
suite, tools/fuzz_geometry.py by hand).  No tests here.

The reads of the other GPU modules vary; the KIT barely does.  This module builds the kits the device code branches
on -- set sizes around the host thresholds, permuted and partial sets of a built-in family, barcode / flank / template
lengths at the edges of the width classes, sets that name one sequence twice -- and runs one (kit, reads) pair down every
device path, each against ONE oracle result: records byte for byte, counts, and on a debug scan every trace field and
every per-barcode row.  Every path proves that it ran (kit binding, timing ring, diagnostics counters)."""
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib
import synth
from qcat_amd import adapters, config, jit, native, scanner

TINY_MAX_WAVES = 20000          # csrc/kernels_tiny.inc: alignments up to which a batch takes the one-wave kernels


# ---- kits ----------------------------------------------------------------------------------------------------------------
def layout(kit, sequence, set1, set2=None, trim_offset=0):
    """an AdapterLayout as a kit file of the reference's format would give it (adapters.read_adapter_layout)"""
    def rows(bcs):
        return [{"name": "barcode%02d" % (i + 1), "id": i + 1, "sequence": s, "fwd_strand": True} for i, s in enumerate(bcs)]
    return adapters._layout_from_dict({"kit": kit, "auto_detect": False, "description": "geometry case", "sequence": sequence,
                                       "trim_offset": trim_offset, "barcode_set_1": rows(set1),
                                       "barcode_set_2": rows(set2) if set2 else []})


def descriptor(layouts, mode="epi2me", ends=native.ENDS_BOTH, cfg=None):
    return native.KitDescriptor(layouts, cfg or config.qcatConfig(), mode=mode, ends=ends)


def random_barcodes(rng, n, length=24):
    """n DISTINCT random barcodes"""
    out = []
    while len(out) < n:
        b = "".join(rng.choice("ACGT") for _ in range(length))
        if b not in out:
            out.append(b)
    return out


def random_flank(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def pbc096():
    """(template sequence, the 96 barcodes) of the shipped PBC096 kit"""
    lay = scanner.factory(kit="PBC096").layouts[0]
    return lay.sequence, [b.sequence for b in lay.get_barcode_set(0)]


def subset_kit(tmp_path, picks):
    """a kit folder holding PBC096's template with the barcodes `picks` of its set, through the YAML loader"""
    import yaml
    seq, bcs = pbc096()
    rows = [{"name": "barcode%02d" % (i + 1), "id": i + 1, "sequence": bcs[p], "fwd_strand": True} for i, p in enumerate(picks)]
    data = {"kit": "SUBSET", "auto_detect": False, "description": "subset", "sequence": seq, "trim_offset": 0,
            "barcode_set_1": rows, "barcode_set_2": []}
    (tmp_path / "s.yml").write_text(yaml.safe_dump(data))
    return scanner.factory(kit="SUBSET", kit_folder=str(tmp_path))


def subset_layouts(picks):
    seq, bcs = pbc096()
    return [layout("SUBSET", seq, [bcs[p] for p in picks])]


PBC_SIZES = (1, 2, 3, 13, 24, 25, 32, 33, 47, 48, 49, 95)


def pbc096_subsets():
    """{name: picks}: first-k and one random subset per size, the set reversed, shuffled, and 50 of the shuffled order"""
    cases = {}
    for k in PBC_SIZES:
        cases["first%d" % k] = list(range(k))
        cases["random%d" % k] = random.Random(9600 + k).sample(range(96), k)
    cases["reversed96"] = list(range(95, -1, -1))
    shuffled = list(range(96))
    random.Random(96).shuffle(shuffled)
    cases["shuffled96"] = shuffled
    cases["shuffled50"] = shuffled[:50]
    return cases


def dual_subset_layouts(n2):
    """the shipped dual kit's templates with set 1 whole and the first n2 barcodes of the 96 of set 2"""
    out = []
    for lay in scanner.factory(mode="dual").layouts:
        s1 = [b.sequence for b in lay.get_barcode_set(0)]
        s2 = [b.sequence for b in lay.get_barcode_set(1)]
        out.append(layout(lay.kit, lay.sequence, s1, s2[:n2], trim_offset=lay.trim_offset))
    return out


def doubled(distinct, form):
    """a set in which every entry of `distinct` is present twice: the copy next to it ("adjacent"), half a set away
    ("half") or mirrored, i / n-1-i ("mirror")"""
    k = len(distinct)
    if form == "adjacent":
        return [distinct[i // 2] for i in range(2 * k)]
    if form == "half":
        return list(distinct) + list(distinct)
    if form == "mirror":
        return list(distinct) + list(distinct)[::-1]
    raise ValueError(form)


def tie_sets():
    """{name: barcode list} of PBC096 barcodes with repeats: 10, 25 and 64 distinct entries doubled in the three forms, one
    barcode at 0, n/2 and n-1, and a set of one sequence throughout"""
    _, bcs = pbc096()
    cases = {}
    for k in (10, 25, 64):
        for form in ("adjacent", "half", "mirror"):
            cases["%dx2_%s" % (k, form)] = doubled(bcs[:k], form)
    triple = list(bcs[:20])
    triple[10] = triple[19] = triple[0]
    cases["triple20"] = triple
    cases["equal20"] = [bcs[7]] * 20
    return cases


def near_duplicates(rng, base):
    """`base` plus one copy each with one base changed at the last, the first and a middle position"""
    out = []
    for pos in (len(base) - 1, 0, len(base) // 2):
        other = rng.choice([c for c in "ACGT" if c != base[pos]])
        out.append(base[:pos] + other + base[pos + 1:])
    return out


FLANK5, FLANK3 = "GGTGCTGAT", "TTAACCTTTCTGTTGGTGCTGATATTGCAA"          # template = FLANK5 + barcode + FLANK3: 63 columns with 24-nt barcodes


def custom_template(rng, blen, tlen=None, up=None, dn=None):
    """a template of random flanks around one barcode placeholder; `tlen` = its whole length, `up` / `dn` = flank lengths"""
    if tlen is not None:
        up = min(11, (tlen - blen) // 2) if up is None else up
        dn = tlen - blen - up
    return random_flank(rng, up) + "N" * blen + random_flank(rng, dn)


def sizes_kit(seed=1):
    """SIZES: five templates with sets of 1, 3, 25, 49 and 50 random 24-nt barcodes"""
    rng = random.Random(seed)
    return [layout("SIZES", custom_template(rng, 24, up=11 + i % 3, dn=20 + 2 * i), random_barcodes(rng, n)) for i, n in enumerate((1, 3, 25, 49, 50))]


def ties20_kit(seed=2):
    """TIES20: a 20-entry set in which every entry is present twice (mirrored, i / n-1-i): seven random barcodes and three
    near-duplicates of the first of them (its last, first, middle base changed: shared prefix m - 1, 0, m / 2)"""
    rng = random.Random(seed)
    base = random_barcodes(rng, 7)
    return [layout("TIES20", FLANK5 + "N" * 24 + FLANK3, doubled(base + near_duplicates(rng, base[0]), "mirror"))]


def ties50_kit(seed=3):
    """TIES50: 25 barcodes doubled half a set apart: four-target chains and left-over pairs with equal targets in different chains"""
    rng = random.Random(seed)
    return [layout("TIES50", "CCGTGACAGT" + "N" * 24 + "AGAGTTTGATCATGGCTCAGGATTCA", doubled(random_barcodes(rng, 25), "half"))]


LENGTHS_OWN = (20, 21, 27, 33, 40, 47, 48)            # own-column counts of the bit-sliced kernels, each forward and reversed
LENGTHS_TARGETS = (32, 40, 41, 56, 57, 63)             # target lengths: edges of the width classes, 0 and 8 padding columns; 63: the
                                                       # longest the bit-sliced kernels take (64: full_width_kit, on the binary16 chains)


def template_has_class(n):
    """does a template of n columns have an adapter width class (40 .. 128 with up to 8 padding columns; none for 65 .. 75, 93 .. 95)"""
    return 32 <= n <= 64 or 76 <= n <= 92 or 96 <= n <= 128


def lengths_shapes():
    """[(upstream flank, barcode length, downstream flank)], at most 16: a cover of LENGTHS_OWN in both directions and of
    LENGTHS_TARGETS, by jit._bs_shape.  The context length is
    11: a flank of 11 context columns is made 25 letters or more (the target keeps 11 of them), so that the flanks carry
    the template's score (normalisation denominator 5 x flanks - barcode >= 60) and every template wins its own reads"""
    need = {("own", c, r) for c in LENGTHS_OWN for r in (False, True)} | {("m", m) for m in LENGTHS_TARGETS}
    cands = []
    for up in (0, 3, 4, 6, 7, 8, 11):
        for dn in (0, 3, 4, 6, 7, 8, 11):
            for blen in range(10, 54):
                m = up + blen + dn
                if not 32 <= m <= 64:
                    continue
                flanks = [(u, v) for u in ([up] if up < 11 else range(25, 40)) for v in ([dn] if dn < 11 else range(25, 40))
                          if template_has_class(u + blen + v) and 5 * (u + v) - blen >= 60]
                if flanks:
                    shape = jit._bs_shape(up, dn, m)
                    cands.append(((flanks[0][0], blen, flanks[0][1]), {("m", m), ("none",) if shape is None else ("own", shape[2], shape[0])}))
    out = []
    # first the shapes that serve an own-column count AND a target length, then what is left
    for both in (True, False):
        for c in cands:
            if c[1] <= need if both else c[1] & need:
                need -= c[1]
                out.append(c[0])
    assert not need and len(out) <= 16, (out, sorted(need))
    return out


def lengths_kit(part=None, seed=5):
    """LENGTHS: one template of 6 barcodes per shape of lengths_shapes(); `part` 0 .. 3: four of them (every own-column count is
    an instantiation of the bit-sliced kernels and 5 s of compile time: four kits compile side by side in a quarter of it)"""
    rng = random.Random(seed)
    lays = [layout("LENGTHS", random_flank(rng, up) + "N" * blen + random_flank(rng, dn), random_barcodes(rng, 6, length=blen))
            for up, blen, dn in lengths_shapes()]
    return lays if part is None else lays[part::4]


def shape_kit(rng, up, blen, dn, n=6, name="SHAPE"):
    """one template whose barcode has flanks of exactly `up` and `dn` letters (context length 11: a shorter flank shortens
    the context), so that jit._bs_shape gives a chosen (direction, shared, own, trailing) split"""
    return [layout(name, random_flank(rng, up) + "N" * blen + random_flank(rng, dn), random_barcodes(rng, n, length=blen))]


TEMPLATE_LENGTHS = (32, 40, 41, 60, 61, 64, 76, 92, 96, 104, 121, 128)


def templates_kit(seed=4):
    """TEMPLATES: template lengths at the edges of the adapter width classes, 6 barcodes each"""
    rng = random.Random(seed)
    return [layout("TEMPLATES", custom_template(rng, 24, tlen=t), random_barcodes(rng, 6)) for t in TEMPLATE_LENGTHS]


def single_kit(rng, n, blen=24, tlen=None, up=9, dn=30, name="CUSTOM"):
    """one template with a set of n random barcodes; `tlen`: its whole length (the downstream flank takes what `up` leaves)"""
    if tlen is not None:
        up = min(up, (tlen - blen) // 2)
    return [layout(name, custom_template(rng, blen, tlen=tlen, up=up, dn=dn), random_barcodes(rng, n, length=blen))]


def bs_shapes(d):
    """per (template, set) group of descriptor `d`: jit._bs_shape -- (reversed, shared, own, trailing columns) or None"""
    n = int(d.desc.barcode_context_length)
    out = []
    for lay in d.layouts:
        for s in range(2 if d.mode == "dual" else 1):
            bs = lay.get_barcode_set(s)
            if bs:
                up, dn = lay.get_upstream_context(n, s), lay.get_downstream_context(n, s)
                out.append(jit._bs_shape(len(up), len(dn), len(up) + len(bs[0].sequence) + len(dn)))
    return out


# ---- reads ---------------------------------------------------------------------------------------------------------------
def _acgt(rng, n):
    return "".join(synth._BASES[rng.below(4)] for _ in range(n))


def edge_reads(layouts, tpl, seed=5):
    """"", a read shorter than the barcode, a read of exactly the window, an N run inside the barcode, a lower-case read"""
    rng = synth.SplitMix64(seed, 0)
    lay = layouts[tpl]
    full = _acgt(rng, 12) + synth.fill(lay, 1, 1) + _acgt(rng, 300)
    s = 12 + lay.barcode_pos_1.start
    blen = lay.get_barcode_length(0)
    n_run = full[:s + blen // 3] + "N" * min(4, blen) + full[s + blen // 3 + min(4, blen):]
    return ["", full[12:12 + max(1, blen - 3)], full[:config.qcatConfig().max_align_length], n_run, full.lower()]


def batch(layouts, n, seed, t5=0, t3=0, error_rate=0.08, **kw):
    """synth_batch at 8 % errors (a shorter insert than its default: the generator is pure Python) plus the edge reads"""
    kw.setdefault("insert_len", 200)
    return synth.synth_batch(n, seed, layouts, t5, t3, error_rate=error_rate, **kw) + edge_reads(layouts, t5)


def forced_reads(layouts, tpl, picks, seed, per=12, error_rate=0.08):
    """reads whose true barcode is one of `picks`"""
    return [synth.synth_read(i, seed, layouts, tpl, tpl, error_rate=error_rate, insert_len=200, force_barcode=b, force_bare=False)
            for i in range(per) for b in picks]


def hybrid_reads(layouts, tpl, n, seed, error_rate=0.0, cut=None):
    """reads whose barcode region is the first part of barcode a joined to the rest of barcode b (a != b, cut at `cut`,
    default the middle): two different targets reach one positive score"""
    lay = layouts[tpl]
    bcs = [b.sequence for b in lay.get_barcode_set(0)]
    s, blen = lay.barcode_pos_1.start, lay.get_barcode_length(0)
    cut = blen // 2 if cut is None else cut
    thr = synth.rate_threshold(error_rate)
    out = []
    for i in range(n):
        rng = synth.SplitMix64(seed, i)
        a = rng.below(len(bcs))
        b = (a + 1 + rng.below(len(bcs) - 1)) % len(bcs)
        tpl_seq = lay.get_adapter_sequences()
        seq = tpl_seq[:s] + bcs[a][:cut] + bcs[b][cut:] + tpl_seq[s + blen:]
        read = [_acgt(rng, 5 + rng.below(36))]
        synth._mutate(rng, seq, thr, read)
        read.append(_acgt(rng, 200))
        out.append("".join(read))
    return out


# ---- the oracle, ties ------------------------------------------------------------------------------------------------------
class Want(object):
    """the oracle's answer for one (kit, reads): computed once, shared by every path"""

    def __init__(self, d, reads, threads=8):
        self.d, self.reads = d, reads
        self.packed = native.pack_reads(reads)
        self.recs, self.cnt, self.traces, self.rows = oracle_lib.scan(d, packed=self.packed, counts=True, trace=True, rows=True, threads=threads)
        self.ends = 1 if d.ends == native.ENDS_5P else 2

    def head(self, n):
        """the same for the first n reads (the one-wave kernels take small batches only)"""
        w = Want.__new__(Want)
        w.d, w.reads, w.ends = self.d, self.reads[:n], self.ends
        w.packed = native.pack_reads(w.reads)
        w.recs, w.traces, w.rows = self.recs[:n], self.traces[:n * self.ends], self.rows[:n * self.ends]
        w.cnt = oracle_lib.scan(self.d, packed=w.packed, counts=True)[1]
        return w


def tie_stats(want):
    """over the read ends (and sets) the oracle aligned barcodes for: (n, tied at the maximum, tied at a maximum > 0, ties
    where the oracle did NOT call the smallest tied index although the maximum is not 0)"""
    rows = want.rows.astype(np.int32)
    valid = rows != -32768
    n = tied = tied_pos = wrong = 0
    mx = np.where(valid, rows, -(1 << 30)).max(axis=2)
    for s in range(rows.shape[1]):
        has = valid[:, s, :].any(axis=1)
        at_max = valid[:, s, :] & (rows[:, s, :] == mx[:, s][:, None])
        t = has & (at_max.sum(axis=1) >= 2)
        first = at_max.argmax(axis=1)
        n += int(has.sum())
        tied += int(t.sum())
        tied_pos += int((t & (mx[:, s] > 0)).sum())
        wrong += int((t & (mx[:, s] != 0) & (want.traces["bc_idx"][:, s] != first)).sum())
    return n, tied, tied_pos, wrong


def tie_share(want):
    """(share of barcode-aligned read ends whose maximum is shared by two or more indices, the same with a maximum > 0)"""
    n, tied, tied_pos, _ = tie_stats(want)
    return (tied / float(n), tied_pos / float(n)) if n else (0.0, 0.0)


# ---- device paths ----------------------------------------------------------------------------------------------------------
_state = {}


def lib():
    return native.HipLibrary.get().lib


def context(generic=False):
    """one context with the timing ring on (and one made under FORCE_GENERIC=1) per process"""
    key = "generic" if generic else "ctx"
    if key not in _state:
        if generic:
            native.set_option("FORCE_GENERIC", 1)                # (read when a context is created)
        try:
            c = native.NativeContext(0)
        finally:
            if generic:
                native.set_option("FORCE_GENERIC", None)
        native.HipLibrary.get().check(lib().qcat_ctx_set_timing(c.handle, 1))
        _state[key] = c
    return _state[key]


def release():
    """give the contexts back (the suite does at the end of the module: nothing of it stays alive beside the modules that follow)"""
    _state.clear()


def ring(ctx):
    names = (C.c_char_p * 16)()
    ms = (C.c_float * 16)()
    return [names[i].decode() for i in range(lib().qcat_ctx_last_timing(ctx.handle, names, ms, 16))]


def set_options(**kw):
    for name, value in kw.items():
        native.set_option(name, value)


def diff(got, want, debug):
    """what differs between a device result and the oracle's, as a list of strings (empty: nothing)"""
    out = []
    recs, cnt, traces, rows = got
    bad = np.nonzero(recs != want.recs)[0]
    if recs.tobytes() != want.recs.tobytes():
        out.append("records of reads %s: %s != %s" % (bad[:5], recs[bad[:2]], want.recs[bad[:2]]))
    if not np.array_equal(cnt, want.cnt):
        out.append("counts")
    if debug:
        for name in native.TRACE_DTYPE.names:
            if not np.array_equal(traces[name], want.traces[name]):
                b = np.nonzero(np.asarray(traces[name] != want.traces[name]).reshape(len(traces), -1).any(axis=1))[0]
                out.append("trace %s of ends %s: %s != %s" % (name, b[:5], traces[name][b[:2]], want.traces[name][b[:2]]))
        if not np.array_equal(rows, want.rows):
            b = np.nonzero((rows != want.rows).reshape(len(rows), -1).any(axis=1))[0]
            out.append("per-barcode rows of ends %s" % b[:5])
    return out


def tiny_reads(d, n_reads):
    """how many reads of a batch stay under the one-wave kernels' limit of alignments"""
    maxb = max(len(lay.get_barcode_set(s) or []) for lay in d.layouts for s in (0, 1))
    per_end = len(d.layouts) + maxb * (2 if d.mode == "dual" else 1)
    ends = 1 if d.ends == native.ENDS_5P else 2
    return max(1, min(n_reads, 4096 // ends, (TINY_MAX_WAVES - 1000) // (per_end * ends)))


#: path -> (library options, debug scan?)
PATHS = {
    "raw": ({}, True),                                            # raw-score mode: a debug scan wants every per-barcode row
    "key": ({"SUMMARY": 1}, False),                                # key mode: (raw, 1023 - index) keys, merged by max
    "default": ({}, False),                                        # what the product does with this batch (merged small-batch launch)
    "table": ({"NO_STATIC": 1}, True),                             # the table kernels
    "bs_static": ({"BITSLICE_MIN": 2048, "BITSLICE_PAD": 128}, False),
    "bs_memory": ({"BITSLICE_MIN": 2048, "BITSLICE_PAD": 128, "NO_BS_STATIC": 1}, False),
    "tiny": ({"NO_TINY": None}, True),                             # one wave per alignment
    "tiny_records": ({"NO_TINY": None}, False),
    "generic": ({}, True),                                         # the int32 fallback
    "abs2": ({"ADAPTER_BITSLICE_MIN": 1, "ABS_STAGES": 2}, True),  # bit-sliced adapter plans, two stages / four stages
    "abs4": ({"ADAPTER_BITSLICE_MIN": 1, "ABS_STAGES": 4}, True),
}


def run_path(path, kit, want, chunk=None, setter=set_options):
    """scan want.reads with `kit` on `path`, prove that the path ran, return diff() against the oracle.  `chunk`:
    QCAT_HIP_CHUNK_BARCODES; `setter(**options)`: how options are set (the suite's hip_options fixture, or set_options)."""
    opts, debug = PATHS[path]
    opts = dict(opts)
    if chunk is not None:
        opts["CHUNK_BARCODES"] = chunk
    if path.startswith("tiny"):
        want = want.head(tiny_reads(want.d, len(want.reads)))
    info = kit.describe()
    bound = info["n_static_groups"] == info["n_groups"] and info["packed"] == 1
    ctx = context(generic=(path == "generic"))
    saved = {name: native.get_option(name) for name in opts}
    setter(**opts)
    try:
        ring(ctx)
        cnt = np.zeros(want.d.n_count_buckets, dtype=np.int64)
        bases, offsets = want.packed
        if debug:
            recs, traces, rows = ctx.scan(kit, bases, offsets, counts=cnt, trace=True, rows=True)
        else:
            recs, traces, rows = ctx.scan(kit, bases, offsets, counts=cnt), None, None
        ran = ring(ctx)
        tiny = lib().qcat_ctx_tiny_ends(ctx.handle)
        tiles = (C.c_uint32 * 3)()
        native.HipLibrary.get().check(lib().qcat_ctx_barcode_bitslice_tiles(ctx.handle, tiles))
    finally:
        setter(**saved)
    problems = diff((recs, cnt, traces, rows), want, debug)
    proof = "ring %s tiny %d tiles %s info %s" % (ran, tiny, list(tiles), info)
    if path.startswith("tiny"):
        ok = tiny == len(want.reads) * want.ends
    elif path == "generic":
        ok = "k_scan_generic" in ran
    elif info["packed"] != 1:
        ok = "k_scan_generic" in ran
    elif path.startswith("bs_"):
        ok = "k_barcode_bitslice" in ran and sum(tiles) > 0 and tiny == 0
    elif path.startswith("abs"):
        ok = "k_adapter_bitslice" in ran and tiny == 0
    elif path == "table" or not bound:
        ok = "k_barcode_packed" in ran and tiny == 0
    else:
        ok = "k_barcode_static" in ran and "k_barcode_packed" not in ran and tiny == 0
    if not ok:
        problems.append("path %s did not run: %s" % (path, proof))
    return problems


def paths_for(kit, d, n_reads, adapter_plans=False):
    """[(path, chunk)] a kit can take with a batch of n_reads reads; `adapter_plans`: also the templates' bit-sliced plans"""
    info = kit.describe()
    out = []
    if info["packed"] != 1:
        return [("generic", None), ("default", None)]
    bound = info["n_static_groups"] == info["n_groups"]
    for chunk in (None, 2, 6):
        out.append(("raw", chunk))
        if bound:
            out.append(("key", chunk))
    out += [("default", None), ("tiny", None), ("tiny_records", None), ("generic", None)]
    if adapter_plans and info["bitslice_templates"] > 0:
        out += [("abs2", None), ("abs4", None)]
    if bound:
        out.append(("table", None))
        ends = 1 if d.ends == native.ENDS_5P else 2
        if info["bitslice_groups"] & 0xFFFF and n_reads * ends >= 3000:
            out.append(("bs_memory", None))
            if info["bitslice_groups"] >> 16:
                out.append(("bs_static", None))
    return out


def check(kit, want, paths=None, setter=set_options):
    """{(path, chunk): problems} over `paths` (default: paths_for); the values are all empty when the device equals the oracle"""
    if paths is None:
        paths = paths_for(kit, want.d, len(want.reads))
    return {pc: run_path(pc[0], kit, want, chunk=pc[1], setter=setter) for pc in paths}


def failures(results):
    return {k: v for k, v in results.items() if v}


# ---- run-time generated kernels: compile several kits side by side -----------------------------------------------------------
#: name -> (layouts, jit.generate switches): QCAT_AMD_JIT_NO_BS leaves the letters-compiled-in bit-sliced barcode kernels out (a
#: second of compile time per barcode; the kit's bit-sliced units then run the letters-from-memory form), QCAT_AMD_JIT_NO_ABS the
#: bit-sliced adapter plans (13 s per template; tests/test_jit.py and the sweep tool's template section run those)
GENERATED = {"TIES20": (ties20_kit, ()), "TIES50": (ties50_kit, ("NO_BS",)), "SIZES": (sizes_kit, ("NO_BS", "NO_ABS")),
             "LENGTHS0": (lambda: lengths_kit(0), ("NO_ABS",)), "LENGTHS1": (lambda: lengths_kit(1), ("NO_ABS",)),
             "LENGTHS2": (lambda: lengths_kit(2), ("NO_ABS",)), "LENGTHS3": (lambda: lengths_kit(3), ("NO_ABS",))}


def full_width_kit():
    """targets of 64 columns, the most a kit may have (11 + 42 + 11): one more than the bit-sliced kernels' counters hold"""
    return single_kit(random.Random(64), 12, blen=42, up=25, dn=30, name="WIDTH64")


#: compiled along with them, for tests of their own
EXTRA = {"WIDTH64": (full_width_kit, ("NO_ABS",))}


class _switches(object):
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = {k: os.environ.get("QCAT_AMD_JIT_" + k) for k in ("NO_BS", "NO_ABS")}
        for k in self.before:
            if k in self.on:
                os.environ["QCAT_AMD_JIT_" + k] = "1"
            else:
                os.environ.pop("QCAT_AMD_JIT_" + k, None)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            os.environ.pop("QCAT_AMD_JIT_" + k, None)
            if v is not None:
                os.environ["QCAT_AMD_JIT_" + k] = v


def generate(d, switches=()):
    with _switches(switches):
        return jit.generate(d)


def generated_kit(d, switches=()):
    """NativeKit with its kernels generated, compiled (or taken from the cache) and attached"""
    with _switches(switches):
        return native.NativeKit(d, jit=True)


def compile_kits(kits, workers=8):
    """generate the sources of `kits` -- [(descriptor, switches)] -- and compile them into the code-object cache
    (jit.cache_dir()), so that generated_kit() finds its code there: one child process per kit (jit.compile_source there,
    the compiler this process would use; `workers` at a time), so the wall time is the longest compile, not the sum.
    Returns the seconds it took."""
    t0 = time.time()
    sources = [generate(d, switches)[0] for d, switches in kits]
    root = os.path.dirname(os.path.dirname(os.path.abspath(jit.__file__)))
    child = "import sys; sys.path.insert(0, %r); from qcat_amd import jit; jit.compile_source(open(sys.argv[1]).read())" % root
    with tempfile.TemporaryDirectory(prefix="qcat_geometry_") as tmp:
        def one(job):
            i, src = job
            path = os.path.join(tmp, "kit%d.hip" % i)
            with open(path, "w") as fh:
                fh.write(src)
            proc = subprocess.run([sys.executable, "-c", child, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            return None if proc.returncode == 0 else "kit %d: %s" % (i, proc.stdout.decode(errors="replace")[-2000:])
        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            failed = [f for f in pool.map(one, enumerate(sources)) if f]
    if failed:
        raise RuntimeError("compile failed:\n" + "\n".join(failed))
    return time.time() - t0

#!/usr/bin/env python3
"""Parity sweep over KIT geometry on the GPU box (the suite's tests/test_kit_geometry_gpu.py over the whole range; cases and
path runner: tests/geometry_cases.py): for every kit one batch (synthetic reads at 8 % errors plus the degenerate ones), ONE
oracle result, and every device path the kit can take against it -- binary16 chains in raw-score and in key mode with
units of the default size, 2 and 6 barcodes, table kernels, both bit-sliced letter forms, the one-wave kernels, the int32
fallback -- records, counts, and on debug scans every trace field and per-barcode row.  Sections:

    builtin     partial / permuted / reversed sets of the PBC096 family and of the dual kit's second set (built-in kernels)
    ties        sets that name a barcode twice at n = 20, 50, 96, 128 (three placements of the copy), on the table kernels and
                -- compiled -- on generated chains and bit-sliced kernels
    sizes       custom sets of --sizes barcodes (default 1 .. 130 and 1024)
    own         every own-column count 20 .. 48 of the bit-sliced barcode kernels, forward and reversed, both letter forms,
                and 49 (no bit-sliced form; fewer than 20 cannot occur: a target of the packed path has 32 columns or more, at
                most 11 of them shared, and trailing columns are only split off while 20 own ones remain)
    targets     every target length 31 .. 65 (31: no width class, general kernel; 65: refused)
    templates   every template length 31 .. 129 (the gaps 65 .. 75 and 93 .. 95: general kernel; 129: refused), with the bit-sliced
                adapter plans of the generated kits forced in both forms, and the twelve-template kit TEMPLATES, which must hold a
                two-stage, a four-narrow and a four-wide plan

A kit outside the built-in bundle runs with jit=False (table kernels) and -- every kit of the ties and own sections, every
--jit-every'th of the others -- on kernels generated for it (compiled side by side into the code-object cache first: QCAT_AMD_JIT_CACHE, so a re-run is cheap;
sets of more than --bs-static-max barcodes leave the letters-compiled-in bit-sliced kernel out, QCAT_AMD_JIT_NO_BS, and only
the template section compiles bit-sliced adapter plans, QCAT_AMD_JIT_NO_ABS elsewhere).
One line per kit (geometry, paths run, mismatches), a summary line, exit status 1 on any mismatch.

    python tools/fuzz_geometry.py [--sections builtin,ties,...] [--sizes 1:131,1024] [--templates 31:130] [--jit-every 1] [--reads 1600] [--compile-only]"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_cases as gc                   # noqa: E402
from qcat_amd import config, jit, native      # noqa: E402


def ranges(text):
    out = []
    for part in text.split(","):
        if ":" in part:
            lo, hi = part.split(":")
            out.extend(range(int(lo), int(hi)))
        elif part:
            out.append(int(part))
    return out


ap = argparse.ArgumentParser()
ap.add_argument("--sections", default="builtin,ties,sizes,own,targets,templates")
ap.add_argument("--sizes", default="1:131,1024")
ap.add_argument("--templates", default="31:130", help="template lengths of the templates section")
ap.add_argument("--jit-every", type=int, default=1,
                help="kernels generated for every K-th kit of the sizes, targets and templates sections (ties and own: every kit; 0: none at all)")
ap.add_argument("--bs-static-max", type=int, default=24)
ap.add_argument("--reads", type=int, default=1600)
ap.add_argument("--workers", type=int, default=8)
ap.add_argument("--compile-only", action="store_true", help="fill the code-object cache and stop (no GPU needed)")
args = ap.parse_args()
sections = args.sections.split(",")

# ---- the kits: (section, name, layouts, mode, config, expectation) ------------------------------------------------------------
kits = []


def add(section, name, layouts, mode="epi2me", cfg=None, expect="packed"):
    if section in sections:
        kits.append((section, name, layouts, mode, cfg, expect))


for name, picks in sorted(gc.pbc096_subsets().items()):
    add("builtin", "PBC096 " + name, gc.subset_layouts(picks), expect="builtin")
for n2 in (49, 95, 96):
    add("builtin", "dual, first %d of set 2" % n2, gc.dual_subset_layouts(n2), mode="dual", expect="builtin")
seq96, bcs96 = gc.pbc096()
for k in (10, 25, 48, 64):
    for form in ("adjacent", "half", "mirror"):
        add("ties", "PBC096 %d x 2 %s" % (k, form), [gc.layout("REPEATS", seq96, gc.doubled(bcs96[:k], form))], expect="repeats")
        rng = random.Random(k)
        add("ties", "custom %d x 2 %s" % (k, form), [gc.layout("REPEATS", gc.custom_template(rng, 24, up=9, dn=30),
                                                                gc.doubled(gc.random_barcodes(rng, k), form))], expect="ties")
for name, (make, _) in sorted(gc.GENERATED.items()):
    add("ties" if name.startswith("TIES") else "sizes", "suite kit " + name, make(), expect="ties" if name.startswith("TIES") else "packed")
for n in ranges(args.sizes):
    add("sizes", "n = %d" % n, gc.single_kit(random.Random(n), n))
OWN = list(range(20, 49))
for own in OWN + [49]:                                     # (a barcode of `own` letters between 11 shared and 4 trailing columns)
    for rev in (False, True):
        up, dn = (4, 11) if rev else (11, 4)
        add("own", "own %d %s" % (own, "reversed" if rev else "forward"), gc.shape_kit(random.Random(own * 2 + rev), up, own, dn),
            expect="own" if own in OWN else "no bit-sliced form")
for m in range(31, 66):
    add("targets", "target %d" % m, gc.shape_kit(random.Random(m), 11, m - 22, 11),
        expect="general" if m == 31 else ("refused: barcode target length" if m == 65 else "packed"))
add("templates", "tier-B kit TEMPLATES", gc.templates_kit(), expect="plans")
for t in ranges(args.templates):
    gap = t < 32 or 65 <= t <= 75 or 93 <= t <= 95
    add("templates", "template %d" % t, gc.single_kit(random.Random(t), 6, tlen=t),
        expect="refused: length must be in" if t == 129 else ("general" if gap else "packed"))

# the own-column list covers the whole range of the kernels' instantiations, in both directions
if "own" in sections:
    seen = set()
    for section, name, layouts, mode, cfg, expect in kits:
        if section == "own" and expect == "own":
            rev, pre, own, post = gc.bs_shapes(gc.descriptor(layouts))[0]
            seen.add((own, rev))
    assert seen == {(c, r) for c in range(jit.BS_C_MIN, jit.BS_C_MAX + 1) for r in (False, True)}, sorted(seen)

# ---- which custom kits get kernels of their own; compile those first, side by side ------------------------------------------
todo, counter = {}, {}
for i, (section, name, layouts, mode, cfg, expect) in enumerate(kits):
    if expect in ("builtin", "repeats", "general") or expect.startswith("refused"):
        continue
    k = counter[section] = counter.get(section, -1) + 1
    nmax = max(len(lay.get_barcode_set(0)) for lay in layouts)
    every = 1 if section in ("ties", "own") and args.jit_every > 0 else args.jit_every
    if name.startswith("suite kit") or (every > 0 and k % every == 0 and (nmax <= 130 or nmax == 1024)):
        # the suite's kits as the suite compiles them; the others without the letters-compiled-in bit-sliced kernels when the set is
        # big, and only the template section with bit-sliced adapter plans (13 s of compile time per template)
        todo[i] = gc.GENERATED[name[10:]][1] if name.startswith("suite kit") else \
            (("NO_BS",) if nmax > args.bs_static_max else ()) + (() if section == "templates" else ("NO_ABS",))
t0 = time.time()
if todo:
    gc.compile_kits([(gc.descriptor(kits[i][2], mode=kits[i][3], cfg=kits[i][4]), switches) for i, switches in sorted(todo.items())], workers=args.workers)
print("# %s" % " ".join(sys.argv[1:]))
print("# %d kits, kernels generated for %d of them (%.0f s, %s)" % (len(kits), len(todo), time.time() - t0, jit.compiler()), flush=True)
if args.compile_only:
    sys.exit(0)

# ---- run -------------------------------------------------------------------------------------------------------------------------
native.set_option("NO_TINY", 1)                              # (small batches on the throughput kernels; the "tiny" paths clear it)
bad = n_paths = 0
for i, (section, name, layouts, mode, cfg, expect) in enumerate(kits):
    d = gc.descriptor(layouts, mode=mode, cfg=cfg)
    geometry = "sets %s targets %s templates %s" % (
        [len(lay.get_barcode_set(s)) for lay in layouts for s in (0, 1) if lay.get_barcode_set(s)],
        sorted({len(lay.get_upstream_context(11, 0)) + lay.get_barcode_length(0) + len(lay.get_downstream_context(11, 0)) for lay in layouts}),
        sorted({len(lay.sequence) for lay in layouts}))
    if expect.startswith("refused"):
        try:
            native.NativeKit(d, jit=False)
            status = "MISMATCH (accepted)"
        except RuntimeError as e:
            status = "ok (refused: %s)" % str(e).split(": ", 1)[-1] if expect[9:] in str(e) else "MISMATCH (%s)" % e
        bad += not status.startswith("ok")
        print("%-9s %-28s %s: %s" % (section, name, geometry, status), flush=True)
        continue
    nt = len(layouts)
    bare = 0.0 if expect in ("ties", "repeats") else 0.05
    if mode == "dual":
        reads = gc.batch(layouts, args.reads, 100 * i, t5=1, t3=0, no_adapter_fraction=bare)
    else:
        reads = []
        for t in range(nt):
            reads += gc.batch(layouts, max(200, args.reads // nt), 100 * i + t, t5=t, t3=t, no_adapter_fraction=bare)
    nmax = max(len(lay.get_barcode_set(0)) for lay in layouts)
    if nmax > 200:
        reads = reads[:200] + reads[-5:]
    reads += gc.forced_reads(layouts, nt - 1, sorted({0, len(layouts[nt - 1].get_barcode_set(0)) // 2, len(layouts[nt - 1].get_barcode_set(0)) - 1}), i, per=4)
    want = gc.Want(d, reads, threads=16)
    variants = [("built-in" if expect == "builtin" else "table", native.NativeKit(d, jit=False) if expect != "builtin" else native.NativeKit(d))]
    if i in todo:
        variants.append(("generated", gc.generated_kit(d, todo[i])))
    notes, problems = [], []
    if expect in ("ties", "repeats"):
        n, tied, tied_pos, wrong = gc.tie_stats(want)
        notes.append("ties %.3f (%.3f > 0)" % (tied / float(n), tied_pos / float(n)))
        if tied < 0.9 * n or tied_pos < 0.8 * n or wrong:
            problems.append("tie share %d / %d / %d, oracle not at the first index on %d" % (n, tied, tied_pos, wrong))
    for label, kit in variants:
        info = kit.describe()
        if expect == "general":
            if info["packed"] != 0:
                problems.append("%s: packed" % label)
        elif info["packed"] != 1:
            problems.append("%s: not packed" % label)
        if label != "table" and info["n_static_groups"] != info["n_groups"]:
            problems.append("%s: %d of %d groups bound" % (label, info["n_static_groups"], info["n_groups"]))
        if expect == "own" and label == "generated" and info["bitslice_groups"] != 0x10001:        # (both letter forms)
            problems.append("%s: bitslice_groups %#x" % (label, info["bitslice_groups"]))
        if expect == "plans" and label == "generated":
            # describe()["bitslice_templates"]: templates with a two-stage plan, << 8 with four narrow stages, << 16 with four wide ones
            two, narrow, wide = (info["bitslice_templates"] >> sh & 0xFF for sh in (0, 8, 16))
            notes.append("plans: %d two-stage, %d four-narrow, %d four-wide" % (two, narrow, wide))
            if not (two and narrow and wide):
                problems.append("a plan form is missing")
        if expect == "no bit-sliced form" and info["bitslice_groups"] != 0:
            problems.append("%s: bitslice_groups %#x" % (label, info["bitslice_groups"]))
        paths = gc.paths_for(kit, d, len(reads), adapter_plans=(section == "templates"))
        if label == "table" and len(variants) > 1:
            paths = [pc for pc in paths if pc[0] in ("raw", "default")]           # (the generated kit below runs the rest)
        results = gc.check(kit, want, paths=paths)
        n_paths += len(results)
        notes.append("%s: %s" % (label, " ".join(sorted({p for p, _ in results}))))
        for (p, c), v in sorted(gc.failures(results).items(), key=str):
            problems.append("%s %s chunk %s: %s" % (label, p, c, "; ".join(v)))
    bad += bool(problems)
    print("%-9s %-28s %s | %s: %s" % (section, name, geometry, "; ".join(notes), "ok" if not problems else "MISMATCH " + " || ".join(problems)), flush=True)
print("%d kits, %d path runs, %d mismatches" % (len(kits), n_paths, bad))
sys.exit(1 if bad else 0)

#!/usr/bin/env python3
"""Generate qcat_amd/csrc/static_generated.inc and bs_static_generated.inc: barcode column chains and bit-sliced rows with
compile-time target letters for every barcode target of the built-in kits (see kernels_static.inc, kernels_bitslice.inc).

A *target* is upstream context + barcode + downstream context exactly as the scanners build it
(qcat_amd.layout.AdapterLayout, mirroring qcat/layout.py:191-238) with the default
barcode_context_length.  Targets that share both flanks form one *family* = one kernel; a kit group
(template, set) can use the kernel when all of its targets are cases of the same family, which the
library checks at kit creation through the registry (FNV-1a 64 of the target codes -> kernel, case).

The text of every struct, the shape rule of the bit-sliced rows and their constants come from qcat_amd/static_text.py,
which qcat_amd/jit.py uses for custom kits; this file decides what is a family, a pair, a quad and a case, and writes
the registries, the launch switches and the merged kernels around the structs.

Run from the repo root:  python tools/gen_static_kernels.py
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qcat_amd import config as qconfig          # noqa: E402
from qcat_amd import scanner                    # noqa: E402
from qcat_amd import static_text as st          # noqa: E402
from qcat_amd.static_text import BS_C_MAX, BS_C_MIN, BS_MAX_TARGET, BS_POSTS, QUAD_MIN_TARGETS, bs_shape  # noqa: E402,F401

OUT = os.path.join(ROOT, "qcat_amd", "csrc", "static_generated.inc")
BS_MIN_TARGETS = 12         # families this large get bit-sliced row loops with the letters compiled in (kernels_bitslice.inc)
BS_PARTS = 6                # translation units the bit-sliced static-letter kernels are split over (__graft_entry__.build)
BS_OUT = os.path.join(ROOT, "qcat_amd", "csrc", "bs_static_generated.inc")
CODE = {"A": 0, "T": 1, "G": 2, "C": 3}
ACODE = {"A": 0, "T": 1, "G": 2, "C": 3, "N": 4}        # adapter templates also hold barcode placeholders


def _codes(seq):
    return [ACODE[c] for c in seq]


def fnv1a64(codes):
    h = 0xCBF29CE484222325
    for c in codes:
        h ^= c
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def pair_up(targets, flank):
    """greedy pairing by longest common prefix: [(ta, tb, shared columns)]; a leftover target is paired
    with itself.  Two targets that run in one row pass share their common prefix columns, so the
    longer the prefix the fewer columns a pair costs (static_barcode_rows2)."""
    rem = list(targets)
    cand = sorted(((st.lcp(a, b), a, b) for i, a in enumerate(rem) for b in rem[i + 1:]),
                  key=lambda x: (-x[0], x[1], x[2]))
    used, pairs = set(), []
    for lcp, a, b in cand:
        if a in used or b in used:
            continue
        used.update((a, b))
        pairs.append((a, b, min(lcp, len(a) - 1)))
    for t in rem:
        if t not in used:
            pairs.append((t, t, flank))
    return sorted(pairs)


def collect():
    """family (up, down) -> ordered list of distinct targets over every mode / kit selection"""
    n = qconfig.qcatConfig().barcode_context_length
    fams = collections.OrderedDict()
    members = {}                                 # target -> the (mode, kit, template, set) groups that scan it
    templates = []
    fused = []                                   # (template A, template B): the two templates of a kit
    for mode in scanner.get_modes():
        kits = [None] + sorted(scanner.get_kits())
        for kit in kits:
            try:
                det = scanner.factory(mode=mode, kit=kit)
            except Exception:
                continue
            by_kit = collections.OrderedDict()
            for lay in det.layouts:
                by_kit.setdefault(lay.kit, []).append(lay.sequence.upper())
            for seqs in by_kit.values():
                if len(seqs) == 2 and all(c in ACODE for q in seqs for c in q):
                    u = st.lcp(*seqs)
                    # both rows plus the shared columns must fit four waves per SIMD (128 VGPRs)
                    if len(seqs[0]) + len(seqs[1]) - u <= 100 and tuple(seqs) not in fused:
                        fused.append(tuple(seqs))
            for lay in det.layouts:
                seq = lay.sequence.upper()
                if seq not in templates and all(c in ACODE for c in seq):
                    templates.append(seq)
                for s in range(2 if mode == "dual" else 1):
                    bs = lay.get_barcode_set(s)
                    if not bs:
                        continue
                    up, dn = lay.get_upstream_context(n, s), lay.get_downstream_context(n, s)
                    for b in bs:
                        t = (up + b.sequence + dn).upper()
                        if any(c not in CODE for c in t):
                            break                       # non-ACGT target: table kernels only
                        lst = fams.setdefault((up, dn, len(t)), [])
                        if t not in lst:
                            lst.append(t)
                        members.setdefault(t, set()).add((mode, kit, lay.sequence, s))
    return fams, templates, fused, members


def switch(cases, indent="    "):
    """the cases of a launch switch and its end"""
    return "".join(indent + "case %s; break;\n" % c for c in cases) + indent + "default: break;\n" + indent + "}\n"


def barcode_families(fams, members):
    """the chain structs of every family; also the target registry (hash, kernel, case, target), the quad registry
    (kernel, quad case, pair a, pair b), per family whether it has bit-sliced rows, and those rows
    (kernel, targets, text of its QBS struct), which go to bs_static_generated.inc"""
    out, reg, quad_reg, has_bs, bs_structs = [], [], [], [], []
    for kid, ((up, dn, m), targets) in enumerate(fams.items()):
        u = len(up)
        out.append("// kernel %d: %s + barcode + %s (%d columns, %d-column flank, %d targets)\n" % (kid, up, dn, m, u, len(targets)))
        # targets that are always scanned together (same set of kit groups) may be paired with each other
        groups = collections.OrderedDict()
        for t in targets:
            groups.setdefault(frozenset(members[t]), []).append(t)
        pairs = []
        quads = []                                   # (pair index a, pair index b): consecutive pairs of one membership group
        for grp in groups.values():
            first = len(pairs)
            pairs.extend(pair_up(grp, u))
            if len(targets) >= QUAD_MIN_TARGETS:
                quads.extend((i, i + 1) for i in range(first, len(pairs) - 1, 2)
                             if pairs[i][0] != pairs[i][1] and pairs[i + 1][0] != pairs[i + 1][1])
        cases = []                                   # (case, target): a pair's targets are cases 2 x pair, 2 x pair + 1
        for pr, (ta, tb, shared) in enumerate(pairs):
            cases.append((2 * pr, ta))
            if tb != ta:
                cases.append((2 * pr + 1, tb))
            out.append(st.pair_struct("QSP_%d_%d" % (kid, pr), _codes(ta), _codes(tb), shared))
        reg.extend((fnv1a64(_codes(t)), kid, case, t) for case, t in cases)
        quad_cases = []
        for q, (pa, pb) in enumerate(quads):
            cpa, cpb = [(_codes(a), _codes(b), shared) for a, b, shared in (pairs[pa], pairs[pb])]
            u0 = st.quad_shared(cpa, cpb)
            quad_reg.append((kid, q, pa, pb))
            out.append(st.quad_struct("QSQ_%d_%d" % (kid, q), cpa, cpb, u0))
            quad_cases.append(("QSQ_%d_%d" % (kid, q), u0, cpa[2] - u0, cpb[2] - u0))
        out.append(st.group_struct("QSG_%d" % kid, m, quad_cases,
                                   [("QSP_%d_%d" % (kid, pr), shared) for pr, (_, _, shared) in enumerate(pairs)]))
        shape = bs_shape(len(up), len(dn), m) if len(targets) >= BS_MIN_TARGETS else None
        has_bs.append(shape is not None)
        if shape:
            rev, pre, own, post = shape
            bs_structs.append((kid, len(targets), st.bs_row_struct(
                "QBS_%d" % kid, "%d" % kid, shape, [(case, _codes(t)) for case, t in cases],
                "%s + barcode + %s: %s, %d shared + %d own + %d trailing columns, %d targets"
                % (up, dn, "reversed" if rev else "forward", pre, own, post, len(targets)))))
        out.append("\n")
    reg.sort()
    assert len(set(h for h, _, _, _ in reg)) == len(reg), "hash collision between targets"
    return "".join(out), reg, quad_reg, has_bs, bs_structs


def target_registry(fams, reg, quad_reg, has_bs):
    """the registries static_match reads and the launcher of k_barcode_static"""
    def ints(values):
        return ", ".join("%d" % v for v in values)
    return ("#ifndef QCAT_STATIC_MULTI_TU      // (static_multi.hip takes the column chains above and the merged kernels only)\n"
            "// (the hash only finds the entry; static_match compares `seq` with the kit's target before binding)\n"
            "struct StaticTarget { uint64_t hash; int16_t kernel, kase; const char* seq; };\n"
            "static const StaticTarget g_static_targets[] = {\n"
            + "".join("    {0x%016XULL, %d, %d, \"%s\"},\n" % r for r in reg)
            + "};\nstatic const int g_n_static_targets = %d;\n" % len(reg)
            + "static const int g_static_kernel_M[] = {%s};\n" % ints(m for (_, _, m) in fams)
            + "// per kernel: upstream / downstream context columns of the family, and whether it has bit-sliced rows (QBS_n)\n"
            + "static const int g_static_kernel_up[] = {%s};\n" % ints(len(up) for (up, _, _) in fams)
            + "static const int g_static_kernel_dn[] = {%s};\n" % ints(len(dn) for (_, dn, _) in fams)
            + "static const int g_static_kernel_bs[] = {%s};\n" % ints(has_bs)
            + "// quads of a kernel: (kernel, quad case, pair case a, pair case b); a kit group runs them when it scans both pairs\n"
            "struct StaticQuad { int16_t kernel, quad, pair_a, pair_b; };\n"
            "static const StaticQuad g_static_quads[] = {\n"
            + "".join("    {%d, %d, %d, %d},\n" % q for q in quad_reg)
            + "    {-1, -1, -1, -1}\n};\nstatic const int g_n_static_quads = %d;\n\n" % len(quad_reg)
            + "static inline void launch_barcode_static(int kernel, dim3 grid, hipStream_t stream, const StaticArgs& a) {\n"
            "    if (kernel >= QCAT_JIT_BASE) { jit_launch(QCAT_JIT_BARCODE, kernel - QCAT_JIT_BASE, grid, stream, &a); return; }\n"
            "    switch (kernel) {\n"
            + switch("%d: hipLaunchKernelGGL(k_barcode_static<QSG_%d>, grid, dim3(PK_WAVES * 64), 0, stream, a)" % (kid, kid)
                     for kid in range(len(fams)))
            + "}\n#endif\n\n")


def barcode_multi(n_kernels):
    return ("// every group of a SMALL batch in one launch (packed_host.inc: packed_barcode): blockIdx.x % n = the group.  A kit-auto batch launches\n"
            "// one kernel per (template, set) group although only the voted kit's groups have jobs, and the runtime's four hardware\n"
            "// queues serialise them around the two or three that do.  Compiled in a translation unit of its own (static_multi.hip).\n"
            "#ifdef QCAT_STATIC_MULTI_TU\n"
            "__global__ void __launch_bounds__(PK_WAVES * 64, 2)\n"
            "k_barcode_multi(StaticBarcodeMulti m) {\n"
            "    __shared__ uint8_t qbuf[PK_ROWS * 64];\n"
            "    const int i = blockIdx.x % (uint32_t)m.n;      // (interleaved: the workgroups of the groups with jobs are resident side by side)\n"
            "    StaticArgs a = m.common;\n"
            "    a.gidx = m.gidx[i]; a.chunk_b = m.chunk_b[i];\n"
            "    switch (m.kernel[i]) {\n"
            + switch("%d: barcode_static_core<QSG_%d>(a, qbuf)" % (kid, kid) for kid in range(n_kernels))
            + "}\n"
            "extern \"C\" void qcat_static_multi_barcode(unsigned grid, void* stream, const void* m) {\n"
            "    hipLaunchKernelGGL(k_barcode_multi, dim3(grid), dim3(PK_WAVES * 64), 0, static_cast<hipStream_t>(stream), *static_cast<const StaticBarcodeMulti*>(m));\n}\n"
            "#else\n"
            "extern \"C\" void qcat_static_multi_barcode(unsigned grid, void* stream, const void* m);\n"
            "static inline void launch_barcode_multi(dim3 grid, hipStream_t stream, const StaticBarcodeMulti& m) { qcat_static_multi_barcode(grid.x, stream, &m); }\n"
            "#endif\n\n")


def bitslice_parts(bs_structs):
    """(the launcher of the bit-sliced static-letter kernels, text of bs_static_generated.inc).  They are compiled in
    translation units of their own (bs_static.hip with QCAT_BS_PART = 0..BS_PARTS-1, in parallel with this one): greedy
    split by number of targets"""
    parts = [[] for _ in range(BS_PARTS)]
    for kid, nt, text in sorted(bs_structs, key=lambda x: -x[1]):
        min(parts, key=lambda p: sum(n for _, n, _ in p)).append((kid, nt, text))
    parts = [sorted(part) for part in parts]
    launcher = ("}  // namespace qk\n#ifndef QCAT_STATIC_MULTI_TU\n"
                + "".join('extern "C" void qcat_bs_launch_part%d(int kernel, unsigned grid, void* stream, const void* args);   // bs_static.hip\n' % p
                          for p in range(BS_PARTS))
                + "#endif\nnamespace qk {\n#ifndef QCAT_STATIC_MULTI_TU\n"
                "static inline void launch_bs_static(int kernel, dim3 grid, hipStream_t stream, const BsArgs& a) {\n"
                "    if (kernel >= QCAT_JIT_BASE) { jit_launch(QCAT_JIT_BITSLICE, kernel - QCAT_JIT_BASE, grid, stream, &a); return; }\n"
                "    switch (kernel) {\n"
                + "".join("    %s qcat_bs_launch_part%d(kernel, grid.x, stream, &a); break;\n"
                          % (" ".join("case %d:" % kid for kid, _, _ in part), p) for p, part in enumerate(parts) if part)
                + "    default: break;\n    }\n}\n#endif\n\n")
    out = ["// GENERATED by tools/gen_static_kernels.py -- do not edit.\n"
           "// Bit-sliced barcode kernels with the target letters compiled in (kernels_bitslice.inc), one struct per target\n"
           "// family; compiled by bs_static.hip in %d parts (QCAT_BS_PART), each in its own namespace.\n\n" % BS_PARTS]
    for p, part in enumerate(parts):
        out.append("#if QCAT_BS_PART == %d\nnamespace qk {\n" % p + "".join(text for _, _, text in part) + "}  // namespace qk\n"
                   + 'extern "C" void qcat_bs_launch_part%d(int kernel, unsigned grid, void* stream, const void* args) {\n'
                   "    const qk::BsArgs& a = *static_cast<const qk::BsArgs*>(args);\n    switch (kernel) {\n" % p
                   + switch("%d: hipLaunchKernelGGL(qk::k_bs_barcode<qk::QBS_%d>, dim3(grid), dim3(qk::BS_WAVES * 64), 0, "
                            "static_cast<hipStream_t>(stream), a)" % (kid, kid) for kid, _, _ in part)
                   + "}\n#endif\n\n")
    return launcher, "".join(out)


def adapter_templates(templates):
    """chain struct, registry and launcher of the adapter templates; also the number of registry entries"""
    out = []
    for tid, seq in enumerate(templates):
        out.append("// adapter template %d: %s\n" % (tid, seq) + st.adapter_chain_struct("QAC_%d" % tid, _codes(seq)))
    areg = sorted((fnv1a64(_codes(seq)), tid, len(seq), seq) for tid, seq in enumerate(templates))
    assert len(set(h for h, _, _, _ in areg)) == len(areg), "hash collision between templates"
    out.append("\n#ifndef QCAT_STATIC_MULTI_TU\nstruct StaticTemplate { uint64_t hash; int16_t kernel, len; const char* seq; };\n"
               "static const StaticTemplate g_static_templates[] = {\n"
               + "".join("    {0x%016XULL, %d, %d, \"%s\"},\n" % r for r in areg)
               + "};\nstatic const int g_n_static_templates = %d;\n\n" % len(areg)
               + "static inline void launch_adapter_static(int kernel, dim3 grid, hipStream_t stream, const StaticAdapterArgs& a) {\n"
               "    if (kernel >= QCAT_JIT_BASE) { jit_launch(QCAT_JIT_ADAPTER, kernel - QCAT_JIT_BASE, grid, stream, &a); return; }\n"
               "    switch (kernel) {\n"
               + switch("%d: hipLaunchKernelGGL((k_adapter_static<%d, QAC_%d>), grid, dim3(PK_WAVES * 64), 0, stream, a)" % (tid, len(seq), tid)
                        for tid, seq in enumerate(templates))
               + "}\n#endif\n\n")
    return "".join(out)


def fused_args(fused):
    """per two-template kit the template arguments of its fused kernel: shared columns, both lengths, chain struct"""
    return ["%d, %d, %d, QAF_%d" % (st.lcp(sa, sb), len(sa), len(sb), fid) for fid, (sa, sb) in enumerate(fused)]


def fused_kits(templates, fused):
    """two-template kits: one fused pass over both templates"""
    out = []
    for fid, (sa, sb) in enumerate(fused):
        u = st.lcp(sa, sb)
        out.append("// fused adapter kernel %d: %d shared columns of\n//   %s\n//   %s\n" % (fid, u, sa, sb)
                   + "struct QAF_%d {\n" % fid
                   + st.chain_fn("pre", _codes(sa[:u]), 5) + st.chain_fn("ta", _codes(sa[u:]), 5) + st.chain_fn("tb", _codes(sb[u:]), 5) + "};\n")
    out.append("\n#ifndef QCAT_STATIC_MULTI_TU\n// (tpl_a / tpl_b: the static adapter kernels of the two templates, which static_match has verified)\n"
               "struct StaticFused { int16_t tpl_a, tpl_b, kernel; };\n"
               "static const StaticFused g_static_fused[] = {\n"
               + "".join("    {%d, %d, %d},\n" % (templates.index(sa), templates.index(sb), fid) for fid, (sa, sb) in enumerate(fused))
               + "};\nstatic const int g_n_static_fused = %d;\n\n" % len(fused)
               + "static inline void launch_adapter_fused(int kernel, dim3 grid, hipStream_t stream, const StaticAdapterArgs& a) {\n"
               "    switch (kernel) {\n"
               + switch("%d: hipLaunchKernelGGL((k_adapter_fused2<%s>), grid, dim3(PK_WAVES * 64), 0, stream, a)" % (fid, args)
                        for fid, args in enumerate(fused_args(fused)))
               + "}\n#endif\n\n")
    return "".join(out)


def adapter_multi(templates, fused):
    return ("// every static-letter adapter chain of a SMALL batch in one launch (packed_host.inc: packed_adapter): blockIdx.y = the unit --\n"
            "// a template or a fused pair.  The units of such a batch are latency chains (one wave per SIMD, 50-110 us each for the\n"
            "// 4000 reads of the reference driver's call), and launches of their own are serialised by the runtime's four hardware queues.\n"
            "#ifdef QCAT_STATIC_MULTI_TU\n"
            "__global__ void __launch_bounds__(PK_WAVES * 64, 2)\n"
            "k_adapter_multi(StaticAdapterMulti m) {\n"
            "    __shared__ uint8_t qbuf[PK_ROWS * 64];\n"
            "    __shared__ uint16_t slow_tbl[5 * 16];\n"
            "    const int i = blockIdx.y;\n"
            "    StaticAdapterArgs a = m.common;\n"
            "    a.bests = m.bests[i]; a.bests2 = m.bests2[i]; a.tpl = m.tpl[i]; a.tpl2 = m.tpl2[i];\n"
            "    const int kernel = m.kernel[i];\n"
            "    if (m.fused[i]) {\n"
            "        switch (kernel) {\n"
            + switch(("%d: adapter_fused2_core<%s>(a, qbuf, slow_tbl)" % (fid, args) for fid, args in enumerate(fused_args(fused))), "        ")
            + "    } else {\n        switch (kernel) {\n"
            + switch(("%d: adapter_static_core<%d, QAC_%d>(a, qbuf, slow_tbl)" % (tid, len(seq), tid) for tid, seq in enumerate(templates)), "        ")
            + "    }\n}\n"
            "extern \"C\" void qcat_static_multi_adapter(unsigned grid_x, unsigned grid_y, void* stream, const void* m) {\n"
            "    hipLaunchKernelGGL(k_adapter_multi, dim3(grid_x, grid_y), dim3(PK_WAVES * 64), 0, static_cast<hipStream_t>(stream), *static_cast<const StaticAdapterMulti*>(m));\n}\n"
            "#else\n"
            "extern \"C\" void qcat_static_multi_adapter(unsigned grid_x, unsigned grid_y, void* stream, const void* m);\n"
            "static inline void launch_adapter_multi(dim3 grid, hipStream_t stream, const StaticAdapterMulti& m) { qcat_static_multi_adapter(grid.x, grid.y, stream, &m); }\n"
            "#endif\n\n")


def middle_launcher(templates):
    return ("// the same column chains over the read interior (--detect-middle, kernels_middle.inc)\n"
            "#ifdef QCAT_HAVE_MIDDLE_KERNELS\n"
            "static inline void launch_adapter_middle(int kernel, dim3 grid, hipStream_t stream, const MiddleAdapterArgs& a) {\n"
            "    if (kernel >= QCAT_JIT_BASE) { jit_launch(QCAT_JIT_MIDDLE, kernel - QCAT_JIT_BASE, grid, stream, &a); return; }\n"
            "    switch (kernel) {\n"
            + switch("%d: hipLaunchKernelGGL((k_adapter_middle<%d, QAC_%d>), grid, dim3(PK_WAVES * 64), 0, stream, a)" % (tid, len(seq), tid)
                     for tid, seq in enumerate(templates))
            + "}\n#endif\n\n")


def render():
    """text of static_generated.inc, (n kernels, n targets, n templates), text of bs_static_generated.inc"""
    fams, templates, fused, members = collect()
    families, reg, quad_reg, has_bs, bs_structs = barcode_families(fams, members)
    bs_launcher, bs_text = bitslice_parts(bs_structs)
    text = ("// GENERATED by tools/gen_static_kernels.py -- do not edit.\n"
            "// %d kernels, %d targets (built-in kits, barcode_context_length = %d).\n\n"
            % (len(fams), sum(len(v) for v in fams.values()), qconfig.qcatConfig().barcode_context_length)
            + "namespace qk {\n\n"
            + families + target_registry(fams, reg, quad_reg, has_bs) + barcode_multi(len(fams)) + bs_launcher
            + adapter_templates(templates) + fused_kits(templates, fused) + adapter_multi(templates, fused)
            + middle_launcher(templates) + "}  // namespace qk\n")
    return text, len(fams), len(reg), len(templates), bs_text


def main():
    text, nk, nt, na, bs_text = render()
    with open(OUT, "w") as out:
        out.write(text)
    with open(BS_OUT, "w") as out:
        out.write(bs_text)
    print("wrote %s: %d barcode kernels, %d targets, %d adapter templates" % (OUT, nk, nt, na))


if __name__ == "__main__":
    main()

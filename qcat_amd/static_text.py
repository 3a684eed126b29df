"""Text of the static-letter kernels (csrc/kernels_static.inc, csrc/kernels_bitslice.inc): the constants, the column
chain, the shape rule of the bit-sliced barcode rows and one emitter per generated struct.

Used twice, like abs_plan.py: tools/gen_static_kernels.py writes csrc/static_generated.inc and
csrc/bs_static_generated.inc for the built-in kits at build time, qcat_amd/jit.py emits the same structs for a custom
kit at run time.  The callers decide what is not text: which targets form a family, a pair, a quad and a case number,
the registries, launch switches and entry points.

Sequences are lists of letter codes (qcat_amd/codes.py: A, T, G, C = 0..3; 4 = the N of a template)."""

QUAD_MIN_TARGETS = 48       # sets this large also get four-target chains (the big sets dominate the run time)
BS_C_MIN, BS_C_MAX = 20, 48 # kit.h: own columns the bit-sliced kernels are instantiated for
BS_POSTS = (11, 8, 7, 6, 4) # kit.h, bs_post_of: trailing columns the reversed DP takes (the instantiations of kernels_bitslice.inc)
BS_MAX_TARGET = 63          # kit.h: a score counter holds up to 63 and a target read without an error scores its length


def lcp(*seqs):
    """length of the common prefix of the sequences"""
    n = 0
    for col in zip(*seqs):
        if any(c != col[0] for c in col):
            break
        n += 1
    return n


def chain(codes):
    """column chain in chunks of four.  Every read of the previous row happens before the chunk's
    first write and the diagonal term of the NEXT chunk's first column is formed inside this chunk,
    so h[] is updated in place: no old h[j] outlives its new value, no register copies at the loop
    back edge."""
    e = ["E[%d]" % c for c in codes]
    out = ["QS_BEGIN(%s)" % e[0]]
    n = len(codes)
    for j in range(0, n, 4):
        k = min(4, n - j)
        inner = e[j + 1:j + k]
        if j + k < n:
            out.append("QS_CHUNK4(%d, %s)" % (j + 1, ", ".join(inner + [e[j + k]])))
        else:
            out.append("QS_LAST%d(%d%s)" % (k, j + 1, "".join(", " + x for x in inner)))
    return " ".join(out)


def bs_shape(uplen, downlen, m):
    """(reversed, shared columns, own columns, trailing columns) of a target family on the bit-sliced kernels, or None: the
    rule of kit_prepare.inc (the longer context leads; 11 / 8 / 4 / 0 of its columns are shared; the other context's
    columns -- 11 / 8 / 7 / 6 / 4 / 0 of them, as long as BS_C_MIN own columns remain -- are computed once per super-tile as
    well, by the reversed DP of bs_core.h)"""
    rev = downlen > uplen
    lead, trail = (downlen, uplen) if rev else (uplen, downlen)
    pre = 11 if lead >= 11 else (8 if lead >= 8 else (4 if lead >= 4 else 0))
    post = next((q for q in BS_POSTS if q <= trail and m - pre - q >= BS_C_MIN), 0)
    own = m - pre - post
    if not (BS_C_MIN <= own <= BS_C_MAX and m <= BS_MAX_TARGET):
        return None
    return rev, pre, own, post


def _words(codes):
    """the two letter bit words of a run of columns: bit j = column j"""
    w1 = w0 = 0
    for j, c in enumerate(codes):
        w1 |= ((c >> 1) & 1) << j
        w0 |= (c & 1) << j
    return w1, w0


def bs_words(codes, rev, pre, own):
    """letter bit words of the own columns in the order the kernel walks them (bit j = own column j)"""
    t = codes[::-1] if rev else codes
    return _words(t[pre:pre + own])


def bs_shared_words(codes, rev, pre):
    """letter bit words of the shared (leading context) columns: bit j = shared column j"""
    t = codes[::-1] if rev else codes
    return _words(t[:pre])


def bs_trailing_words(codes, rev, post):
    """letter bit words of the trailing context's columns in the order the REVERSED DP walks them (bit j = its column j =
    the target's last column but j, in walk order)"""
    t = codes[::-1] if rev else codes
    return _words(t[::-1][:post])


def chain_fn(name, codes, letters=4):
    """one member function of a chain struct: the columns `codes` (none: an empty body) over h[0 .. len(codes)]"""
    return ("    static __device__ __forceinline__ void %s(h2 (&h)[%d], h2& carry, h2& left, const h2 (&E)[%d]) { %s }\n"
            % (name, len(codes) + 1, letters, chain(codes) if codes else ""))


def pair_struct(name, ta, tb, shared):
    """two targets in one row pass (static_barcode_rows2): their `shared` leading columns once, then each tail; a target
    without a partner is paired with itself"""
    return ("struct %s {      // %d shared columns\n" % (name, shared)
            + chain_fn("pre", ta[:shared]) + chain_fn("ta", ta[shared:]) + chain_fn("tb", tb[shared:]) + "};\n")


def quad_shared(pair_a, pair_b):
    """columns that all four targets of two pairs (ta, tb, shared columns) have in common"""
    (a1, a2, ua), (b1, b2, ub) = pair_a, pair_b
    return min(lcp(a1, a2, b1, b2), ua, ub)


def quad_struct(name, pair_a, pair_b, u0):
    """two pairs (ta, tb, shared columns) in ONE row pass (static_barcode_rows4): the u0 = quad_shared() columns all four
    targets share (at least the flank) and the per-row work (selector, score registers, boundary) are paid once per four
    targets"""
    (a1, a2, ua), (b1, b2, ub) = pair_a, pair_b
    return ("struct %s {      // %d columns shared by all four, +%d / +%d inside the pairs\n" % (name, u0, ua - u0, ub - u0)
            + chain_fn("pre0", a1[:u0])
            + chain_fn("prea", a1[u0:ua]) + chain_fn("ta", a1[ua:]) + chain_fn("tb", a2[ua:])
            + chain_fn("preb", b1[u0:ub]) + chain_fn("tc", b1[ub:]) + chain_fn("td", b2[ub:]) + "};\n")


def group_struct(name, m, quads, pairs):
    """what k_barcode_static takes: targets of m columns, `quads` = [(quad struct, u0, columns +a, +b)] and `pairs` =
    [(pair struct, shared columns)]; the position in the list is the case number"""
    out = ["struct %s {\n    static constexpr int M = %d;\n    static constexpr int HAS_QUADS = %d;\n" % (name, m, 1 if quads else 0),
           "    static __device__ __forceinline__ void run4(int quad, const uint8_t* qbuf, int lane, int Lmax, h2 gL2, "
           "u32 special, const u32 (&ltr)[4], h2 rowoff, h2 coloff, u32& ra, u32& rb, u32& rc, u32& rd) {\n"
           "        ra = 0; rb = 0; rc = 0; rd = 0;\n        switch (quad) {\n"]
    for q, (struct, u0, da, db) in enumerate(quads):
        out.append("        case %d: static_barcode_rows4<M, %d, %d, %d, %s>(qbuf, lane, Lmax, gL2, special, ltr, rowoff, coloff, ra, rb, rc, rd); break;\n"
                   % (q, u0, da, db, struct))
    out.append("        default: break;\n        }\n    }\n"
               "    static __device__ __forceinline__ void run(int pair, const uint8_t* qbuf, int lane, int Lmax, h2 gL2, "
               "u32 special, const u32 (&ltr)[4], h2 rowoff, h2 coloff, u32& ra, u32& rb) {\n        ra = 0; rb = 0;\n        switch (pair) {\n")
    for pr, (struct, shared) in enumerate(pairs):
        out.append("        case %d: static_barcode_rows2<M, %d, %s>(qbuf, lane, Lmax, gL2, special, ltr, rowoff, coloff, ra, rb); break;\n"
                   % (pr, shared, struct))
    out.append("        default: break;\n        }\n    }\n};\n")
    return "".join(out)


def bs_row_struct(name, kernel, shape, cases, comment=None):
    """bit-sliced rows with the letters compiled in (kernels_bitslice.inc) for a set of shape = bs_shape(); `kernel`: the
    expression of its kernel number, `cases` = [(case number, target)].  With a `comment` (the generated files of the
    built-in kits, which people read) the letter words of the two contexts stand on annotated lines of their own."""
    rev, pre, own, post = shape
    s1, s0 = bs_shared_words(cases[0][1], rev, pre)
    t1, t0 = bs_trailing_words(cases[0][1], rev, post)
    out = ["struct %s {%s\n    static constexpr int C = %d, KERNEL = %s, PRE = %d, POST = %d;\n"
           % (name, "      // " + comment if comment else "", own, kernel, pre, post)]
    if comment:
        out.append("    static constexpr unsigned S1 = 0x%Xu, S0 = 0x%Xu;      // letters of the shared columns\n"
                   "    static constexpr unsigned T1 = 0x%Xu, T0 = 0x%Xu;      // letters of the trailing columns, last column first\n"
                   % (s1, s0, t1, t0))
    else:
        out.append("    static constexpr unsigned S1 = 0x%Xu, S0 = 0x%Xu, T1 = 0x%Xu, T0 = 0x%Xu;\n" % (s1, s0, t1, t0))
    out.append("    static __device__ __forceinline__ void rows(int kase, const BsRowArgs& ra, "
               "u32 (&h1)[C], u32 (&h0)[C], u32 (&f)[BS_ND]) {\n        switch (kase) {\n")
    for kase, codes in cases:
        out.append("        case %d: bs_rows_static<C, PRE != 0, 0x%XULL, 0x%XULL>(ra, h1, h0, f); break;\n"
                   % ((kase,) + bs_words(codes, rev, pre, own)))
    out.append("        default: break;\n        }\n    }\n};\n")
    return "".join(out)


def adapter_chain_struct(name, codes):
    """the column chain of one adapter template (k_adapter_static, k_adapter_middle): five letters, N among them"""
    return "struct %s { %s };\n" % (name, chain_fn("run", codes, 5).strip())

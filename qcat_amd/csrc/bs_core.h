// bs_core.h -- the BARCODE DP in bit-sliced difference form: the arithmetic shared by the device kernels
// (kernels_bitslice.inc) and by the host check of the same arithmetic (tests/bs_host_check.cpp, plain g++).
//
// find_highest_scoring_barcode (qcat/scanner_base.py:63-141) aligns every barcode target to the barcode region with
// match +1 / mismatch -1 / gap open = extend = 1 (config.py:26, scanner_base.py:111-117) and consumes the SCORE only
// (:119, :141).  With those scores the differences between neighbouring DP cells take four values,
//       dv(i,j) = H(i,j) - H(i-1,j),   dh(i,j) = H(i,j) - H(i,j-1)      in {-1, 0, 1, 2},
// and one cell is a boolean function of five bits: with a = dv(i,j-1) + 1, b = dh(i-1,j) + 1 (two bits each) and
// eq = [query letter == target letter],
//       m = eq ? 3 : max(a, b, 1)          ( = H(i,j) - H(i-1,j-1) + 2 )
//       dv(i,j) + 1 = m - b,   dh(i,j) + 1 = m - a.
// Bit-slicing ACROSS ALIGNMENTS puts bit k of a quantity of 32 different alignments into one 32-bit word.
//
// Round 5 -- BOTH contexts of a target shared.  A target is  leading context (P columns) + barcode + trailing context
// (Q columns), M = P + C + Q.  The gap cost is linear, so every path that reaches a column beyond c = P + C passes
// through exactly one LAST lattice point (i, c) of the line in front of the trailing context, and what it scores after
// that point is a semi-global alignment of the rest of the region against the trailing context that STARTS in that
// point -- read backwards: the DP R of the reversed region against the reversed trailing context, ending in its last
// column.  With H the forward DP over the columns <= c:
//       score = max( max_{0<=i<=L} [ H(i,c) + R(L-i, Q) ],      paths that cross the line at row i
//                    max_{1<=j<=c} H(L,j),                      paths that end in the last row before it
//                    max_{1<=j<=Q} R(L,j) )                     paths that lie behind it altogether
// which is exact (every path of the full DP is one of the three kinds and every term is a path of the full DP).
// R depends on the region and the trailing context only -- not on the barcode: its last column is computed ONCE per
// 2048 alignments beside the leading context's columns, one difference dvR(k) = R(k,Q) - R(k-1,Q) per row, and a
// barcode walks  G(i) = H(i,c) + R(L-i,Q)  down its last own column as a deficit counter whose step is
// dv(i,c) - dvR(L-i+1) in [-3, 3] (bs_deficit_split), G(L) = H(L,c).  A barcode's row costs C cells instead of C + Q.
//
// Everything here is a pure function of 32-bit words, so the host check runs the very same code 32 alignments at a
// time against the oracle's scalar DP.
#ifndef QCAT_BS_CORE_H
#define QCAT_BS_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define BS_FN __host__ __device__ __forceinline__
#else
#define BS_FN inline
#endif

namespace qk {

typedef uint32_t u32;

// bit (x << 2 | y << 1 | z) of the table is f(x, y, z) -- the convention of v_bitop3_b32
BS_FN u32 bs_lut_host(u32 x, u32 y, u32 z, unsigned t) {
    u32 r = 0;
    for (int i = 0; i < 8; ++i)
        if ((t >> i) & 1u) r |= ((i & 4) ? x : ~x) & ((i & 2) ? y : ~y) & ((i & 1) ? z : ~z);
    return r;
}

}  // namespace qk

// gfx950 has v_bitop3_b32, an arbitrary boolean function of three registers given by its truth table.
// QB3(x, y, z, f) evaluates f on the constants 0xF0 / 0xCC / 0xAA at compile time to get the table, QT3 takes a table.
#if defined(__HIP_DEVICE_COMPILE__)
#define BS_LUT(X, Y, Z, T) __builtin_amdgcn_bitop3_b32((X), (Y), (Z), (unsigned)(T))
#else
#define BS_LUT(X, Y, Z, T) qk::bs_lut_host((X), (Y), (Z), (unsigned)(T))
#endif
#define QB3(X, Y, Z, ...) BS_LUT((X), (Y), (Z), ([](unsigned x, unsigned y, unsigned z) constexpr { return (unsigned)(__VA_ARGS__) & 0xFFu; }(0xF0u, 0xCCu, 0xAAu)))
#define QT3(X, Y, Z, TABLE) BS_LUT((X), (Y), (Z), (TABLE))

namespace qk {

constexpr int BS_NB = 7;                      // planes of a score counter: H + 64 in [0, 127]
constexpr int BS_OFF = 64;
constexpr int BS_NF = 8;                      // planes of the (unsplit) deficit counter
constexpr int BS_ND = 7;                      // planes of the split form's deficit: G stays within [-M, M], M <= 59
constexpr int BS_POST_MAX = 12;               // trailing columns the split form takes out of a barcode's rows

BS_FN u32 bs_bfi(u32 m, u32 x, u32 y) { return QB3(m, x, y, (x & y) | (~x & z)); }

// g += (p1 p0) - 1        (p in 0..3; never leaves [0, 127] by construction): one ripple pass over the planes with
// p - 1 in two's complement = (.., sg, sg, ~(p1 ^ p0), ~p0), sg = [p = 0]
BS_FN void bs_step(u32 (&g)[BS_NB], u32 p1, u32 p0) {
    u32 c = QB3(g[0], p0, p0, x & ~y);
    g[0] = QB3(g[0], p0, p0, ~(x ^ y));
    {
        const u32 x1 = QB3(p1, p0, p0, ~(x ^ y));
        const u32 n1 = QB3(g[1], x1, c, x ^ y ^ z);
        c = QB3(g[1], x1, c, (x & y) | (x & z) | (y & z));
        g[1] = n1;
    }
    const u32 sg = QB3(p1, p0, p0, ~x & ~y);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 2; k < BS_NB; ++k) {
        const u32 n = QB3(g[k], sg, c, x ^ y ^ z);
        c = QB3(g[k], sg, c, (x & y) | (x & z) | (y & z));
        g[k] = n;
    }
}

// mask of the alignments with x > y
BS_FN u32 bs_gt(const u32 (&x)[BS_NB], const u32 (&y)[BS_NB]) {
    u32 gt = QB3(x[BS_NB - 1], y[BS_NB - 1], y[BS_NB - 1], x & ~y);
    u32 eq = QB3(x[BS_NB - 1], y[BS_NB - 1], y[BS_NB - 1], ~(x ^ y));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = BS_NB - 2; k >= 0; --k) {
        gt |= QB3(eq, x[k], y[k], x & y & ~z);
        if (k) eq = QB3(eq, x[k], y[k], x & ~(y ^ z));
    }
    return gt;
}

BS_FN void bs_max(u32 (&best)[BS_NB], const u32 (&x)[BS_NB]) {
    const u32 gt = bs_gt(x, best);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < BS_NB; ++k) best[k] = bs_bfi(gt, x[k], best[k]);
}

// one DP cell for 32 alignments per lane: SEVEN three-input boolean instructions (a minimal-size network found by
// tools/lut3_search.cpp; no six-node network turned up).  neq: letter mismatch mask; (a1 a0) = dv + 1 of the left cell
// (in: column j - 1, out: column j); (b1 b0) = dh + 1 of column j (in: row i - 1, out: row i).
// m = eq ? 3 : max(a, b, 1); out a = m - b, out b = m - a.
BS_FN void bs_cell(u32 neq, u32& a1, u32& a0, u32& b1, u32& b0) {
    const u32 n5 = QT3(a1, a0, neq, 0xd5);
    const u32 n6 = QT3(b1, a1, n5, 0x5b);
    const u32 n7 = QT3(a0, b1, b0, 0x73);
    const u32 p0 = QT3(b0, b1, n6, 0x16);                 // out a, bit 0
    const u32 q1 = QT3(n5, a1, n7, 0x31);                 // out b, bit 1
    const u32 p1 = QT3(n5, b0, n6, 0xa1);                 // out a, bit 1
    const u32 q0 = QT3(b0, p0, a0, 0x16);                 // out b, bit 0
    a1 = p1; a0 = p0; b1 = q1; b0 = q0;
}

// Front padding (round 5: regions a few bases shorter than the nominal length share the nominal units).  An alignment whose
// region has p rows fewer than the unit starts p rows late: semi-global alignment starts from H(0, j) = 0 whatever came
// before, so until its first row it is simply HELD at the boundary state -- after each of the unit's first rows the dh
// planes of the alignments that have not started (mask hm) go back to 1 (bs_hold), the trailing columns' reversed DP, which
// meets those rows LAST, keeps the state it had after the alignment's own last row and hands out r = 0 for them
// (bs_keep; with r = 0 the deficit stays 0: D' = max(0 + 0 - a, 0)), and every alignment ends in the unit's last row.
BS_FN void bs_hold(u32& h1, u32& h0, u32 hm) { h1 &= ~hm; h0 |= hm; }
BS_FN void bs_keep(u32& h, u32 old, u32 hm) { h = bs_bfi(hm, old, h); }

// letter mismatch mask: planes (c1 c0) of the alignments' letters against the wave-uniform letter (L1 L0), each 0 / ~0
BS_FN u32 bs_neq(u32 c1, u32 c0, u32 L1, u32 L0) {
    return QB3(c1 ^ L1, c0, L0, x | (y ^ z));
}

// mismatch mask against a compile-time letter: one of the four masks a row has (the optimiser forms each once per row)
template <int LETTER>
BS_FN u32 bs_neq_static(u32 c1, u32 c0) {
    return LETTER == 0 ? (c1 | c0) : (LETTER == 1 ? (u32)QB3(c1, c0, c0, x | ~y) : (LETTER == 2 ? (u32)QB3(c1, c0, c0, ~x | y) : (u32)QB3(c1, c0, c0, ~(x & y))));
}
BS_FN u32 bs_neq_letter(int letter, u32 c1, u32 c0) {
    return letter == 0 ? bs_neq_static<0>(c1, c0) : (letter == 1 ? bs_neq_static<1>(c1, c0) : (letter == 2 ? bs_neq_static<2>(c1, c0) : bs_neq_static<3>(c1, c0)));
}

// UNSPLIT form.  F = deficit + 1 of the last column (F = 0 before the first row): F = max(F + 1 - a, 1) = F + 1 - min(a, F)
BS_FN void bs_deficit(u32 (&f)[BS_NF], u32 a1, u32 a0) {
    const u32 t1 = QB3(f[2], f[3], f[4], x | y | z), t2 = QB3(f[5], f[6], f[7], x | y | z);   // F >= 4
    const u32 g1 = QB3(t1, t2, f[1], x | y | z), g0 = QB3(t1, t2, f[0], x | y | z);           // min(F, 3)
    const u32 e1 = a1 & g1;                                                                    // min(a, F): bit 1
    const u32 same = QB3(a1, g1, g1, ~(x ^ y));
    const u32 pick = bs_bfi(a1, g0, a0);                                                       // a > F in bit 1: F's bit 0; else a's
    const u32 e0 = QB3(same, a0 & g0, pick, (x & y) | (~x & z));
    // F += 1 - e:  x = 1 - e in two's complement = (e1, ~e0), sign e1
    u32 c = QB3(f[0], e0, e0, x & ~y);
    f[0] = QB3(f[0], e0, e0, ~(x ^ y));
    {
        const u32 s1 = QB3(f[1], e1, c, x ^ y ^ z);
        c = QB3(f[1], e1, c, (x & y) | (x & z) | (y & z));
        f[1] = s1;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 2; k < BS_NF; ++k) {
        const u32 s = QB3(f[k], e1, c, x ^ y ^ z);
        if (k + 1 < BS_NF) c = QB3(f[k], e1, c, (x & y) | (x & z) | (y & z));
        f[k] = s;
    }
}

// SPLIT form.  D = (running maximum of G) - G(i) along the line in front of the trailing context, G(i) = H(i,c) + R(L-i,Q):
//       D' = max(D + r - a, 0),    a = dv(i,c) + 1 (this row's last own cell),  r = dvR(L-i+1) + 1 (the R row that pairs with it)
// D = 0 before the first row (G(0) = R(L,Q) is a path of its own).  t = r - a in [-3, 3] as (sign, t1, t0); x = D + t over
// seven planes and a sign; a negative x becomes 0.  23 instructions (the unsplit update is 25, with 7 more columns in front).
BS_FN void bs_deficit_split(u32 (&d)[BS_ND], u32 a1, u32 a0, u32 r1, u32 r0) {
    u32 s[BS_ND];
    s[0] = QB3(d[0], r0, a0, x ^ y ^ z);
    u32 c = QB3(d[0], r0, a0, x & (y ^ z));
    const u32 bw = QB3(r0, a0, a0, ~x & y);                                   // borrow of r0 - a0
    const u32 t1 = QB3(r1, a1, bw, x ^ y ^ z);
    const u32 sg = QB3(r1, a1, bw, (~x & y) | (~(x ^ y) & z));               // borrow out of bit 1 = sign of t
    s[1] = QB3(d[1], t1, c, x ^ y ^ z);
    c = QB3(d[1], t1, c, (x & y) | (x & z) | (y & z));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 2; k < BS_ND - 1; ++k) {
        s[k] = QB3(d[k], sg, c, x ^ y ^ z);
        c = QB3(d[k], sg, c, (x & y) | (x & z) | (y & z));
    }
    // the top plane and the sign of x are functions of (d[6], sg, c): x6 = d ^ sg ^ c, carry = maj, negative = sg ^ carry
    const u32 neg = QB3(d[BS_ND - 1], sg, c, y ^ ((x & y) | (x & z) | (y & z)));
    d[BS_ND - 1] = QB3(d[BS_ND - 1], sg, c, (x ^ y ^ z) & ~(y ^ ((x & y) | (x & z) | (y & z))));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < BS_ND - 1; ++k) d[k] = QB3(s[k], neg, neg, x & ~y);
}

// SPLIT form, the end of a barcode: r = H(L,c) + 64 (the last row summed up to the line), d = the deficit, rowbest = the
// last row's maximum over the columns <= c, cmax = max_j R(L,j): raw + 64 = max(r + d, rowbest, cmax) into rowbest
BS_FN void bs_finish_split(u32 (&rowbest)[BS_NB], u32 (&r)[BS_NB], const u32 (&d)[BS_ND], const u32 (&cmax)[BS_NB]) {
    static_assert(BS_ND == BS_NB, "one ripple over both");
    u32 c = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < BS_NB; ++q) {
        const u32 sum = QB3(r[q], d[q], c, x ^ y ^ z);
        c = QB3(r[q], d[q], c, (x & y) | (x & z) | (y & z));
        r[q] = sum;
    }
    bs_max(rowbest, r);
    bs_max(rowbest, cmax);
}

// UNSPLIT form, the end of a barcode: the last column's maximum = H(L,M) + deficit = r + F - 1 (mod 128: the value fits)
BS_FN void bs_finish(u32 (&rowbest)[BS_NB], u32 (&r)[BS_NB], const u32 (&f)[BS_NF]) {
    u32 c = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < BS_NB; ++q) {
        const u32 sum = QB3(r[q], f[q], c, x ^ y ^ z);
        c = QB3(r[q], f[q], c, (x & y) | (x & z) | (y & z));
        r[q] = sum;
    }
    u32 bw = ~r[0];
    r[0] = bw;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 1; q < BS_NB; ++q) { const u32 t = QB3(r[q], bw, bw, ~x & y); r[q] ^= bw; bw = t; }
    bs_max(rowbest, r);
}

// ---------------------------------------------------------------------------------------------
// The END of a barcode without a score counter per column (round 7).  After the row loops a barcode holds the C last-row
// codes  code_j = dh(L,j) + 1  of its own columns and the deficit D of the line in front of the trailing context, and needs
//       raw = max( H(L,c) + D,  max_{1<=j<=c} H(L,j),  cmax )                                  (c = P + C, see above).
// Stepping a 7-plane counter and taking a 7-plane maximum once per column (bs_step + bs_max: 41 instructions a column) is
// replaced by two cheaper walks over the codes:
//  * the row maximum as a DEFICIT.  E_j = max(rowbest0, max_{k<=j} H(L,k)) - H(L,j), rowbest0 = the maximum over the shared
//    columns.  E_j = max(E_{j-1} + 1 - code_j, 0) -- the recurrence of bs_deficit -- and the row maximum is H(L,c) + E_c.
//    Range: the maximum is attained in a column k in [1, j] and dh >= -1, so 0 <= E_j <= j - k <= j - 1 <= 62 for targets of
//    up to BS_MAX_TARGET = 63 columns: BS_NE = 6 planes, and E + 1 - min(code, E + 1) <= 63 inside the update.
//    E_P = rowbest0 - H(L,P) depends on the shared columns only (bs_last_row_start, once per unit).  A set without shared
//    columns has no column 0 candidate (H(L,0) = 0 is not a cell of the last row): its first own column sets E_1 = 0.
//  * H(L,c) as ONE sum.  H(L,c) + 64 = [H(L,P) + 64 - C] + sum_j code_j.  The bracket ("base") comes from the producer of the
//    shared columns: in [64 - P - C, 64 + P - C], within [1, 127] for P + C <= 63, seven planes.  The C low bits of the
//    codes and the C high bits are counted by carry-save trees (bs_popcount: a full adder is one parity and one majority
//    instruction; the two lowest planes of base ride along as the trees' spare carry inputs), at most 49 ones each for the
//    C <= 48 the kernels instantiate: six planes.  low + 2 high + 4 (base >> 2) is taken modulo 128; the value itself,
//    H(L,c) + 64, lies in [64 - c, 64 + c], within [1, 127].
// Then  raw + 64 = max( H(L,c) + 64 + max(D, E_c), cmax ):  H(L,c) + D = max_i G(i) <= M <= 63 and H(L,c) + E_c = the row
// maximum <= c <= 63, so the sum stays within seven planes.
// ---------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define BS_UNROLL _Pragma("unroll")
#define BS_PHASE_END() __builtin_amdgcn_sched_barrier(0)        // the scheduler keeps the phases of bs_last_row apart: what one needs is not live in the others
#else
#define BS_UNROLL
#define BS_PHASE_END() ((void)0)
#endif

constexpr int BS_NE = 6;                      // planes of the last row's deficit E in [0, 62]

// E' = max(E + 1 - a, 0) = E + 1 - m,  m = min(a, E + 1)  (a = dh + 1 of the last row's next column): 16 instructions
BS_FN void bs_rowmax_deficit(u32 (&e)[BS_NE], u32 a1, u32 a0) {
    const u32 hi = QB3(e[2], e[3], e[4], x | y | z);
    const u32 big = QB3(hi, e[5], e[1], x | y | z);                                           // E >= 2: m = a
    const u32 m1 = QB3(a1, big, e[0], x & (y | z));                                            // a >= 2 and E >= 1
    const u32 t = QB3(a0, big, e[0], (x & (y | ~z)) | (~x & ~y & ~z));                         // a = 3: E != 1; a = 2: E = 0
    const u32 m0 = bs_bfi(a1, t, a0);
    // E += 1 - m: in two's complement (.., m1, m1, ~m0)
    u32 c = QB3(e[0], m0, m0, x & ~y);
    e[0] = QB3(e[0], m0, m0, ~(x ^ y));
    BS_UNROLL
    for (int k = 1; k < BS_NE; ++k) {
        const u32 s = QB3(e[k], m1, c, x ^ y ^ z);
        if (k + 1 < BS_NE) c = QB3(e[k], m1, c, (x & y) | (x & z) | (y & z));
        e[k] = s;
    }
}

constexpr int bs_planes_of(int n) { int b = 0; while ((1 << b) <= n) ++b; return b; }         // planes that hold 0 .. n

// out (bs_planes_of(N) planes) = how many of the N words in[] have the bit set, per bit: a tree of full adders -- the last
// word is the carry input of the adder that joins the counts of the two halves
template <int N>
BS_FN void bs_popcount(const u32* in, u32* out) {
    if constexpr (N == 1) {
        out[0] = in[0];
    } else if constexpr (N == 2) {
        out[0] = in[0] ^ in[1];
        out[1] = in[0] & in[1];
    } else {
        constexpr int NL = N / 2, NR = N - 1 - NL, WL = bs_planes_of(NL), WR = bs_planes_of(NR), W = bs_planes_of(N);
        static_assert(NL >= NR && NR >= 1 && W <= WL + 1, "the left count is the wider one");
        u32 l[WL], r[WR];
        bs_popcount<NL>(in, l);
        bs_popcount<NR>(in + NL, r);
        u32 c = in[N - 1];
        BS_UNROLL
        for (int k = 0; k < WL; ++k) {
            const bool more = k + 1 < W;                                                      // (the count fits W planes: no carry beyond)
            if (k < WR) {
                out[k] = QB3(l[k], r[k], c, x ^ y ^ z);
                if (more) c = QB3(l[k], r[k], c, (x & y) | (x & z) | (y & z));
            } else {
                out[k] = l[k] ^ c;
                if (more) c = l[k] & c;
            }
        }
        if (W > WL) out[WL] = c;
    }
}

// acc += y << SH modulo 2^BS_NB.  AW: planes of acc that can be set on entry, W: planes of y -- absent planes cost nothing
template <int AW, int W, int SH>
BS_FN void bs_add_planes(u32 (&acc)[BS_NB], const u32* y) {
    u32 c = 0u;
    bool carry = false;
    BS_UNROLL
    for (int k = SH; k < BS_NB; ++k) {
        const bool ha = k < AW, hy = k < SH + W, last = k + 1 == BS_NB;
        if (ha && hy && carry) {
            const u32 s = QB3(acc[k], y[k - SH], c, x ^ y ^ z);
            if (!last) c = QB3(acc[k], y[k - SH], c, (x & y) | (x & z) | (y & z));
            acc[k] = s;
        } else if (ha && (hy || carry)) {
            const u32 o = hy ? y[k - SH] : c;
            const u32 s = acc[k] ^ o;
            if (!last) c = acc[k] & o;
            acc[k] = s;
            carry = true;
        } else if (hy && carry) {
            acc[k] = y[k - SH] ^ c;
            if (!last) c = y[k - SH] & c;
        } else if (hy || carry) {
            acc[k] = hy ? y[k - SH] : c;
            carry = false;
        }
    }
}

// what the producer of the shared columns leaves for bs_last_row: base = H(L,P) + 64 - C and E_P = rowbest0 - H(L,P), from the
// last-row codes (h1 h0) of the P shared columns and the number C of own columns.  P = 0: base = 64 - C, E = 0.
BS_FN void bs_last_row_start(u32 (&base)[BS_NB], u32 (&e)[BS_NE], const u32* h1, const u32* h0, int P, int C) {
    u32 best[BS_NB];
    BS_UNROLL
    for (int q = 0; q < BS_NB; ++q) { base[q] = ((BS_OFF - C) >> q) & 1 ? 0xFFFFFFFFu : 0u; best[q] = 0u; }
    BS_UNROLL
    for (int j = 0; j < P; ++j) { bs_step(base, h1[j], h0[j]); bs_max(best, base); }         // (base >= 64 - C - P >= 1 > the start of best)
    u32 bw = 0u;
    BS_UNROLL
    for (int q = 0; q < BS_NE; ++q) {
        e[q] = P > 0 ? (u32)QB3(best[q], base[q], bw, x ^ y ^ z) : 0u;
        bw = QB3(best[q], base[q], bw, (~x & y) | (~(x ^ y) & z));
    }
}

// the end of a barcode: raw + 64 = max(H(L,c) + 64 + max(D, E_c), cmax) from the C last-row codes (h1 h0), the deficit d and
// the unit's tail (header comment above): tail(q) = plane q of base, tail(BS_NB + q) = plane q of E_P -- both as
// bs_last_row_start leaves them -- and tail(2 BS_NB + q) = plane q of cmax = max_j R(L,j) + 64; each is fetched where it is
// needed.  SHARED: the set has shared columns.
template <int C, bool SHARED, class TAIL>
BS_FN void bs_last_row(u32 (&raw)[BS_NB], const u32 (&h1)[C], const u32 (&h0)[C], TAIL tail, const u32 (&d)[BS_ND]) {
    static_assert(BS_ND == BS_NB && BS_NE == BS_NB - 1, "the maximum of D and E below");
    constexpr int WP = bs_planes_of(C + 1);
    static_assert(C >= 2 && WP + 1 <= BS_NB, "the two counts of code bits fit the score planes");
    u32 e[BS_NE];
    BS_UNROLL
    for (int q = 0; q < BS_NE; ++q) e[q] = tail(BS_NB + q);
    BS_UNROLL
    for (int j = SHARED ? 0 : 1; j < C; ++j) bs_rowmax_deficit(e, h1[j], h0[j]);
    BS_PHASE_END();
    u32 base[BS_NB];
    BS_UNROLL
    for (int q = 0; q < BS_NB; ++q) base[q] = tail(q);
    u32 lo[C + 1], hi[C + 1], cl[WP], ch[WP];
    BS_UNROLL
    for (int j = 0; j < C; ++j) { lo[j] = h0[j]; hi[j] = h1[j]; }
    lo[C] = base[0]; hi[C] = base[1];
    bs_popcount<C + 1>(lo, cl);
    bs_popcount<C + 1>(hi, ch);
    BS_UNROLL
    for (int q = 0; q < BS_NB; ++q) raw[q] = q < WP ? cl[q] : 0u;
    bs_add_planes<WP, WP, 1>(raw, ch);
    bs_add_planes<(WP + 2 < BS_NB ? WP + 2 : BS_NB), BS_NB - 2, 2>(raw, &base[2]);            // raw = H(L,c) + 64
    BS_PHASE_END();
    // max(D, E): E has no top plane
    u32 gt = QB3(e[BS_NE - 1], d[BS_NE - 1], d[BS_NE], x & ~y & ~z);
    u32 eq = QB3(e[BS_NE - 1], d[BS_NE - 1], d[BS_NE], ~(x ^ y) & ~z);
    BS_UNROLL
    for (int k = BS_NE - 2; k >= 0; --k) {
        gt |= QB3(eq, e[k], d[k], x & y & ~z);
        if (k) eq = QB3(eq, e[k], d[k], x & ~(y ^ z));
    }
    u32 c = 0u;
    BS_UNROLL
    for (int q = 0; q < BS_NB; ++q) {
        const u32 m = q < BS_NE ? bs_bfi(gt, e[q], d[q]) : d[q];
        const u32 s = q ? (u32)QB3(raw[q], m, c, x ^ y ^ z) : raw[q] ^ m;
        if (q + 1 < BS_NB) c = q ? (u32)QB3(raw[q], m, c, (x & y) | (x & z) | (y & z)) : raw[q] & m;
        raw[q] = s;
    }
    u32 cmax[BS_NB];
    BS_UNROLL
    for (int q = 0; q < BS_NB; ++q) cmax[q] = tail(2 * BS_NB + q);
    bs_max(raw, cmax);
}

// ---------------------------------------------------------------------------------------------
// 32 x 32 bit matrix in registers, transposed in place: out[b] bit k = in[k] bit b (five butterfly stages of 16 word pairs,
// a shift and a bit-field insert per word)
BS_FN void bs_transpose32(u32 (&a)[32]) {
    BS_UNROLL
    for (int s = 0; s < 5; ++s) {
        const int j = 16 >> s;
        const u32 m = s == 0 ? 0x0000FFFFu : (s == 1 ? 0x00FF00FFu : (s == 2 ? 0x0F0F0F0Fu : (s == 3 ? 0x33333333u : 0x55555555u)));
        BS_UNROLL
        for (int k = 0; k < 32; ++k) {
            if (k & j) continue;
            const u32 lo = a[k], hi = a[k + j];
            a[k] = bs_bfi(m, lo, hi << j);
            a[k + j] = bs_bfi(m, lo >> j, hi);
        }
    }
}

// The hand-over of a wave's best (raw + 64, barcode index) planes as one key per alignment: the key of kernels_packed.inc,
//       barcode_key(raw, b) = (raw + 32768) << 16 | (1023 - b),
// is itself a bit pattern of the planes.  With v = raw + 64 in [0, 127]: raw + 32768 = 0x7FC0 + v = (v & 63) | (v6 ? 0x8000 :
// 0x7FC0) -- bits 0..5 are v's, bits 6..14 are ~v6, bit 15 is v6 -- and 1023 - b = ~b in ten bits for b < 128.  So the 32 rows
// below, transposed, are the 32 keys of a lane: no bit is picked out of a plane word one alignment at a time.
BS_FN void bs_keys32(u32 (&key)[32], const u32 (&bestv)[BS_NB], const u32 (&besti)[BS_NB]) {
    BS_UNROLL
    for (int q = 0; q < 32; ++q) {
        u32 w;
        if (q < BS_NB) w = ~besti[q];
        else if (q < 10) w = 0xFFFFFFFFu;
        else if (q < 16) w = 0u;
        else if (q < 16 + BS_NB - 1) w = bestv[q - 16];
        else if (q < 31) w = ~bestv[BS_NB - 1];
        else w = bestv[BS_NB - 1];
        key[q] = w;
    }
    bs_transpose32(key);
}

}  // namespace qk
#endif

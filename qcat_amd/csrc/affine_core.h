// affine_core.h -- the ADAPTER DP with affine gap costs (Gotoh) in packed 16-bit lanes, two alignments per 32-bit word, as
// pure functions that compile for the device and for the host.  No kernel of the library uses it yet (DESIGN.md 3.6b:
// kits with gap_open != gap_extend still run k_scan_generic); the host check tests/affine_host_check.cpp (plain g++)
// drives it row by row against the scalar DPs.
//
// Semantics: those of dev_sg_generic (kernels_generic.inc) -- a gap of k letters costs open + (k - 1) * extend, E and F
// start at minus infinity, the ends are free on all four borders, score and end_query under rule R1.
//
// With e = extend, o = open, d = o - e (d may be negative) and every cell biased by e * (i + j), X' = X + e * (i + j):
//       E'(i,j) = max(E'(i,j-1), H'(i,j-1) - d)
//       F'(i,j) = max(F'(i-1,j), H'(i-1,j) - d)
//       H'(i,j) = max(H'(i-1,j-1) + W', E'(i,j), F'(i,j)),      W' = w + 2e
//       H'(i,0) = e * i,  H'(0,j) = e * j
// * No infinities: E'(i,0) = H'(i,0) - d and F'(0,j) = H'(0,j) - d give the exact first step (E(i,1) = H(i,0) - o).
// * W' may be clamped from below at -2d: H(i,j) >= H(i-1,j-1) - 2o always (one gap of each kind; at the borders one
//   of them is free), that is H'(i,j) >= H'(i-1,j-1) - 2d, so a diagonal term below that never decides a cell.
// * Lower bounds: H(i,j) >= -o - (min(i,j) - 1) * e  =>  H'(i,j) >= e * max(i,j) - d >= -max(d, 0), and the same for
//   E' and F'.  Values can be negative: the lanes are SIGNED 16-bit (v_pk_add_i16 / v_pk_sub_i16 / v_pk_max_i16).
//
// Lane format.  With ad = |d|, D = max(d, 0), TB = 2D (so that TB - d = ad), one lane half keeps
//       S(i,j)  = H'(i,j) + ad          the gap source: what E' and F' take their maxima over, up to the shift below
//       FZ(i,j) = F'(i,j) + TB,  EZ = E'(i,j) + TB            =>  FZ = max(FZ, S_up), EZ = max(EZ, S_left)
//       T       = max(W', -2d) + TB  in [0, 255]               the score table byte, looked up with v_perm_b32
//       hz      = max(H'(i-1,j-1) + T, EZ, FZ) = H'(i,j) + TB,  S(i,j) = hz - (TB - ad)
// which is 8 packed operations per column and row (two cells): perm, add, sub (the diagonal H' = S - ad), three max for
// E / F / H... one more max and the final sub.
//
// Range (aff_range_ok): every lane value lies in [-D, top + 2 * ad], top = maxw * min(R, C) + e * (R + C) for R rows
// and C columns (H <= maxw * min(i,j); S, EZ, FZ <= top + ad; hz and the diagonal term <= top + TB).
//
// Rows beyond a lane half's own window length (ragged tiles): the half's S and F rows are FROZEN from row L + 1 on
// (one v_bfi_b32 per register), so the last row is read after the loop; a frozen row's last-column value only falls
// (the row constant e * i grows, or its key 255 - i falls), so it never enters the last-column maximum.  A wave whose
// windows all have one length runs the instantiation without the masks.
#ifndef QCAT_AFFINE_CORE_H
#define QCAT_AFFINE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define AFF_FN __host__ __device__ __forceinline__
#define AFF_UNROLL _Pragma("unroll")
#else
#define AFF_FN inline
#define AFF_UNROLL
#endif

namespace qk {

typedef uint32_t u32;

constexpr int AFF_PADMAX = 8;           // most leading padding columns of a width class (kit.h PADMAX)
#define AFF_SEL_KEY_LO 0x0C050400u      /* [c, v.b0, v.b1, 0]: (lo half of v) << 8 | c */
#define AFF_SEL_KEY_HI 0x0C070600u      /* [c, v.b2, v.b3, 0]: (hi half of v) << 8 | c */

struct AffCost {
    int e, d, ad, D, TB, csrc;          // extend, open - extend, |d|, max(d, 0), 2D, TB - ad
};
AFF_FN AffCost aff_cost(int open, int extend) {
    AffCost c;
    c.e = extend; c.d = open - extend; c.ad = c.d < 0 ? -c.d : c.d; c.D = c.d > 0 ? c.d : 0; c.TB = 2 * c.D; c.csrc = c.TB - c.ad;
    return c;
}
// the table value of a substitution score w (a byte when the kit is in range)
AFF_FN int aff_table_value(int w, const AffCost& c) {
    int v = w + 2 * c.e;
    if (v < -2 * c.d) v = -2 * c.d;
    return v + c.TB;
}
// do all lane values of a DP of `rows` x `cols` cells with substitution scores <= maxw fit signed 16-bit lanes, and the
// table values a byte?  Lowest value -D, highest top + 2 * ad (see above).
AFF_FN bool aff_range_ok(int maxw, int minw, int open, int extend, int rows, int cols) {
    const AffCost c = aff_cost(open, extend);
    if (maxw < 0) maxw = 0;
    const int64_t top = (int64_t)maxw * (rows < cols ? rows : cols) + (int64_t)c.e * (rows + cols);
    if (top + 2 * (int64_t)c.ad > 32767 || c.D > 32767) return false;
    return aff_table_value(maxw, c) <= 255 && aff_table_value(minw, c) >= 0;
}

// ---- packed operations on two 16-bit halves ---------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef short aff_ss2 __attribute__((ext_vector_type(2)));
typedef unsigned short aff_us2 __attribute__((ext_vector_type(2)));
AFF_FN u32 aff_add(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(aff_ss2, a) + __builtin_bit_cast(aff_ss2, b)); }
AFF_FN u32 aff_sub(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(aff_ss2, a) - __builtin_bit_cast(aff_ss2, b)); }
AFF_FN u32 aff_max(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(aff_ss2, a), __builtin_bit_cast(aff_ss2, b))); }
AFF_FN u32 aff_subsat_u(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_elementwise_sub_sat(__builtin_bit_cast(aff_us2, a), __builtin_bit_cast(aff_us2, b))); }
AFF_FN u32 aff_perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#else
AFF_FN u32 aff_add(u32 a, u32 b) { return ((a + b) & 0xFFFFu) | (((a >> 16) + (b >> 16)) << 16); }
AFF_FN u32 aff_sub(u32 a, u32 b) { return ((a - b) & 0xFFFFu) | (((a >> 16) - (b >> 16)) << 16); }
AFF_FN u32 aff_max(u32 a, u32 b) {
    const int16_t al = (int16_t)(a & 0xFFFFu), bl = (int16_t)(b & 0xFFFFu), ah = (int16_t)(a >> 16), bh = (int16_t)(b >> 16);
    return (u32)(uint16_t)(al > bl ? al : bl) | ((u32)(uint16_t)(ah > bh ? ah : bh) << 16);
}
AFF_FN u32 aff_subsat_u(u32 a, u32 b) {
    const u32 al = a & 0xFFFFu, bl = b & 0xFFFFu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al - bl : 0u) | ((ah > bh ? ah - bh : 0u) << 16);
}
// v_perm_b32: byte k of the result is byte sel.k of {hi, lo} (0..3: lo, 4..7: hi), 0x0C: 0x00, 0x0D and above: 0xFF
AFF_FN u32 aff_perm(u32 hi, u32 lo, u32 sel) {
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    u32 r = 0;
    for (int k = 0; k < 4; ++k) {
        const u32 s = (sel >> (8 * k)) & 0xFFu;
        const u32 b = s <= 7 ? (u32)((src >> (8 * s)) & 0xFFu) : (s >= 0x0D ? 0xFFu : 0u);
        r |= b << (8 * k);
    }
    return r;
}
#endif
AFF_FN u32 aff_bfi(u32 mask, u32 a, u32 b) { return (a & mask) | (b & ~mask); }        // v_bfi_b32
AFF_FN u32 aff_splat(int v) { const u32 x = (u32)v & 0xFFFFu; return x | (x << 16); }
AFF_FN u32 aff_umax(u32 a, u32 b) { return a > b ? a : b; }
// selector of v_perm_b32 for one query row byte (code of the lo window | code of the hi window << 4): two zero-extended
// table bytes (kernels_packed.inc make_sel)
AFF_FN u32 aff_sel(u32 qb) { return (((qb << 12) | qb) & 0x000F000Fu) | 0x0C000C00u; }
// which halves of a lane are still inside their windows at row i
AFF_FN u32 aff_row_mask(int i, int L0, int L1) { return (i <= L0 ? 0x0000FFFFu : 0u) | (i <= L1 ? 0xFFFF0000u : 0u); }

// ---- the DP: W columns, the template of M = W - start letters right-aligned ----------------------------------------------
// Columns 1 .. start are padding and are skipped (wave-uniformly): column start + 1 then sees exactly the free boundary --
// H'(i,0) = e * i as its left and diagonal neighbours and E' = H'(i,0) - d.

// row 0: S(0,j) = e * jr + ad and FZ(0,j) = F'(0,j) + TB = e * jr - d + TB, the same number (jr = j - start)
template <int W>
AFF_FN void aff_init(u32 (&S)[W + 1], u32 (&F)[W + 1], int start, const AffCost& c) {
    const u32 e2 = aff_splat(c.e);
    u32 r = aff_splat(c.ad - c.e * start);
    S[0] = F[0] = 0;
AFF_UNROLL
    for (int j = 1; j <= W; ++j) { r = aff_add(r, e2); S[j] = r; F[j] = r; }
}

// row i (1-based) for both halves; tbl(j) = the table dword of column j + 1 (tbl.fence(j): a hook in front of column j's
// read, for tables in the LDS), PADCAP = the most padding columns the caller can have, sel = aff_sel(row byte), special = the pool
// of the query codes N, X, other, PAD.  RAGGED: halves outside `mask` keep their rows.  Returns S(i, W).
template <int W, bool RAGGED, int PADCAP = AFF_PADMAX, class Tbl>
AFF_FN u32 aff_row(u32 (&S)[W + 1], u32 (&F)[W + 1], int start, int i, u32 sel, u32 special, const Tbl& tbl,
                   const AffCost& c, u32 ad2, u32 csrc2, u32 mask) {
    const u32 s0 = aff_splat(c.e * i + c.ad);
    u32 carry = aff_splat(c.e * (i - 1)), E = s0, sleft = s0;
AFF_UNROLL
    for (int j = 1; j <= W; ++j) {
        if (j <= PADCAP && j <= start) continue;
        tbl.fence(j);
        const u32 T = aff_perm(special, tbl(j - 1), sel);
        const u32 u = S[j];
        u32 f = aff_max(F[j], u);
        const u32 dg = aff_add(carry, T);
        carry = aff_sub(u, ad2);
        E = aff_max(E, sleft);
        u32 sn = aff_sub(aff_max(aff_max(dg, E), f), csrc2);
        if (RAGGED) { sn = aff_bfi(mask, sn, u); f = aff_bfi(mask, f, F[j]); }
        S[j] = sn; F[j] = f; sleft = sn;
    }
    return sleft;
}

// last-column keys: ((H(i,M) + e * M + D) << 8) | (255 - i), the maximum keeps the first row of the best value
AFF_FN void aff_col_keys(u32 sW, int i, const AffCost& c, u32 (&ck)[2]) {
    const u32 v = aff_subsat_u(sW, aff_splat(c.e * i + c.ad - c.D));
    const u32 ci = (u32)(255 - i);
    ck[0] = aff_umax(ck[0], aff_perm(v, ci, AFF_SEL_KEY_LO));
    ck[1] = aff_umax(ck[1], aff_perm(v, ci, AFF_SEL_KEY_HI));
}

// last-row keys after the loop: ((H(L,j) + e * L + D + 1) << 8) | (255 - j), first column of the best value
template <int W, int PADCAP = AFF_PADMAX>
AFF_FN void aff_row_keys(const u32 (&S)[W + 1], int start, const AffCost& c, u32 (&rk)[2]) {
    const u32 e2 = aff_splat(c.e);
    u32 r = aff_splat(c.ad - c.D - 1 - c.e * start);
    rk[0] = rk[1] = 0;
AFF_UNROLL
    for (int j = 1; j <= W; ++j) {
        r = aff_add(r, e2);
        if (j <= PADCAP && j <= start) continue;
        const u32 v = aff_sub(S[j], r);
        const u32 cj = (u32)(255 - j);
        rk[0] = aff_umax(rk[0], aff_perm(v, cj, AFF_SEL_KEY_LO));
        rk[1] = aff_umax(rk[1], aff_perm(v, cj, AFF_SEL_KEY_HI));
    }
}

// Score tables of one template (codes t[0..m), matrix [target * 7 + query]) right-aligned in `width` dwords, one byte per
// query letter A, T, G, C; the query codes N, X and other must score the same against every column and go to the shared
// pool *special (0xFFFFFFFF: not set yet; its PAD byte is 0 -- rows of PAD letters are frozen rows).  False: not
// representable (a value outside a byte, a column with a pool of its own).
inline bool aff_build_table(const int8_t* mat, const uint8_t* t, int m, const AffCost& c, u32* out, u32* special, int width) {
    for (int j = 0; j < width - m; ++j) out[j] = 0;
    out += width - m;
    for (int j = 0; j < m; ++j) {
        u32 w = 0, sp = 0;
        for (int q = 0; q < 7; ++q) {
            const int v = aff_table_value(mat[t[j] * 7 + q], c);
            if (v < 0 || v > 255) return false;
            if (q < 4) w |= (u32)v << (8 * q); else sp |= (u32)v << (8 * (q - 4));
        }
        out[j] = w;
        if (*special == 0xFFFFFFFFu) *special = sp;
        else if (*special != sp) return false;
    }
    return true;
}

// score and end_query of one half under rule R1 (include/qcat_hip.h QCAT_R1_*), from its two keys (L >= 1)
struct AffResult { int score, end_query; };
AFF_FN AffResult aff_decode(u32 rk, u32 ck, int L, int M, int start, const AffCost& c, bool r1_scalar) {
    const int vr = (int)(rk >> 8) - 1 - c.D, jr = 255 - (int)(rk & 255u) - start;
    const int vc = (int)(ck >> 8) - c.D, ic = 255 - (int)(ck & 255u);
    const int s_row = vr - c.e * L, s_col = vc - c.e * M;
    const bool col = s_col > s_row || (s_col == s_row && (jr == M || r1_scalar));
    AffResult r;
    r.score = col ? s_col : s_row;
    r.end_query = col ? ic - 1 : L - 1;
    return r;
}

}  // namespace qk

#endif

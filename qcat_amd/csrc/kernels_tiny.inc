// kernels_tiny.inc -- the scan of a HANDFUL of read ends (the reference's library call: detect_barcode on one read,
// qcat/scanner_base.py:521-604; qcat/test/test_barcode.py:84): one WAVE per alignment, its lanes along an anti-diagonal.
//
// The throughput kernels put 128 (binary16) or 2048 (bit-sliced) alignments on a wave and walk each one cell by cell: with
// two windows in the batch that is one wave walking 150 x 60 cells while the chip idles -- 64 us for the adapter pair and
// 110 us for the 96 barcodes of a PBC096 call (tools/api1_trace.sh).  Here lane l of a wave owns target column l + 1 (and
// l + 65: templates of up to 128 letters) and the wave steps through the anti-diagonals d = i + j: L + M steps instead of
// L x M, every (read end, template) and every (read end, set, barcode) on a wave of its own -- 192 waves for a PBC096 read,
// a fifth of the chip's SIMDs, each for ~100-200 steps.
//
//   k_tiny_adapter  one wave per (read end, template)      -> tiny_tpl[end][template] = (raw, end_query)
//   k_tiny_decide   one thread per read end                -> EndRec: template choice, region path, regions (as k_scan_generic)
//   k_tiny_barcode  one wave per (read end, set, barcode)   -> tiny_sc[end][set][barcode] = raw
//   k_tiny_select   one wave per (read end, set)           -> EndRec: rule R2 over the scores in list order
//
// then k_finalize as after every other scan kernel.  int32 cells, any 7 x 7 matrix.  Read-end scans run LINEAR gaps (open ==
// extend: the adapter scoring of every shipped configuration, and the barcode scoring always; with open == extend Gotoh's
// three matrices collapse to H(i,j) = max(H(i-1,j-1) + W, H(i-1,j) - g, H(i,j-1) - g)).  Same records as k_scan_generic by
// construction -- the decision code IS that kernel's -- and checked against the oracle like every other path
// (tests/test_tiny_gpu.py: every intermediate through qcat_scan_debug).
//
// Whole sequences (qcat_scan_sequences) and plain pairs (qcat_sg_align) use the same wave with every configuration:
//   k_tiny_adapter_affine   k_tiny_adapter under Gotoh's recurrences (gap_open != gap_extend; the barcode waves stay linear 1/1)
//   k_tiny_simple_barcode   simple mode: one wave per (sequence, barcode of the list), the barcode's own length -> (raw, end_query)
//   k_tiny_simple_select    simple mode: one wave per sequence, rule R2 over the normalised scores in list order -> EndRec
//   k_sg_wave               one wave per (query, target) pair from ASCII, linear or affine, either R1 rule -> qcat_alignment
// (tests/test_wave_configs_gpu.py; the affine cell on the host: wave_core.h, tests/wave_affine_check.cpp).
// Included by qcat_hip.hip after kernels_generic.inc.

#include "wave_core.h"

namespace qk {

constexpr int TINY_BIAS = 1 << 20;            // cells are kept biased: the last row's key is an unsigned compare
constexpr int TINY_MAX_WAVES = 20000;          // alignments (= waves) of a batch up to which the scan takes this path (option TINY_MAX_ENDS: a limit in read ends instead)

// lane l receives lane l - 1's value; lane 0 receives `first` (v_mov_b32_dpp wave_shr:1 -- one instruction, no LDS)
__device__ __forceinline__ int tiny_from_left(int first, int v) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

struct TinyCol {                              // one target column of a lane
    uint64_t tbl;                             // W(query code 0..6, this column's letter): seven signed bytes
    int up, diag, h;                          // H(i-1, j) and H(i-1, j-1), biased; h: what this lane shows its neighbour (its last cell)
    int letter;                               // query code of the row this lane is on (travels from lane to lane beside the cells)
    int row_last;                             // H(L, j), biased
    int cmax, ci;                             // running maximum of this column over the rows and the FIRST row reaching it
};

__device__ __forceinline__ void tiny_col_init(TinyCol& c, const uint8_t* __restrict__ t, int j, int M, const int8_t* mat) {
    const int tj = j <= M ? (int)t[j - 1] : 0;
    uint64_t tbl = 0;
#pragma unroll
    for (int qc = 0; qc < 7; ++qc) tbl |= (uint64_t)(uint8_t)mat[tj * 7 + qc] << (8 * qc);
    c.tbl = tbl; c.up = TINY_BIAS; c.diag = TINY_BIAS; c.h = TINY_BIAS; c.letter = 0; c.row_last = 0; c.cmax = GEN_NEG; c.ci = 0;
}

// one cell of column j at row i (any i: rows outside 1..L leave the boundary value 0 and touch no result); `left` is the
// neighbour column's cell of the same row, `qc` the row's letter -- which does not depend on any cell, so that the score
// lookup stays off the chain cell -> neighbour -> cell
__device__ __forceinline__ void tiny_cell(TinyCol& c, int left, int qc, int i, int L, int g) {
    const int w = (int)(int8_t)(c.tbl >> (8 * qc));
    int h = max(c.diag + w, max(c.up, left) - g);
    const bool inside = i >= 1 && i <= L;
    h = i >= 1 ? h : TINY_BIAS;
    c.row_last = i == L ? h : c.row_last;
    const bool better = inside && (h - TINY_BIAS) > c.cmax;
    c.cmax = better ? h - TINY_BIAS : c.cmax;
    c.ci = better ? i : c.ci;
    c.diag = left; c.up = h;
    c.h = h;
}

// Semi-global alignment of q[0, L) (codes, one byte each) against t[0, M), all end gaps free, linear gap g, on ONE wave;
// the result (rule R1: the last row's maximum at its first column, then the last column's at its first row, the column
// winning ties only when the row's maximum sits in the last column -- dev_sg_generic above) in every lane.
template <bool TWO /* M > 64 */, class Q>
__device__ inline DevAlign dev_sg_wave(const Q q, int L, const uint8_t* __restrict__ t, int M, int g, const int8_t* mat, int lane, bool r1_scalar = false) {
    TinyCol a, b;
    tiny_col_init(a, t, lane + 1, M, mat);
    if (TWO) tiny_col_init(b, t, lane + 65, M, mat);
    int ia = 1 - (lane + 1);                                   // row of column lane + 1 on anti-diagonal d = 2 is 2 - j; kept one behind, incremented first
    // the query's letters in blocks of 64 rows, one register per block and one block ahead (lane l of a block holds row
    // 64 * block + l + 1): a step reads its row's letter with one v_readlane instead of waiting for memory inside the loop;
    // any query length (windows: at most 160 letters; whole sequences, qcat_scan_sequences: whatever they are)
    int q_cur = lane < L ? q(lane) : 0, q_next = lane + 64 < L ? q(lane + 64) : 0;
    for (int d = 2; d <= L + M; ++d) {
        ++ia;                                                   // ia = d - (lane + 1)
        // column 1 is on row d - 1: its letter enters at lane 0, every other lane takes the letter of its left neighbour's
        // last step (the same row)
        const int r = d - 2;
        if (r > 0 && (r & 63) == 0) { q_cur = q_next; q_next = r + 64 + lane < L ? q(r + 64 + lane) : 0; }
        const int first = __builtin_amdgcn_readlane(q_cur, r & 63);
        int carry_l = 0, carry_h = 0;
        if (TWO) { carry_l = __builtin_amdgcn_readlane(a.letter, 63); carry_h = __builtin_amdgcn_readlane(a.h, 63); }   // column 64 -> column 65
        a.letter = tiny_from_left(first, a.letter);
        const int left_a = tiny_from_left(TINY_BIAS, a.h);      // H(i, 0) = 0 in front of column 1
        tiny_cell(a, left_a, a.letter, ia, L, g);
        if (TWO) {
            b.letter = tiny_from_left(carry_l, b.letter);
            const int left_b = tiny_from_left(carry_h, b.h);
            tiny_cell(b, left_b, b.letter, ia - 64, L, g);
        }
    }
    // last row: the largest value, the smallest column among equals
    unsigned key = lane + 1 <= M ? ((unsigned)a.row_last << 8) | (unsigned)(255 - lane) : 0u;
    if (TWO) { const unsigned kb = lane + 65 <= M ? ((unsigned)b.row_last << 8) | (unsigned)(255 - (lane + 64)) : 0u; key = max(key, kb); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
    DevAlign r;
    r.score = (int)(key >> 8) - TINY_BIAS; r.end_r = 255 - (int)(key & 255u); r.end_q = L - 1;
    // last column: lane (M - 1) & 63 of the half that holds column M
    const int src = (M - 1) & 63;
    int cmax = __shfl(a.cmax, src, 64), ci = __shfl(a.ci, src, 64);
    if (TWO && M > 64) { cmax = __shfl(b.cmax, src, 64); ci = __shfl(b.ci, src, 64); }
    if (cmax > r.score || (cmax == r.score && (r.end_r == M - 1 || r1_scalar))) { r.score = cmax; r.end_r = M - 1; r.end_q = ci - 1; }   // (QCAT_R1_*)
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same wave under Gotoh's recurrences (gap_open != gap_extend) with dev_sg_generic's semantics: F (the gap that consumes
// query letters) is the same column one step earlier and stays in the lane, E comes from the left neighbour's last step beside
// h -- one more v_mov_b32_dpp, -inf in front of column 1; column 64 -> 65: one more v_readlane.  A routine of its own, so that
// the linear one above and every kernel built on it stay exactly the code they were; the column and its cell (wave_core.h)
// are plain C++ that the host check drives as well.
// ---------------------------------------------------------------------------------------------------------------------------
// Calls of the entry points that reach the wave since it took every configuration stay on the general kernels beyond these many
// alignments (option WAVE_MAX: another limit for all three).  tools/bench_waves.py, profiles/wave_configs_ab.txt: the waves win at
// every measured size (1 .. 100 000 sequences or pairs; the smallest margin 1.33 x, qcat_sg_align at 100 000 pairs, and falling
// with n there), so the limits are the largest sizes measured, not a crossover.
constexpr uint64_t WAVE_SG_MAX = 100000;           // qcat_sg_align without statistics: pairs
constexpr uint64_t WAVE_AFFINE_MAX = 100000;    // qcat_scan_sequences, gap_open != gap_extend: sequences
constexpr uint64_t WAVE_SIMPLE_MAX = 12000000;       // qcat_scan_sequences, simple lists: sequences x barcodes

static_assert(WAVE_BIAS == TINY_BIAS, "one bias for both cells");

template <bool TWO /* M > 64 */, class Q>
__device__ inline DevAlign dev_sg_wave_affine(const Q q, int L, const uint8_t* __restrict__ t, int M, int open, int ext, const int8_t* mat, int lane, bool r1_scalar) {
    WaveCol a, b;
    wave_col_init(a, t, lane + 1, M, mat);
    if (TWO) wave_col_init(b, t, lane + 65, M, mat);
    int ia = 1 - (lane + 1);
    int q_cur = lane < L ? q(lane) : 0, q_next = lane + 64 < L ? q(lane + 64) : 0;     // (the query's letters: as dev_sg_wave)
    for (int d = 2; d <= L + M; ++d) {
        ++ia;
        const int r = d - 2;
        if (r > 0 && (r & 63) == 0) { q_cur = q_next; q_next = r + 64 + lane < L ? q(r + 64 + lane) : 0; }
        const int first = __builtin_amdgcn_readlane(q_cur, r & 63);
        int carry_l = 0, carry_h = 0, carry_e = 0;
        if (TWO) { carry_l = __builtin_amdgcn_readlane(a.letter, 63); carry_h = __builtin_amdgcn_readlane(a.h, 63); carry_e = __builtin_amdgcn_readlane(a.e, 63); }
        a.letter = tiny_from_left(first, a.letter);
        const int left_h = tiny_from_left(TINY_BIAS, a.h), left_e = tiny_from_left(WAVE_NEG, a.e);   // H(i, 0) = 0, E(i, 0) = -inf
        wave_cell_affine(a, left_h, left_e, a.letter, ia, L, open, ext);
        if (TWO) {
            b.letter = tiny_from_left(carry_l, b.letter);
            const int lh = tiny_from_left(carry_h, b.h), le = tiny_from_left(carry_e, b.e);
            wave_cell_affine(b, lh, le, b.letter, ia - 64, L, open, ext);
        }
    }
    unsigned key = lane + 1 <= M ? ((unsigned)a.row_last << 8) | (unsigned)(255 - lane) : 0u;
    if (TWO) { const unsigned kb = lane + 65 <= M ? ((unsigned)b.row_last << 8) | (unsigned)(255 - (lane + 64)) : 0u; key = max(key, kb); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
    DevAlign r;
    r.score = (int)(key >> 8) - TINY_BIAS; r.end_r = 255 - (int)(key & 255u); r.end_q = L - 1;
    const int src = (M - 1) & 63;
    int cmax = __shfl(a.cmax, src, 64), ci = __shfl(a.ci, src, 64);
    if (TWO && M > 64) { cmax = __shfl(b.cmax, src, 64); ci = __shfl(b.ci, src, 64); }
    if (cmax > r.score || (cmax == r.score && (r.end_r == M - 1 || r1_scalar))) { r.score = cmax; r.end_r = M - 1; r.end_q = ci - 1; }   // (QCAT_R1_*)
    return r;
}

struct TinyArgs {
    KitPtrs kp;
    const uint8_t* win; const int32_t* wlen;       // byte windows (k_pack_windows without the lazy switch)
    const uint8_t* seq; const uint64_t* seq_off;   // ... or, qcat_scan_sequences: whole sequences in ASCII, one "read end" each (win null)
    uint32_t n_ends;
    EndRec* recs;
    int32_t* tpl;                                   // [n_ends][MAX_T][2]: raw, end_query
    int16_t* sc;                                    // [n_ends][2][sc_stride]: raw score per barcode
    uint32_t sc_stride;
    int32_t* dbg_tpl; int16_t* dbg_rows; uint32_t dbg_stride;       // debug scans (qcat_scan_debug), or null
    int32_t adapter_only;
};

__device__ __forceinline__ int tiny_len(const TinyArgs& a, uint32_t e) {
    return a.win ? a.wlen[e] : (int)(a.seq_off[e + 1] - a.seq_off[e]);
}

__global__ void __launch_bounds__(64)
k_tiny_adapter(TinyArgs a) {
    __shared__ uint8_t wq[WIN_STRIDE];
    __shared__ int8_t amat[49];
    const DevKit* k = a.kp.kit;
    const uint32_t e = blockIdx.x / (uint32_t)k->nt;
    const int t = (int)(blockIdx.x % (uint32_t)k->nt), lane = (int)threadIdx.x;
    if (lane < 49) amat[lane] = k->amat[lane];
    if (a.win) for (int i = lane; i < WIN_STRIDE; i += 64) wq[i] = a.win[(size_t)e * WIN_STRIDE + i];
    __syncthreads();
    const int L = tiny_len(a, e);
    const DevTpl& p = k->tpl[t];
    DevAlign r; r.score = 0; r.end_q = -1; r.end_r = -1;
    if (L > 0) {
        const uint8_t* tc = a.kp.codes + p.code_off;
        const bool r1s = k->r1_scalar != 0;
        if (a.win) r = p.len > 64 ? dev_sg_wave<true>(WinSeq{wq}, L, tc, p.len, k->gap_open, amat, lane, r1s)
                                  : dev_sg_wave<false>(WinSeq{wq}, L, tc, p.len, k->gap_open, amat, lane, r1s);
        else {
            const AsciiSeq q{a.seq + a.seq_off[e]};
            r = p.len > 64 ? dev_sg_wave<true>(q, L, tc, p.len, k->gap_open, amat, lane, r1s)
                           : dev_sg_wave<false>(q, L, tc, p.len, k->gap_open, amat, lane, r1s);
        }
    }
    if (lane == 0) { a.tpl[((size_t)e * MAX_T + t) * 2] = r.score; a.tpl[((size_t)e * MAX_T + t) * 2 + 1] = r.end_q; }
}

// the same for a kit whose gap_open != gap_extend, whole sequences only (qcat_scan_sequences: a.seq).  A kernel of its own and
// not a branch in k_tiny_adapter: that kernel is the latency path of detect_barcode on one read and keeps its code
__global__ void __launch_bounds__(64)
k_tiny_adapter_affine(TinyArgs a) {
    __shared__ int8_t amat[49];
    const DevKit* k = a.kp.kit;
    const uint32_t e = blockIdx.x / (uint32_t)k->nt;
    const int t = (int)(blockIdx.x % (uint32_t)k->nt), lane = (int)threadIdx.x;
    if (lane < 49) amat[lane] = k->amat[lane];
    __syncthreads();
    const int L = tiny_len(a, e);
    const DevTpl& p = k->tpl[t];
    DevAlign r; r.score = 0; r.end_q = -1; r.end_r = -1;
    if (L > 0) {
        const AsciiSeq q{a.seq + a.seq_off[e]};
        const uint8_t* tc = a.kp.codes + p.code_off;
        r = p.len > 64 ? dev_sg_wave_affine<true>(q, L, tc, p.len, k->gap_open, k->gap_extend, amat, lane, k->r1_scalar != 0)
                       : dev_sg_wave_affine<false>(q, L, tc, p.len, k->gap_open, k->gap_extend, amat, lane, k->r1_scalar != 0);
    }
    if (lane == 0) { a.tpl[((size_t)e * MAX_T + t) * 2] = r.score; a.tpl[((size_t)e * MAX_T + t) * 2 + 1] = r.end_q; }
}

// find_best_adapter_template + the region decision of scan(), one thread per read end: k_scan_generic's own lines over the
// scores k_tiny_adapter left
__global__ void __launch_bounds__(64)
k_tiny_decide(TinyArgs a) {
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n_ends) return;
    const DevKit* k = a.kp.kit;
    const int L = tiny_len(a, e);
    int best = -1, best_end = -1, best_raw = -1, best_den = 100;     // -1.0 == -1*100/100
    if (L > 0) {
        for (int t = 0; t < k->nt; ++t) {
            const DevTpl& p = k->tpl[t];
            const int raw = a.tpl[((size_t)e * MAX_T + t) * 2], end_q = a.tpl[((size_t)e * MAX_T + t) * 2 + 1];
            if (a.dbg_tpl) {
                a.dbg_tpl[((size_t)e * 2 + 0) * MAX_T + t] = raw;
                a.dbg_tpl[((size_t)e * 2 + 1) * MAX_T + t] = end_q;
            }
            if ((int64_t)best_raw * p.den < (int64_t)raw * best_den) { best = t; best_end = end_q; best_raw = raw; best_den = p.den; }
        }
    }
    EndRec r;
    r.window_len = L; r.best_tpl = best; r.best_end = best_end; r.best_raw = best_raw;
    r.used_tpl = best < 0 ? k->nt - 1 : best;
    const DevTpl& p = k->tpl[r.used_tpl];
    const bool dual = k->mode == QCAT_MODE_DUAL;
    r.region_path = (dual || p.is_double || (best >= 0 && best_raw >= p.region_min_raw)) ? 1 : 0;
    for (int s = 0; s < 2; ++s) { r.region_start[s] = 0; r.region_len[s] = 0; r.bc_idx[s] = -1; r.bc_raw[s] = 0; }
    const int nsets = a.adapter_only ? 0 : (dual ? 2 : 1);
    for (int s = 0; s < nsets; ++s) {
        if (r.region_path) dev_region(p.len, p.bc_end[s], p.bc_len[s], k->ext, best_end, L, &r.region_start[s], &r.region_len[s]);
        else { r.region_start[s] = 0; r.region_len[s] = L < k->max_align ? L : k->max_align; }
    }
    a.recs[e] = r;
}

// grid: (barcode, read end * 2 + set); a wave whose barcode index lies beyond the set of the template this end uses leaves
__global__ void __launch_bounds__(64)
k_tiny_barcode(TinyArgs a) {
    __shared__ uint8_t wq[WIN_STRIDE];
    __shared__ int8_t bmat[49];
    const DevKit* k = a.kp.kit;
    const uint32_t e = blockIdx.y >> 1;
    const int s = (int)(blockIdx.y & 1u), b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int used = a.recs[e].used_tpl, start = a.recs[e].region_start[s], rl = a.recs[e].region_len[s];
    const DevSet& bs = k->tpl[used].sets[s];
    if (b >= bs.n || rl <= 0 || (s == 1 && k->mode != QCAT_MODE_DUAL)) return;
    if (lane < 49) bmat[lane] = k->bmat[lane];
    if (a.win) for (int i = lane; i < WIN_STRIDE; i += 64) wq[i] = a.win[(size_t)e * WIN_STRIDE + i];
    __syncthreads();
    const uint8_t* tc = a.kp.codes + bs.tgt_off + (size_t)b * bs.tlen;
    const DevAlign r = a.win ? dev_sg_wave<false>(WinSeq{wq + start}, rl, tc, bs.tlen, 1, bmat, lane)
                             : dev_sg_wave<false>(AsciiSeq{a.seq + a.seq_off[e] + start}, rl, tc, bs.tlen, 1, bmat, lane);
    if (lane == 0) a.sc[((size_t)e * 2 + s) * a.sc_stride + b] = (int16_t)r.score;
}

// find_highest_scoring_barcode's running best with the `not max_score` replacement (R2), in list order: one wave per (read
// end, set).  The running best ends at (first index of the maximum M, M) whenever M != 0 (kernels_packed.inc: barcode_key) --
// a wave-wide maximum of (raw, first index) keys; a list whose maximum is exactly 0 is walked in order by lane 0.
__global__ void __launch_bounds__(64)
k_tiny_select(TinyArgs a) {
    const uint32_t id = blockIdx.x;
    const uint32_t e = id >> 1;
    const int s = (int)(id & 1u), lane = (int)threadIdx.x;
    const DevKit* k = a.kp.kit;
    if (s == 1 && k->mode != QCAT_MODE_DUAL) return;
    EndRec* r = a.recs + e;
    const DevSet& bs = k->tpl[r->used_tpl].sets[s];
    int bi = -1, braw = 0;
    if (r->region_len[s] > 0 && bs.n > 0) {
        const int16_t* sc = a.sc + ((size_t)e * 2 + s) * a.sc_stride;
        unsigned key = 0;
        for (int b = lane; b < bs.n; b += 64) {
            const int v = sc[b];
            if (a.dbg_rows) a.dbg_rows[((size_t)e * 2 + s) * a.dbg_stride + b] = (int16_t)v;
            key = max(key, ((unsigned)(v + 32768) << 16) | (unsigned)(65535 - b));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
        braw = (int)(key >> 16) - 32768; bi = 65535 - (int)(key & 0xFFFFu);
        if (braw == 0) {                                        // (wave-uniform) R2's replacement chain: in list order
            bi = -1; braw = 0;
            for (int b = 0; b < bs.n; ++b) {
                const int v = sc[b];
                if (bi < 0 || braw == 0 || braw < v) { bi = b; braw = v; }
            }
        }
    }
    if (lane == 0) { r->bc_idx[s] = bi; r->bc_raw[s] = braw; }
}

// qcat_scan_sequences: the records of whole sequences as scan() returns them -- no thresholds, no trims (k_scan_sequences' last line)
__global__ void __launch_bounds__(64)
k_tiny_store_sequences(TinyArgs a, qcat_result* __restrict__ results) {
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n_ends) return;
    dev_store_result(results + e, dev_make_scan(a.kp, a.recs[e]), 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Simple mode on whole sequences (BarcodeScannerSimple.scan, qcat/scanner_simple.py:41-91, as k_scan_sequences runs it): every
// barcode of the kit's one list against the WHOLE sequence, gaps 1/1, the barcode's own length (a user FASTA may hold barcodes
// of unequal length), the winners compared by their normalised scores.
// ---------------------------------------------------------------------------------------------------------------------------
// grid: (barcode, sequence) -> sc[sequence][barcode] = (raw, end_query).  The end of a barcode alignment is placed in the
// striped order under either R1 rule (kernels_simple.inc, dev_simple_end: no r1_scalar there).
__global__ void __launch_bounds__(64)
k_tiny_simple_barcode(TinyArgs a, int32_t* __restrict__ sc) {
    __shared__ int8_t bmat[49];
    const DevKit* k = a.kp.kit;
    const uint32_t e = blockIdx.y;
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const DevSet& bs = k->tpl[0].sets[0];
    if (lane < 49) bmat[lane] = k->bmat[lane];
    __syncthreads();
    const int L = tiny_len(a, e);
    const int tl = bs.len_off >= 0 ? a.kp.ids[bs.len_off + 3 * b] : bs.tlen;
    DevAlign r; r.score = 0; r.end_q = -1; r.end_r = -1;
    if (L > 0 && tl > 0)                                        // (tl <= QCAT_MAX_TARGET_LEN = 64, kit_prepare.inc: one column per lane)
        r = dev_sg_wave<false>(AsciiSeq{a.seq + a.seq_off[e]}, L, a.kp.codes + bs.tgt_off + (size_t)b * bs.tlen, tl, 1, bmat, lane, false);
    if (lane == 0) { sc[((size_t)e * bs.n + b) * 2] = r.score; sc[((size_t)e * bs.n + b) * 2 + 1] = r.end_q; }
}

// Rule R2 as k_scan_sequences applies it -- the running best replaced when `bi < 0 || braw == 0 || braw * tl < score * blen` --
// one wave per sequence.  The chain ends at the largest normalised score with the smallest list index among equals unless the
// largest raw score is exactly 0 (a running best of 0 is replaced by whatever follows): a wave-wide reduction with the
// cross-multiplied comparison, and lane 0 walks the chain in list order for the sequences whose winner scores 0.
__global__ void __launch_bounds__(64)
k_tiny_simple_select(TinyArgs a, const int32_t* __restrict__ sc) {
    const uint32_t e = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const DevKit* k = a.kp.kit;
    const DevSet& bs = k->tpl[0].sets[0];
    const int L = tiny_len(a, e);
    int bi = -1, braw = 0, bend = -1;
    if (L > 0 && bs.n > 0) {
        const int32_t* s = sc + (size_t)e * bs.n * 2;
        int blen = 1;
        for (int b = lane; b < bs.n; b += 64) {                 // ascending: the first index among a lane's equals stays
            const int v = s[2 * b], tl = bs.len_off >= 0 ? a.kp.ids[bs.len_off + 3 * b] : bs.tlen;
            if (bi < 0 || braw * tl < v * blen) { bi = b; braw = v; blen = tl; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int oi = __shfl_xor(bi, o, 64), oraw = __shfl_xor(braw, o, 64), olen = __shfl_xor(blen, o, 64);
            const int lhs = braw * olen, rhs = oraw * blen;      // mine < theirs  <=>  lhs < rhs
            if (oi >= 0 && (bi < 0 || lhs < rhs || (lhs == rhs && oi < bi))) { bi = oi; braw = oraw; blen = olen; }
        }
        if (braw == 0) {                                        // (wave-uniform) the replacement chain, in list order
            bi = -1; braw = 0; blen = 1;
            for (int b = 0; b < bs.n; ++b) {
                const int v = s[2 * b], tl = bs.len_off >= 0 ? a.kp.ids[bs.len_off + 3 * b] : bs.tlen;
                if (bi < 0 || braw == 0 || braw * tl < v * blen) { bi = b; braw = v; blen = tl; }
            }
        }
        bend = s[2 * bi + 1];
    }
    if (lane == 0) {
        EndRec r;
        r.window_len = L; r.best_tpl = -1; r.used_tpl = 0; r.best_end = bend; r.best_raw = -1; r.region_path = 0;
        for (int q = 0; q < 2; ++q) { r.region_start[q] = 0; r.region_len[q] = 0; r.bc_idx[q] = -1; r.bc_raw[q] = 0; }
        r.region_len[0] = L; r.bc_idx[0] = bi; r.bc_raw[0] = braw;      // (kernels_simple.inc: simple_rec)
        a.recs[e] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_sg_wave: qcat_sg_align without statistics, one wave per (query, target) pair straight from ASCII (k_sg_align's mapping of
// the letters: X and "other" keep their own codes).  The target's codes are staged in the LDS; linear or Gotoh by the costs
// (wave-uniform), rule R1 in either order.  Writes what k_sg_align writes for QCAT_STATS_NONE: matches = length = 0, and
// (0, -1, -1) for an empty query or target.
// ---------------------------------------------------------------------------------------------------------------------------
struct AsciiSeqAll {
    const uint8_t* p;
    __device__ __forceinline__ int operator()(int i) const { return (int)dev_code_of_ascii(p[i]); }
};

__global__ void __launch_bounds__(64)
k_sg_wave(const uint8_t* __restrict__ q, const uint64_t* __restrict__ qoff, const uint8_t* __restrict__ t,
          const uint64_t* __restrict__ toff, uint32_t n, int open, int ext, SgMatrix mat, int r1_scalar, qcat_alignment* __restrict__ out) {
    __shared__ uint8_t tc[MAX_TLEN];
    __shared__ int8_t m[49];
    const uint32_t a = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (a >= n) return;
    const uint8_t* s2 = t + toff[a];
    const int L = (int)(qoff[a + 1] - qoff[a]), M = (int)(toff[a + 1] - toff[a]);
    qcat_alignment r; r.score = 0; r.end_query = -1; r.end_ref = -1; r.matches = 0; r.length = 0;
    if (L > 0 && M > 0 && M <= MAX_TLEN) {                     // (wave-uniform)
        if (lane < 49) m[lane] = mat.m[lane];
        for (int j = lane; j < M; j += 64) tc[j] = dev_code_of_ascii(s2[j]);
        __syncthreads();
        const AsciiSeqAll qs{q + qoff[a]};
        const bool r1s = r1_scalar != 0;
        DevAlign al;
        if (open != ext) al = M > 64 ? dev_sg_wave_affine<true>(qs, L, tc, M, open, ext, m, lane, r1s) : dev_sg_wave_affine<false>(qs, L, tc, M, open, ext, m, lane, r1s);
        else al = M > 64 ? dev_sg_wave<true>(qs, L, tc, M, open, m, lane, r1s) : dev_sg_wave<false>(qs, L, tc, M, open, m, lane, r1s);
        r.score = al.score; r.end_query = al.end_q; r.end_ref = al.end_r;
    }
    if (lane == 0) out[a] = r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// --detect-middle on reads whose interior the packed interior scan does not take (more than 16 384 letters, kernels_middle.inc):
// k_scan_middle walks such a read on ONE lane -- half a second for a 50 kb read, and nanopore runs hold such reads.  The same
// scan (scan() of read[n:-n] and of its reverse complement with the templates of the called kit, a hit when every set's best
// barcode reaches middle_min_score: qcat/scanner_base.py:479-519, :593-595) on one wave per alignment: a work list of the
// flagged reads, then grid-strided kernels over (read, strand, template) and (read, strand, set, barcode) items.  The host
// does not know how many reads are listed: the grids are fixed and the kernels read the count.
// ---------------------------------------------------------------------------------------------------------------------------
struct MidWaveArgs {
    KitPtrs kp;
    const uint8_t* bases; const uint64_t* offsets; uint32_t n_reads;
    qcat_result* results;
    uint8_t* only;                                  // reads left to the general kernel; a listed read's flag is cleared
    uint32_t* list; uint32_t* count; uint32_t cap;  // the listed reads (count may run past cap: min(count, cap) are listed)
    int32_t* tpl;                                   // [cap * 2 strands][MAX_T][2]
    EndRec* recs;                                   // [cap * 2]
    int16_t* sc; uint32_t sc_stride;                // [cap * 2][2 sets][sc_stride]
};

__device__ __forceinline__ int midw_interior(const DevKit* k, const uint64_t* offsets, uint32_t r, int64_t* len_out) {
    const int64_t len = (int64_t)(offsets[r + 1] - offsets[r]);
    const int64_t m = len - 2 * (int64_t)k->max_align;
    *len_out = len;
    return m < 0 ? 0 : (int)m;
}

__global__ void __launch_bounds__(256)
k_midw_list(MidWaveArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_reads || !a.only[r] || a.results[r].adapter_idx < 0) return;
    int64_t len;
    if (midw_interior(a.kp.kit, a.offsets, r, &len) <= 0) return;          // (no interior: no hit; the general kernel says so at once)
    const uint32_t pos = atomicAdd(a.count, 1u);
    if (pos < a.cap) { a.list[pos] = r; a.only[r] = 0; }
}

__global__ void __launch_bounds__(64)
k_midw_adapter(MidWaveArgs a) {
    __shared__ int8_t amat[49];
    const DevKit* k = a.kp.kit;
    const int lane = (int)threadIdx.x;
    if (lane < 49) amat[lane] = k->amat[lane];
    __syncthreads();
    const uint32_t nq = min(*a.count, a.cap);
    const uint64_t items = (uint64_t)nq * 2 * (uint64_t)k->nt;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t q = (uint32_t)(it / (2u * (uint32_t)k->nt));
        const int strand = (int)((it / (uint32_t)k->nt) & 1u), t = (int)(it % (uint32_t)k->nt);
        const uint32_t r = a.list[q];
        const DevTpl& p = k->tpl[t];
        if (p.kit_slot != k->tpl[a.results[r].adapter_idx].kit_slot) continue;
        int64_t len;
        const int m = midw_interior(k, a.offsets, r, &len);
        const MidSeq seq{a.bases + a.offsets[r], len, k->max_align, strand, 0};
        const uint8_t* tc = a.kp.codes + p.code_off;
        const DevAlign al = p.len > 64 ? dev_sg_wave<true>(seq, m, tc, p.len, k->gap_open, amat, lane, k->r1_scalar != 0)
                                       : dev_sg_wave<false>(seq, m, tc, p.len, k->gap_open, amat, lane, k->r1_scalar != 0);
        if (lane == 0) { a.tpl[(((size_t)q * 2 + strand) * MAX_T + t) * 2] = al.score; a.tpl[(((size_t)q * 2 + strand) * MAX_T + t) * 2 + 1] = al.end_q; }
    }
}

// dev_scan_any's decision lines (kernels_generic.inc) over the scores k_midw_adapter left
__global__ void __launch_bounds__(64)
k_midw_decide(MidWaveArgs a) {
    const uint32_t id = blockIdx.x * 64 + threadIdx.x;
    if (id >= min(*a.count, a.cap) * 2) return;
    const DevKit* k = a.kp.kit;
    const uint32_t q = id >> 1, r = a.list[q];
    const int kit_slot = k->tpl[a.results[r].adapter_idx].kit_slot;
    int64_t len;
    const int m = midw_interior(k, a.offsets, r, &len), n = k->max_align;
    int best = -1, best_end = -1, best_raw = -1, best_den = 100, last = -1;
    for (int t = 0; t < k->nt; ++t) {
        const DevTpl& p = k->tpl[t];
        if (p.kit_slot != kit_slot) continue;
        last = t;
        const int raw = a.tpl[((size_t)id * MAX_T + t) * 2], end_q = a.tpl[((size_t)id * MAX_T + t) * 2 + 1];
        if ((int64_t)best_raw * p.den < (int64_t)raw * best_den) { best = t; best_end = end_q; best_raw = raw; best_den = p.den; }
    }
    EndRec rec;
    rec.window_len = m; rec.best_tpl = best; rec.best_end = best_end; rec.best_raw = best_raw;
    rec.used_tpl = best < 0 ? last : best;
    const DevTpl& p = k->tpl[rec.used_tpl];
    const bool dual = k->mode == QCAT_MODE_DUAL;
    rec.region_path = (dual || p.is_double || (best >= 0 && best_raw >= p.region_min_raw)) ? 1 : 0;
    const int nsets = dual ? 2 : 1;
    for (int s = 0; s < 2; ++s) { rec.region_start[s] = 0; rec.region_len[s] = 0; rec.bc_idx[s] = -1; rec.bc_raw[s] = 0; }
    for (int s = 0; s < nsets; ++s) {
        int start = 0, rl = m < n ? m : n;
        if (rec.region_path) dev_region(p.len, p.bc_end[s], p.bc_len[s], k->ext, best_end, m, &start, &rl);
        rec.region_start[s] = start; rec.region_len[s] = rl;
    }
    a.recs[id] = rec;
}

__global__ void __launch_bounds__(64)
k_midw_barcode(MidWaveArgs a) {
    __shared__ int8_t bmat[49];
    const DevKit* k = a.kp.kit;
    const int lane = (int)threadIdx.x;
    if (lane < 49) bmat[lane] = k->bmat[lane];
    __syncthreads();
    const uint32_t nq = min(*a.count, a.cap);
    const int nsets = k->mode == QCAT_MODE_DUAL ? 2 : 1;
    const uint64_t items = (uint64_t)nq * 2 * (uint64_t)nsets * a.sc_stride;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int b = (int)(it % a.sc_stride);
        const uint64_t rest = it / a.sc_stride;
        const int s = (int)(rest % (uint64_t)nsets);
        const uint32_t id = (uint32_t)(rest / (uint64_t)nsets);             // (listed read, strand)
        const EndRec& rec = a.recs[id];
        const DevSet& bs = k->tpl[rec.used_tpl].sets[s];
        if (b >= bs.n || rec.region_len[s] <= 0) continue;
        const uint32_t r = a.list[id >> 1];
        const int64_t len = (int64_t)(a.offsets[r + 1] - a.offsets[r]);
        const MidSeq seq{a.bases + a.offsets[r], len, k->max_align, (int)(id & 1u), rec.region_start[s]};
        const DevAlign al = dev_sg_wave<false>(seq, rec.region_len[s], a.kp.codes + bs.tgt_off + (size_t)b * bs.tlen, bs.tlen, 1, bmat, lane);
        if (lane == 0) a.sc[((size_t)id * 2 + s) * a.sc_stride + b] = (int16_t)al.score;
    }
}

// per listed read: rule R2 over each set's scores on both strands, the middle_min_score thresholds, and the verdict 997
__global__ void __launch_bounds__(64)
k_midw_finish(MidWaveArgs a) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= min(*a.count, a.cap)) return;
    const DevKit* k = a.kp.kit;
    const int nsets = k->mode == QCAT_MODE_DUAL ? 2 : 1;
    bool hit = false;
    for (int strand = 0; strand < 2 && !hit; ++strand) {
        const uint32_t id = q * 2 + (uint32_t)strand;
        const EndRec& rec = a.recs[id];
        const DevTpl& p = k->tpl[rec.used_tpl];
        bool ok = true;
        for (int s = 0; s < nsets && ok; ++s) {
            const DevSet& bs = p.sets[s];
            int bi = -1, braw = 0;
            if (rec.region_len[s] > 0) {
                const int16_t* sc = a.sc + ((size_t)id * 2 + s) * a.sc_stride;
                for (int b = 0; b < bs.n; ++b) { const int v = sc[b]; if (bi < 0 || braw == 0 || braw < v) { bi = b; braw = v; } }
            }
            if ((bi < 0 ? 0 : braw) < bs.min_raw_middle) ok = false;      // barcode None (scores 0.0) / score < 50 (dual: min of both)
        }
        hit = ok;
    }
    if (hit) {
        qcat_result res = a.results[a.list[q]];
        res.barcode_idx = -1; res.barcode2_idx = -1; res.adapter_idx = -1; res.exit_status = 997;
        res.adapter_end = 0; res.raw_score = 0; res.score_den = 1;
        a.results[a.list[q]] = res;
    }
}

}  // namespace qk

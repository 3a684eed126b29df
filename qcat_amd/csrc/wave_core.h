// wave_core.h -- the per-cell arithmetic of the one-wave-per-alignment kernels under AFFINE gap costs (kernels_tiny.inc:
// dev_sg_wave_affine): what one lane does with one target column on one anti-diagonal step.  Plain C++ without builtins, so
// that the host can drive it: tests/wave_affine_check.cpp emulates the 64-lane schedule (the hand-over from the left neighbour
// as an array shift, the carry from column 64 to column 65) around these functions and compares with a plain Gotoh loop.
//
// Gotoh's recurrences with the semantics of dev_sg_generic (kernels_generic.inc):
//     F(i,j) = max(F(i-1,j) - ext, H(i-1,j) - open)      the gap that consumes query letters: same column, previous step -- lane-local
//     E(i,j) = max(E(i,j-1) - ext, H(i,j-1) - open)      the gap that consumes target letters: the left neighbour's last step
//     H(i,j) = max(H(i-1,j-1) + W, E(i,j), F(i,j)),      H(0,j) = H(i,0) = 0, F(0,j) = E(i,0) = -inf
// (The linear cell, tiny_cell, stays device code in kernels_tiny.inc.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QW_HD __host__ __device__ __forceinline__
#else
#define QW_HD inline
#endif

namespace qk {

constexpr int WAVE_BIAS = 1 << 20;            // cells are kept biased (= TINY_BIAS): the last row's key is an unsigned compare
constexpr int WAVE_NEG = -(1 << 28);          // "-inf" of E and F (and the start of the running column maximum: GEN_NEG)
// gap costs up to which the affine cells stay inside the biased range: H(i,j) >= E(i,j) >= H(i,j-1) - open >= ... >= -j * open
// (128 columns at most), so 128 * open < WAVE_BIAS; larger costs stay on the general kernels
constexpr int WAVE_GAP_MAX = 4096;

struct WaveCol {                              // one target column of a lane
    uint64_t tbl;                             // W(query code 0..6, this column's letter): seven signed bytes
    int up, diag, h;                          // H(i-1, j) and H(i-1, j-1), biased; h: what this lane shows its neighbour (its last cell)
    int f, e;                                 // F(i-1, j), biased, and E(i, j) of the last cell (shown to the neighbour like h)
    int letter;                               // query code of the row this lane is on (travels from lane to lane beside the cells)
    int row_last;                             // H(L, j), biased
    int cmax, ci;                             // running maximum of this column over the rows and the FIRST row reaching it
};

QW_HD int wave_max(int a, int b) { return a > b ? a : b; }

// one cell of column j at row i; `left_h`, `left_e`: H(i, j-1) and E(i, j-1) (column 1: 0 and -inf), `qc` the row's letter.
// Rows i < 1 keep H(0,j) = 0 and F(0,j) = -inf; rows i > L compute on (nothing reads them: row_last, cmax and the rows <= L of the
// columns to the right do not depend on them).
// "-inf" cannot wrap: F is WAVE_NEG only while i < 1, where it is re-set and never decremented; the first real row takes
// max(WAVE_NEG - ext, H(0,j) - open) = -open, and from then on H(i-1,j) - open bounds F from below.  E is WAVE_NEG only as
// column 1's input, fed afresh every step and decremented once: every E a lane shows is >= H(i,j-1) - open.  H itself is bounded
// below by -j * open through E (WAVE_GAP_MAX above), also on the rows before 1 and beyond L.
QW_HD void wave_cell_affine(WaveCol& c, int left_h, int left_e, int qc, int i, int L, int open, int ext) {
    const int w = (int)(int8_t)(c.tbl >> (8 * qc));
    const int e = wave_max(left_e - ext, left_h - open);
    int f = wave_max(c.f - ext, c.up - open);
    int h = wave_max(c.diag + w, wave_max(e, f));
    const bool inside = i >= 1 && i <= L;
    h = i >= 1 ? h : WAVE_BIAS;
    f = i >= 1 ? f : WAVE_NEG;
    c.row_last = i == L ? h : c.row_last;
    const bool better = inside && (h - WAVE_BIAS) > c.cmax;
    c.cmax = better ? h - WAVE_BIAS : c.cmax;
    c.ci = better ? i : c.ci;
    c.diag = left_h; c.up = h;
    c.h = h; c.f = f; c.e = e;
}

// a column's start: the score bytes of its letter, the boundary values of row 0
QW_HD void wave_col_init(WaveCol& c, const uint8_t* t, int j, int M, const int8_t* mat) {
    const int tj = j <= M ? (int)t[j - 1] : 0;
    uint64_t tbl = 0;
    for (int qc = 0; qc < 7; ++qc) tbl |= (uint64_t)(uint8_t)mat[tj * 7 + qc] << (8 * qc);
    c.tbl = tbl; c.up = WAVE_BIAS; c.diag = WAVE_BIAS; c.h = WAVE_BIAS; c.f = WAVE_NEG; c.e = WAVE_NEG;
    c.letter = 0; c.row_last = 0; c.cmax = WAVE_NEG; c.ci = 0;
}

}  // namespace qk

// wave_affine_check.cpp -- the one-wave-per-alignment schedule (qcat_amd/csrc/kernels_tiny.inc: dev_sg_wave_affine) on the CPU,
// around the cell functions the kernels themselves call (qcat_amd/csrc/wave_core.h: wave_col_init, wave_cell_affine).
//
// The emulation keeps what the kernel keeps: 64 lanes, lane l on target column l + 1 (and l + 65), one anti-diagonal per step;
// the hand-over from the left neighbour (v_mov_b32_dpp wave_shr:1) is a shift of the lanes' previous values with the boundary
// value entering at lane 0, the step from column 64 to column 65 (v_readlane 63) a read of lane 63's previous values; the last
// row's key and the last column's running maximum are combined under rule R1 as the kernel combines them.  Checked against
//   1. the independent scalar DP's recorded answers for the affine family of tests/golden/sg_vectors.json (a file the test
//      writes, one line per case; both R1 rules);
//   2. a plain Gotoh loop (below: the recurrences of dev_sg_generic, kernels_generic.inc) on ALL queries of up to 6 letters
//      against ALL targets of up to 4 letters over ACGT, gap costs (3,1), (5,2), (2,1), (1,3) and (2,2) (Gotoh's
//      recurrences with open == extend are the linear ones);
//   3. the same loop on targets of 64, 65 and 128 columns (one column per lane to its last lane, the first column of the
//      second half, both halves full) with queries of 1 to 300 letters.
// Prints one line per section: "<section>: <n> cases, <k> mismatches".
//
// usage: wave_affine_check <golden case file> [<largest query length of section 2>]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kit.h"
#include "wave_core.h"

using namespace qk;

struct Res { int score, end_q, end_r; };

// the plain loop: Gotoh with free end gaps, rule R1 (r1_scalar: the last column wins every tie of the two borders' maxima)
static Res plain_gotoh(const uint8_t* q, int L, const uint8_t* t, int M, int open, int ext, const int8_t* mat, bool r1_scalar) {
    const int NEG = -(1 << 28);
    int H[QCAT_MAX_TEMPLATE_LEN + 1], F[QCAT_MAX_TEMPLATE_LEN + 1];
    for (int j = 0; j <= M; ++j) { H[j] = 0; F[j] = NEG; }
    int cmax = NEG, ci = 0;
    for (int i = 1; i <= L; ++i) {
        int diag = 0, hleft = 0, e = NEG;
        for (int j = 1; j <= M; ++j) {
            const int up = H[j];
            const int f = std::max(F[j] - ext, up - open);
            const int ee = std::max(e - ext, hleft - open);
            const int h = std::max(std::max(diag + mat[t[j - 1] * 7 + q[i - 1]], ee), f);
            diag = up; H[j] = h; F[j] = f; e = ee; hleft = h;
        }
        if (hleft > cmax) { cmax = hleft; ci = i; }
    }
    Res a{NEG, L - 1, 0};
    for (int j = 1; j <= M; ++j) if (H[j] > a.score) { a.score = H[j]; a.end_r = j - 1; }
    if (cmax > a.score || (cmax == a.score && (a.end_r == M - 1 || r1_scalar))) { a.score = cmax; a.end_r = M - 1; a.end_q = ci - 1; }
    return a;
}

// the wave: `lanes` of the 64 are emulated -- a lane reads its left neighbours only, so the lanes beyond the target's last
// column (whose cells no result reads) may be left out; sections 1 and 3 run all 64
static void wave(const uint8_t* q, int L, const uint8_t* t, int M, int open, int ext, const int8_t* mat, int lanes, Res out[2]) {
    const bool two = M > 64;
    WaveCol a[64], b[64], pa[64], pb[64];
    for (int l = 0; l < lanes; ++l) { wave_col_init(a[l], t, l + 1, M, mat); if (two) wave_col_init(b[l], t, l + 65, M, mat); }
    for (int d = 2; d <= L + M; ++d) {
        const int r = d - 2;
        const int first = r < L ? q[r] : 0;                       // the letter of row d - 1 enters at lane 0
        memcpy(pa, a, sizeof(WaveCol) * lanes);
        if (two) memcpy(pb, b, sizeof(WaveCol) * lanes);
        for (int l = 0; l < lanes; ++l) {
            const int ia = d - (l + 1);
            a[l].letter = l ? pa[l - 1].letter : first;
            const int left_h = l ? pa[l - 1].h : WAVE_BIAS, left_e = l ? pa[l - 1].e : WAVE_NEG;
            wave_cell_affine(a[l], left_h, left_e, a[l].letter, ia, L, open, ext);
            if (two) {
                b[l].letter = l ? pb[l - 1].letter : pa[63].letter;
                const int lh = l ? pb[l - 1].h : pa[63].h, le = l ? pb[l - 1].e : pa[63].e;
                wave_cell_affine(b[l], lh, le, b[l].letter, ia - 64, L, open, ext);
            }
        }
    }
    unsigned key = 0;
    for (int l = 0; l < lanes; ++l) {
        if (l + 1 <= M) key = std::max(key, ((unsigned)a[l].row_last << 8) | (unsigned)(255 - l));
        if (two && l + 65 <= M) key = std::max(key, ((unsigned)b[l].row_last << 8) | (unsigned)(255 - (l + 64)));
    }
    const int src = (M - 1) & 63;
    const int cmax = two ? b[src].cmax : a[src].cmax, ci = two ? b[src].ci : a[src].ci;
    for (int rule = 0; rule < 2; ++rule) {
        Res r{(int)(key >> 8) - WAVE_BIAS, L - 1, 255 - (int)(key & 255u)};
        if (cmax > r.score || (cmax == r.score && (r.end_r == M - 1 || rule == 1))) { r.score = cmax; r.end_r = M - 1; r.end_q = ci - 1; }
        out[rule] = r;
    }
}

struct Tally { long cases = 0, bad = 0; };

static void compare(const char* what, const Res& got, int score, int end_q, int end_r, int rule, int open, int ext,
                    const std::string& qs, const std::string& ts, Tally* tally) {
    tally->cases++;
    if (got.score == score && got.end_q == end_q && (end_r < 0 || got.end_r == end_r)) return;
    if (tally->bad++ < 5)
        fprintf(stderr, "%s: rule %d open %d ext %d: got (%d, %d, %d) want (%d, %d, %d)\n  t=%s\n  q=%s\n", what, rule, open, ext,
                got.score, got.end_q, got.end_r, score, end_q, end_r, ts.c_str(), qs.c_str());
}

static std::vector<uint8_t> codes(const std::string& s) {
    std::vector<uint8_t> c(s.size() + 1);
    for (size_t i = 0; i < s.size(); ++i) c[i] = code_of_ascii((uint8_t)s[i]);
    return c;
}

// one (query, target) pair under every gap configuration
static const int GAPS[5][2] = {{3, 1}, {5, 2}, {2, 1}, {1, 3}, {2, 2}};

static void against_plain_1(const char* what, const std::string& qs, const std::string& ts, const uint8_t* q, const uint8_t* t, int open, int ext,
                            const int8_t* mat, int lanes, Tally* tally) {
    Res got[2];
    wave(q, (int)qs.size(), t, (int)ts.size(), open, ext, mat, lanes, got);
    for (int rule = 0; rule < 2; ++rule) {
        const Res want = plain_gotoh(q, (int)qs.size(), t, (int)ts.size(), open, ext, mat, rule == 1);
        compare(what, got[rule], want.score, want.end_q, want.end_r, rule, open, ext, qs, ts, tally);
    }
}

static void against_plain(const char* what, const std::string& qs, const std::string& ts, const int8_t* mat, int lanes, Tally* tally) {
    uint8_t q[512], t[QCAT_MAX_TEMPLATE_LEN];
    for (size_t i = 0; i < qs.size(); ++i) q[i] = code_of_ascii((uint8_t)qs[i]);
    for (size_t j = 0; j < ts.size(); ++j) t[j] = code_of_ascii((uint8_t)ts[j]);
    for (int g = 0; g < 5; ++g) against_plain_1(what, qs, ts, q, t, GAPS[g][0], GAPS[g][1], mat, lanes, tally);
}

static void table(int8_t* mat, int match, int mismatch, int nmatch) {
    memset(mat, 0, 49);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) mat[i * 7 + j] = (int8_t)(i == j ? match : mismatch);
    for (int i = 0; i < 5; ++i) { mat[4 * 7 + i] = (int8_t)nmatch; mat[i * 7 + 4] = (int8_t)nmatch; }
}

static uint64_t g_rng = 88172645463325252ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: wave_affine_check <golden case file> [<largest query length of section 2>]\n"); return 2; }
    const int max_q = argc > 2 ? atoi(argv[2]) : 6;

    // 1. the recorded answers: <open> <ext> <49 scores> <target> <query> <score> <end_query> <end_ref> <scalar end_query or -9> <scalar end_ref>
    Tally golden;
    {
        FILE* fh = fopen(argv[1], "r");
        if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        int open, ext;
        while (fscanf(fh, "%d %d", &open, &ext) == 2) {
            int8_t mat[49];
            for (int i = 0; i < 49; ++i) { int v; if (fscanf(fh, "%d", &v) != 1) return 2; mat[i] = (int8_t)v; }
            char tb[512], qb[512];
            int score, eq, er, eqs, ers;
            if (fscanf(fh, "%500s %500s %d %d %d %d %d", tb, qb, &score, &eq, &er, &eqs, &ers) != 7) return 2;
            const std::string ts(tb), qs(qb);
            const std::vector<uint8_t> q = codes(qs), t = codes(ts);
            Res got[2];
            wave(q.data(), (int)qs.size(), t.data(), (int)ts.size(), open, ext, mat, 64, got);
            compare("golden", got[0], score, eq, er, 0, open, ext, qs, ts, &golden);
            if (eqs != -9) compare("golden", got[1], score, eqs, ers, 1, open, ext, qs, ts, &golden);
        }
        fclose(fh);
    }
    printf("golden affine family: %ld cases, %ld mismatches\n", golden.cases, golden.bad);

    // 2. everything small
    Tally small;
    {
        int8_t mat[49];
        table(mat, 3, -2, -1);
        const char* alpha = "ACGT";
        for (int M = 1; M <= 4; ++M)
            for (int tv = 0; tv < (1 << (2 * M)); ++tv) {
                std::string ts(M, 'A');
                for (int j = 0; j < M; ++j) ts[j] = alpha[(tv >> (2 * j)) & 3];
                for (int L = 1; L <= max_q; ++L)
                    for (int qv = 0; qv < (1 << (2 * L)); ++qv) {
                        std::string qs(L, 'A');
                        for (int i = 0; i < L; ++i) qs[i] = alpha[(qv >> (2 * i)) & 3];
                        against_plain("exhaustive", qs, ts, mat, M, &small);
                    }
            }
    }
    printf("exhaustive %d x 4: %ld cases, %ld mismatches\n", max_q, small.cases, small.bad);

    // 3. the lanes' edges: 64 columns, the carry into column 65, both halves full
    Tally wide;
    {
        const int ms[3] = {64, 65, 128}, ls[8] = {1, 2, 63, 64, 65, 130, 131, 300};
        for (int rep = 0; rep < 6; ++rep)
            for (int mi = 0; mi < 3; ++mi)
                for (int li = 0; li < 8; ++li) {
                    int8_t mat[49];
                    table(mat, 1 + (int)rnd(9), -(1 + (int)rnd(6)), -(int)rnd(3));
                    const int M = ms[mi], L = ls[li];
                    std::string ts(M, 'A'), qs(L, 'A');
                    const char* ta = rep % 3 ? "ACGT" : "ACGTN";
                    for (int j = 0; j < M; ++j) ts[j] = ta[rnd((uint32_t)strlen(ta))];
                    for (int i = 0; i < L; ++i) qs[i] = "ACGTNRx*"[rnd(rnd(8) ? 4 : 8)];
                    if (rep & 1)                                  // a noisy copy of the target somewhere in the query: long diagonals, gaps of both kinds
                        for (int i = (int)rnd(20), j = 0; i < L && j < M; ++i, ++j) {
                            if (rnd(12) == 0) { j += (int)rnd(3); continue; }
                            if (rnd(12) == 0) { --j; continue; }
                            if (j < M && rnd(10)) qs[i] = ts[j] == 'N' ? 'A' : ts[j];
                        }
                    against_plain("wide", qs, ts, mat, 64, &wide);
                }
    }
    printf("targets of 64, 65 and 128 columns: %ld cases, %ld mismatches\n", wide.cases, wide.bad);
    return (golden.bad || small.bad || wide.bad) ? 1 : 0;
}

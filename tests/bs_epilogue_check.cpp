// bs_epilogue_check.cpp -- host check of the END of a bit-sliced barcode (test infrastructure, plain g++).
//
// qcat_amd/csrc/bs_core.h is a pure function of 32-bit words, so the routines the device kernels run after a barcode's
// row loops are executed here 32 alignments at a time:
//  * bs_last_row (the row maximum as a deficit, H(L,c) as one carry-save sum) and its start bs_last_row_start against the
//    composition they replace -- bs_step + bs_max once per column, then bs_finish_split -- bit for bit on the final planes:
//    every code sequence of up to six own columns crossed with a grid of starting values, random last rows of 24 and of 48
//    own columns (the most the kernels instantiate) behind 0 / 4 / 8 / 11 shared ones, and the extremes;
//  * bs_keys32 (the keys of 32 alignments as a bit-matrix transposition of the planes) against picking 14 bits per
//    alignment and kernels_packed.inc's barcode_key.
// Built and run by tests/test_bs_epilogue_host.py:
//     g++ -O2 -std=c++17 -I qcat_amd/csrc tests/bs_epilogue_check.cpp -o <tmp>/bs_epilogue_check && bs_epilogue_check <seed>
// Values are chosen inside the ranges the header comment of bs_core.h states (the old composition wraps outside them too):
// H(L,j) in [-j, min(j, 63)], steps of -1 .. 2, rowbest0 - H(L,P) <= P - 1, H(L,c) + D <= 63.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bs_core.h"

using namespace qk;

static uint64_t g_s;
static uint64_t rnd() { g_s += 0x9E3779B97F4A7C15ull; uint64_t z = g_s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static int below(int n) { return (int)((rnd() >> 33) % (uint64_t)n); }

template <int N>
static void planes_of(u32 (&p)[N], const int (&v)[32]) {
    for (int q = 0; q < N; ++q) { p[q] = 0u; for (int k = 0; k < 32; ++k) p[q] |= (u32)((v[k] >> q) & 1) << k; }
}
template <int N>
static int value_of(const u32 (&p)[N], int k) { int v = 0; for (int q = 0; q < N; ++q) v |= (int)((p[q] >> k) & 1u) << q; return v; }

// one last row of an alignment: codes of its own columns, and what it starts from
template <int C>
struct Case {
    int code[C];
    int hp, rb0, D, cmax;            // H(L,P), rowbest0 (shared sets: >= hp), the deficit, cmax + 64 as the planes hold it (0: none)
};

static long g_cases = 0, g_bad = 0;

// 32 cases: the old composition against bs_last_row
template <int C, bool SHARED>
static void check32(const Case<C> (&cs)[32]) {
    u32 h1[C], h0[C];
    for (int j = 0; j < C; ++j) {
        h1[j] = h0[j] = 0u;
        for (int k = 0; k < 32; ++k) { h1[j] |= (u32)((cs[k].code[j] >> 1) & 1) << k; h0[j] |= (u32)(cs[k].code[j] & 1) << k; }
    }
    int vr[32], vb[32], vd[32], vc[32], vbase[32], ve[32];
    for (int k = 0; k < 32; ++k) {
        vr[k] = cs[k].hp + BS_OFF; vb[k] = SHARED ? cs[k].rb0 + BS_OFF : 0; vd[k] = cs[k].D; vc[k] = cs[k].cmax;
        vbase[k] = cs[k].hp + BS_OFF - C; ve[k] = SHARED ? cs[k].rb0 - cs[k].hp : 0;
    }
    u32 r[BS_NB], rowbest[BS_NB], d[BS_ND], cmax[BS_NB], base[BS_NB], e[BS_NB], raw[BS_NB];
    planes_of(r, vr); planes_of(rowbest, vb); planes_of(d, vd); planes_of(cmax, vc); planes_of(base, vbase); planes_of(e, ve);
    for (int j = 0; j < C; ++j) { bs_step(r, h1[j], h0[j]); bs_max(rowbest, r); }
    bs_finish_split(rowbest, r, d, cmax);
    // the unit's tail as the kernels lay it out: base, E (its BS_NE planes), cmax
    bs_last_row<C, SHARED>(raw, h1, h0, [&](int q) { return q < BS_NB ? base[q] : (q < 2 * BS_NB ? e[q - BS_NB] : cmax[q - 2 * BS_NB]); }, d);
    g_cases += 32;
    for (int q = 0; q < BS_NB; ++q)
        if (raw[q] != rowbest[q]) {
            const u32 diff = raw[q] ^ rowbest[q];
            for (int k = 0; k < 32; ++k)
                if ((diff >> k) & 1u) {
                    if (g_bad < 5) {
                        fprintf(stderr, "MISMATCH C %d shared %d hp %d rb0 %d D %d cmax %d: got %d want %d, codes", C, (int)SHARED, cs[k].hp, cs[k].rb0, cs[k].D,
                                cs[k].cmax, value_of(raw, k), value_of(rowbest, k));
                        for (int j = 0; j < C; ++j) fprintf(stderr, " %d", cs[k].code[j]);
                        fprintf(stderr, "\n");
                    }
                    ++g_bad;
                }
            break;
        }
}

template <int C, bool SHARED>
struct Batch {
    Case<C> cs[32];
    int n = 0;
    void add(const Case<C>& c) { cs[n++] = c; if (n == 32) flush(); }
    void flush() {
        if (!n) return;
        for (int k = n; k < 32; ++k) cs[k] = cs[0];
        check32<C, SHARED>(cs);
        n = 0;
    }
};

// every code sequence of C columns x a grid of starting values
template <int C>
static void exhaustive() {
    static const int HP[] = {-11, -3, 0, 5, 11}, GAP[] = {0, 1, 4, 10}, DD[] = {0, 1, 7, 30}, CM[] = {0, BS_OFF - 3, BS_OFF, BS_OFF + 9, BS_OFF + 40};
    Batch<C, true> sh;
    Batch<C, false> un;
    for (int seq = 0; seq < (1 << (2 * C)); ++seq) {
        Case<C> c;
        for (int j = 0; j < C; ++j) c.code[j] = (seq >> (2 * j)) & 3;
        for (int d : DD)
            for (int cm : CM) {
                c.D = d; c.cmax = cm;
                for (int hp : HP)
                    for (int gap : GAP) {
                        if (hp + gap > 11) continue;          // rowbest0 <= P = 11
                        c.hp = hp; c.rb0 = hp + gap;
                        sh.add(c);
                    }
                c.hp = 0; c.rb0 = 0;
                un.add(c);
            }
    }
    sh.flush(); un.flush();
}

// a random last row: H(L,j) stays in [-j, min(j, 63)] over all P + C columns, steps -1 .. 2.  kind: 0 random, 1 mostly
// matches, 2 mostly falling
static void random_codes(int* code, int n, int& h, int j0, int kind) {
    for (int j = 0; j < n; ++j) {
        const int col = j0 + j + 1;
        for (;;) {
            int c = kind == 1 ? (below(8) ? 2 : below(4)) : (kind == 2 ? (below(6) ? below(2) : below(4)) : below(4));
            const int nh = h + c - 1;
            if (nh < -col || nh > std::min(col, 63)) continue;
            code[j] = c; h = nh;
            break;
        }
    }
}

// random rows behind P shared columns: bs_last_row_start against the producer's old counters, then the whole end
template <int C>
static void random_rows(int rounds) {
    static const int PS[] = {0, 4, 8, 11};
    for (int round = 0; round < rounds; ++round)
        for (int P : PS) {
            int pc[32][11], hp[32], rb0[32];
            Case<C> cs[32];
            for (int k = 0; k < 32; ++k) {
                int h = 0;
                const int kind = below(3);
                random_codes(pc[k], P, h, 0, kind);
                int run = 0, best = -BS_OFF;
                for (int j = 0; j < P; ++j) { run += pc[k][j] - 1; best = std::max(best, run); }
                hp[k] = h; rb0[k] = best;
                random_codes(cs[k].code, C, h, P, below(3));
                cs[k].hp = hp[k]; cs[k].rb0 = P ? rb0[k] : 0;
                cs[k].D = below(64 - h);                                   // H(L,c) + D <= 63
                cs[k].cmax = below(4) ? BS_OFF - 12 + below(25) : 0;
            }
            u32 h1[11], h0[11];
            for (int j = 0; j < P; ++j) {
                h1[j] = h0[j] = 0u;
                for (int k = 0; k < 32; ++k) { h1[j] |= (u32)((pc[k][j] >> 1) & 1) << k; h0[j] |= (u32)(pc[k][j] & 1) << k; }
            }
            u32 base[BS_NB], e[BS_NE];
            bs_last_row_start(base, e, h1, h0, P, C);
            for (int k = 0; k < 32; ++k) {
                const int wb = hp[k] + BS_OFF - C, we = P ? rb0[k] - hp[k] : 0;
                if (value_of(base, k) != wb || value_of(e, k) != we) {
                    if (g_bad < 5) fprintf(stderr, "MISMATCH start P %d C %d: base %d want %d, E %d want %d\n", P, C, value_of(base, k), wb, value_of(e, k), we);
                    ++g_bad;
                }
            }
            if (P) check32<C, true>(cs); else check32<C, false>(cs);
        }
}

template <int C>
static void extremes() {
    Batch<C, true> sh;
    Batch<C, false> un;
    Case<C> c;
    // all codes 3 (as far as seven planes go: 2 C + 11 + 64 <= 127), all codes 0
    if (2 * C + 11 + BS_OFF <= 127)
        for (int hp : {-11, 0, 11})
            for (int d : {0, 127 - BS_OFF - 11 - 2 * C}) {
                for (int j = 0; j < C; ++j) c.code[j] = 3;
                c.hp = hp; c.rb0 = std::min(11, hp + 10); c.D = d; c.cmax = 0;
                sh.add(c);
                c.cmax = BS_OFF + 20; sh.add(c);
                c.hp = 0; c.rb0 = 0; un.add(c);
            }
    for (int hp : {-11, 0, 11})
        for (int d : {0, 5, 40}) {
            for (int j = 0; j < C; ++j) c.code[j] = 0;
            c.hp = hp; c.rb0 = std::min(11, hp + 10); c.D = d; c.cmax = 0;
            sh.add(c);
            c.cmax = BS_OFF - 2; sh.add(c);
            c.hp = 0; c.rb0 = 0; un.add(c);
        }
    // a perfect read of a 63-column target: 11 shared + C own columns all +1, the rest of the 63 through the deficit
    for (int j = 0; j < C; ++j) c.code[j] = 2;
    c.hp = 11; c.rb0 = 11; c.D = 63 - 11 - C; c.cmax = BS_OFF + 63 - 11 - C;
    sh.add(c);
    c.hp = 0; c.rb0 = 0; c.D = 63 - C; un.add(c);
    // rowbest0 attained in the shared prefix only: the own columns never come back up to it
    for (int gap : {1, 4, 10})
        for (int kind = 0; kind < 3; ++kind) {
            for (int j = 0; j < C; ++j) c.code[j] = kind == 0 ? 1 : (kind == 1 ? (j % 3 == 0 ? 0 : 1) : (j < gap - 1 ? 2 : (j % 2 ? 0 : 2)));
            c.hp = 11 - gap; c.rb0 = 11; c.cmax = 0;
            for (int d : {0, gap - 1, gap, gap + 1}) { c.D = d; sh.add(c); }
        }
    sh.flush(); un.flush();
}

// bs_keys32 against the bit-picking loop
static u32 key_of(int raw, int b) { return ((u32)(raw + 32768) << 16) | (u32)(1023 - b); }       // kernels_packed.inc: barcode_key
static void keys(int rounds) {
    for (int round = 0; round < rounds; ++round)
        for (int lane = 0; lane < 64; ++lane) {
            u32 bestv[BS_NB], besti[BS_NB];
            const int kind = (round + lane) % 4;
            for (int q = 0; q < BS_NB; ++q) {
                besti[q] = (u32)rnd();
                // 0: any planes; 1: one raw score for all 32 alignments, different indices; 2: two scores; 3: the ends of the range
                bestv[q] = kind == 0 ? (u32)rnd() : (kind == 1 ? ((round >> q) & 1 ? 0xFFFFFFFFu : 0u) : (kind == 2 ? (q ? 0xFFFFFFFFu * (u32)((lane >> q) & 1) : 0x0F0F0F0Fu) : (lane & 1 ? 0xFFFF0000u : (q == 6 ? 0x00FFFF00u : 0u))));
            }
            u32 key[32];
            bs_keys32(key, bestv, besti);
            for (int bit = 0; bit < 32; ++bit) {
                u32 val = 0, idx = 0;
                for (int q = 0; q < BS_NB; ++q) { val |= ((bestv[q] >> bit) & 1u) << q; idx |= ((besti[q] >> bit) & 1u) << q; }
                const u32 want = key_of((int)val - BS_OFF, (int)idx);
                ++g_cases;
                if (key[bit] != want) {
                    if (g_bad < 5) fprintf(stderr, "MISMATCH key lane %d bit %d: got %08x want %08x\n", lane, bit, key[bit], want);
                    ++g_bad;
                }
            }
        }
    // the transposition itself
    u32 a[32], b[32];
    for (int k = 0; k < 32; ++k) a[k] = b[k] = (u32)rnd();
    bs_transpose32(b);
    for (int k = 0; k < 32; ++k)
        for (int q = 0; q < 32; ++q)
            if (((b[q] >> k) & 1u) != ((a[k] >> q) & 1u)) ++g_bad;
}

#define SECTION(NAME, CALL) do { const long c0 = g_cases, b0 = g_bad; CALL; printf("%s: %ld cases, %ld mismatches\n", NAME, g_cases - c0, g_bad - b0); } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: bs_epilogue_check <seed>\n"); return 2; }
    g_s = strtoull(argv[1], nullptr, 10);
    SECTION("exhaustive C=2", exhaustive<2>());
    SECTION("exhaustive C=3", exhaustive<3>());
    SECTION("exhaustive C=4", exhaustive<4>());
    SECTION("exhaustive C=5", exhaustive<5>());
    SECTION("exhaustive C=6", exhaustive<6>());
    SECTION("random C=20", random_rows<20>(400));
    SECTION("random C=24", random_rows<24>(1500));
    SECTION("random C=37", random_rows<37>(400));
    SECTION("random C=48", random_rows<48>(1500));
    SECTION("extremes C=24", extremes<24>());
    SECTION("extremes C=48", extremes<48>());
    SECTION("keys", keys(64));
    return g_bad ? 1 : 0;
}

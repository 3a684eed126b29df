// abs_ncell_check.cpp -- host check of the NARROW N cell of the bit-sliced adapter arithmetic (test infrastructure, plain g++).
//
// qcat_amd/csrc/abs_core.h: in an N column of a template the difference b = G(i,j) - G(i,j-1) stays in 0..3, so abs_cell_n2
// keeps two planes of row state per N column.  Three checks, each against something that does not share the cell's code:
//   (a) abs_cell_n2 against abs_cell_n_ref on all 40 valid inputs (a in 0..9, b in 0..3), with garbage in b[2], b[3];
//   (b) the premise itself, on a scalar DP of the adapter scoring written here in plain ints: b <= 3 in every N cell, for
//       templates with an N run first, last, twice, of one column, and nothing but N;
//   (c) plans emitted for those templates by qcat_amd/abs_plan.py at test time (the shipped kits hold none of these
//       shapes), two-stage, four-stage and front-padded, 32 alignments at a time against the oracle's qo_sg, score and
//       end_query -- with garbage in the upper planes of every N column's row state, which must come back untouched.
// Built and run by tests/test_abs_ncell_host.py, which writes abs_ncell_plans.inc / abs_ncell_cases.inc:
//     g++ -O2 -std=c++17 -I qcat_amd/csrc -I <tmp> tests/abs_ncell_check.cpp -o <tmp>/abs_ncell_check -L oracle -lqcat_oracle
//     abs_ncell_check <seed> <rounds>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "abs_core.h"
#include "abs_ncell_plans.inc"

extern "C" int qo_sg_rule(const char* s1, int L, const char* s2, int M, int open, int extend, const int8_t* mat, int rule,
                          int32_t* score, int32_t* end_query, int32_t* end_ref);

using namespace qabs;

static uint64_t g_s;
static uint64_t rnd() { g_s += 0x9E3779B97F4A7C15ull; uint64_t z = g_s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static int below(int n) { return (int)((rnd() >> 33) % (uint64_t)n); }
static const char BASES[] = "ATGC";                 // plane codes 0..3 (qcat_amd/codes.py)
static const u32 JUNK2 = 0xDEADBEEFu, JUNK3 = 0x5A5AA5A5u;

static void adapter_matrix(int8_t* m) {             // qcat/config.py:236-253, [target code * 7 + query code]; codes A T G C N X other
    for (int t = 0; t < 7; ++t)
        for (int q = 0; q < 7; ++q)
            m[t * 7 + q] = (int8_t)((t >= 5 || q >= 5) ? 0 : ((t == 4 || q == 4) ? -1 : (t == q ? 5 : -2)));
}

// random / tandem-repeat / adapter-bearing (whole or a suffix, with errors) window of L letters
static std::string make_window(const std::string* tpls, int nt, int L) {
    std::string w;
    const int kind = below(10);
    if (kind == 0) {
        const int p = 1 + below(3);
        char unit[4];
        for (int i = 0; i < p; ++i) unit[i] = BASES[below(4)];
        for (int i = 0; i < L; ++i) w.push_back(unit[i % p]);
        return w;
    }
    if (kind == 1) {
        for (int i = 0; i < L; ++i) w.push_back(BASES[below(4)]);
        return w;
    }
    const std::string& t = tpls[below(nt)];
    const int lead = below(60);
    for (int i = 0; i < lead; ++i) w.push_back(BASES[below(4)]);
    const int err = below(25);
    const int from = kind == 2 ? below((int)t.size()) : 0;
    for (size_t j = (size_t)from; j < t.size(); ++j) {
        const char c = t[j] == 'N' ? BASES[below(4)] : t[j];
        if (below(100) < err) {
            const int k = below(3);
            if (k == 0) w.push_back(BASES[below(4)]);
            else if (k == 2) { w.push_back(BASES[below(4)]); w.push_back(c); }
        } else w.push_back(c);
    }
    while ((int)w.size() < L) w.push_back(BASES[below(4)]);
    w.resize((size_t)L);
    return w;
}

// ---- (a) ----
static int check_cell() {
    int bad = 0;
    for (int base = 0; base < 40; base += 32) {
        u32 a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        const int n = std::min(32, 40 - base);
        for (int bit = 0; bit < n; ++bit) {
            const int av = (base + bit) / 4, bv = (base + bit) % 4;
            for (int k = 0; k < 4; ++k) { a[k] |= (u32)((av >> k) & 1) << bit; b[k] |= (u32)((bv >> k) & 1) << bit; }
        }
        const u32 live = n == 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
        u32 ar[4], br[4];
        for (int k = 0; k < 4; ++k) { ar[k] = a[k]; br[k] = b[k]; }
        abs_cell_n_ref(ar, br);
        u32 got[2][6];
        for (int g = 0; g < 2; ++g) {
            u32 a2[4], b2[4];
            for (int k = 0; k < 4; ++k) { a2[k] = a[k]; b2[k] = b[k]; }
            b2[2] = g ? JUNK2 : ~JUNK2; b2[3] = g ? JUNK3 : ~JUNK3;                 // the upper planes: garbage, either way round
            abs_cell_n2(a2, b2);
            bad += b2[2] != (g ? JUNK2 : ~JUNK2) || b2[3] != (g ? JUNK3 : ~JUNK3);     // ... untouched
            for (int k = 0; k < 4; ++k) bad += ((a2[k] ^ ar[k]) & live) != 0;
            for (int k = 0; k < 2; ++k) bad += ((b2[k] ^ br[k]) & live) != 0;
            bad += ((br[2] | br[3]) & live) != 0;                                   // the reference's b' fits two planes
            for (int k = 0; k < 4; ++k) got[g][k] = a2[k] & live;
            got[g][4] = b2[0] & live; got[g][5] = b2[1] & live;
        }
        bad += memcmp(got[0], got[1], sizeof got[0]) != 0;                          // ... and without influence
    }
    printf("cell: abs_cell_n2 against abs_cell_n_ref on all 40 valid inputs, garbage in b[2], b[3]: %d mismatches\n", bad);
    return bad;
}

// ---- (b) ----  H(i,0) = H(0,j) = 0; H = max(diagonal + W, up - 2, left - 2); b = H(i,j) - H(i,j-1) + 2
static int check_premise(const char* name, const std::string& tpl, int rounds) {
    const int M = (int)tpl.size();
    int bad = 0, bmax = 0;
    long cells = 0;
    for (int r = 0; r < rounds; ++r) {
        const int L = r < 150 ? r + 1 : 1 + below(150);                // every row count 1..150 at least once
        const std::string w = make_window(&tpl, 1, L);
        std::vector<int> prev((size_t)M + 1, 0), cur((size_t)M + 1, 0);
        for (int i = 1; i <= L; ++i) {
            cur[0] = 0;
            for (int j = 1; j <= M; ++j) {
                const int W = tpl[(size_t)j - 1] == 'N' ? -1 : (tpl[(size_t)j - 1] == w[(size_t)i - 1] ? 5 : -2);
                cur[(size_t)j] = std::max(prev[(size_t)j - 1] + W, std::max(prev[(size_t)j] - 2, cur[(size_t)j - 1] - 2));
                if (tpl[(size_t)j - 1] == 'N') {
                    const int b = cur[(size_t)j] - cur[(size_t)j - 1] + 2;
                    ++cells;
                    bmax = std::max(bmax, b);
                    if (b < 0 || b > 3) ++bad;
                }
            }
            std::swap(prev, cur);
        }
    }
    printf("premise %s: %d windows of 1..150 rows, %ld N cells, largest b %d: %d mismatches\n", name, rounds, cells, bmax, bad);
    return bad;
}

// ---- (c) ----  row state with garbage in the upper planes of the N columns
template <int NC, class T>
static void init_rows(u32 (&h)[NC][4], const T (&isn)[NC]) {
    for (int j = 0; j < NC; ++j) { abs_set2(h[j]); if (isn[j]) { h[j][2] = JUNK2; h[j][3] = JUNK3; } }
}
template <int NC, class T>
static int rows_untouched(const u32 (&h)[NC][4], const T (&isn)[NC]) {
    int bad = 0;
    for (int j = 0; j < NC; ++j) if (isn[j]) bad += h[j][2] != JUNK2 || h[j][3] != JUNK3;
    return bad;
}
template <int NC, class T>
static void hold_rows(u32 (&h)[NC][4], const T (&isn)[NC], u32 hold) {        // what kernels_abs_mid.inc's abs_hold2_cols does
    for (int j = 0; j < NC; ++j) { if (isn[j]) abs_hold2_n(h[j], hold); else abs_hold2(h[j], hold); }
}

static void planes_of(const std::vector<std::string>& win, const int* len, int L, std::vector<u32>& c1, std::vector<u32>& c0, std::vector<u32>& ns) {
    c1.assign((size_t)L, 0u); c0.assign((size_t)L, 0u); ns.assign((size_t)L, 0u);
    for (int i = 0; i < L; ++i)
        for (int b = 0; b < 32; ++b) {
            const int pad = L - len[b];
            if (i < pad) { ns[(size_t)i] |= 1u << b; if (rnd() & 1) c1[(size_t)i] |= 1u << b; continue; }     // (whatever letters: the hold wipes them)
            const int code = (int)(strchr(BASES, win[(size_t)b][(size_t)(i - pad)]) - BASES);
            c1[(size_t)i] |= (u32)((code >> 1) & 1) << b;
            c0[(size_t)i] |= (u32)(code & 1) << b;
        }
}

static int compare(const char* name, int r, int t, const AbsBorder& bd, const AbsLastRow& lr, int L, const std::vector<std::string>& win, const int* len,
                   const std::string& tpl, const int8_t* mat) {
    u32 val[ABS_NF + 1], endq[ABS_NI];
    abs_decide(bd, lr, (unsigned)(L - 1), val, endq, false);
    const int M = (int)tpl.size();
    int bad = 0;
    for (int b = 0; b < 32; ++b) {
        int v = 0, e = 0;
        for (int k = 0; k <= ABS_NF; ++k) v |= (int)((val[k] >> b) & 1u) << k;
        for (int k = 0; k < ABS_NI; ++k) e |= (int)((endq[k] >> b) & 1u) << k;
        const int score = v - 2 * M - 1;
        e -= L - len[b];
        int32_t ws, wq, wr;
        qo_sg_rule(win[(size_t)b].c_str(), len[b], tpl.c_str(), M, 2, 2, mat, 0, &ws, &wq, &wr);
        if (score != ws || e != wq) {
            if (bad < 5) fprintf(stderr, "%s round %d template %d alignment %d (len %d of %d): got (%d, %d), oracle (%d, %d)\n  %s\n", name, r, t, b, len[b], L,
                                 score, e, ws, wq, win[(size_t)b].c_str());
            ++bad;
        }
    }
    return bad;
}

// a two-stage plan; padded: 32 queries of unequal length padded at the front, held at the boundary state until they start
// (the calls of kernels_abs_mid.inc's two stages in their order; single-template plans)
template <class P>
static int check_plan(const char* name, const std::string* tpls, int rounds, int L, bool padded) {
    int8_t mat[49];
    adapter_matrix(mat);
    int bad = 0;
    for (int r = 0; r < rounds; ++r) {
        std::vector<std::string> win(32);
        int len[32], pz = 0;
        for (int b = 0; b < 32; ++b) {
            len[b] = (!padded || b == 0) ? L : L - below(r % 2 ? L : std::min(L, 71));
            win[(size_t)b] = make_window(tpls, P::NT, len[b]);
            pz = std::max(pz, L - len[b]);
        }
        std::vector<u32> c1, c0, ns;
        planes_of(win, len, L, c1, c0, ns);
        static u32 h0[P::NC0][4], h1[P::NC1][4];
        init_rows(h0, P::N0); init_rows(h1, P::N1);
        AbsBorder bd[P::NT];
        memset(bd, 0, sizeof bd);
        u32 prev_ns = 0xFFFFFFFFu;
        for (int i = 0; i < L; ++i) {
            u32 nq[4], ho[P::NH][4];
            const u32 nsm = i < pz ? ns[(size_t)i] : 0u;
            abs_neq_masks(c1[(size_t)i], c0[(size_t)i], nq);
            P::row0(nq, h0, ho);
            if (i < pz) { hold_rows(h0, P::N0, nsm); for (int k = 0; k < P::NH; ++k) abs_hold2(ho[k], nsm); }
            const u32 first = prev_ns & ~nsm;
            prev_ns = nsm;
            P::row1(nq, h1, ho, bd, first, (unsigned)i);
            if (i < pz) hold_rows(h1, P::N1, nsm);
        }
        AbsLastRow lo[P::NH], lr[P::NT];
        P::last0(h0, lo);
        P::last1(h1, lo, lr);
        bad += rows_untouched(h0, P::N0) + rows_untouched(h1, P::N1);
        for (int t = 0; t < P::NT; ++t) bad += compare(name, r, t, bd[t], lr[t], L, win, len, tpls[t], mat);
    }
    printf("%s%s: %d rounds x 32 alignments x %d template(s), L = %d: %d mismatches\n", name, padded ? " front-padded" : "", rounds, P::NT, L, bad);
    return bad;
}

// a plan of four stages: the stages of a row one after the other, each handing its differences to the next
template <class P>
static int check_multi(const char* name, const std::string* tpls, int rounds, int L) {
    static_assert(P::NS == 4, "four stages");
    typedef typename P::S0 A0; typedef typename P::S1 A1; typedef typename P::S2 A2; typedef typename P::S3 A3;
    int8_t mat[49];
    adapter_matrix(mat);
    int bad = 0;
    for (int r = 0; r < rounds; ++r) {
        std::vector<std::string> win(32);
        int len[32];
        for (int b = 0; b < 32; ++b) { len[b] = L; win[(size_t)b] = make_window(tpls, P::NT, L); }
        std::vector<u32> c1, c0, ns;
        planes_of(win, len, L, c1, c0, ns);
        static u32 h0[A0::NC][4], h1[A1::NC][4], h2[A2::NC][4], h3[A3::NC][4];
        init_rows(h0, A0::N); init_rows(h1, A1::N); init_rows(h2, A2::N); init_rows(h3, A3::N);
        AbsBorder b0[A0::BD], b1[A1::BD], b2[A2::BD], b3[A3::BD];
        memset(b0, 0, sizeof b0); memset(b1, 0, sizeof b1); memset(b2, 0, sizeof b2); memset(b3, 0, sizeof b3);
        for (int i = 0; i < L; ++i) {
            u32 nq[4], x0[A0::HI][4], o0[A0::HO][4], o1[A1::HO][4], o2[A2::HO][4], o3[A3::HO][4];
            const u32 first = i == 0 ? 0xFFFFFFFFu : 0u;
            abs_neq_masks(c1[(size_t)i], c0[(size_t)i], nq);
            A0::row(nq, h0, x0, o0, b0, first, (unsigned)i);
            A1::row(nq, h1, o0, o1, b1, first, (unsigned)i);
            A2::row(nq, h2, o1, o2, b2, first, (unsigned)i);
            A3::row(nq, h3, o2, o3, b3, first, (unsigned)i);
        }
        AbsLastRow y0[A0::HI], l0[A0::HO], l1[A1::HO], l2[A2::HO], l3[A3::HO], r0[A0::BD], r1[A1::BD], r2[A2::BD], r3[A3::BD];
        A0::last(h0, y0, l0, r0);
        A1::last(h1, l0, l1, r1);
        A2::last(h2, l1, l2, r2);
        A3::last(h3, l2, l3, r3);
        bad += rows_untouched(h0, A0::N) + rows_untouched(h1, A1::N) + rows_untouched(h2, A2::N) + rows_untouched(h3, A3::N);
        AbsBorder bd[2]; AbsLastRow lr[2];
        int seen = 0;
        auto take = [&](int t, const AbsBorder& b, const AbsLastRow& l) { if (t >= 0) { bd[t] = b; lr[t] = l; ++seen; } };
        take(A0::BT0, b0[0], r0[0]); if (A0::NBD > 1) take(A0::BT1, b0[A0::BD - 1], r0[A0::BD - 1]);
        take(A1::BT0, b1[0], r1[0]); if (A1::NBD > 1) take(A1::BT1, b1[A1::BD - 1], r1[A1::BD - 1]);
        take(A2::BT0, b2[0], r2[0]); if (A2::NBD > 1) take(A2::BT1, b2[A2::BD - 1], r2[A2::BD - 1]);
        take(A3::BT0, b3[0], r3[0]); if (A3::NBD > 1) take(A3::BT1, b3[A3::BD - 1], r3[A3::BD - 1]);
        if (seen != P::NT) { fprintf(stderr, "%s: %d borders for %d templates\n", name, seen, P::NT); return 1000; }
        for (int t = 0; t < P::NT; ++t) bad += compare(name, r, t, bd[t], lr[t], L, win, len, tpls[t], mat);
    }
    printf("%s: %d rounds x 32 alignments x %d template(s), L = %d: %d mismatches\n", name, rounds, P::NT, L, bad);
    return bad;
}

int main(int argc, char** argv) {
    g_s = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 12;
    int bad = check_cell();
#include "abs_ncell_cases.inc"
    return bad ? 1 : 0;
}

// affine_host_check.cpp -- the lane arithmetic of an affine-gap adapter alignment (qcat_amd/csrc/affine_core.h) on the CPU:
// the packed recurrence two alignments per "lane" (the 16-bit halves of every word, one shared template), driven row by
// row the way a packed kernel would drive it -- tables from aff_build_table, rows beyond a half's own window frozen, keys of
// the last column per row and of the last row after the loop, aff_decode under both R1 rules -- against
//   1. the independent scalar DP's recorded answers for the affine family of tests/golden/sg_vectors.json (a file the
//      test writes: one line per case), the other half of the lane holding a shorter cut of the same window;
//   2. the oracle's DP (qo_sg_rule) on random cases: open < extend and open = extend + 1..4, match 1..9, mismatch -1..-6,
//      N in the target, windows of 1..150 letters (any letter), template lengths at both edges of every width class, in
//      the adapter width classes with their padding cap;
//   3. the oracle's DP on ALL windows of up to 6 letters against ALL templates of up to 4 letters over ACGT (W = 8).
// Prints one line per section: "<section>: <n> cases, <k> mismatches".
//
// usage: affine_host_check <golden case file> <seed>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kit.h"
#include "affine_core.h"

extern "C" int qo_sg_rule(const char* s1, int L, const char* s2, int M, int open, int extend, const int8_t* mat, int rule,
                          int32_t* score, int32_t* end_query, int32_t* end_ref);

using namespace qk;

struct HostTbl {
    const u32* t;
    u32 operator()(int j) const { return t[j]; }
    void fence(int) const {}
};

template <int W, int PADCAP, bool RAGGED>
static void lane_run(const u32* tbl, u32 special, int M, const AffCost& c, const uint8_t* q0, int L0, const uint8_t* q1, int L1,
                     u32 (&rk)[2], u32 (&ck)[2]) {
    u32 S[W + 1], F[W + 1];
    const int start = W - M, Lmax = L0 > L1 ? L0 : L1;
    aff_init<W>(S, F, start, c);
    const u32 ad2 = aff_splat(c.ad), csrc2 = aff_splat(c.csrc);
    ck[0] = ck[1] = 0;
    const HostTbl ht{tbl};
    for (int i = 1; i <= Lmax; ++i) {
        const u32 qb = (u32)(i <= L0 ? q0[i - 1] : QCAT_CODE_PAD) | ((u32)(i <= L1 ? q1[i - 1] : QCAT_CODE_PAD) << 4);
        const u32 mask = RAGGED ? aff_row_mask(i, L0, L1) : 0xFFFFFFFFu;
        const u32 sW = aff_row<W, RAGGED, PADCAP>(S, F, start, i, aff_sel(qb), special, ht, c, ad2, csrc2, mask);
        aff_col_keys(sW, i, c, ck);
    }
    aff_row_keys<W, PADCAP>(S, start, c, rk);
}

template <int W, int PADCAP>
static void lane_dispatch(bool ragged, const u32* tbl, u32 special, int M, const AffCost& c, const uint8_t* q0, int L0,
                          const uint8_t* q1, int L1, u32 (&rk)[2], u32 (&ck)[2]) {
    if (ragged) lane_run<W, PADCAP, true>(tbl, special, M, c, q0, L0, q1, L1, rk, ck);
    else lane_run<W, PADCAP, false>(tbl, special, M, c, q0, L0, q1, L1, rk, ck);
}

struct Expect { int score[2], endq[2]; bool have[2]; };      // per R1 rule: [0] striped, [1] scalar

static Expect from_oracle(const std::string& q, const std::string& t, int open, int ext, const int8_t* mat) {
    Expect e;
    const int rules[2] = {QCAT_R1_STRIPED, QCAT_R1_SCALAR};
    for (int r = 0; r < 2; ++r) {
        int32_t sc = 0, eq = 0, er = 0;
        if (qo_sg_rule(q.data(), (int)q.size(), t.data(), (int)t.size(), open, ext, mat, rules[r], &sc, &eq, &er) != 0) {
            fprintf(stderr, "qo_sg_rule failed\n");
            exit(2);
        }
        e.score[r] = sc; e.endq[r] = eq; e.have[r] = true;
    }
    return e;
}

struct Tally { long cases = 0, bad = 0, ineligible = 0; };

// one lane: template t against the windows q[0] (lo half) and q[1] (hi half); width 0: the widest array with any padding
// (W = 128, PADCAP = 128), 8: the small array of the exhaustive section, else an adapter width class (PADCAP = 8)
static void check_lane(int width, bool force_ragged, const std::string& t, const std::string q[2], int open, int ext,
                       const int8_t* mat, const Expect ex[2], Tally* tally, const char* what) {
    const int M = (int)t.size();
    const int W = width ? width : 128;
    std::vector<uint8_t> tc(M), qc[2];
    for (int j = 0; j < M; ++j) tc[j] = code_of_ascii((uint8_t)t[j]);
    for (int h = 0; h < 2; ++h) {
        qc[h].resize(q[h].size() + 1);
        for (size_t i = 0; i < q[h].size(); ++i) qc[h][i] = code_of_ascii((uint8_t)q[h][i]);
    }
    const AffCost c = aff_cost(open, ext);
    std::vector<u32> tbl(W);
    u32 special = 0xFFFFFFFFu;
    if (!aff_build_table(mat, tc.data(), M, c, tbl.data(), &special, W)) { tally->ineligible++; return; }
    const int L0 = (int)q[0].size(), L1 = (int)q[1].size();
    const bool ragged = force_ragged || L0 != L1;
    u32 rk[2], ck[2];
    switch (width) {
#define CASE_W(WW) case WW: lane_dispatch<WW, AFF_PADMAX>(ragged, tbl.data(), special, M, c, qc[0].data(), L0, qc[1].data(), L1, rk, ck); break;
        CASE_W(8) CASE_W(40) CASE_W(48) CASE_W(56) CASE_W(60) CASE_W(64) CASE_W(84) CASE_W(92) CASE_W(104) CASE_W(112) CASE_W(120) CASE_W(128)
#undef CASE_W
        case 0: lane_dispatch<128, 128>(ragged, tbl.data(), special, M, c, qc[0].data(), L0, qc[1].data(), L1, rk, ck); break;
        default: fprintf(stderr, "no such width %d\n", width); exit(2);
    }
    for (int h = 0; h < 2; ++h) {
        const int L = h ? L1 : L0;
        if (L < 1) continue;
        for (int r = 0; r < 2; ++r) {
            if (!ex[h].have[r]) continue;
            const AffResult got = aff_decode(rk[h], ck[h], L, M, W - M, c, r == 1);
            tally->cases++;
            if (got.score != ex[h].score[r] || got.end_query != ex[h].endq[r]) {
                if (tally->bad++ < 5)
                    fprintf(stderr, "%s: half %d rule %d open %d ext %d W %d: got (%d, %d) want (%d, %d)\n  t=%s\n  q=%s\n", what, h, r, open, ext, W,
                            got.score, got.end_query, ex[h].score[r], ex[h].endq[r], t.c_str(), q[h].c_str());
            }
        }
    }
}

static uint64_t g_rng = 1;
static uint32_t rnd(uint32_t n) {        // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (uint32_t)(z % n);
}
static std::string rand_seq(int n, const char* alpha) {
    const int na = (int)strlen(alpha);
    std::string s((size_t)n, 'A');
    for (int i = 0; i < n; ++i) s[i] = alpha[rnd(na)];
    return s;
}
static void custom_table(int match, int mismatch, int nmatch, int8_t* m) {      // [target * 7 + query], qcat/config.py:236-253
    memset(m, 0, 49);
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m[i * 7 + j] = (int8_t)(i == j ? match : mismatch);
    for (int j = 0; j < 5; ++j) { m[4 * 7 + j] = (int8_t)nmatch; m[j * 7 + 4] = (int8_t)nmatch; }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <golden case file> <seed>\n", argv[0]); return 2; }
    g_rng = strtoull(argv[2], nullptr, 10);
    long total_bad = 0;

    {   // ---- 1. the independent DP's answers --------------------------------------------------------------------------------
        // line: open extend <49 table values> target window score end_query_striped end_query_scalar (-9: not recorded)
        Tally tl;
        FILE* fh = fopen(argv[1], "r");
        if (!fh) { perror(argv[1]); return 2; }
        std::vector<char> tb(4096), qb(4096);
        long line = 0;
        for (;; ++line) {
            int open, ext, tv[49];
            if (fscanf(fh, "%d %d", &open, &ext) != 2) break;
            int8_t mat[49];
            for (int x = 0; x < 49; ++x) { if (fscanf(fh, "%d", &tv[x]) != 1) return 2; mat[x] = (int8_t)tv[x]; }
            int score, eq_striped, eq_scalar;
            if (fscanf(fh, "%4000s %4000s %d %d %d", tb.data(), qb.data(), &score, &eq_striped, &eq_scalar) != 5) return 2;
            const std::string t(tb.data()), q(qb.data());
            if (!aff_range_ok(9, -6, open, ext, 151, 128)) { fprintf(stderr, "golden case out of range\n"); return 2; }
            // the partner half: a shorter cut of the same window (its answers from the oracle), alternately lo and hi
            const size_t cut = q.size() > 1 ? 1 + (size_t)rnd((uint32_t)q.size() - 1) : 1;
            const std::string partner = (line & 2) ? q.substr(q.size() - cut) : q.substr(0, cut);
            Expect golden;
            golden.score[0] = golden.score[1] = score; golden.endq[0] = eq_striped; golden.endq[1] = eq_scalar;
            golden.have[0] = true; golden.have[1] = eq_scalar != -9;
            Expect ex[2];
            std::string qs[2];
            const int gh = (int)(line & 1);
            qs[gh] = q; ex[gh] = golden;
            qs[1 - gh] = partner; ex[1 - gh] = from_oracle(partner, t, open, ext, mat);
            ex[1 - gh].have[0] = ex[1 - gh].have[1] = false;          // (counted in section 2's terms only: this section counts the recorded answers)
            Tally side;
            check_lane(0, false, t, qs, open, ext, mat, ex, &tl, "golden");
            ex[gh].have[0] = ex[gh].have[1] = false; ex[1 - gh].have[0] = ex[1 - gh].have[1] = true;
            check_lane(0, false, t, qs, open, ext, mat, ex, &side, "golden partner");
            tl.bad += side.bad;
        }
        fclose(fh);
        printf("golden affine family: %ld cases, %ld mismatches\n", tl.cases, tl.bad);
        if (tl.ineligible) { printf("golden affine family: %ld lanes without tables\n", tl.ineligible); total_bad += tl.ineligible; }
        total_bad += tl.bad;
    }

    {   // ---- 2. random cases in the adapter width classes ---------------------------------------------------------------------
        Tally tl;
        const int widths[] = {40, 48, 56, 60, 64, 84, 92, 104, 112, 120, 128};
        int lo_edge[11], hi_edge[11];
        for (int w = 0; w < 11; ++w) {
            lo_edge[w] = hi_edge[w] = widths[w];
            for (int len = 1; len <= 128; ++len) if (adapter_width_class(len) == widths[w] && len < lo_edge[w]) lo_edge[w] = len;
        }
        for (int n = 0; n < 24000; ++n) {
            const int w = (int)rnd(11);
            const int pick = (int)rnd(4);
            const int M = pick == 0 ? lo_edge[w] : (pick == 1 ? hi_edge[w] : lo_edge[w] + (int)rnd((uint32_t)(hi_edge[w] - lo_edge[w] + 1)));
            const int ext = (int)rnd(5);                                         // 0..4
            const int open = rnd(3) == 0 ? (int)rnd((uint32_t)ext + 1) - (ext > 0 && rnd(2) ? 0 : 0) : ext + 1 + (int)rnd(4);
            if (open == ext) { --n; continue; }                                   // (linear gaps are another kernel's)
            int8_t mat[49];
            custom_table(1 + (int)rnd(9), -(1 + (int)rnd(6)), -(int)rnd(3), mat);
            if (!aff_range_ok(9, -6, open, ext, 151, 128)) { fprintf(stderr, "random case out of range\n"); return 2; }
            const std::string t = rand_seq(M, rnd(3) == 0 ? "ACGTN" : "ACGT");
            std::string qs[2];
            Expect ex[2];
            const int Lsame = 1 + (int)rnd(150);
            const bool same = rnd(4) == 0;
            for (int h = 0; h < 2; ++h) {
                const int L = same ? Lsame : (rnd(3) == 0 ? 150 : 1 + (int)rnd(150));
                const char* alpha = rnd(8) == 0 ? "ACGTNacgtnRYKMSWXx*-U." : (rnd(4) == 0 ? "ACGTN" : "ACGT");
                std::string q;
                if (rnd(2)) {                                                    // a noisy copy of the template somewhere in the window
                    q = rand_seq((int)rnd(60), "ACGT");
                    for (int j = 0; j < M; ++j) {
                        const uint32_t r = rnd(100);
                        if (r < 5) continue;                                     // deletion
                        if (r < 10) q += rand_seq(1 + (int)rnd(rnd(4) == 0 ? 9 : 2), "ACGT");     // insertion
                        q += r < 18 ? "ACGT"[rnd(4)] : (t[j] == 'N' ? 'A' : t[j]);
                        if (r == 99) j += (int)rnd(9);                           // a long deletion
                    }
                    q += rand_seq(150, alpha);
                    q = q.substr(0, (size_t)L);
                } else q = rand_seq(L, alpha);
                qs[h] = q;
                ex[h] = from_oracle(q, t, open, ext, mat);
            }
            check_lane(widths[w], same && rnd(2), t, qs, open, ext, mat, ex, &tl, "random");
        }
        printf("random against the oracle: %ld cases, %ld mismatches\n", tl.cases, tl.bad);
        if (tl.ineligible) { printf("random against the oracle: %ld lanes without tables\n", tl.ineligible); total_bad += tl.ineligible; }
        total_bad += tl.bad;
    }

    {   // ---- 3. every window of up to 6 letters against every template of up to 4 letters --------------------------------------
        Tally tl;
        std::vector<std::string> wins, tpls;
        for (int len = 1; len <= 6; ++len)
            for (int x = 0; x < (1 << (2 * len)); ++x) {
                std::string s((size_t)len, 'A');
                for (int i = 0; i < len; ++i) s[i] = "ACGT"[(x >> (2 * i)) & 3];
                wins.push_back(s);
                if (len <= 4) tpls.push_back(s);
            }
        const int cfg[4][4] = {{3, 1, 5, -2}, {1, 3, 5, -2}, {2, 1, 1, -1}, {6, 2, 9, -6}};        // open, extend, match, mismatch
        for (int k = 0; k < 4; ++k) {
            int8_t mat[49];
            custom_table(cfg[k][2], cfg[k][3], -1, mat);
            // the oracle's answers once per (window, template)
            for (const std::string& t : tpls) {
                std::vector<Expect> ex(wins.size());
                for (size_t i = 0; i < wins.size(); ++i) ex[i] = from_oracle(wins[i], t, cfg[k][0], cfg[k][1], mat);
                // halves: window i with window n - 1 - i (a short one beside a long one), and with itself (the uniform form)
                for (size_t i = 0; i < wins.size(); ++i) {
                    const size_t o = (i & 1) ? i : wins.size() - 1 - i;
                    const std::string qs[2] = {wins[i], wins[o]};
                    const Expect e2[2] = {ex[i], ex[o]};
                    check_lane(8, false, t, qs, cfg[k][0], cfg[k][1], mat, e2, &tl, "exhaustive");
                }
            }
        }
        printf("exhaustive 6 x 4: %ld cases, %ld mismatches\n", tl.cases, tl.bad);
        if (tl.ineligible) { printf("exhaustive 6 x 4: %ld lanes without tables\n", tl.ineligible); total_bad += tl.ineligible; }
        total_bad += tl.bad;
    }
    return total_bad ? 1 : 0;
}

// eval_check.cpp -- the passes of qcat_batch_eval on the host (no GPU): the classify pass's vector and lane schedule and the ROC
// kernel's rows run through the functions the kernels call (qcat_amd/csrc/eval_core.h), against a byte-by-byte sequential
// restatement of qcat/eval.py and qcat/eval_roc.py written here with strings and doubles.
//   tokenizer    (one lane, and every lane of the group shape against it) titles at every alignment 0..15 of the text plane, of one byte, ending at the plane's last byte, with the keys
//                straddling every 16-byte boundary position, longer than 4096 bytes; loads outside the plane's slack are counted
//   membership   bc in V.split(","), bc == V, V == "none" for single and dual call texts
//   buckets      q < bucket against score < q / 10.0 in doubles for every denominator 1..255 and raw score 0..den + den / 4
//   batches      both shapes of the classify pass -- one lane and a group of EVAL_GROUP lanes per read, whose exchange of masks is
//                played by computing the other lane's masks --: 0, 1, 63, 64, 65, 257 reads (and one more than a full grid's
//                first round): classes, kinds,
//                buckets, the four counts, the histogram and the 1001 x 6 table, dropped reads included; the first bad read
// Usage: eval_check SEED.  Built with -I qcat_amd/csrc -I tests.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "check_common.h"
#include "eval_core.h"

using namespace qev;

// ---- the restatement ---------------------------------------------------------------------------------------------------------------
static std::vector<std::string> split(const std::string& s, char c) {
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        const size_t p = s.find(c, at);
        out.push_back(s.substr(at, p == std::string::npos ? std::string::npos : p - at));
        if (p == std::string::npos) return out;
        at = p + 1;
    }
}
// _parse_reads_info: false when the key is missing
static bool info_of(const std::string& comment, const std::string& key, std::string* value) {
    bool has = false;
    for (const std::string& pair : split(comment, ' ')) {
        const std::vector<std::string> cols = split(pair, '=');
        if (cols.size() == 2 && cols[0] == key) { has = true; *value = cols[1]; }
    }
    return has;
}
struct Want { uint8_t cls, kind; uint32_t bucket; double score; bool called; };
// eval.py:146-165 and the kind eval_roc.py:41-64 needs; title: tabs are blanks already
static Want want_of(const std::string& title, bool from_comment, const std::string& bc_text, bool called, int raw, int den) {
    Want w; w.cls = 0; w.kind = 0; w.bucket = 0; w.score = -1.0; w.called = false;
    const size_t blank = title.find(' ');
    const std::string name = title.substr(0, blank), comment = blank == std::string::npos ? std::string() : title.substr(blank + 1);
    std::string V, bc = "none";
    if (from_comment) {
        if (!info_of(comment, "truebc", &V)) { w.cls = CLS_BAD | BAD_NO_TRUEBC; return w; }
        std::string b;
        if (!info_of(comment, "barcode", &b)) { w.cls = CLS_BAD | BAD_NO_BARCODE; return w; }
        if (!b.empty()) bc = b;
    } else {
        if (name.empty()) { w.cls = CLS_BAD | BAD_EMPTY_NAME; return w; }
        if (name.compare(0, 4, "name") == 0) { w.cls = CLS_BAD | BAD_NAME_HEADER; return w; }
        if (!info_of(comment, "truebc", &V)) { w.cls = CLS_BAD | BAD_NO_TRUEBC; return w; }
        if (called) {
            if (den < 1 || raw < 0) { w.cls = CLS_BAD | BAD_SCORE; return w; }
            bc = bc_text; w.called = true; w.score = (double)raw * 100.0 / (1.0 * (double)den);
        }
    }
    const std::vector<std::string> truebc = split(V, ',');
    if (std::find(truebc.begin(), truebc.end(), bc) != truebc.end()) w.cls = CLS_CORRECT;
    else if (bc == "none") w.cls = CLS_FN;
    else if (truebc.size() == 1 && truebc[0] == "none") w.cls = CLS_FP;
    else w.cls = CLS_INCORRECT;
    w.kind = V == "none" ? KIND_TRUTH_NONE : bc == V ? KIND_WHOLE : KIND_OTHER;
    if (bc == "none") w.called = false;
    if (w.called) for (uint32_t q = 0; q < EVAL_Q && !(w.score < q / 10.0); ++q) w.bucket = q + 1;
    return w;
}

// ---- a text plane of titles ----------------------------------------------------------------------------------------------------------
struct Titles {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    void add(const std::string& t, uint32_t gap) {
        bytes.insert(bytes.end(), gap, (uint8_t)'\n');
        off.push_back(bytes.size()); len.push_back((uint32_t)t.size());
        bytes.insert(bytes.end(), t.begin(), t.end());
    }
};
static const char* const TOKENS[] = {"truebc=1", "truebc=12", "truebc=1,12,3", "truebc=none", "truebc=", "truebc=1=2", "xtruebc=1", "truebc", "ch=3",
                                     "", "start_time=2018-08-01T13:31:17Z", "barcode=7", "barcode=", "barcode=none", "barcode=3/7", "truebc=3/7",
                                     "=", "==", "a=b=c", "truebd=1", "barcodes=2", "truebc=12,none", "x", "read=20208"};
static std::string random_tokens(uint32_t max_tokens) {
    std::string t;
    const uint32_t k = (uint32_t)rnd_below(max_tokens + 1);
    for (uint32_t i = 0; i < k; ++i) t += " " + std::string(TOKENS[rnd_below(sizeof TOKENS / sizeof *TOKENS)]);
    return t;
}
static std::string random_title(uint32_t max_tokens) {
    std::string t = rnd_below(16) ? std::string("r") + std::to_string(rnd_below(100000)) : std::string(rnd_below(2) ? "" : "names");
    t += random_tokens(max_tokens);
    while (!t.empty() && t.back() == ' ') t.pop_back();                     // (a stored title is right-stripped)
    return t;
}

static void scan_against(Section& s, Plane& p, uint64_t t0, uint32_t len) {
    const std::string title(p.at0() + t0, p.at0() + t0 + len);
    Scan S;
    scan_title(S, p.at0(), [&](uint64_t a) { return p.load16((int64_t)a); }, t0, len);
    // the group shape: every lane of the group ends with the one-lane scan's state; a lane's own masks are what the exchange hands out
    const auto load16 = [&](uint64_t a) { return p.load16((int64_t)a); };
    for (uint32_t gl = 0; gl < EVAL_GROUP; ++gl) {
        Scan G;
        scan_title_group(G, p.at0(), load16, [&](uint32_t mine, uint32_t k, uint64_t v0) {
            const uint32_t m = vector_masks(load16, v0, t0 + len);
            if (k == gl && m != mine) ++s.bad;
            return m;
        }, gl, t0, len);
        if (G.name_len != S.name_len || G.has_truebc != S.has_truebc || G.has_barcode != S.has_barcode ||
            (S.has_truebc && (G.truebc.b != S.truebc.b || G.truebc.e != S.truebc.e)) ||
            (S.has_barcode && (G.barcode.b != S.barcode.b || G.barcode.e != S.barcode.e))) ++s.bad;
    }
    const size_t blank = title.find(' ');
    const std::string comment = blank == std::string::npos ? std::string() : title.substr(blank + 1);
    std::string v, got;
    ++s.cases;
    if (S.name_len != (blank == std::string::npos ? title.size() : blank)) ++s.bad;
    for (int k = 0; k < 2; ++k) {
        const bool has = info_of(comment, k ? "barcode" : "truebc", &v);
        const Span sp = k ? S.barcode : S.truebc;
        if (has != ((k ? S.has_barcode : S.has_truebc) != 0)) { ++s.bad; continue; }
        if (has && (sp.e < sp.b || sp.e > t0 + len || std::string(p.at0() + sp.b, p.at0() + sp.e) != v)) ++s.bad;
        // the LAST counting token: no later one in the comment
        if (has && info_of(std::string(p.at0() + sp.e, p.at0() + t0 + len), k ? "barcode" : "truebc", &got)) ++s.bad;
    }
}

static void check_tokenizer(Section& s) {
    // every alignment, random titles; the last title ends at the plane's last byte
    for (uint32_t a = 0; a < 16; ++a)
        for (uint32_t round = 0; round < 40; ++round) {
            Titles t;
            t.add(random_title(8), a);
            t.add(round % 4 == 0 ? std::string(1, "x= "[round / 4 % 2]) : random_title(3), (uint32_t)rnd_below(40));
            t.add(random_title(8), (uint32_t)rnd_below(40));
            Plane p(t.bytes);
            for (size_t i = 0; i < t.off.size(); ++i) scan_against(s, p, t.off[i], t.len[i]);
            if (p.stray) ++s.bad;
        }
    // a comment longer than 4096 bytes: the key straddles every boundary position once, a later "truebc" wins
    for (uint32_t a = 0; a < 16; ++a) {
        std::string title = "read";
        for (uint32_t k = 0; k < 16; ++k) {
            title += " p=";
            while ((a + title.size() + 1) % 16 != (16 - k) % 16) title += 'z';
            title += " truebc=" + std::to_string(k + 1) + std::string(270, 'y') + " barcode=" + std::to_string(k);
        }
        Titles t;
        t.add(title, a);
        Plane p(t.bytes);
        scan_against(s, p, t.off[0], t.len[0]);
        if (title.size() <= 4096 || p.stray) ++s.bad;
    }
}

// ---- membership ------------------------------------------------------------------------------------------------------------------------
static void check_membership(Section& s) {
    const char* const values[] = {"1", "12", "2", "123", "none", "", "1,12,3", "12,1", "3/7", "3/7,1/2", "7/3", "none,1", ",", "1,", ",1", "nonee", "non", "3/", "/7"};
    const char* const calls[][2] = {{"1", nullptr}, {"12", nullptr}, {"2", nullptr}, {"123", nullptr}, {"3", "7"}, {"1", "2"}, {"", nullptr}};
    for (const char* value : values)
        for (size_t ci = 0; ci <= sizeof calls / sizeof *calls; ++ci) {
            Call c = call_none();
            std::string bc = "none";
            if (ci < sizeof calls / sizeof *calls) {
                c.none = 0; c.a = (const uint8_t*)calls[ci][0]; c.la = (uint32_t)strlen(calls[ci][0]);
                c.b = (const uint8_t*)calls[ci][1]; c.lb = calls[ci][1] ? (uint32_t)strlen(calls[ci][1]) : 0;
                bc = std::string(calls[ci][0]) + (calls[ci][1] ? "/" + std::string(calls[ci][1]) : std::string());
            }
            const std::string text = "pad" + std::string(value);
            const Span V{3, text.size()};
            const std::vector<std::string> list = split(value, ',');
            ++s.cases;
            if (list_holds_call((const uint8_t*)text.data(), V, c) != (std::find(list.begin(), list.end(), bc) != list.end())) ++s.bad;
            if (span_is_call((const uint8_t*)text.data(), V, c) != (bc == value)) ++s.bad;
            if (span_is_call((const uint8_t*)text.data(), V, call_none()) != (std::string(value) == "none")) ++s.bad;
            if (call_is_none(c) != (bc == "none")) ++s.bad;
        }
}

// ---- buckets ---------------------------------------------------------------------------------------------------------------------------
static void check_buckets(Section& s) {
    for (int den = 1; den <= 255; ++den)
        for (int raw = 0; raw <= den + den / 4; ++raw) {
            const double score = (double)raw * 100.0 / (1.0 * (double)den);
            const uint32_t b = bucket_of(raw, den);
            ++s.cases;
            for (uint32_t q = 0; q < EVAL_Q; ++q) if ((score < q / 10.0) == (q < b)) { ++s.bad; break; }
        }
}

// ---- batches: the classify pass's schedule and the ROC kernel's ---------------------------------------------------------------------------
static uint64_t g_seen_cls[5], g_seen_kind[3], g_seen_bucket[EVAL_BUCKETS], g_seen_bad[6];     // what the batches held, over the run
static void check_batch(Section& s, uint32_t n, bool dual, bool from_comment, int drop, int n_bad, bool group) {
    ++s.cases;
    // the id tables: one template, ids 1..130 (and 1..12 of the second set)
    std::vector<int32_t> ids0(130), ids1(12);
    for (size_t i = 0; i < ids0.size(); ++i) ids0[i] = (int32_t)i + 1;
    for (size_t i = 0; i < ids1.size(); ++i) ids1[i] = (int32_t)i + 1;
    const uint32_t n_ids[2] = {130, dual ? 12u : 0u};
    const int32_t* const ids[2] = {ids0.data(), dual ? ids1.data() : nullptr};
    const char* const kit_name[1] = {nullptr};
    qtsv::ScoreTable scores;
    for (uint32_t i = 0; i <= qtsv::TSV_MAX_DEN; ++i) scores.den_first[i] = scores.den_last[i] = -1;
    std::vector<uint8_t> blob;
    qtsv::Tables T;
    uint32_t den_off = 0;
    if (!qtsv::tables_build(false, dual, 1, n_ids, ids, kit_name, scores, &blob, &T, &den_off).empty()) { ++s.bad; return; }
    // titles, records, dropped reads
    Titles t;
    struct Rec { int bc, bc2, adapter, raw, den; bool dropped; };
    std::vector<Rec> recs(n);
    std::vector<Want> want(n);
    uint32_t first_bad = EVAL_NO_BAD;
    for (uint32_t r = 0; r < n; ++r) {
        Rec& x = recs[r];
        x.bc = rnd_below(4) ? (int)rnd_below(rnd_below(3) ? 13 : 130) : -1;
        x.bc2 = dual ? (int)rnd_below(12) : -1;
        x.adapter = rnd_below(10) ? 0 : (rnd_below(2) ? -1 : 1);
        x.den = 40 + (int)rnd_below(3);
        x.raw = (int)rnd_below((uint64_t)x.den + 3);
        x.dropped = !from_comment && (drop == 3 || (drop == 0 && r == 0) || (drop == 1 && r == n / 2) || (drop == 2 && r + 1 == n));
        std::string title = std::string("r") + std::to_string(r) + random_tokens(6) + " truebc=" +
                            (rnd_below(5) ? std::to_string(x.bc + 1) + (dual && rnd_below(3) ? "/" + std::to_string(x.bc2 + 1) : "") : std::string(rnd_below(2) ? "none" : "1,12,3"));
        if (from_comment) title += rnd_below(4) ? " barcode=" + std::to_string(rnd_below(4)) : std::string(rnd_below(2) ? " barcode=none" : " barcode=");
        if (rnd_below(6) == 0) title += " ch=" + std::to_string(r);
        const bool make_bad = n_bad && (r == n / 3 || (n_bad > 1 && r == n / 3 + 2 * n / 5));
        if (make_bad) title = r % 2 ? "name" + title : " " + title.substr(title.find(' ') + 1);
        if (make_bad && from_comment) title = "r" + std::to_string(r) + (r % 2 ? " ch=1 barcode=2" : " truebc=2 barcodes=2");
        t.add(title, (uint32_t)rnd_below(300));
        const bool called = qtsv::called(T, x.bc, x.bc2, x.adapter);
        const std::string bc_text = called ? std::to_string(ids0[x.bc]) + (dual ? "/" + std::to_string(ids1[x.bc2]) : std::string()) : std::string("none");
        want[r] = want_of(title, from_comment, bc_text, called, x.raw, x.den);
        if (x.dropped) { want[r] = Want(); want[r].cls = CLS_DROPPED; want[r].kind = 0; want[r].bucket = 0; want[r].called = false; want[r].score = -1; }
        if ((want[r].cls & CLS_BAD) && first_bad == EVAL_NO_BAD) first_bad = r + 1;
    }
    Plane p(t.bytes);
    // the kernel: workgroups, lanes, rounds; the workgroup's histogram, then the adds
    std::vector<uint8_t> cls(n, 0xEE), kind(n, 0xEE);
    std::vector<uint16_t> bucket(n, 0xEEEE);
    std::vector<uint32_t> hist(EVAL_HIST, 0);
    uint32_t bad = EVAL_NO_BAD;
    const uint32_t blocks = group ? classify_group_blocks(n) : classify_blocks(n);
    const uint32_t lanes = group ? EVAL_GROUP : 1u, per_block = EVAL_THREADS / lanes;
    const auto load16 = [&](uint64_t a) { return p.load16((int64_t)a); };
    for (uint32_t blk = 0; blk < blocks; ++blk) {
        std::vector<uint32_t> s_hist(EVAL_HIST, 0);
        for (uint32_t tid = 0; tid < EVAL_THREADS; ++tid) {
            const uint32_t gl = tid % lanes;
            for (uint64_t r = (uint64_t)blk * per_block + tid / lanes; r < n; r += (uint64_t)blocks * per_block) {
                if (gl == 0 && cls[r] != 0xEE) ++s.bad;                        // one writer per read
                if (recs[r].dropped) { if (gl == 0) { cls[r] = CLS_DROPPED; kind[r] = 0; bucket[r] = 0; } continue; }
                const Verdict v = !group ? read_verdict(T, p.at0(), load16, t.off[r], t.len[r], from_comment, recs[r].bc, recs[r].bc2, recs[r].adapter, recs[r].raw, recs[r].den)
                                         : read_verdict_group(T, p.at0(), load16, [&](uint32_t, uint32_t, uint64_t v0) { return vector_masks(load16, v0, t.off[r] + t.len[r]); },
                                                              gl, t.off[r], t.len[r], from_comment, recs[r].bc, recs[r].bc2, recs[r].adapter, recs[r].raw, recs[r].den);
                if (gl != 0) { if (v.cls != cls[r] || (!(v.cls & CLS_BAD) && (v.kind != kind[r] || v.bucket != bucket[r]))) ++s.bad; continue; }   // (lane 0 ran first)
                cls[r] = v.cls; kind[r] = v.kind; bucket[r] = v.bucket;
                if (v.cls & CLS_BAD) { if (r + 1 < bad) bad = (uint32_t)r + 1; continue; }
                ++s_hist.at(hist_slot(v.kind, v.bucket));
                ++s_hist.at(class_slot(v.cls));
            }
        }
        for (uint32_t i = 0; i < EVAL_HIST; ++i) hist[i] += s_hist[i];
    }
    if (p.stray) ++s.bad;
    if (bad != first_bad) ++s.bad;
    for (uint32_t r = 0; r < n; ++r) {
        if (want[r].cls & CLS_BAD) { ++g_seen_bad[want[r].cls & 7]; continue; }
        ++g_seen_cls[want[r].cls];
        if (want[r].cls != CLS_DROPPED) { ++g_seen_kind[want[r].kind]; ++g_seen_bucket[want[r].bucket]; }
    }
    for (uint32_t r = 0; r < n; ++r)
        if (cls[r] != want[r].cls || (!(cls[r] & CLS_BAD) && (kind[r] != want[r].kind || bucket[r] != want[r].bucket))) { ++s.bad; break; }
    // counts and table by the definitions, read by read
    uint64_t counts[5] = {0, 0, 0, 0, 0};
    for (uint32_t r = 0; r < n; ++r) if (want[r].cls >= CLS_CORRECT && want[r].cls <= CLS_FP) ++counts[want[r].cls];
    for (uint32_t k = CLS_CORRECT; k <= CLS_FP; ++k) if (hist[class_slot(k)] != counts[k]) ++s.bad;
    // the ROC kernel: one pass of suffix sums per kind, then a row per threshold
    std::vector<uint32_t> suf(EVAL_KINDS * (EVAL_BUCKETS + 1), 0xEEEEEEEEu);
    for (uint32_t k = 0; k < EVAL_KINDS; ++k)
        suffix_sums([&](uint32_t i) { return hist.at(i); }, k, [&](uint32_t b, uint32_t v) { suf.at(k * (EVAL_BUCKETS + 1) + b) = v; });
    for (uint32_t q = 0; q < EVAL_Q; ++q) {
        if (n > 1000 && q % 37 && q != EVAL_Q - 1) continue;                  // (the large batch: every 37th threshold and the last)
        int64_t row[EVAL_ROC_COLS], ref[EVAL_ROC_COLS] = {0, 0, 0, 0, 0, 0};
        roc_row([&](uint32_t k, uint32_t b) { return suf.at(k * (EVAL_BUCKETS + 1) + b); }, q, row);
        for (uint32_t r = 0; r < n; ++r) {
            const Want& w = want[r];
            if (w.cls < CLS_CORRECT || w.cls > CLS_FP) continue;
            const bool none = !w.called || w.score < q / 10.0;                // summary(): score < min_score
            ++ref[0];
            if (none) ++ref[w.kind == KIND_TRUTH_NONE ? 3 : 4];
            else ++ref[w.kind == KIND_TRUTH_NONE ? 5 : w.kind == KIND_WHOLE ? 1 : 2];
        }
        if (memcmp(row, ref, sizeof row) != 0) { ++s.bad; break; }
    }
}

int main(int argc, char** argv) {
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    Section tok{"tokenizer"}, mem{"membership"}, buck{"buckets"}, bat{"batches"};
    check_tokenizer(tok);
    check_membership(mem);
    check_buckets(buck);
    for (int group = 0; group < 2; ++group) {
        for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 257u})
            for (int dual = 0; dual < 2; ++dual) {
                check_batch(bat, n, dual != 0, false, -1, 0, group != 0);
                check_batch(bat, n, dual != 0, true, -1, 0, group != 0);
                for (int drop = 0; drop < 4; ++drop) check_batch(bat, n, dual != 0, false, drop, 0, group != 0);
                for (int n_bad = 1; n_bad < 3; ++n_bad) { check_batch(bat, n, dual != 0, false, -1, n_bad, group != 0); check_batch(bat, n, dual != 0, true, -1, n_bad, group != 0); }
            }
        check_batch(bat, 1u + EVAL_MAX_BLOCKS * (group ? EVAL_GROUPS : EVAL_THREADS), false, false, 1, 0, group != 0);      // (a second round)
    }
    // the data did what the section is about: every class, kind and refusal many times, buckets at both ends and many between
    uint64_t buckets = 0;
    for (uint32_t b = 0; b < EVAL_BUCKETS; ++b) buckets += g_seen_bucket[b] != 0;
    for (uint64_t c : g_seen_cls) if (c < 50) ++bat.bad;
    for (uint64_t c : g_seen_kind) if (c < 50) ++bat.bad;
    for (uint32_t w = BAD_NO_TRUEBC; w <= BAD_NO_BARCODE; ++w) if (g_seen_bad[w] < 5) ++bat.bad;
    if (buckets < 40 || !g_seen_bucket[0] || !g_seen_bucket[1] || !g_seen_bucket[EVAL_Q]) ++bat.bad;
    printf("seen: classes %llu %llu %llu %llu %llu, kinds %llu %llu %llu, refusals %llu %llu %llu %llu, %llu buckets\n", (unsigned long long)g_seen_cls[0],
           (unsigned long long)g_seen_cls[1], (unsigned long long)g_seen_cls[2], (unsigned long long)g_seen_cls[3], (unsigned long long)g_seen_cls[4],
           (unsigned long long)g_seen_kind[0], (unsigned long long)g_seen_kind[1], (unsigned long long)g_seen_kind[2], (unsigned long long)g_seen_bad[1],
           (unsigned long long)g_seen_bad[2], (unsigned long long)g_seen_bad[3], (unsigned long long)g_seen_bad[4], (unsigned long long)buckets);
    uint64_t bad = 0;
    for (const Section* s : {&tok, &mem, &buck, &bat}) { report(*s); bad += s->bad; }
    return bad ? 1 : 0;
}

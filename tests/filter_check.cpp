// filter_check.cpp -- --filter-barcodes of the device (qcat_amd/csrc/kernels_filter.inc) on the CPU: the batch loop of the three
// kernels (count by key, floor of the row's maximum, rewrite) run on the host through the very functions the kernels call
// (qcat_amd/csrc/filter_core.h), against a restatement written here on its own: get_valid(counts, 0.05) and filter_barcodes of
// the reference driver over a std::map keyed by the barcodes' IDS (not their slots), `none` counted like a barcode.
// Usage: filter_check <seed>.  Prints "<section>: <n> cases, <m> mismatches" per section; exit status 1 on any mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "filter_core.h"
#include "qcat_hip.h"

namespace {

// a kit as the filter sees it: per template one or two barcode sets, a barcode is an id; the slot of an id is its rank among
// the kit's distinct ids
struct Kit {
    bool dual = false, simple = false;
    std::vector<std::vector<int>> ids[2];          // [set][template][barcode index] -> id
    std::vector<int> distinct;                     // sorted
    uint32_t n_slots() const { return (uint32_t)distinct.size(); }
    uint32_t slot(int t, int s, int i) const {
        return (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), ids[s][(size_t)t][(size_t)i]) - distinct.begin());
    }
};

Kit make_kit(std::mt19937_64& rng, bool dual, bool simple, int n_tpl, int n_ids) {
    Kit k;
    k.dual = dual; k.simple = simple;
    std::vector<int> pool;
    for (int i = 0; i < n_ids; ++i) pool.push_back(1 + 3 * i);                   // (ids are not their own slots)
    for (int s = 0; s < (dual ? 2 : 1); ++s)
        for (int t = 0; t < n_tpl; ++t) {
            std::vector<int> set = pool;
            std::shuffle(set.begin(), set.end(), rng);                           // (the same id at another index in every template)
            set.resize((size_t)std::max(1, n_ids - t));
            k.ids[s].push_back(set);
        }
    k.distinct = pool;
    return k;
}

qcat_result called(int t, int b0, int b1, std::mt19937_64& rng) {
    qcat_result q;
    q.barcode_idx = (int16_t)b0; q.barcode2_idx = (int16_t)b1; q.adapter_idx = (int16_t)t; q.exit_status = 0;
    q.adapter_end = 20 + (int)(rng() % 60); q.trim5p = (int)(rng() % 90); q.trim3p = 400 + (int)(rng() % 90);
    q.raw_score = (int16_t)(50 + rng() % 40); q.score_den = 99;
    return q;
}

qcat_result uncalled(std::mt19937_64& rng) {
    qcat_result q;
    q.barcode_idx = -1; q.barcode2_idx = -1; q.adapter_idx = (int16_t)(rng() % 3 == 0 ? 0 : -1);     // (an adapter without a barcode is no call)
    q.exit_status = (int16_t)(rng() % 2 ? 1 : 1002);
    q.adapter_end = (int)(rng() % 50); q.trim5p = (int)(rng() % 90); q.trim3p = 400 + (int)(rng() % 90);
    q.raw_score = 0; q.score_den = 1;
    return q;
}

bool same(const qcat_result& a, const qcat_result& b) {
    return a.barcode_idx == b.barcode_idx && a.barcode2_idx == b.barcode2_idx && a.adapter_idx == b.adapter_idx &&
           a.exit_status == b.exit_status && a.adapter_end == b.adapter_end && a.trim5p == b.trim5p && a.trim3p == b.trim3p &&
           a.raw_score == b.raw_score && a.score_den == b.score_den;
}

// the device's way: per batch a row of counters indexed by key, the floor of its maximum, the rewrite (filter_core.h)
void run_core(const Kit& k, std::vector<qcat_result>& recs, uint32_t batch_reads) {
    const uint32_t n = (uint32_t)recs.size(), n_bins = qfilt::bins_of(k.dual, k.n_slots());
    const uint32_t per = (batch_reads == 0 || batch_reads > n) ? std::max(n, 1u) : batch_reads;
    auto key = [&](const qcat_result& q) {
        return qfilt::key_of(q, k.dual, k.simple, k.n_slots(), [&](int t, int s, int i) { return k.slot(t, s, i); });
    };
    std::vector<uint32_t> row(n_bins);
    for (uint32_t r0 = 0; r0 < n; r0 += per) {
        const uint32_t r1 = std::min(n, r0 + per);
        std::fill(row.begin(), row.end(), 0u);
        for (uint32_t r = r0; r < r1; ++r) ++row[key(recs[r])];
        const uint32_t floor = (uint32_t)qfilt::floor_of(*std::max_element(row.begin(), row.end()));
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t kv = key(recs[r]);
            if (kv >= n_bins - 1u || qfilt::survives(row[kv], floor)) continue;
            qfilt::make_empty(recs[r]);
        }
    }
}

// the reference's way, restated: counts by barcode id ("0" for no call), valid = count > int(top * 0.05), every called record
// whose id is not valid becomes empty_return_dict() with trims 0
void run_map(const Kit& k, std::vector<qcat_result>& recs, uint32_t batch_reads) {
    const size_t n = recs.size();
    const size_t per = (batch_reads == 0 || batch_reads > n) ? std::max<size_t>(n, 1) : batch_reads;
    typedef std::pair<long, long> Id;
    auto is_called = [&](const qcat_result& q) { return q.barcode_idx >= 0 && (k.simple || q.adapter_idx >= 0); };
    auto id_of = [&](const qcat_result& q) {
        if (!is_called(q)) return Id(-1, -1);
        const size_t t = q.adapter_idx < 0 ? 0 : (size_t)q.adapter_idx;
        return Id(k.ids[0][t][(size_t)q.barcode_idx], k.dual ? k.ids[1][t][(size_t)q.barcode2_idx] : 0);
    };
    for (size_t r0 = 0; r0 < n; r0 += per) {
        const size_t r1 = std::min(n, r0 + per);
        std::map<Id, unsigned long> count;
        for (size_t r = r0; r < r1; ++r) count[id_of(recs[r])] += 1;
        unsigned long top = 0;
        for (std::map<Id, unsigned long>::const_iterator it = count.begin(); it != count.end(); ++it) top = std::max(top, it->second);
        const unsigned long min_count = (unsigned long)((double)top * 0.05);
        for (size_t r = r0; r < r1; ++r) {
            qcat_result& q = recs[r];
            if (!is_called(q) || count[id_of(q)] > min_count) continue;
            q.barcode_idx = -1; q.barcode2_idx = -1; q.adapter_idx = -1; q.adapter_end = 0; q.raw_score = 0; q.score_den = 1;
            q.exit_status = 1; q.trim5p = 0; q.trim3p = 0;
        }
    }
}

int g_failed = 0;
struct Section {
    std::string name; int cases = 0, bad = 0;
    explicit Section(const char* n) : name(n) {}
    void check(bool ok) { ++cases; if (!ok) ++bad; }
    ~Section() { printf("%s: %d cases, %d mismatches\n", name.c_str(), cases, bad); if (bad) g_failed = 1; }
};

// both ways over one input: equal records
bool agree(const Kit& k, const std::vector<qcat_result>& in, uint32_t batch_reads, std::vector<qcat_result>* out = nullptr) {
    std::vector<qcat_result> a = in, b = in;
    run_core(k, a, batch_reads);
    run_map(k, b, batch_reads);
    bool ok = a.size() == b.size();
    for (size_t i = 0; ok && i < a.size(); ++i) ok = same(a[i], b[i]);
    if (out) *out = a;
    return ok;
}

qcat_result random_call(const Kit& k, std::mt19937_64& rng, int hot) {
    // a skewed choice: a few ids hold most reads, the rest are the rare ones the filter is about
    const int t = (int)(rng() % k.ids[0].size());
    auto pick = [&](int s) {
        const int sz = (int)k.ids[s][(size_t)t].size();
        return (int)(rng() % 10 < 7 ? rng() % (uint64_t)std::min(hot, sz) : rng() % (uint64_t)sz);
    };
    const int b0 = pick(0), b1 = k.dual ? pick(1) : -1;
    qcat_result q = called(k.simple ? -1 : t, b0, b1, rng);
    if (k.simple) q.adapter_idx = -1;
    return q;
}

const uint32_t BATCHES[5] = {1, 7, 64, 100, 4000};

void random_section(const char* name, std::mt19937_64& rng, bool dual, bool simple, int none_percent) {
    Section s(name);
    for (int round = 0; round < 4; ++round) {
        const Kit k = make_kit(rng, dual, simple, simple ? 1 : 1 + round % 3, dual ? 12 : 24 + 8 * round);
        for (uint32_t batch : BATCHES) {
            const uint32_t n = 2 * batch + 3 + (uint32_t)(rng() % 5);                       // never a multiple of the batch: a short last one
            std::vector<qcat_result> in;
            for (uint32_t r = 0; r < n; ++r)
                in.push_back((int)(rng() % 100) < none_percent ? uncalled(rng) : random_call(k, rng, 3));
            s.check(agree(k, in, batch));
        }
        std::vector<qcat_result> in;
        for (uint32_t r = 0; r < 501; ++r) in.push_back((int)(rng() % 100) < none_percent ? uncalled(rng) : random_call(k, rng, 3));
        s.check(agree(k, in, 0));                                                           // one batch
        s.check(agree(k, in, 100000));                                                      // a batch longer than the records
    }
}

}  // namespace

int main(int argc, char** argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    random_section("random, single kit", rng, false, false, 10);
    random_section("random, dual kit", rng, true, false, 10);
    random_section("random, simple kit", rng, false, true, 10);
    random_section("the maximum is none", rng, false, false, 85);
    random_section("the maximum is none, dual kit", rng, true, false, 85);
    {
        // strictly greater survives: int(19 * 0.05) = 0, int(20 * 0.05) = 1, 39 -> 1, 40 -> 2, 41 -> 2
        Section s("floor edges");
        const int maxima[5] = {19, 20, 39, 40, 41}, floors[5] = {0, 1, 1, 2, 2};
        Kit k = make_kit(rng, false, false, 2, 24);
        if (k.ids[0][1][2] == k.ids[0][0][5]) std::swap(k.ids[0][1][2], k.ids[0][1][3]);     // (the rival is another id than the maximum)
        for (int with_none = 0; with_none < 2; ++with_none)
            for (int m = 0; m < 5; ++m)
                for (int rival = 1; rival <= 3; ++rival) {
                    s.check(qfilt::floor_of((uint64_t)maxima[m]) == (uint64_t)floors[m]);
                    std::vector<qcat_result> in;
                    for (int i = 0; i < maxima[m]; ++i) in.push_back(with_none ? uncalled(rng) : called(0, 5, -1, rng));     // the maximum: a barcode, or none
                    for (int i = 0; i < rival; ++i) in.push_back(called(1, 2, -1, rng));
                    std::shuffle(in.begin(), in.end(), rng);
                    std::vector<qcat_result> out;
                    bool ok = agree(k, in, 0, &out);
                    int left = 0;
                    for (const qcat_result& q : out) if (q.adapter_idx == 1 && q.barcode_idx == 2) ++left;
                    ok = ok && left == (rival > floors[m] ? rival : 0);
                    for (size_t i = 0; ok && i < in.size(); ++i)                            // the maximum itself and records without a call: untouched
                        if (!(in[i].adapter_idx == 1 && in[i].barcode_idx == 2)) ok = same(in[i], out[i]);
                    s.check(ok);
                }
    }
    {
        Section s("a batch of one read");
        for (int dual = 0; dual < 2; ++dual) {
            const Kit k = make_kit(rng, dual != 0, false, 2, 12);
            std::vector<qcat_result> in;
            for (int i = 0; i < 9; ++i) in.push_back(i % 4 == 3 ? uncalled(rng) : random_call(k, rng, 12));
            std::vector<qcat_result> out;
            bool ok = agree(k, in, 1, &out);
            for (size_t i = 0; ok && i < in.size(); ++i) ok = same(in[i], out[i]);          // max 1, floor 0, 1 > 0: every read survives
            s.check(ok);
        }
    }
    {
        // (a, b) x 40, (a, c) x 2, (a, d) x 3: the first id is shared, the pairs are counted each on its own -- floor 2
        Section s("dual keys that share the first id");
        Kit k = make_kit(rng, true, false, 1, 12);
        for (int swap = 0; swap < 2; ++swap) {
            std::vector<qcat_result> in;
            auto pair = [&](int x, int y) { return swap ? called(0, y, x, rng) : called(0, x, y, rng); };
            for (int i = 0; i < 40; ++i) in.push_back(pair(4, 1));
            for (int i = 0; i < 2; ++i) in.push_back(pair(4, 7));
            for (int i = 0; i < 3; ++i) in.push_back(pair(4, 9));
            std::shuffle(in.begin(), in.end(), rng);
            std::vector<qcat_result> out;
            bool ok = agree(k, in, 0, &out);
            int big = 0, two = 0, three = 0;
            for (const qcat_result& q : out) {
                const int other = swap ? q.barcode_idx : q.barcode2_idx;
                if (q.adapter_idx != 0) continue;
                if (other == 1) ++big; else if (other == 7) ++two; else if (other == 9) ++three;
            }
            s.check(ok && big == 40 && two == 0 && three == 3);
        }
    }
    return g_failed;
}

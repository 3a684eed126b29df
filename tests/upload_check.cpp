// upload_check.cpp -- the device-free part of a host-buffer call's upload (qcat_amd/csrc/upload_core.h, used by
// batch_upload_windows of batch_host.inc) against a naive restatement: what is staged of a read, the length pass in both input
// forms with its three refusals, the slice bounds, and the two schedules that spread the compaction over host threads.  The
// sliced schedule runs with a sender that copies [o0, o1) from the staging into a second buffer AT THE MOMENT it is called: that
// buffer must end up as the expected compaction and the ranges must tile [0, total) in ascending order -- a slice handed over
// before its worker finished shows as wrong bytes here and as a data race under the thread sanitizer.  Slices are scaled down
// to a few hundred bytes so that thousands of them run in well under a second.
// Built three times by tests/test_upload_host.py: plain, -fsanitize=address,undefined, -fsanitize=thread.
//   usage: upload_check <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <system_error>
#include <utility>
#include <vector>

#include "upload_core.h"
#include "check_common.h"

using namespace qupload;

static bool differs(const uint8_t* a, const uint8_t* b, uint64_t n) { return n && memcmp(a, b, (size_t)n) != 0; }      // (n = 0: the pointers may be null)

// a batch in both input forms: the concatenated bases with their offsets, and a copy of every read in an allocation of its own
// (exactly its length, so that a byte read past a read's end is the address sanitizer's; an empty read has a null pointer)
struct Batch {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets, lens;
    std::vector<std::vector<uint8_t>> own;
    std::vector<const uint8_t*> ptrs;
    explicit Batch(const std::vector<uint64_t>& lengths) {
        offsets.push_back(0);
        for (uint64_t len : lengths) {
            std::vector<uint8_t> r((size_t)len);
            for (auto& x : r) x = (uint8_t)rnd();
            bases.insert(bases.end(), r.begin(), r.end());
            offsets.push_back(bases.size());
            lens.push_back(len);
            own.push_back(std::move(r));
        }
        for (auto& r : own) ptrs.push_back(r.empty() ? nullptr : r.data());
    }
    uint32_t n() const { return (uint32_t)lens.size(); }
    Reads form(bool pointers) const {
        return pointers ? Reads{nullptr, nullptr, ptrs.data(), lens.data(), n()} : Reads{bases.data(), offsets.data(), nullptr, nullptr, n()};
    }
};

// the naive restatement: read by read, byte by byte
struct Expected { std::vector<uint8_t> staged; std::vector<uint64_t> off; std::vector<uint32_t> len; };
static Expected expect(const Batch& b, uint64_t n, bool both, bool whole) {
    Expected e;
    e.off.push_back(0);
    for (uint32_t r = 0; r < b.n(); ++r) {
        const std::vector<uint8_t>& s = b.own[r];
        const uint64_t len = s.size();
        e.len.push_back((uint32_t)len);
        if (whole || len <= (both ? 2 * n : n)) for (uint64_t i = 0; i < len; ++i) e.staged.push_back(s[i]);
        else {
            for (uint64_t i = 0; i < n; ++i) e.staged.push_back(s[i]);
            if (both) for (uint64_t i = len - n; i < len; ++i) e.staged.push_back(s[i]);
        }
        e.off.push_back(e.staged.size());
    }
    return e;
}

static std::vector<uint64_t> ragged(uint64_t n) { return {0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1, 3 * n}; }

// thread factories for the schedules: the first `limit` threads start, the next one fails like std::thread does
struct LimitedSpawn {
    unsigned limit;
    unsigned* started;
    template <class F> void operator()(std::vector<std::thread>& pool, F fn) const {
        if (*started >= limit) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
        pool.emplace_back(fn);
        ++*started;
    }
};

// length pass + compaction of one batch in one form, single-threaded and on the even split with 1, 2, 3 and 8 threads
static uint64_t run_staging(const Batch& b, bool pointers, uint64_t n, bool both, bool whole) {
    const Expected e = expect(b, n, both, whole);
    const Reads in = b.form(pointers);
    const Keep k = keep_of(n, both, whole);
    std::vector<uint32_t> len(b.n() + 1, 0xDDDDDDDDu);
    std::vector<uint64_t> off(b.n() + 1, ~0ull);
    uint64_t total = ~0ull, bad = 0;
    if (length_pass(in, k, len.data(), off.data(), &total) != OK) return 1;
    if (total != e.staged.size() || off != e.off) ++bad;
    if (len[b.n()] != 0xDDDDDDDDu || !std::equal(e.len.begin(), e.len.end(), len.begin())) ++bad;
    if (bad) return bad;
    for (unsigned threads : {0u, 1u, 2u, 3u, 8u}) {
        std::vector<uint8_t> staging((size_t)total + 1, 0xEE);                 // (one byte behind the end: it must stay)
        auto work = [&](uint32_t r0, uint32_t r1) { compact(in, k, off.data(), staging.data(), r0, r1); };
        if (!threads) work(0, b.n());
        else run_even(b.n(), threads, work);
        if (staging[(size_t)total] != 0xEE || differs(staging.data(), e.staged.data(), total)) ++bad;
    }
    return bad;
}

static void staging_section(Section& s) {
    for (uint64_t n : {150ull, 4ull})
        for (int order = 0; order < 4; ++order) {
            std::vector<uint64_t> lengths = ragged(n);
            if (order == 1) std::reverse(lengths.begin(), lengths.end());
            if (order >= 2) {                                   // every length three times, shuffled, among reads of random lengths
                std::vector<uint64_t> more;
                for (int rep = 0; rep < 3; ++rep) for (uint64_t len : lengths) { more.push_back(len); more.push_back(rnd_below(4 * n)); }
                for (size_t i = more.size(); i > 1; --i) std::swap(more[i - 1], more[(size_t)rnd_below(i)]);
                lengths = more;
            }
            const Batch b(lengths);
            for (int pointers = 0; pointers < 2; ++pointers)
                for (int both = 0; both < 2; ++both)
                    for (int whole = 0; whole < 2; ++whole) { ++s.cases; s.bad += run_staging(b, pointers != 0, n, both != 0, whole != 0) ? 1 : 0; }
        }
    // no reads at all, and reads that are all empty (the concatenated form may then come without bases)
    for (uint32_t count : {0u, 5u}) {
        const Batch b(std::vector<uint64_t>(count, 0));
        for (int pointers = 0; pointers < 2; ++pointers) { ++s.cases; s.bad += run_staging(b, pointers != 0, 150, true, false) ? 1 : 0; }
        Reads in{nullptr, b.offsets.data(), nullptr, nullptr, count};
        std::vector<uint32_t> len(count + 1);
        std::vector<uint64_t> off(count + 1, ~0ull);
        uint64_t total = ~0ull;
        std::vector<uint8_t> staging(512, 0xEE);                 // (nothing may be written; room for a read, which keeps the compiler's
                                                                 //  bounds warnings quiet about the branches that are not taken)
        ++s.cases;
        if (length_pass(in, keep_of(150, true, false), len.data(), off.data(), &total) != OK || total != 0) ++s.bad;
        else {
            compact(in, keep_of(150, true, false), off.data(), staging.data(), 0, count);
            if (staging != std::vector<uint8_t>(512, 0xEE)) ++s.bad;
        }
    }
}

// the three refusals, each at the first, a middle and the last read: the code, and nothing written for the refused read or behind it
static void refusal_section(Section& s) {
    const std::vector<uint64_t> lengths = {7, 0, 300, 12, 150, 1, 0, 301, 40};
    const Batch b(lengths);
    const Keep k = keep_of(150, true, false);
    const Expected e = expect(b, 150, true, false);
    const uint32_t n = b.n();
    auto check = [&](const Reads& in, uint32_t at, Refusal want) {
        std::vector<uint32_t> len(n + 1, 0xDDDDDDDDu);
        std::vector<uint64_t> off(n + 1, ~0ull);
        uint64_t total = 0x1234;
        ++s.cases;
        bool good = length_pass(in, k, len.data(), off.data(), &total) == want && total == 0x1234;
        for (uint32_t r = 0; r < n; ++r) good = good && len[r] == (r < at ? e.len[r] : 0xDDDDDDDDu);
        for (uint32_t r = 0; r <= n; ++r) good = good && off[r] == (r <= at ? e.off[r] : ~0ull);
        if (!good) ++s.bad;
    };
    for (uint32_t at : {0u, 4u, n - 1}) {
        // a null pointer with a length (the reads at these places are not empty)
        std::vector<const uint8_t*> ptrs = b.ptrs;
        ptrs[at] = nullptr;
        check(Reads{nullptr, nullptr, ptrs.data(), b.lens.data(), n}, at, NULL_READ);
        // a read longer than 4 Gb, in both forms (the pass looks at no base: a length alone is enough)
        std::vector<uint64_t> lens = b.lens;
        lens[at] = 0x100000000ull;
        check(Reads{nullptr, nullptr, b.ptrs.data(), lens.data(), n}, at, TOO_LONG);
        std::vector<uint64_t> offsets = b.offsets;
        for (uint32_t r = at + 1; r <= n; ++r) offsets[r] += 0x100000000ull;
        check(Reads{b.bases.data(), offsets.data(), nullptr, nullptr, n}, at, TOO_LONG);
        // decreasing offsets
        offsets = b.offsets;
        if (at == 0) { offsets[0] = 5; offsets[1] = 4; }
        else offsets[at + 1] = offsets[at] - 1;
        check(Reads{b.bases.data(), offsets.data(), nullptr, nullptr, n}, at, DECREASING);
    }
    // a null pointer WITHOUT a length and a read of exactly 4 Gb - 1 are accepted (the second by its length alone)
    {
        std::vector<uint64_t> lens = {0, 0xFFFFFFFFull, 3};
        const uint8_t some[3] = {1, 2, 3};
        const uint8_t* ptrs[3] = {nullptr, some, some};
        std::vector<uint32_t> len(3);
        std::vector<uint64_t> off(4);
        uint64_t total = 0;
        ++s.cases;
        if (length_pass(Reads{nullptr, nullptr, ptrs, lens.data(), 3}, k, len.data(), off.data(), &total) != OK || total != 303 ||
            len[1] != 0xFFFFFFFFu || off[1] != 0 || off[2] != 300 || off[3] != 303) ++s.bad;
    }
}

// slice bounds against a linear restatement, and their properties
static uint64_t check_bounds(const std::vector<uint64_t>& off, uint64_t slice_bytes, const std::vector<uint32_t>& bound) {
    const uint32_t n = (uint32_t)off.size() - 1;
    const uint64_t total = off[n];
    std::vector<uint32_t> want;
    want.push_back(0);
    for (uint64_t at = slice_bytes; at < total; at += slice_bytes) {
        uint32_t r = 0;
        while (r < n && off[r] < at) ++r;
        if (r > want.back() && r < n) want.push_back(r);
    }
    want.push_back(n);
    uint64_t bad = bound != want ? 1 : 0;
    for (size_t j = 0; j + 1 < bound.size(); ++j) if (bound[j] >= bound[j + 1] && !(n == 0 && bound.size() == 2)) ++bad;
    return bad;
}

// one run of the sliced schedule; `limit`: threads that start before the factory fails (~0u: all of them)
static uint64_t run_sliced_case(const Batch& b, bool pointers, uint64_t n, bool both, bool whole, uint64_t slice_bytes, unsigned threads,
                                unsigned limit, uint64_t* n_slices) {
    const Expected e = expect(b, n, both, whole);
    const Reads in = b.form(pointers);
    const Keep k = keep_of(n, both, whole);
    std::vector<uint32_t> len(b.n() + 1);
    std::vector<uint64_t> off(b.n() + 1);
    uint64_t total = 0, bad = 0;
    if (length_pass(in, k, len.data(), off.data(), &total) != OK || total != e.staged.size()) return 1;
    const std::vector<uint32_t> bound = slice_bounds(off.data(), b.n(), total, slice_bytes);
    bad += check_bounds(off, slice_bytes, bound);
    *n_slices += bound.size() - 1;
    std::vector<uint8_t> staging((size_t)total + 1, 0xEE), arrived((size_t)total + 1, 0x77);
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    auto work = [&](uint32_t r0, uint32_t r1) { compact(in, k, off.data(), staging.data(), r0, r1); };
    auto send = [&](uint64_t o0, uint64_t o1) {
        if (o1 > total || o0 >= o1) { ++bad; return false; }
        memcpy(arrived.data() + o0, staging.data() + o0, (size_t)(o1 - o0));     // now, not at the end
        ranges.emplace_back(o0, o1);
        return true;
    };
    unsigned started = 0;
    const bool ok = limit == ~0u ? run_sliced(bound, off.data(), threads, work, send)
                                 : run_sliced(bound, off.data(), threads, work, send, LimitedSpawn{limit, &started});
    if (!ok) ++bad;
    if (limit != ~0u && started != std::min(limit, threads)) ++bad;
    uint64_t at = 0;
    for (auto& r : ranges) { if (r.first != at) ++bad; at = r.second; }      // ascending, no gap, no overlap
    if (at != total) ++bad;
    if (arrived[(size_t)total] != 0x77 || differs(arrived.data(), e.staged.data(), total)) ++bad;
    if (staging[(size_t)total] != 0xEE || differs(staging.data(), e.staged.data(), total)) ++bad;
    return bad;
}

static void sliced_section(Section& s, Section& fallback, uint64_t* n_slices) {
    const uint64_t slice_bytes = 256;
    struct Shape { const char* what; std::vector<uint64_t> lengths; };
    std::vector<Shape> shapes;
    {   // whole reads around 1000 bases: most slices hold no read start, every read is longer than a slice
        Shape a{"reads longer than a slice", {}};
        for (int i = 0; i < 300; ++i) a.lengths.push_back(700 + rnd_below(700));
        shapes.push_back(a);
        // reads that end exactly on slice bounds with runs of empty reads there, and empty reads at both ends of the batch
        Shape e{"empty reads at slice bounds", {0, 0}};
        for (int i = 0; i < 900; ++i) {
            e.lengths.push_back(i % 3 == 0 ? 256 : (i % 3 == 1 ? 100 : 156));
            if (i % 3 != 1) for (uint64_t z = rnd_below(4); z > 0; --z) e.lengths.push_back(0);
        }
        e.lengths.push_back(0); e.lengths.push_back(0);
        shapes.push_back(e);
        // the ragged lengths around n = 150 many times over (head and tail of the long ones)
        Shape r{"ragged", {}};
        for (int i = 0; i < 100; ++i) for (uint64_t len : ragged(150)) r.lengths.push_back(len);
        shapes.push_back(r);
        // one read far longer than everything else, short reads around it
        Shape o{"one long read", {}};
        for (int i = 0; i < 40; ++i) o.lengths.push_back(rnd_below(60));
        o.lengths.push_back(200000);
        for (int i = 0; i < 40; ++i) o.lengths.push_back(rnd_below(60));
        shapes.push_back(o);
    }
    for (const Shape& sh : shapes) {
        const Batch b(sh.lengths);
        for (int pointers = 0; pointers < 2; ++pointers)
            for (int mode = 0; mode < 3; ++mode)                // whole reads; both ends; 5' only
                for (unsigned threads : {1u, 2u, 3u, 8u}) {
                    ++s.cases;
                    s.bad += run_sliced_case(b, pointers != 0, 150, mode == 1, mode == 0, slice_bytes, threads, ~0u, n_slices) ? 1 : 0;
                }
        // no thread at all (the calling thread does all the work, then sends), and a factory that fails after the first or second
        for (unsigned limit : {0u, 1u, 2u}) {
            ++fallback.cases;
            fallback.bad += run_sliced_case(b, limit == 1, 150, false, true, slice_bytes, 8, limit, n_slices) ? 1 : 0;
        }
    }
    // a sender that stops: the schedule returns false, nothing is sent after the refusal, the workers still finish
    {
        std::vector<uint64_t> lengths(400, 1000);
        const Batch b(lengths);
        const Reads in = b.form(false);
        const Keep k = keep_of(150, true, true);
        std::vector<uint64_t> off(b.n() + 1);
        uint64_t total = 0;
        (void)length_pass(in, k, nullptr, off.data(), &total);
        std::vector<uint8_t> staging((size_t)total, 0xEE);
        const std::vector<uint32_t> bound = slice_bounds(off.data(), b.n(), total, slice_bytes);
        int calls = 0;
        auto work = [&](uint32_t r0, uint32_t r1) { compact(in, k, off.data(), staging.data(), r0, r1); };
        const bool ok = run_sliced(bound, off.data(), 3, work, [&](uint64_t, uint64_t) { ++calls; return false; });
        ++s.cases;
        if (ok || calls != 1 || differs(staging.data(), b.bases.data(), total)) ++s.bad;
    }
}

// the even split when threads cannot be started: the calling thread takes the shares nobody got
static void even_fallback_section(Section& s) {
    std::vector<uint64_t> lengths;
    for (int i = 0; i < 1001; ++i) lengths.push_back(rnd_below(700));
    const Batch b(lengths);
    const Expected e = expect(b, 150, true, false);
    const Reads in = b.form(true);
    const Keep k = keep_of(150, true, false);
    std::vector<uint32_t> len(b.n());
    std::vector<uint64_t> off(b.n() + 1);
    uint64_t total = 0;
    (void)length_pass(in, k, len.data(), off.data(), &total);
    for (unsigned threads : {2u, 3u, 8u, 2000u})
        for (unsigned limit : {0u, 1u, 5u}) {
            std::vector<uint8_t> staging((size_t)total + 1, 0xEE);
            unsigned started = 0;
            run_even(b.n(), threads, [&](uint32_t r0, uint32_t r1) { compact(in, k, off.data(), staging.data(), r0, r1); }, LimitedSpawn{limit, &started});
            ++s.cases;
            if (started > limit || staging[(size_t)total] != 0xEE || total != e.staged.size() || differs(staging.data(), e.staged.data(), total)) ++s.bad;
        }
}

int main(int argc, char** argv) {
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    Section staging{"staged bytes, offsets and lengths"}, refusals{"refusals"}, sliced{"sliced schedule"},
            fallback{"sliced schedule without threads"}, even{"even split without threads"};
    uint64_t n_slices = 0;
    staging_section(staging);
    refusal_section(refusals);
    sliced_section(sliced, fallback, &n_slices);
    even_fallback_section(even);
    uint64_t bad = 0;
    for (const Section* s : {&staging, &refusals, &sliced, &fallback, &even}) { report(*s); bad += s->bad; }
    printf("slices run: %llu\n", (unsigned long long)n_slices);
    return bad ? 1 : 0;
}

// upload_core.h -- the host side of a host-buffer call's upload (batch_host.inc: batch_upload_windows) that needs no device, on
// the standard library alone: what is kept of a read, the length pass with its refusals, the slices of a big staging and the
// two ways the compaction is spread over host threads.  tests/upload_check.cpp runs all of it against a naive restatement,
// the sliced schedule with a sender that copies each range at the moment it is handed over, also under the thread sanitizer.
//
// Vocabulary.  A read of `len` bases is STAGED whole when len <= keep, else as its first n bases and -- both ends scanned --
// its last n behind them (keep = 2n or n; whole reads: keep = ~0).  off[0..n_reads] are the staged reads' byte offsets in the
// staging (off[n_reads] = total); a SLICE is a run of consecutive reads of about slice_bytes staged bytes.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <exception>
#include <memory>
#include <thread>
#include <vector>

namespace qupload {

// the reads of a host batch: concatenated (bases + offsets[n + 1]), or one pointer and one length per read (ptrs non-null)
struct Reads {
    const uint8_t* bases;
    const uint64_t* offsets;
    const uint8_t* const* ptrs;
    const uint64_t* lens;
    uint32_t n;
    const uint8_t* src(uint32_t r) const { return ptrs ? ptrs[r] : bases + offsets[r]; }
    uint64_t len(uint32_t r) const { return ptrs ? lens[r] : offsets[r + 1] - offsets[r]; }
};

struct Keep {
    uint64_t n;                                    // bases of one scanned end
    bool both;                                     // both ends are scanned
    uint64_t keep;                                 // staged bytes of a read at most
};
static inline Keep keep_of(uint64_t n, bool both, bool whole) { return Keep{n, both, whole ? ~0ull : (both ? 2 * n : n)}; }

// the copy of one read: whole when len <= keep, else head, plus tail when both ends are scanned
static inline void copy_read(uint8_t* dst, const uint8_t* src, uint64_t len, const Keep& k) {
    if (len <= k.keep) { if (len) memcpy(dst, src, (size_t)len); return; }
    memcpy(dst, src, (size_t)k.n);
    if (k.both) memcpy(dst + k.n, src + len - k.n, (size_t)k.n);
}

// reads [r0, r1) into the staging
static inline void compact(const Reads& in, const Keep& k, const uint64_t* off, uint8_t* staging, uint32_t r0, uint32_t r1) {
    for (uint32_t r = r0; r < r1; ++r) copy_read(staging + off[r], in.src(r), in.len(r), k);
}

enum Refusal { OK = 0, NULL_READ = 1, DECREASING = 2, TOO_LONG = 3 };

// The length pass: len_out[r] (null: not wanted) the real lengths, off_out[0 .. n] the staged offsets, *total their end.  The
// first read that is refused ends the pass: nothing behind it has been looked at, nothing for it or behind it is written.
static inline Refusal length_pass(const Reads& in, const Keep& k, uint32_t* len_out, uint64_t* off_out, uint64_t* total) {
    uint64_t sum = 0;
    off_out[0] = 0;
    for (uint32_t r = 0; r < in.n; ++r) {
        if (!in.ptrs && in.offsets[r + 1] < in.offsets[r]) return DECREASING;
        const uint64_t len = in.len(r);
        if (in.ptrs && len && !in.ptrs[r]) return NULL_READ;
        if (len > 0xFFFFFFFFull) return TOO_LONG;
        if (len_out) len_out[r] = (uint32_t)len;
        sum += len <= k.keep ? len : k.keep;
        off_out[r + 1] = sum;
    }
    *total = sum;
    return OK;
}

// slice j = reads [bound[j], bound[j + 1]): a cut at the first read that starts at or behind every multiple of slice_bytes (a
// read is never split, so a read longer than a slice makes a longer slice; no slice is without reads)
static inline std::vector<uint32_t> slice_bounds(const uint64_t* off, uint32_t n_reads, uint64_t total, uint64_t slice_bytes) {
    std::vector<uint32_t> bound;
    bound.push_back(0);
    for (uint64_t at = slice_bytes; at < total; at += slice_bytes) {
        const uint32_t r = (uint32_t)(std::lower_bound(off, off + n_reads, at) - off);
        if (r > bound.back() && r < n_reads) bound.push_back(r);
    }
    bound.push_back(n_reads);
    return bound;
}

// how a schedule starts a thread: spawn(pool, fn) appends one to the pool or throws (std::system_error: no more threads)
struct StdSpawn {
    template <class F> void operator()(std::vector<std::thread>& pool, F fn) const { pool.emplace_back(fn); }
};

// The even split: work(r0, r1) over n_reads reads in nthreads equal shares, the first of them on the calling thread; shares
// no thread could be started for run on the calling thread as well.
template <class Work, class Spawn = StdSpawn>
static inline void run_even(uint32_t n_reads, unsigned nthreads, Work work, Spawn spawn = Spawn()) {
    std::vector<std::thread> pool;
    const uint32_t per = (n_reads + nthreads - 1) / nthreads;
    uint32_t done_to = std::min<uint32_t>(n_reads, per);          // [0, per) is this thread's share
    for (unsigned t = 1; t < nthreads; ++t) {
        const uint32_t r0 = std::min<uint32_t>(n_reads, t * per), r1 = std::min<uint32_t>(n_reads, r0 + per);
        if (r0 >= r1) break;
        try { spawn(pool, [=] { work(r0, r1); }); }
        catch (const std::exception&) { break; }                 // no more threads: the rest runs here
        done_to = r1;
    }
    work(0, std::min<uint32_t>(n_reads, per));
    if (done_to < n_reads) work(done_to, n_reads);
    for (auto& th : pool) th.join();
}

// The sliced schedule: nthreads workers draw slices from a counter, work(r0, r1) each, and set done[j] with release.  The
// calling thread waits for slice j (acquire), extends the run while the slices behind it are done as well, and hands each run
// over once as send(o0, o1), the staged byte range -- in ascending order, every staged byte exactly once; a run of empty reads
// is not sent.  send returns false to stop (the workers still finish).  Without a single worker thread the calling thread does
// all the work first.  Returns false when a send stopped the hand-over.
template <class Work, class Send, class Spawn = StdSpawn>
static inline bool run_sliced(const std::vector<uint32_t>& bound, const uint64_t* off, unsigned nthreads, Work work, Send send,
                              Spawn spawn = Spawn()) {
    const size_t n_slices = bound.size() - 1;
    std::unique_ptr<std::atomic<uint8_t>[]> done(new std::atomic<uint8_t>[n_slices]);
    for (size_t j = 0; j < n_slices; ++j) done[j].store(0, std::memory_order_relaxed);
    std::atomic<size_t> next{0};
    auto drain = [&] {
        for (;;) {
            const size_t j = next.fetch_add(1);
            if (j >= n_slices) break;
            work(bound[j], bound[j + 1]);
            done[j].store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthreads; ++t) {
        try { spawn(pool, drain); }
        catch (const std::exception&) { break; }
    }
    if (pool.empty()) drain();
    bool ok = true;
    for (size_t j = 0; j < n_slices && ok; ) {
        while (!done[j].load(std::memory_order_acquire)) std::this_thread::yield();
        size_t k = j + 1;
        while (k < n_slices && done[k].load(std::memory_order_acquire)) ++k;
        const uint64_t o0 = off[bound[j]], o1 = off[bound[k]];
        if (o1 > o0) ok = send(o0, o1);
        j = k;
    }
    for (auto& th : pool) th.join();
    return ok;
}

}  // namespace qupload

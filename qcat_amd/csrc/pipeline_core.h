// pipeline_core.h -- the host side of the chunked host-buffer scan (pipeline_host.inc: scan_batch_pipelined) that needs no
// device, on the standard library and upload_core.h alone: the persistent worker pool, the choice of the chunk size and the
// cuts, the rule the two stage slots are sized by, and what the pool does per chunk -- the length sums of the parts with their
// refusals, the exclusive scan over the parts, the compaction of a part into the pinned staging with its software prefetch --
// and the split of a slot's records over the pool.  tests/pipeline_check.cpp runs all of it against a naive restatement, also
// under the address, undefined-behaviour and thread sanitizers.
//
// Vocabulary (upload_core.h): a read of `len` bases is STAGED whole when len <= keep, else as its first n bases and -- both
// ends scanned -- its last n behind them.  A CHUNK is reads [r0, r0 + nr) of the call; its host work is cut into PARTS of
// consecutive reads, one task of the pool each.  A reads accessor `in` answers src(r), len(r) and decreasing(r) for the
// absolute read r of the call (pipeline.h: ReadView; qupload::Reads has the first two).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <ctime>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "upload_core.h"

namespace qk {

// CPU nanoseconds the pools' parts have taken in this process (compaction of the scanned windows into the staging buffers;
// PIPELINE_TRACE prints it beside the file loop's other stages)
static std::atomic<uint64_t> g_host_pool_cpu_ns{0};
static inline uint64_t host_thread_cpu_ns() {
    struct timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec : 0;
}

// persistent pool: run(n, fn) executes fn(part) for part = 0..n-1 on the workers + the caller
class HostPool {
public:
    explicit HostPool(unsigned workers) {
        for (unsigned i = 0; i < workers; ++i) {
            try { threads_.emplace_back([this] { loop(); }); }
            catch (const std::exception&) { break; }               // fewer threads: the caller takes the rest
        }
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; ++gen_; }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    unsigned size() const { return (unsigned)threads_.size() + 1; }
    void run(int parts, const std::function<void(int)>& fn) {
        if (parts <= 0) return;
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn; parts_ = parts; next_ = 0; left_ = parts; ++gen_;
        }
        cv_.notify_all();
        work();                                                    // the caller works too
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return left_ == 0; });
        fn_ = nullptr;
    }

private:
    void work() {
        for (;;) {
            int p;
            const std::function<void(int)>* fn;
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (!fn_ || next_ >= parts_) return;
                p = next_++; fn = fn_;
            }
            const uint64_t c0 = host_thread_cpu_ns();
            (*fn)(p);
            g_host_pool_cpu_ns.fetch_add(host_thread_cpu_ns() - c0, std::memory_order_relaxed);
            std::lock_guard<std::mutex> lk(mu_);
            if (--left_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
            }
            work();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    int parts_ = 0, next_ = 0, left_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

}  // namespace qk

namespace qpipe {

// ---- the plan of a call: chunk size, cuts ---------------------------------------------------------------------------------------
// chunks of 256 k .. 1 M reads (a quarter of the batch): big enough to fill the chip (1 000+ tiles of 128
// alignments), small enough that the first chunk's compaction and the last chunk's scan -- the only
// stages nothing overlaps -- are a small part of the call
// (heavier per-chunk launches lose less to the tails of the persistent barcode kernels: large batches take 1 M-read chunks)
// (a chunk costs ~0.3 ms of host time in launches and copies whatever its size: 1 M reads of a small kit run
// 166 M reads/s in four chunks, 137 M in eight, 97 M in sixteen)
// (reads of a FASTQ mapping: a one-shot process pays for every pinned byte it sets up, 0.2 ms per MiB, and the host side
// bounds the rate anyway -- 256 k-read chunks)
// forced: the option PIPELINE_CHUNK is set, to forced_reads -- 4096 reads at least
static inline uint32_t chunk_reads(uint32_t n_reads, bool fastq_form, bool forced, int forced_reads) {
    if (forced) return (uint32_t)std::max(4096, forced_reads);
    return fastq_form ? 262144u : std::min<uint32_t>(1048576u, std::max<uint32_t>(262144u, n_reads / 4u));
}

// chunk q = reads [cuts[q], cuts[q + 1]).  The first and the last chunk are a third of the others -- nothing overlaps the
// first chunk's compaction and the last chunk's upload + scan + download; a forced chunk size cuts at its multiples
static inline std::vector<uint32_t> chunk_cuts(uint32_t n_reads, uint32_t chunk, bool forced) {
    std::vector<uint32_t> cuts;
    cuts.push_back(0);
    if (!forced && n_reads > 2 * chunk) {
        const uint32_t edge = chunk / 3, mid = n_reads - 2 * edge, m = (uint32_t)(((uint64_t)mid + chunk - 1) / chunk);   // (64 bits, as below)
        for (uint32_t q = 0; q <= m; ++q) cuts.push_back(edge + (uint32_t)((uint64_t)mid * q / m));    // equal middle chunks
    } else {
        for (uint64_t pos = chunk; pos < n_reads; pos += chunk) cuts.push_back((uint32_t)pos);        // (64 bits: n_reads near 2^32)
    }
    cuts.push_back(n_reads);
    return cuts;
}

static inline uint32_t largest_chunk(const std::vector<uint32_t>& cuts) {
    uint32_t largest = 0;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) largest = std::max(largest, cuts[q + 1] - cuts[q]);
    return largest;
}

// ---- the size of a stage slot -----------------------------------------------------------------------------------------------
// Staging for the LARGEST chunk of this call: `largest` + 1 offsets and `largest` x keep bases + slack.  A slot that is in use
// (capacity > 0) and too small grows with headroom, need x 1.5, capped at what a chunk of `chunk` reads can ask for; a first
// use (capacity 0, also after an allocation that failed) gets the exact need, and a slot that is big enough is left alone.
struct StageNeed { size_t reads, bases; };
static inline StageNeed stage_need(uint32_t largest, uint32_t chunk, uint64_t keep, size_t slack, size_t cap_reads, size_t cap_bases) {
    size_t need_reads = (size_t)largest + 1, need_bases = (size_t)largest * keep + slack;
    if (need_reads > cap_reads && cap_reads) need_reads = std::min<size_t>((size_t)chunk + 1, need_reads + need_reads / 2);
    if (need_bases > cap_bases && cap_bases) need_bases = std::min<size_t>((size_t)chunk * keep + slack, need_bases + need_bases / 2);
    return StageNeed{need_reads, need_bases};
}

// ---- a range over the pool --------------------------------------------------------------------------------------------------
// n items in `parts` runs of `per` (the last ones shorter or empty): max_parts at most, and no more than one per `grain` items
struct Split {
    int parts;
    uint32_t per;
    uint32_t n;
    uint32_t begin(int part) const { return (uint32_t)std::min<uint64_t>(n, (uint64_t)part * per); }
    uint32_t end(int part) const { return (uint32_t)std::min<uint64_t>(n, (uint64_t)begin(part) + per); }
};
static inline Split split_over(uint32_t n, uint32_t max_parts, uint32_t grain) {
    const int parts = (int)std::min<uint32_t>(max_parts, std::max<uint32_t>(1u, n / grain));
    return Split{parts, (n + parts - 1) / parts, n};
}
constexpr int MAX_PARTS = 256;
// the parts of a chunk's host work: four per thread of the pool, of 4096 reads at least
static inline Split chunk_parts(uint32_t nr, unsigned pool_size) { return split_over(nr, std::min<uint32_t>(pool_size * 4, (uint32_t)MAX_PARTS), 4096u); }
// ... of a slot's records on their way to the caller's array: one per thread, of 65536 records at least
static inline Split record_parts(uint32_t cnt, unsigned pool_size) { return split_over(cnt, pool_size, 65536u); }

// ---- lengths ----------------------------------------------------------------------------------------------------------------
// the staged bytes of reads [r0 + a, r0 + b), up to the first read that is refused
struct PartSum { uint64_t bytes; qupload::Refusal refused; };
template <class Reads>
static inline PartSum part_lengths(const Reads& in, uint32_t r0, uint32_t a, uint32_t b, uint64_t keep) {
    uint64_t sum = 0;
    for (uint32_t r = a; r < b; ++r) {
        if (in.decreasing(r0 + r)) return PartSum{sum, qupload::DECREASING};
        const uint64_t len = in.len(r0 + r);
        if (len > 0xFFFFFFFFull) return PartSum{sum, qupload::TOO_LONG};
        sum += len <= keep ? len : keep;
    }
    return PartSum{sum, qupload::OK};
}

// the exclusive scan over the parts: ps[q].bytes becomes the staged offset of part q's first read, *total the chunk's staged
// bytes.  Returns the refusal of the first refused read in read order (the parts are in read order, and each stopped at its
// first), as qupload::length_pass does.
static inline qupload::Refusal scan_parts(PartSum* ps, int parts, uint64_t* total) {
    qupload::Refusal refused = qupload::OK;
    uint64_t sum = 0;
    for (int q = 0; q < parts; ++q) {
        if (refused == qupload::OK) refused = ps[q].refused;
        const uint64_t t = ps[q].bytes; ps[q].bytes = sum; sum += t;
    }
    *total = sum;
    return refused;
}

// offsets + real lengths of the compacted chunk, first half: per-part sums in parallel, a serial scan over the parts
template <class Reads>
static inline qupload::Refusal stage_lengths(qk::HostPool& pool, const Reads& in, uint32_t r0, const Split& s, uint64_t keep,
                                             PartSum* ps, uint64_t* total) {
    pool.run(s.parts, [&](int part) { ps[part] = part_lengths(in, r0, s.begin(part), s.end(part), keep); });
    return scan_parts(ps, s.parts, total);
}

// ---- compaction -------------------------------------------------------------------------------------------------------------
// reads [r0 + a, r0 + b) of a chunk into its staging from byte `pos` on; off[r + 1] and len_out[r] are indexed by the read's
// place in the chunk
template <class Reads>
static inline void compact_part(const Reads& in_, uint32_t r0, uint32_t a, uint32_t b, uint64_t pos, const qupload::Keep& k_,
                                uint8_t* staging, uint64_t* off, uint32_t* len_out) {
    const Reads in = in_;                                    // (copies: the byte stores below may alias anything behind a reference,
    const qupload::Keep k = k_;                              //  and the loop would load both again for every read)
    constexpr uint32_t AHEAD = 12;                           // reads: the windows are 150 B out of every ~700, each a cache
    for (uint32_t r = a; r < b; ++r) {                       // miss the hardware prefetcher does not see coming
        if (r + AHEAD < b) {
            const uint8_t* ps = in.src(r0 + r + AHEAD);
            const uint64_t plen = in.len(r0 + r + AHEAD);
            __builtin_prefetch(ps, 0, 0); __builtin_prefetch(ps + 64, 0, 0); __builtin_prefetch(ps + 128, 0, 0);
            if (k.both && plen > k.keep) {
                const uint8_t* pt = ps + plen - k.n;
                __builtin_prefetch(pt, 0, 0); __builtin_prefetch(pt + 64, 0, 0); __builtin_prefetch(pt + 128, 0, 0);
            }
        }
        const uint64_t len = in.len(r0 + r);
        len_out[r] = (uint32_t)len;
        qupload::copy_read(staging + pos, in.src(r0 + r), len, k);
        pos += len <= k.keep ? len : k.keep;
        off[r + 1] = pos;
    }
}

// ... second half: every part writes its offsets and copies its reads (ps: as stage_lengths left it)
template <class Reads>
static inline void stage_compact(qk::HostPool& pool, const Reads& in, uint32_t r0, const Split& s, const qupload::Keep& k,
                                 const PartSum* ps, uint8_t* staging, uint64_t* off, uint32_t* len_out) {
    off[0] = 0;
    pool.run(s.parts, [&](int part) { compact_part(in, r0, s.begin(part), s.end(part), ps[part].bytes, k, staging, off, len_out); });
}

// ---- records ----------------------------------------------------------------------------------------------------------------
// cnt records of a slot to the caller's array, split over the pool
template <class Rec>
static inline void copy_records(qk::HostPool& pool, Rec* dst, const Rec* src, uint32_t cnt) {
    const Split s = record_parts(cnt, pool.size());
    pool.run(s.parts, [&](int part) {
        const uint32_t a = s.begin(part), b = s.end(part);
        if (b > a) memcpy(dst + a, src + a, (size_t)(b - a) * sizeof(Rec));
    });
}

}  // namespace qpipe

// pipeline_check.cpp -- the device-free part of the chunked host-buffer scan (qcat_amd/csrc/pipeline_core.h, used by
// scan_batch_pipelined of pipeline_host.inc) against a naive restatement: the chunk size and the cuts, the rule the stage slots
// are sized by, the length sums of a chunk's parts with their refusals, the compaction of a chunk into its staging on the
// persistent pool -- concatenated reads and reads scattered through a file, 5' only and both ends -- and the split of a slot's
// records over the pool.  Every buffer a read lies in is an allocation of exactly its size, so a byte read past it is the
// address sanitizer's; the pool runs with 0, 1, 2 and 7 workers, so a part that writes another part's range is the thread
// sanitizer's.
// Built three times by tests/test_pipeline_host.py: plain, -fsanitize=address,undefined, -fsanitize=thread.
//   usage: pipeline_check <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pipeline_core.h"
#include "check_common.h"

using qk::HostPool;

static const unsigned WORKERS[] = {0u, 1u, 2u, 7u};

// ---- cuts -----------------------------------------------------------------------------------------------------------------------
static bool cuts_ok(uint32_t n_reads, bool fastq_form, bool forced, int forced_reads) {
    const uint32_t want_chunk = forced ? (uint32_t)(forced_reads < 4096 ? 4096 : forced_reads)
                                       : (fastq_form ? 262144u : (n_reads / 4 < 262144u ? 262144u : (n_reads / 4 > 1048576u ? 1048576u : n_reads / 4)));
    const uint32_t chunk = qpipe::chunk_reads(n_reads, fastq_form, forced, forced_reads);
    if (chunk != want_chunk) return false;
    const std::vector<uint32_t> cuts = qpipe::chunk_cuts(n_reads, chunk, forced);
    if (cuts.size() < 2 || cuts.front() != 0 || cuts.back() != n_reads) return false;
    uint32_t largest = 0;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) {
        if (cuts[q + 1] <= cuts[q] || cuts[q + 1] - cuts[q] > chunk) return false;
        largest = cuts[q + 1] - cuts[q] > largest ? cuts[q + 1] - cuts[q] : largest;
    }
    if (largest != qpipe::largest_chunk(cuts)) return false;
    const size_t n_chunks = cuts.size() - 1;
    if (forced || n_reads <= 2 * (uint64_t)chunk) {         // multiples of the chunk, the rest in the last one
        if (n_chunks != ((uint64_t)n_reads + chunk - 1) / chunk) return false;
        for (size_t q = 0; q < n_chunks; ++q) if (cuts[q] != (uint64_t)q * chunk) return false;
    } else if (n_chunks > 2) {
        if (cuts[1] != chunk / 3 || n_reads - cuts[n_chunks - 1] != chunk / 3) return false;
    } else return false;                                    // (more than two chunks' worth of reads in two chunks)
    return true;
}

static void cuts_section(Section& s) {
    std::vector<uint32_t> sizes;
    for (uint32_t n = 32768; n <= 33000; ++n) sizes.push_back(n);
    for (uint32_t n : {524288u, 524289u, 786433u, 1048577u, 4194305u, 10000000u, 0xFFFFFFFFu}) sizes.push_back(n);
    const int random_forced[3] = {(int)rnd_below(4096), 4097 + (int)rnd_below(100000), 100000 + (int)rnd_below(3000000)};
    for (uint32_t n : sizes)
        for (int form = 0; form < 2; ++form) {
            ++s.cases; if (!cuts_ok(n, form == 1, false, 0)) ++s.bad;
            for (int forced : {4096, 10000, 32768, random_forced[0], random_forced[1], random_forced[2]}) {
                ++s.cases; if (!cuts_ok(n, form == 1, true, forced)) ++s.bad;
            }
        }
}

// ---- stage sizing ---------------------------------------------------------------------------------------------------------------
// a slot as the host layer keeps it: ensure(n) leaves a buffer that fits alone, else allocates exactly n
struct Slot { size_t reads = 0, bases = 0; };
static bool size_step(Slot& slot, uint32_t largest, uint32_t chunk, uint64_t keep, size_t slack) {
    const qpipe::StageNeed got = qpipe::stage_need(largest, chunk, keep, slack, slot.reads, slot.bases);
    size_t want_reads = (size_t)largest + 1, want_bases = (size_t)largest * keep + slack;
    if (slot.reads != 0 && want_reads > slot.reads) { want_reads = want_reads * 3 / 2; if (want_reads > (size_t)chunk + 1) want_reads = (size_t)chunk + 1; }
    if (slot.bases != 0 && want_bases > slot.bases) { want_bases = want_bases * 3 / 2; if (want_bases > (size_t)chunk * keep + slack) want_bases = (size_t)chunk * keep + slack; }
    const bool ok = got.reads == want_reads && got.bases == want_bases && got.reads >= (size_t)largest + 1 && got.bases >= (size_t)largest * keep + slack;
    if (got.reads > slot.reads) slot.reads = got.reads;
    if (got.bases > slot.bases) slot.bases = got.bases;
    return ok;
}

static void sizing_section(Section& s) {
    for (uint64_t keep : {300ull, 150ull}) {
        // the calls of test_pipeline_stages_grow_between_calls (tests/test_ctx_buffers_gpu.py): forced chunks on one context
        Slot slot;
        const uint32_t calls[4][2] = {{33000, 4096}, {70000, 4096}, {70000, 8192}, {33000, 4096}};
        const size_t reads_after[4] = {4097, 4097, 8193, 8193};
        for (int i = 0; i < 4; ++i) {
            const std::vector<uint32_t> cuts = qpipe::chunk_cuts(calls[i][0], calls[i][1], true);
            ++s.cases;
            if (!size_step(slot, qpipe::largest_chunk(cuts), calls[i][1], keep, 128) || slot.reads != reads_after[i] ||
                slot.bases != (reads_after[i] - 1) * keep + 128) ++s.bad;
        }
        // segments of a file loop, one chunk each, chunks of 262144: first use, growth by half, growth capped, a need that fits,
        // and a slot whose allocation failed (capacity 0 again)
        Slot seg;
        const uint32_t largest[5] = {40000, 100000, 250000, 180000, 262144};
        const size_t want_reads[5] = {40001, 150001, 262145, 262145, 262145};
        for (int i = 0; i < 5; ++i) {
            ++s.cases;
            if (!size_step(seg, largest[i], 262144, keep, 128) || seg.reads != want_reads[i]) ++s.bad;
        }
        Slot failed;
        ++s.cases;
        if (!size_step(failed, 70000, 262144, keep, 128) || failed.reads != 70001 || failed.bases != 70000 * keep + 128) ++s.bad;
    }
}

// ---- length sums and refusals -----------------------------------------------------------------------------------------------------
// offsets alone: no base is touched by the length pass
struct OffsetsOnly {
    const uint64_t* offsets;
    const uint8_t* src(uint32_t) const { return nullptr; }
    uint64_t len(uint32_t r) const { return offsets[r + 1] - offsets[r]; }
    bool decreasing(uint32_t r) const { return offsets[r + 1] < offsets[r]; }
};

static void lengths_section(Section& s) {
    const uint32_t nr = 40000, keep = 300;
    for (unsigned workers : WORKERS) {
        HostPool pool(workers);
        const qpipe::Split parts = qpipe::chunk_parts(nr, pool.size());
        for (uint32_t r0 : {0u, 123u})
            for (int scenario = 0; scenario < 6; ++scenario) {
                // 0: nothing refused; 1: decreasing offsets; 2: a read over 2^32 - 1; 3: decreasing in an earlier part than the long
                // read; 4: the long read in the earlier part; 5: both in one part, the long read first
                const int pa = (int)rnd_below(parts.parts - 1), pb = pa + 1 + (int)rnd_below(parts.parts - 1 - pa);
                auto in_part = [&](int p) { return parts.begin(p) + (uint32_t)rnd_below(parts.end(p) - parts.begin(p)); };
                int64_t dec = -1, lng = -1;
                if (scenario == 1) dec = in_part(pb);
                if (scenario == 2) lng = in_part(pa);
                if (scenario == 3) { dec = in_part(pa); lng = in_part(pb); }
                if (scenario == 4) { lng = in_part(pa); dec = in_part(pb); }
                if (scenario == 5) { lng = parts.begin(pb); dec = parts.begin(pb) + 2; }
                std::vector<uint64_t> off(r0 + nr + 1);
                off[0] = 0;
                for (uint32_t r = 0; r < r0 + nr; ++r) {
                    const int64_t in_chunk = (int64_t)r - r0;
                    if (in_chunk == dec && off[r] > 0) off[r + 1] = off[r] - 1;
                    else if (in_chunk == lng) off[r + 1] = off[r] + 0x100000000ull;
                    else off[r + 1] = off[r] + 1 + rnd_below(3 * keep);
                }
                // the naive pass: read by read
                qupload::Refusal want = qupload::OK;
                uint64_t want_total = 0;
                std::vector<uint64_t> want_start(parts.parts, 0);
                for (uint32_t r = 0; r < nr && want == qupload::OK; ++r) {
                    for (int p = 0; p < parts.parts; ++p) if (parts.begin(p) == r) want_start[p] = want_total;
                    if (off[r0 + r + 1] < off[r0 + r]) want = qupload::DECREASING;
                    else if (off[r0 + r + 1] - off[r0 + r] > 0xFFFFFFFFull) want = qupload::TOO_LONG;
                    else want_total += off[r0 + r + 1] - off[r0 + r] <= keep ? off[r0 + r + 1] - off[r0 + r] : keep;
                }
                qpipe::PartSum sums[qpipe::MAX_PARTS];
                uint64_t total = ~0ull;
                const qupload::Refusal got = qpipe::stage_lengths(pool, OffsetsOnly{off.data()}, r0, parts, keep, sums, &total);
                ++s.cases;
                bool ok = got == want && parts.parts >= 2;
                if (want == qupload::OK) {
                    ok = ok && total == want_total;
                    for (int p = 0; p < parts.parts; ++p) ok = ok && sums[p].bytes == want_start[p];
                }
                // the upload of a resident batch refuses the same read for the same reason
                std::vector<uint64_t> off2(nr + 1);
                uint64_t total2 = 0;
                const qupload::Reads same{nullptr, off.data() + r0, nullptr, nullptr, nr};
                ok = ok && qupload::length_pass(same, qupload::keep_of(keep / 2, true, false), nullptr, off2.data(), &total2) == want;
                if (!ok) ++s.bad;
            }
    }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------------
static std::vector<uint64_t> ragged(uint64_t n) { return {0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1, 3 * n}; }

// the reads of a call in both forms, each in an allocation of exactly its size: concatenated with offsets, and scattered through a
// "file" with a few bytes of other text in front of every read -- the last read ends the file
struct FileRec { uint64_t seq; uint32_t seq_len; };
struct ConcatReads {
    const uint8_t* bases; const uint64_t* offsets;
    const uint8_t* src(uint32_t r) const { return bases + offsets[r]; }
    uint64_t len(uint32_t r) const { return offsets[r + 1] - offsets[r]; }
    bool decreasing(uint32_t r) const { return offsets[r + 1] < offsets[r]; }
};
struct FileReads {
    const uint8_t* data; const FileRec* recs;
    const uint8_t* src(uint32_t r) const { return data + recs[r].seq; }
    uint64_t len(uint32_t r) const { return recs[r].seq_len; }
    bool decreasing(uint32_t) const { return false; }
};
struct Call {
    std::vector<std::vector<uint8_t>> reads;
    std::unique_ptr<uint8_t[]> bases, file;
    std::vector<uint64_t> offsets;
    std::vector<FileRec> recs;
    explicit Call(const std::vector<uint64_t>& lengths) {
        uint64_t total = 0, file_size = 0;
        std::vector<uint64_t> gap;
        for (uint64_t len : lengths) {
            std::vector<uint8_t> r((size_t)len);
            for (auto& x : r) x = (uint8_t)rnd();
            reads.push_back(std::move(r));
            gap.push_back(1 + rnd_below(20));
            total += len; file_size += gap.back() + len;
        }
        bases.reset(new uint8_t[(size_t)total]);
        file.reset(new uint8_t[(size_t)file_size]);
        memset(file.get(), '@', (size_t)file_size);
        uint64_t at = 0, fat = 0;
        offsets.push_back(0);
        for (size_t r = 0; r < reads.size(); ++r) {
            const size_t len = reads[r].size();
            if (len) { memcpy(bases.get() + at, reads[r].data(), len); memcpy(file.get() + fat + gap[r], reads[r].data(), len); }
            recs.push_back(FileRec{fat + gap[r], (uint32_t)len});
            at += len; fat += gap[r] + len;
            offsets.push_back(at);
        }
    }
};

// what the chunk [r0, r0 + nr) stages, read by read, byte by byte
struct Expected { std::vector<uint8_t> staged; std::vector<uint64_t> off; std::vector<uint32_t> len; };
static Expected expect(const Call& c, uint32_t r0, uint32_t nr, uint64_t n, bool both) {
    Expected e;
    e.off.push_back(0);
    for (uint32_t r = r0; r < r0 + nr; ++r) {
        const std::vector<uint8_t>& s = c.reads[r];
        const uint64_t len = s.size();
        e.len.push_back((uint32_t)len);
        if (len <= (both ? 2 * n : n)) for (uint64_t i = 0; i < len; ++i) e.staged.push_back(s[i]);
        else {
            for (uint64_t i = 0; i < n; ++i) e.staged.push_back(s[i]);
            if (both) for (uint64_t i = len - n; i < len; ++i) e.staged.push_back(s[i]);
        }
        e.off.push_back(e.staged.size());
    }
    return e;
}

template <class Reads>
static bool staged_as_expected(HostPool& pool, const Reads& in, uint32_t r0, uint32_t nr, const qupload::Keep& k, const Expected& e) {
    const qpipe::Split parts = qpipe::chunk_parts(nr, pool.size());
    qpipe::PartSum sums[qpipe::MAX_PARTS];
    uint64_t total = ~0ull;
    if (qpipe::stage_lengths(pool, in, r0, parts, k.keep, sums, &total) != qupload::OK || total != e.staged.size()) return false;
    std::vector<uint8_t> staging((size_t)total + 1, 0xEE);                     // (one element behind each end: it must stay)
    std::vector<uint64_t> off((size_t)nr + 2, ~0ull);
    std::vector<uint32_t> len((size_t)nr + 1, 0xDDDDDDDDu);
    qpipe::stage_compact(pool, in, r0, parts, k, sums, staging.data(), off.data(), len.data());
    if (staging[(size_t)total] != 0xEE || off[(size_t)nr + 1] != ~0ull || len[nr] != 0xDDDDDDDDu) return false;
    if (total && memcmp(staging.data(), e.staged.data(), (size_t)total) != 0) return false;
    return std::equal(e.off.begin(), e.off.end(), off.begin()) && std::equal(e.len.begin(), e.len.end(), len.begin());
}

static void compaction_section(Section& s) {
    for (uint64_t n : {150ull, 4ull})
        for (uint32_t nr : {9u, 12293u}) {
            // the ragged lengths around every border of a part, for every size of the pool; random lengths between them
            const uint32_t r0_max = 7;
            std::vector<uint64_t> lengths(r0_max + nr);
            for (auto& l : lengths) l = rnd_below(3 * n + 1);
            const std::vector<uint64_t> rag = ragged(n);
            for (uint32_t r0 : {0u, r0_max})
                for (unsigned workers : WORKERS) {
                    const qpipe::Split parts = qpipe::chunk_parts(nr, workers + 1);
                    for (int p = 0; p <= parts.parts; ++p)
                        for (int d = -9; d < 9; ++d) {
                            const int64_t r = (int64_t)r0 + (p < parts.parts ? parts.begin(p) : nr) + d;
                            if (r >= 0 && r < (int64_t)lengths.size()) lengths[(size_t)r] = rag[(size_t)(r % 9)];
                        }
                }
            const Call call(lengths);
            for (int both = 0; both < 2; ++both) {
                const qupload::Keep k = qupload::keep_of(n, both == 1, false);
                for (uint32_t r0 : {0u, r0_max}) {
                    const Expected e = expect(call, r0, nr, n, both == 1);
                    // the upload of a resident batch stages the same bytes of the same reads (concatenated form)
                    std::vector<uint64_t> off2((size_t)nr + 1);
                    std::vector<uint32_t> len2(nr);
                    uint64_t total2 = 0;
                    const qupload::Reads same{call.bases.get(), call.offsets.data() + r0, nullptr, nullptr, nr};
                    bool upload_same = qupload::length_pass(same, k, len2.data(), off2.data(), &total2) == qupload::OK && total2 == e.staged.size() &&
                                       off2 == e.off && len2 == e.len;
                    std::vector<uint8_t> staging2((size_t)total2 + 1);
                    if (upload_same) qupload::compact(same, k, off2.data(), staging2.data(), 0, nr);
                    upload_same = upload_same && (!total2 || memcmp(staging2.data(), e.staged.data(), (size_t)total2) == 0);
                    for (unsigned workers : WORKERS) {
                        HostPool pool(workers);
                        ++s.cases;
                        if (!upload_same || !staged_as_expected(pool, ConcatReads{call.bases.get(), call.offsets.data()}, r0, nr, k, e)) ++s.bad;
                        ++s.cases;
                        if (!staged_as_expected(pool, FileReads{call.file.get(), call.recs.data()}, r0, nr, k, e)) ++s.bad;
                    }
                }
            }
        }
}

// ---- record flush -----------------------------------------------------------------------------------------------------------------
struct Rec24 { uint64_t a, b, c; };

static void flush_section(Section& s) {
    for (uint32_t cnt : {1u, 65535u, 65536u, 200001u})
        for (unsigned workers : WORKERS) {
            HostPool pool(workers);
            ++s.cases;
            // every record in exactly one part
            const qpipe::Split parts = qpipe::record_parts(cnt, pool.size());
            std::vector<uint8_t> times(cnt, 0);
            for (int p = 0; p < parts.parts; ++p)
                for (uint32_t i = parts.begin(p); i < parts.end(p); ++i) ++times[i];
            bool ok = parts.parts >= 1 && parts.parts <= (int)pool.size();
            for (uint32_t i = 0; i < cnt; ++i) ok = ok && times[i] == 1;
            std::vector<Rec24> src(cnt), dst((size_t)cnt + 1, Rec24{~0ull, ~0ull, ~0ull});
            for (auto& r : src) r = Rec24{rnd(), rnd(), rnd()};
            qpipe::copy_records(pool, dst.data(), src.data(), cnt);
            ok = ok && memcmp(dst.data(), src.data(), (size_t)cnt * sizeof(Rec24)) == 0 && dst[cnt].a == ~0ull && dst[cnt].c == ~0ull;
            if (!ok) ++s.bad;
        }
}

int main(int argc, char** argv) {
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    Section cuts{"cuts"}, sizing{"stage sizing"}, lengths{"length sums and refusals"}, compaction{"compaction"}, flush{"record flush"};
    cuts_section(cuts); report(cuts);
    sizing_section(sizing); report(sizing);
    lengths_section(lengths); report(lengths);
    compaction_section(compaction); report(compaction);
    flush_section(flush); report(flush);
    return cuts.bad || sizing.bad || lengths.bad || compaction.bad || flush.bad ? 1 : 0;
}

// partition_check.cpp -- the copy kernel of qcat_batch_partition (qcat_amd/csrc/kernels_partition.inc: k_part_chunks,
// k_part_copy) run on the host, lane by lane, through the functions of qcat_amd/csrc/partition_core.h that the kernel itself
// calls: the chunk's first segment, the search of its last, the LDS table or the global arrays, the ownership of a 16-byte
// destination vector, the two aligned source vectors and their shift.  Source and destination are allocated with exactly the
// slack a device batch has (64 bytes on either side), every load is checked against it, every destination byte must be stored
// exactly once and nothing outside the output's vectors at all; the bytes are compared with plain concatenation.
// Built twice by tests/test_partition_host.py: plain, and with -fsanitize=address,undefined.
//   usage: partition_check <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "partition_core.h"
#include "check_common.h"

using namespace qpart;

struct Seg { uint64_t gap; uint64_t len; };               // `gap` source bytes that are not kept, then `len` kept bytes

// one run of the device schedule over a segment list; returns the number of wrong / doubly stored / stray bytes and loads outside the slack
static uint64_t run_copy(const std::vector<Seg>& segs, uint64_t tail_gap, uint64_t* lds_chunks = nullptr, uint64_t* global_chunks = nullptr) {
    const uint32_t n = (uint32_t)segs.size();
    std::vector<uint64_t> dst_off(n + 1), src_pos(n ? n : 1);
    uint64_t n_src = 0, total = 0;
    for (uint32_t j = 0; j < n; ++j) { n_src += segs[j].gap; src_pos[j] = n_src; dst_off[j] = total; n_src += segs[j].len; total += segs[j].len; }
    dst_off[n] = total;
    n_src += tail_gap;
    // the input batch: slack, n_src bases, slack; the output batch: slack, room for the input's bases, slack (the grid is sized by
    // the input's bases)
    std::vector<uint8_t> payload(n_src);
    for (auto& b : payload) b = (uint8_t)rnd();
    Plane in(payload);
    const uint8_t* src = payload.data();
    const CopyRun r = copy_schedule(dst_off, src_pos, n_src, [&](uint32_t, int64_t a) { return in.load16(a); });
    if (lds_chunks) *lds_chunks += r.lds_chunks;
    if (global_chunks) *global_chunks += r.global_chunks;
    uint64_t bad = r.bad + in.stray;
    // the bytes are the concatenation
    const uint8_t* dst = r.out.data();
    uint64_t d = 0;
    for (uint32_t j = 0; j < n; ++j)
        for (uint64_t i = 0; i < segs[j].len; ++i, ++d) if (dst[d] != src[src_pos[j] + i]) ++bad;
    for (; d < r.out.size(); ++d) if (dst[d] != 0) ++bad;        // (the last vector's bytes behind the total are zeros)
    return bad;
}

static void filler(std::vector<Seg>& segs, uint64_t bytes) {      // kept bytes in segments of about 700
    while (bytes) {
        const uint64_t l = bytes < 900 ? bytes : 500 + rnd_below(400);
        segs.push_back({rnd_below(40), l});
        bytes -= l;
    }
}

int main(int argc, char** argv) {
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    uint64_t failed = 0;

    {   // the small functions against their definitions
        Section s{"primitives"};
        for (uint32_t sh = 0; sh < 16; ++sh) {
            uint8_t b[32]; for (auto& x : b) x = (uint8_t)rnd();
            Vec16 lo, hi; memcpy(lo.w, b, 16); memcpy(hi.w, b + 16, 16);
            const Vec16 v = shift_pair(lo, hi, sh);
            ++s.cases; if (memcmp(v.w, b + sh, 16) != 0) ++s.bad;
        }
        for (uint32_t p = 0; p < 16; ++p) for (uint32_t q = p + 1; q <= 16; ++q) {
            uint8_t want[16]; for (uint32_t i = 0; i < 16; ++i) want[i] = (i >= p && i < q) ? 0xFF : 0;
            uint32_t got[4]; for (uint32_t i = 0; i < 4; ++i) got[i] = byte_mask(p, q, i);
            ++s.cases; if (memcmp(got, want, 16) != 0) ++s.bad;
        }
        const int64_t lens[] = {0, 1, 5, 100}, trims[] = {0, 1, 3, 5, 99, 100, 101, 110};
        for (int64_t len : lens) for (int64_t t5 : trims) for (int64_t t3 : trims) for (int tr = 0; tr < 2; ++tr) {
            uint64_t st, kp; slice_of(len, t5, t3, tr != 0, &st, &kp);
            int64_t a = t5 < len ? t5 : len, b = t3 < len ? t3 : len;                   // sequence[t5:t3]
            const uint64_t ws = tr ? (uint64_t)a : 0, wk = tr ? (uint64_t)(b > a ? b - a : 0) : (uint64_t)len;
            ++s.cases; if (st != ws || kp != wk || st + kp > (uint64_t)len) ++s.bad;
        }
        const uint32_t bins[] = {3, 98, 255, 256, 257, 9218, 65536, 65537, 1024u * 1024u + 2u};
        const uint32_t want_passes[] = {1, 1, 1, 1, 2, 2, 2, 3, 3};
        for (int i = 0; i < 9; ++i) { ++s.cases; if (key_passes(bins[i]) != want_passes[i]) ++s.bad; }
        report(s); failed += s.bad;
    }
    {   // every source residue x every destination residue mod 16, lengths around the vector size
        Section s{"residues"};
        const uint64_t lens[] = {1, 2, 15, 16, 17, 31, 32, 33, 70, 700};
        for (uint64_t sr = 0; sr < 16; ++sr) for (uint64_t dr = 0; dr < 16; ++dr) for (uint64_t len : lens) {
            std::vector<Seg> segs;
            segs.push_back({3, 32 + dr});                                    // the segment under test begins at destination residue dr
            const uint64_t at = 3 + 32 + dr;                                 // source bytes so far
            segs.push_back({(sr + 16 - at % 16) % 16, len});                 // ... and at source residue sr
            segs.push_back({7, 45});
            ++s.cases; if (run_copy(segs, 5)) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // lengths 0..70 at the start, in the middle and at the end of a chunk (the segment under test straddles the chunk's end)
        Section s{"lengths at chunk positions"};
        for (uint64_t len = 0; len <= 70; ++len) for (int where = 0; where < 3; ++where) for (uint64_t sr = 0; sr < 16; sr += 5) {
            std::vector<Seg> segs;
            const uint64_t before = where == 0 ? PART_CHUNK : where == 1 ? PART_CHUNK + 12345 : 2 * (uint64_t)PART_CHUNK - len / 2 - (len & 1);
            filler(segs, before);
            segs.push_back({sr, len});
            filler(segs, 3000 + rnd_below(64));
            ++s.cases; if (run_copy(segs, rnd_below(20))) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // a segment longer than several chunks (and longer than 100 kb), between short ones and alone
        Section s{"long segments"};
        for (int k = 0; k < 6; ++k) {
            std::vector<Seg> segs;
            if (k & 1) filler(segs, 1000 + rnd_below(5000));
            segs.push_back({rnd_below(33), 5 * (uint64_t)PART_CHUNK + 777 + rnd_below(4000)});
            if (k & 2) filler(segs, 100 + rnd_below(5000));
            ++s.cases; if (run_copy(segs, rnd_below(20))) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // runs of empty segments: short ones, and runs longer than the chunk's LDS table (the search falls back to the global arrays)
        Section s{"runs of empty segments"};
        uint64_t lds = 0, glob = 0;
        const uint32_t runs[] = {1, 10, PART_LDS_SEGS - 1, PART_LDS_SEGS, PART_LDS_SEGS + 1, 3000};
        for (uint32_t run : runs) for (int where = 0; where < 4; ++where) {
            std::vector<Seg> segs;
            if (where != 0) filler(segs, where == 3 ? PART_CHUNK - 8 : 5000 + rnd_below(100));
            for (uint32_t i = 0; i < run; ++i) segs.push_back({rnd_below(3), 0});
            if (where != 2) filler(segs, 2000 + rnd_below(100));
            ++s.cases; if (run_copy(segs, 3, &lds, &glob)) ++s.bad;
        }
        {   // nothing but empty segments, and no segment at all
            std::vector<Seg> segs(50, Seg{2, 0});
            ++s.cases; if (run_copy(segs, 0)) ++s.bad;
            ++s.cases; if (run_copy(std::vector<Seg>(), 0)) ++s.bad;
        }
        if (!lds || !glob) ++s.bad;                                          // both table forms ran
        report(s); failed += s.bad;
    }
    {   // the vectors on either side of a chunk boundary hold three segments each, one of them crossing the boundary (a chunk
        // boundary is a vector boundary: "inside a vector" is the pair of vectors around it)
        Section s{"three segments around a chunk boundary"};
        for (uint64_t sr = 0; sr < 16; ++sr) for (uint32_t empties = 0; empties < 3; ++empties) {
            std::vector<Seg> segs;
            filler(segs, PART_CHUNK - 10);
            segs.push_back({sr, 5});                                         // [CHUNK - 10, CHUNK - 5)
            for (uint32_t i = 0; i < empties; ++i) segs.push_back({1, 0});
            segs.push_back({3, 8});                                          // [CHUNK - 5, CHUNK + 3): crosses the boundary
            segs.push_back({0, 4});                                          // [CHUNK + 3, CHUNK + 7)
            filler(segs, 1500);
            ++s.cases; if (run_copy(segs, 9)) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // seeded mixtures
        Section s{"random"};
        for (int k = 0; k < 150; ++k) {
            std::vector<Seg> segs;
            const uint32_t n = 1 + (uint32_t)rnd_below(400);
            for (uint32_t j = 0; j < n; ++j) {
                const uint64_t kind = rnd_below(100);
                const uint64_t len = kind < 15 ? 0 : kind < 40 ? rnd_below(16) : kind < 60 ? rnd_below(71) : kind < 97 ? 400 + rnd_below(600)
                                                                                                             : rnd_below(3 * (uint64_t)PART_CHUNK);
                segs.push_back({rnd_below(kind & 1 ? 50 : 2), len});
            }
            ++s.cases; if (run_copy(segs, rnd_below(70))) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    return failed ? 1 : 0;
}

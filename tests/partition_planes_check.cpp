// partition_planes_check.cpp -- the two-plane copy of qcat_batch_partition (qcat_amd/csrc/kernels_partition.inc:
// k_part_copy<2>, bases and qualities in one pass) run on the host, lane by lane, through qpart::gather_vectors<P> of
// qcat_amd/csrc/partition_core.h, the function the kernel calls.  The schedule is the one of tests/partition_check.cpp (chunk's
// first segment, search of its last, LDS table or global arrays, one owner per 16-byte destination vector); here two source
// planes with DIFFERENT contents (plane 1 is a fixed permutation of plane 0's byte values, slack included) go through one
// segment walk.  Both planes are allocated with exactly the slack of a device batch, every load is checked against it, every
// destination byte of either plane must be stored exactly once and nothing outside the output's vectors; both outputs are
// compared with plain concatenation.  For every destination vector, gather_vectors<1> must equal gather_vector.
// Built twice by tests/test_partition_planes_host.py: plain, and with -fsanitize=address,undefined.
//   usage: partition_planes_check <seed>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "partition_core.h"
#include "check_common.h"

using namespace qpart;

static uint8_t permuted(uint8_t x) { return (uint8_t)(x * 167u + 13u); }       // (167 is odd: a permutation of 0..255 without a fixed byte pattern)

struct Seg { uint64_t gap; uint64_t len; };               // `gap` source bytes that are not kept, then `len` kept bytes

// one run of the device schedule over a segment list with two planes; returns the number of wrong / doubly stored / stray bytes,
// loads outside the slack and vectors on which the one-plane form of gather_vectors differs from gather_vector
static uint64_t run_copy(const std::vector<Seg>& segs, uint64_t tail_gap, uint64_t* lds_chunks = nullptr, uint64_t* global_chunks = nullptr) {
    constexpr uint32_t P = 2;
    const uint32_t n = (uint32_t)segs.size();
    std::vector<uint64_t> dst_off(n + 1), src_pos(n ? n : 1);
    uint64_t n_src = 0, total = 0;
    for (uint32_t j = 0; j < n; ++j) { n_src += segs[j].gap; src_pos[j] = n_src; dst_off[j] = total; n_src += segs[j].len; total += segs[j].len; }
    dst_off[n] = total;
    n_src += tail_gap;
    const size_t alloc = n_src + 2 * PART_SLACK;
    std::vector<uint8_t> src_alloc[P], dst_alloc[P], stored[P];
    for (uint32_t k = 0; k < P; ++k) { src_alloc[k].resize(alloc); dst_alloc[k].assign(alloc, 0xEE); stored[k].assign(alloc, 0); }
    for (size_t i = 0; i < alloc; ++i) { src_alloc[0][i] = (uint8_t)rnd(); src_alloc[1][i] = permuted(src_alloc[0][i]); }
    const uint8_t* src[P] = {src_alloc[0].data() + PART_SLACK, src_alloc[1].data() + PART_SLACK};
    uint8_t* dst[P] = {dst_alloc[0].data() + PART_SLACK, dst_alloc[1].data() + PART_SLACK};
    uint64_t bad = 0;
    const auto load16 = [&](uint32_t k, int64_t a) {
        Vec16 v; v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
        if (k >= P || (a & 15) != 0 || a < -(int64_t)PART_SLACK || a + 16 > (int64_t)(n_src + PART_SLACK)) { ++bad; return v; }
        memcpy(v.w, src[k] + a, 16);
        return v;
    };
    const auto load16_plane0 = [&](int64_t a) { return load16(0u, a); };
    const auto goff = [&](uint32_t j) { return dst_off[j]; };
    // k_part_chunks (the grid is sized by the input's bases)
    const uint64_t max_chunks = chunks_of(n_src);
    std::vector<uint32_t> chunk_first(max_chunks + 1, 0xFFFFFFFFu);
    for (uint64_t c = 0; c < max_chunks; ++c) {
        if (c * PART_CHUNK >= total) continue;
        chunk_first[c] = find_segment(goff, 0u, n, c * PART_CHUNK);
    }
    // k_part_copy<2>
    for (uint64_t c = 0; c < max_chunks; ++c) {
        const uint64_t c0 = c * PART_CHUNK;
        if (c0 >= total) continue;
        const uint64_t cend = c0 + PART_CHUNK < total ? c0 + PART_CHUNK : total;
        const uint32_t jf = chunk_first[c];
        const uint32_t hi = cend < total ? chunk_first[c + 1] + 1u : n;
        const uint32_t jl = find_segment(goff, jf, hi, cend - 1);
        if (!(dst_off[jf] <= c0 && dst_off[jf + 1] > c0 && dst_off[jl] <= cend - 1 && dst_off[jl + 1] > cend - 1)) ++bad;
        const uint32_t m = jl - jf + 1u;
        const bool in_lds = m <= PART_LDS_SEGS;
        std::vector<uint64_t> s_off, s_src;                   // (sized like the kernel's arrays: a sanitizer sees an index behind them)
        if (in_lds) {
            s_off.resize(PART_LDS_SEGS + 1); s_src.resize(PART_LDS_SEGS);
            for (uint32_t i = 0; i <= m; ++i) { s_off.at(i) = dst_off[jf + i]; if (i < m) s_src.at(i) = src_pos[jf + i]; }
            if (lds_chunks) ++*lds_chunks;
        } else if (global_chunks) ++*global_chunks;
        const auto loff = [&](uint32_t j) { return s_off.at(j); };
        const auto lsrc = [&](uint32_t j) { return s_src.at(j); };
        const auto gsrc = [&](uint32_t j) { return src_pos[j]; };
        for (uint32_t tid = 0; tid < PART_THREADS; ++tid)
            for (uint32_t it = 0; it < PART_VECS_PER_LANE; ++it) {
                const uint64_t d0 = c0 + ((uint64_t)it * PART_THREADS + tid) * PART_VEC;
                if (d0 >= cend) break;
                Vec16 v[P], one[1], old;
                if (in_lds) {
                    gather_vectors<P>(loff, lsrc, load16, 0u, m, d0, total, v);
                    gather_vectors<1>(loff, lsrc, load16, 0u, m, d0, total, one);
                    old = gather_vector(loff, lsrc, load16_plane0, 0u, m, d0, total);
                } else {
                    gather_vectors<P>(goff, gsrc, load16, jf, jl + 1u, d0, total, v);
                    gather_vectors<1>(goff, gsrc, load16, jf, jl + 1u, d0, total, one);
                    old = gather_vector(goff, gsrc, load16_plane0, jf, jl + 1u, d0, total);
                }
                if (memcmp(one[0].w, old.w, 16) != 0 || memcmp(one[0].w, v[0].w, 16) != 0) ++bad;
                if (d0 + PART_VEC > n_src + PART_SLACK) { ++bad; continue; }             // a store behind the allocation
                for (uint32_t k = 0; k < P; ++k) {
                    memcpy(dst[k] + d0, v[k].w, 16);
                    for (uint32_t i = 0; i < 16; ++i) ++stored[k][PART_SLACK + d0 + i];
                }
            }
    }
    // every byte of the output's vectors stored once in each plane, nothing else touched, the bytes are the concatenation
    const uint64_t vec_end = (total + PART_VEC - 1) / PART_VEC * PART_VEC;
    for (uint32_t k = 0; k < P; ++k) {
        for (uint64_t i = 0; i < alloc; ++i) {
            const bool inside = i >= PART_SLACK && i < PART_SLACK + vec_end;
            if (stored[k][i] != (inside ? 1 : 0)) ++bad;
            if (!inside && dst_alloc[k][i] != 0xEE) ++bad;
        }
        uint64_t d = 0;
        for (uint32_t j = 0; j < n; ++j)
            for (uint64_t i = 0; i < segs[j].len; ++i, ++d) if (dst[k][d] != src[k][src_pos[j] + i]) ++bad;
        for (; d < vec_end; ++d) if (dst[k][d] != 0) ++bad;          // (the last vector's bytes behind the total are zeros)
    }
    // the planes differ wherever there are bytes: a plane stored into the other's output would have shown above
    for (uint64_t d = 0; d < total; ++d) if (dst[1][d] != permuted(dst[0][d])) ++bad;
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
    {   // the vectors on either side of a chunk boundary hold three segments each, one of them crossing the boundary
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

// check_common.h -- what the stand-alone check programs (tests/*_check.cpp) share: the seeded generator, the section report,
// and for the programs that run a copy kernel on the host -- k_part_copy<1> (partition_check, fqtext_check) and k_annot_copy
// (textstream_check) -- a plane with the device's slack and the kernels' chunk-and-lane schedule, once, parametrised by the load.
// Built with -I qcat_amd/csrc -I tests.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "partition_core.h"

static uint64_t g_rng = 1;
static inline uint64_t rnd() {                            // SplitMix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline uint64_t rnd_below(uint64_t n) { return n ? rnd() % n : 0; }

struct Section { const char* name; uint64_t cases = 0, bad = 0; };
static inline void report(const Section& s) { printf("%s: %llu cases, %llu mismatches\n", s.name, (unsigned long long)s.cases, (unsigned long long)s.bad); }

// a plane as the device holds it: slack, payload, slack; offsets count from the payload, which is 16-byte aligned there
struct Plane {
    std::vector<uint8_t> mem;
    uint64_t stray = 0;                                    // loads outside the allocation or unaligned
    explicit Plane(const std::vector<uint8_t>& payload) : mem(payload.size() + 2 * qpart::PART_SLACK, 0xA5) {
        if (!payload.empty()) memcpy(mem.data() + qpart::PART_SLACK, payload.data(), payload.size());
    }
    uint8_t* at0() { return mem.data() + qpart::PART_SLACK; }
    qpart::Vec16 load16(int64_t a) {
        qpart::Vec16 v; v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
        if ((a & 15) != 0 || a < -(int64_t)qpart::PART_SLACK || a + 16 > (int64_t)(mem.size() - qpart::PART_SLACK)) { ++stray; return v; }
        memcpy(v.w, at0() + a, 16);
        return v;
    }
};

// one run of k_part_chunks and of the copy kernel's schedule -- chunk by chunk, the LDS table or the global arrays, lane by lane,
// qpart::gather_vectors<1> as both kernels call it -- over the segment table dst_off[n + 1] / src_pos[n], into a destination
// sized for `bound` bytes with the device's slack (the grid follows the bound).  load16(0, a): the kernel's load, which counts
// its own faults.  `bad`: a chunk whose first and last segment do not bracket it, a store behind the allocation, a byte of the
// output's vectors not stored exactly once, a byte outside them touched.  `out`: the output's whole vectors.
struct CopyRun { uint64_t bad = 0, lds_chunks = 0, global_chunks = 0; std::vector<uint8_t> out; };
template <class Load>
static CopyRun copy_schedule(const std::vector<uint64_t>& dst_off, const std::vector<uint64_t>& src_pos, uint64_t bound, const Load& load16) {
    using namespace qpart;
    CopyRun r;
    const uint32_t n = (uint32_t)(dst_off.size() - 1);
    const uint64_t total = dst_off[n];
    if (total > bound) ++r.bad;
    std::vector<uint8_t> dst_alloc(bound + 2 * PART_SLACK, 0xEE), stored(bound + 2 * PART_SLACK, 0);
    uint8_t* dst = dst_alloc.data() + PART_SLACK;
    const auto goff = [&](uint32_t j) { return dst_off[j]; };
    const uint64_t max_chunks = chunks_of(bound);
    std::vector<uint32_t> chunk_first(max_chunks + 1, 0xFFFFFFFFu);
    for (uint64_t c = 0; c < max_chunks; ++c) if (c * PART_CHUNK < total) chunk_first[c] = find_segment(goff, 0u, n, c * PART_CHUNK);
    for (uint64_t c = 0; c < max_chunks; ++c) {
        const uint64_t c0 = c * PART_CHUNK;
        if (c0 >= total) continue;
        const uint64_t cend = c0 + PART_CHUNK < total ? c0 + PART_CHUNK : total;
        const uint32_t jf = chunk_first[c];
        const uint32_t hi = cend < total ? chunk_first[c + 1] + 1u : n;
        const uint32_t jl = find_segment(goff, jf, hi, cend - 1);
        if (!(dst_off[jf] <= c0 && dst_off[jf + 1] > c0 && dst_off[jl] <= cend - 1 && dst_off[jl + 1] > cend - 1)) ++r.bad;
        const uint32_t m = jl - jf + 1u;
        const bool in_lds = m <= PART_LDS_SEGS;
        ++(in_lds ? r.lds_chunks : r.global_chunks);
        std::vector<uint64_t> s_off, s_src;                   // (sized like the kernel's arrays: a sanitizer sees an index behind them)
        if (in_lds) {
            s_off.resize(PART_LDS_SEGS + 1); s_src.resize(PART_LDS_SEGS);
            for (uint32_t i = 0; i <= m; ++i) { s_off.at(i) = dst_off[jf + i]; if (i < m) s_src.at(i) = src_pos[jf + i]; }
        }
        for (uint32_t tid = 0; tid < PART_THREADS; ++tid)
            for (uint32_t it = 0; it < PART_VECS_PER_LANE; ++it) {
                const uint64_t d0 = c0 + ((uint64_t)it * PART_THREADS + tid) * PART_VEC;
                if (d0 >= cend) break;
                Vec16 v[1];
                if (in_lds) gather_vectors<1>([&](uint32_t j) { return s_off.at(j); }, [&](uint32_t j) { return s_src.at(j); }, load16, 0u, m, d0, total, v);
                else gather_vectors<1>(goff, [&](uint32_t j) { return src_pos.at(j); }, load16, jf, jl + 1u, d0, total, v);
                if (d0 + PART_VEC > bound + PART_SLACK) { ++r.bad; continue; }               // a store behind the allocation
                memcpy(dst + d0, v[0].w, 16);
                for (uint32_t i = 0; i < 16; ++i) ++stored[PART_SLACK + d0 + i];
            }
    }
    const uint64_t vec_end = (total + PART_VEC - 1) / PART_VEC * PART_VEC;
    for (uint64_t i = 0; i < stored.size(); ++i) {
        const bool inside = i >= PART_SLACK && i < PART_SLACK + vec_end;
        if (stored[i] != (inside ? 1 : 0)) ++r.bad;
        if (!inside && dst_alloc[i] != 0xEE) ++r.bad;
    }
    r.out.assign(dst, dst + (vec_end < bound + PART_SLACK ? vec_end : bound + PART_SLACK));
    return r;
}

// partition_core.h -- the lane arithmetic of the stable partition of a resident batch (kernels_partition.inc), as pure
// functions that compile for host and device: the kept slice of a read, the search of a destination byte's read in the
// output offsets, the ownership of a 16-byte destination vector and its assembly from aligned 16-byte source vectors.
// tests/partition_check.cpp runs the copy kernel's chunk and lane schedule through these on the host, tests/partition_planes_check.cpp
// its two-plane form.
//
// Vocabulary.  The output is the concatenation of n segments (the kept slices in sorted order); dst_off[0..n] are their
// byte offsets in the output (dst_off[n] = total), src_pos[j] the byte offset of segment j's first byte in the input.
// The output is cut into VECTORS of 16 bytes at 16-byte aligned addresses and into CHUNKS of PART_CHUNK bytes, one
// workgroup each.  A vector has ONE owner lane, which gathers every segment that overlaps it and stores it once: no
// destination byte is stored twice and no store touches a byte it does not own (the last vector of the output is stored
// whole, its bytes behind `total` as zeros: they lie in the batch's back slack).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QP_HD __host__ __device__ __forceinline__
#else
#define QP_HD static inline
#endif

namespace qpart {

constexpr uint32_t PART_THREADS = 256;                         // lanes of a copy workgroup
constexpr uint32_t PART_VEC = 16;                              // bytes of a destination vector
constexpr uint32_t PART_VECS_PER_LANE = 8;
constexpr uint32_t PART_CHUNK = PART_THREADS * PART_VECS_PER_LANE * PART_VEC;     // 32 KiB of the output per workgroup
constexpr uint32_t PART_LDS_SEGS = 1024;                       // boundaries of a chunk kept in the LDS; a chunk with more
                                                               // segments (runs of empty slices) searches the global arrays
constexpr uint32_t PART_SLACK = 64;                            // bytes in front of and behind a batch's bases (BATCH_SLACK)

struct Vec16 { uint32_t w[4]; };

// the kept slice of a read of `len` bases: sequence[trim5p:trim3p] when the kit trims and scans both ends (the writers'
// slice, Python semantics for non-negative bounds), the whole read otherwise
QP_HD void slice_of(int64_t len, int64_t trim5, int64_t trim3, bool trimming, uint64_t* start, uint64_t* keep) {
    if (!trimming) { *start = 0; *keep = (uint64_t)len; return; }
    const int64_t a = trim5 < len ? (trim5 < 0 ? 0 : trim5) : len;
    const int64_t b = trim3 < len ? (trim3 < 0 ? 0 : trim3) : len;
    *start = (uint64_t)a;
    *keep = b > a ? (uint64_t)(b - a) : 0;
}

// bits of the sort key that hold a bin below n_bins, and the 8-bit digits (passes of the radix sort) that cover them
QP_HD uint32_t key_passes(uint32_t n_bins) {
    uint32_t bits = 1;
    while (bits < 32 && (n_bins - 1) >> bits) ++bits;
    return (bits + 7) / 8;
}

// the segment that holds destination byte d (d < dst_off[hi]): the LAST j in [lo, hi) with off(j) <= d -- empty segments
// share their offset with the segment behind them, so the last one is the one with bytes.  off(lo) <= d is required.
template <class Off>
QP_HD uint32_t find_segment(const Off& off, uint32_t lo, uint32_t hi, uint64_t d) {
    while (hi - lo > 1) {                                      // invariant: off(lo) <= d, off(hi) > d (hi may be the end)
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off(mid) <= d) lo = mid; else hi = mid;
    }
    return lo;
}

// chunks that cover `total` bytes (the last vector is stored whole)
QP_HD uint64_t chunks_of(uint64_t total) { return (total + PART_CHUNK - 1) / PART_CHUNK; }

// (hi:lo) >> 8 * sh, low dword: v_alignbyte_b32
QP_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3)));
#endif
}

// 16 bytes that start `sh` (0..15) bytes into the aligned pair (lo, hi): a dword select, then four byte alignments
// (selects instead of a run-time register index: nothing goes to scratch memory)
QP_HD Vec16 shift_pair(const Vec16& lo, const Vec16& hi, uint32_t sh) {
    const uint32_t q = sh >> 2, r = sh & 3;
    uint32_t t0 = lo.w[0], t1 = lo.w[1], t2 = lo.w[2], t3 = lo.w[3], t4 = hi.w[0];
    if (q == 1) { t0 = lo.w[1]; t1 = lo.w[2]; t2 = lo.w[3]; t3 = hi.w[0]; t4 = hi.w[1]; }
    if (q == 2) { t0 = lo.w[2]; t1 = lo.w[3]; t2 = hi.w[0]; t3 = hi.w[1]; t4 = hi.w[2]; }
    if (q == 3) { t0 = lo.w[3]; t1 = hi.w[0]; t2 = hi.w[1]; t3 = hi.w[2]; t4 = hi.w[3]; }
    Vec16 o;
    o.w[0] = alignbyte(t1, t0, r); o.w[1] = alignbyte(t2, t1, r); o.w[2] = alignbyte(t3, t2, r); o.w[3] = alignbyte(t4, t3, r);
    return o;
}

// dword i of the mask with 0xFF in bytes [p, q) of a vector (0 <= p < q <= 16)
QP_HD uint32_t byte_mask(uint32_t p, uint32_t q, uint32_t i) {
    const uint32_t b0 = 4 * i;                                 // bytes [b0, b0 + 4)
    const uint32_t a = p > b0 ? p - b0 : 0, e = q < b0 + 4 ? (q > b0 ? q - b0 : 0) : 4;
    if (e <= a) return 0u;
    const uint32_t upto_e = e >= 4 ? 0xFFFFFFFFu : ((1u << (8 * e)) - 1u);
    const uint32_t upto_a = (1u << (8 * a)) - 1u;              // (a <= 3 here)
    return upto_e & ~upto_a;
}

// One destination vector: the 16 bytes of the output at byte offset d0 (a multiple of 16, d0 < total), gathered from the
// segments [seg_lo, seg_hi) that may overlap it (off(seg_lo) <= d0; off(seg_hi) is the first offset the table does not
// hold bytes for).  load16(a) returns the aligned source vector at SIGNED byte offset a (a multiple of 16) from the first
// base of the input: the function asks for offsets from -16 (a slice that starts inside the first vector, shifted back by
// its place in the destination vector) to less than n_bases + 32, both inside the batch's slack of 64 bytes.
// Per overlapping segment: the two aligned vectors around the virtual source start are loaded and shifted, never single
// bytes; a vector inside one segment -- nearly all of them -- takes one round.
//
// A batch may hold P PLANES of one byte per base (bases, qualities) on the same offsets, in allocations with the same slack
// and the same alignment: one destination vector of every plane has the same segments, source offset, shift and byte masks.
// gather_vectors walks the segments ONCE and applies them to P loads and P output vectors; load16(k, a) is plane k's
// aligned source vector at offset a.
template <uint32_t P, class Off, class Src, class Load>
QP_HD void gather_vectors(const Off& off, const Src& src, const Load& load16, uint32_t seg_lo, uint32_t seg_hi,
                          uint64_t d0, uint64_t total, Vec16 (&out)[P]) {
    for (uint32_t k = 0; k < P; ++k) out[k].w[0] = out[k].w[1] = out[k].w[2] = out[k].w[3] = 0u;
    const uint64_t vend = d0 + PART_VEC < total ? d0 + PART_VEC : total;
    uint64_t d = d0;
    uint32_t lo = seg_lo;
    while (d < vend) {
        const uint32_t j = find_segment(off, lo, seg_hi, d);
        const uint64_t seg_begin = off(j), seg_end = off(j + 1);
        const uint64_t e = seg_end < vend ? seg_end : vend;
        const uint32_t p = (uint32_t)(d - d0), q = (uint32_t)(e - d0);
        // byte p of the vector comes from source byte s; the vector's byte 0 would come from s - p
        const int64_t s0 = (int64_t)(src(j) + (d - seg_begin)) - (int64_t)p;
        const int64_t a = s0 & ~(int64_t)15;
        const uint32_t sh = (uint32_t)(s0 - a);
        Vec16 v[P];
        for (uint32_t k = 0; k < P; ++k) v[k] = load16(k, a);
        if (sh) for (uint32_t k = 0; k < P; ++k) v[k] = shift_pair(v[k], load16(k, a + 16), sh);
        if (p == 0 && q == PART_VEC) { for (uint32_t k = 0; k < P; ++k) out[k] = v[k]; return; }
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t m = byte_mask(p, q, i);
            for (uint32_t k = 0; k < P; ++k) out[k].w[i] = (out[k].w[i] & ~m) | (v[k].w[i] & m);
        }
        d = e;
        lo = j;
    }
}

// one plane: load16(a)
template <class Off, class Src, class Load>
QP_HD Vec16 gather_vector(const Off& off, const Src& src, const Load& load16, uint32_t seg_lo, uint32_t seg_hi,
                          uint64_t d0, uint64_t total) {
    Vec16 out[1];
    gather_vectors<1>(off, src, [&](uint32_t, int64_t a) { return load16(a); }, seg_lo, seg_hi, d0, total, out);
    return out[0];
}

}  // namespace qpart

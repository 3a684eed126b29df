// kernels_fqtext.inc -- FASTQ text in device memory (qcat_batch_upload_fastq_text, qcat_batch_demux_text):
//   k_fq_count       newlines per block of FQ_BLOCK bytes of the text (aligned 16-byte loads, a SWAR compare, popcounts)
//   (k_scan_reduce / _top / _add of kernels_partition.inc: the first line of every block)
//   k_fq_lines       the same bytes again: every byte's line is known now, so its kind (line mod 4) is -- the byte classes of
//                    fq_parse by kind, and line_start[k] for every line; the rank of a newline inside the block comes from wave
//                    ballots and a cross-wave prefix, as k_part_scatter ranks its keys
//   k_fq_records     one lane per record: '@', '+', the lengths, the '+' line's tail, the title's right strip; the record table,
//                    the sequence lengths (their scan: the batch's offsets) and sources of the bases' copy; tabs of the title
//                    become blanks ("the titles as the writers print them")
//   k_fq_segments    six (length, source) segments per read of the partition's sorted order (qfq::record_segments)
//   k_fq_firsts      rec_first / bin_first_bytes out of the scanned segment offsets
// The copies are k_part_chunks / k_part_copy<1> of kernels_partition.inc with the text plane as the source.
// No workgroup waits for another, no atomic hands out a position: the first bad line is an atomicMin, whose result does not
// depend on the order.  The arithmetic is fqtext_core.h's.  Included by qcat_hip.hip.
#include "fqtext_core.h"

namespace qk {

// what the host reads back of a parse
struct FqStatus {
    unsigned long long bad_line;               // the smallest line with a failed check (qfq::FQ_NO_LINE: none)
};

__device__ __forceinline__ qpart::Vec16 dev_fq_load(const uint8_t* __restrict__ text, uint64_t off) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + off);
    qpart::Vec16 o; o.w[0] = v.x; o.w[1] = v.y; o.w[2] = v.z; o.w[3] = v.w;
    return o;
}
// the valid bytes of the vector at `off` (the plane goes on behind the text: constants, slack)
__device__ __forceinline__ uint32_t dev_fq_valid(uint64_t off, uint64_t n_bytes) {
    return off >= n_bytes ? 0u : (n_bytes - off >= qfq::FQ_VEC ? 0xFFFFu : qfq::below((uint32_t)(n_bytes - off)));
}

// counts[b] = newlines of block b; counts[n_blocks] = 0 (the scan turns it into the total)
__global__ void __launch_bounds__(256)
k_fq_count(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t* __restrict__ counts) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * qfq::FQ_BLOCK;
    uint32_t mine = 0;
    for (uint32_t t = 0; t < qfq::FQ_ROUNDS; ++t) {
        const uint64_t off = base + (uint64_t)t * qfq::FQ_ROUND + (uint64_t)threadIdx.x * qfq::FQ_VEC;
        const uint32_t valid = dev_fq_valid(off, n_bytes);
        if (valid) mine += qfq::popc32(qfq::nl_mask16(dev_fq_load(text, off)) & valid);
    }
    if (mine) atomicAdd(&total, mine);                                 // (a count, not a position: any order gives the same sum)
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = total;
        if (blockIdx.x == 0) counts[gridDim.x] = 0;
    }
}

// first[b]: newlines in front of block b (the scanned counts), first[n_blocks]: all of them.  line_start holds first[n_blocks] + 2
// entries.
__global__ void __launch_bounds__(256)
k_fq_lines(const uint8_t* __restrict__ text, uint64_t n_bytes, const uint64_t* __restrict__ first, uint64_t n_blocks,
           uint64_t* __restrict__ line_start, FqStatus* __restrict__ status) {
    __shared__ uint32_t wtot[4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * qfq::FQ_BLOCK;
    uint64_t line = first[blockIdx.x];                                 // the line of the round's first byte
    if (blockIdx.x == 0 && tid == 0) line_start[0] = 0;
    for (uint32_t t = 0; t < qfq::FQ_ROUNDS; ++t) {
        const uint64_t off = base + (uint64_t)t * qfq::FQ_ROUND + (uint64_t)tid * qfq::FQ_VEC;
        const uint32_t valid = dev_fq_valid(off, n_bytes);
        qpart::Vec16 v; v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
        if (valid) v = dev_fq_load(text, off);
        const uint32_t nl = qfq::nl_mask16(v) & valid;
        uint32_t rank = 0, wsum = 0;
        if (__ballot(nl != 0)) {                                       // (the same for the whole wave)
            uint64_t bal[qfq::FQ_VEC];
#pragma unroll
            for (uint32_t b = 0; b < qfq::FQ_VEC; ++b) bal[b] = __ballot((nl >> b) & 1u);
            rank = qfq::wave_rank(bal, lane);
            wsum = qfq::wave_total(bal);
        }
        if (lane == 0) wtot[wave] = wsum;
        __syncthreads();
        uint64_t mine = line + rank;                                   // the line of this vector's first byte
        for (uint32_t w = 0; w < wave; ++w) mine += wtot[w];
        const uint32_t round_total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
        line += round_total;
        if (!valid) continue;                                          // (behind the barriers: nobody is left at one)
        const uint32_t bad = qfq::lines_bad(nl, qfq::odd_title16(v) & valid, qfq::odd_seq16(v) & valid, (uint32_t)(mine & 3u));
        if (bad) {
            const uint32_t b = (uint32_t)__ffs((int)bad) - 1u;
            atomicMin(&status->bad_line, (unsigned long long)(mine + qfq::popc32(nl & qfq::below(b))));
        }
        uint32_t rest = nl;
        uint64_t k = mine;
        while (rest) {
            const uint32_t b = (uint32_t)__ffs((int)rest) - 1u;
            line_start[++k] = off + b + 1;                             // (the byte behind the text's last newline: the closing entry)
            rest &= rest - 1u;
        }
        // a text whose last byte is no newline: its owner closes the table behind the last line
        if (off + qfq::FQ_VEC >= n_bytes && !((nl >> (uint32_t)(n_bytes - 1 - off)) & 1u)) line_start[first[n_blocks] + 1] = n_bytes + 1;
    }
}

// One lane per record of n_lines lines.  A record that fails a check -- or has fewer than four lines -- lowers status->bad_line to
// its first line; the others write their table entry, their length into lens[r] (lens[n_rec] = 0: the scan makes the offsets)
// and the source of their bases, and turn the tabs of their title into blanks.
__global__ void __launch_bounds__(256)
k_fq_records(uint8_t* __restrict__ text, const uint64_t* __restrict__ line_start, uint64_t n_lines, uint32_t n_rec,
             qfq::Rec* __restrict__ recs, uint64_t* __restrict__ lens, uint64_t* __restrict__ seq_src, FqStatus* __restrict__ status) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { lens[r] = 0; return; }
    lens[r] = 0; seq_src[r] = 0;
    if (4 * r + 4 > n_lines) { atomicMin(&status->bad_line, (unsigned long long)(4 * r)); return; }
    uint64_t ls[5];
    for (uint32_t i = 0; i < 5; ++i) ls[i] = line_start[4 * r + i];
    qfq::Rec rec;
    if (!qfq::record_of([&](uint64_t i) { return text[i]; }, ls, &rec)) { atomicMin(&status->bad_line, (unsigned long long)(4 * r)); return; }
    recs[r] = rec;
    lens[r] = rec.seq_len;
    seq_src[r] = rec.seq_off;
    if (rec.title_blank)
        for (uint64_t i = 0; i < rec.title_len; ++i) if (text[rec.title_off + i] == '\t') text[rec.title_off + i] = ' ';
}

// segment table of the output text: sorted read j (read source[j] of the batch, bin key_sorted[j]; the last bin: skipped) gets
// segments 6 j .. 6 j + 5; the kept slice is the partition's (start[r] - offsets[r], keep[r])
__global__ void __launch_bounds__(256)
k_fq_segments(const uint32_t* __restrict__ source, const uint32_t* __restrict__ key_sorted, const uint64_t* __restrict__ start,
              const uint64_t* __restrict__ keep, const uint64_t* __restrict__ offsets, const qfq::Rec* __restrict__ recs, uint32_t n,
              uint32_t skipped_bin, uint64_t const_off, uint64_t* __restrict__ seg_off, uint64_t* __restrict__ seg_src) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { seg_off[(uint64_t)qfq::FQ_SEGS * n] = 0; return; }
    const uint32_t r = source[j];
    uint64_t len[qfq::FQ_SEGS], src[qfq::FQ_SEGS];
    qfq::record_segments(recs[r], start[r] - offsets[r], keep[r], key_sorted[j] == skipped_bin, const_off, len, src);
#pragma unroll
    for (uint32_t i = 0; i < qfq::FQ_SEGS; ++i) { seg_off[qfq::FQ_SEGS * j + i] = len[i]; seg_src[qfq::FQ_SEGS * j + i] = src[i]; }
}

// rec_first[j] = first byte of sorted record j (n + 1 entries); bin_bytes[b] = first byte of bin b (n_bins + 1 entries)
__global__ void __launch_bounds__(256)
k_fq_firsts(const uint64_t* __restrict__ seg_off, uint32_t n, const uint64_t* __restrict__ bin_first, uint32_t n_bins,
            uint64_t* __restrict__ rec_first, uint64_t* __restrict__ bin_bytes) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= n) rec_first[j] = seg_off[(uint64_t)qfq::FQ_SEGS * j];
    if (j <= n_bins) bin_bytes[j] = seg_off[(uint64_t)qfq::FQ_SEGS * bin_first[j]];
}

}  // namespace qk

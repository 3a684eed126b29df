// kernels_textstream.inc -- FASTA text in device memory and the driver's annotated single stream (qcat_batch_upload_text,
// qcat_batch_demux_text on a FASTA batch, qcat_batch_annot_text):
//   k_fa_records       beside k_fq_records: one lane per record of TWO lines -- '>', a non-empty sequence line, the title's right
//                      strip; the record table (qual_off = 0), the sequence lengths and sources, tabs of the title become blanks.
//                      A lane whose own first line lacks '>' lowers the bad line to the record IN FRONT of it, a lane whose
//                      sequence line is missing or empty to itself (qfq::fa_record_of / fa_blamed_line: fa_parse's verdicts)
//   k_fa_segments      beside k_fq_segments: the six segments of a FASTA output record (qfq::fa_record_segments)
//   k_annot_segments   one lane per read in READ order: the kept slice and the minimum-length verdict (the partition's), the ten
//                      segments of the stream's record (qann::record_segments) -- text-plane and tag-plane sources
//   (k_scan_reduce / _top / _add, k_part_chunks of kernels_partition.inc: the offsets, the first segment of every chunk)
//   k_annot_firsts     rec_first out of the scanned segment offsets
//   k_annot_copy       beside k_part_copy: the same chunks, LDS table, owners and aligned 16-byte stores
//                      (qpart::gather_vectors<1>); the load picks the source plane of a segment by qann::ANNOT_TAG in its position
// No workgroup waits for another and no atomic hands out a position.  The arithmetic is fqtext_core.h's and textstream_core.h's.
// Included by qcat_hip.hip behind kernels_tsvtext.inc.
#include "textstream_core.h"

namespace qk {

__global__ void __launch_bounds__(256)
k_fa_records(uint8_t* __restrict__ text, const uint64_t* __restrict__ line_start, uint64_t n_lines, uint32_t n_rec,
             qfq::Rec* __restrict__ recs, uint64_t* __restrict__ lens, uint64_t* __restrict__ seq_src, FqStatus* __restrict__ status) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { lens[r] = 0; return; }
    lens[r] = 0; seq_src[r] = 0;
    const uint32_t lines = 2 * r + 2 <= n_lines ? 2u : 1u;                     // (r < n_rec: line 2 r exists)
    uint64_t ls[3] = {0, 0, 0};
    for (uint32_t i = 0; i <= lines; ++i) ls[i] = line_start[2 * r + i];
    qfq::Rec rec;
    const uint32_t verdict = qfq::fa_record_of([&](uint64_t i) { return text[i]; }, ls, lines, &rec);
    if (verdict != qfq::FA_OK) { atomicMin(&status->bad_line, (unsigned long long)qfq::fa_blamed_line(r, verdict)); return; }
    recs[r] = rec;
    lens[r] = rec.seq_len;
    seq_src[r] = rec.seq_off;
    if (rec.title_blank)
        for (uint64_t i = 0; i < rec.title_len; ++i) if (text[rec.title_off + i] == '\t') text[rec.title_off + i] = ' ';
}

__global__ void __launch_bounds__(256)
k_fa_segments(const uint32_t* __restrict__ source, const uint32_t* __restrict__ key_sorted, const uint64_t* __restrict__ start,
              const uint64_t* __restrict__ keep, const uint64_t* __restrict__ offsets, const qfq::Rec* __restrict__ recs, uint32_t n,
              uint32_t skipped_bin, uint64_t const_off, uint64_t* __restrict__ seg_off, uint64_t* __restrict__ seg_src) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { seg_off[(uint64_t)qfq::FQ_SEGS * n] = 0; return; }
    const uint32_t r = source[j];
    uint64_t len[qfq::FQ_SEGS], src[qfq::FQ_SEGS];
    qfq::fa_record_segments(recs[r], start[r] - offsets[r], keep[r], key_sorted[j] == skipped_bin, const_off, len, src);
#pragma unroll
    for (uint32_t i = 0; i < qfq::FQ_SEGS; ++i) { seg_off[qfq::FQ_SEGS * j + i] = len[i]; seg_src[qfq::FQ_SEGS * j + i] = src[i]; }
}

// read r gets segments 10 r .. 10 r + 9 (lengths into seg_off: the scan turns them into offsets; seg_off[10 n] = 0: the total)
__global__ void __launch_bounds__(256)
k_annot_segments(KitPtrs kp, qtsv::Tables T, const qcat_result* __restrict__ results, const uint64_t* __restrict__ offsets,
                 const qfq::Rec* __restrict__ recs, uint32_t n, uint32_t fasta, uint64_t const_off, uint64_t* __restrict__ seg_off,
                 uint64_t* __restrict__ seg_src) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) { seg_off[(uint64_t)qann::ANNOT_SEGS * n] = 0; return; }
    const DevKit* k = kp.kit;
    const qcat_result res = results[r];
    const int64_t rlen = (int64_t)(offsets[r + 1] - offsets[r]);
    const bool skipped = dev_skipped(k, rlen, res.trim5p, res.trim3p);
    uint64_t s, l;
    qpart::slice_of(rlen, res.trim5p, res.trim3p, k->trim_reads && k->ends != QCAT_ENDS_5P, &s, &l);
    uint64_t len[qann::ANNOT_SEGS], src[qann::ANNOT_SEGS];
    qann::record_segments(T, recs[r], fasta != 0, s, l, skipped, res.barcode_idx, res.barcode2_idx, res.adapter_idx, const_off, len, src);
#pragma unroll
    for (uint32_t i = 0; i < qann::ANNOT_SEGS; ++i) { seg_off[qann::ANNOT_SEGS * r + i] = len[i]; seg_src[qann::ANNOT_SEGS * r + i] = src[i]; }
}

// rec_first[r] = first byte of record r of the stream (n + 1 entries)
__global__ void __launch_bounds__(256)
k_annot_firsts(const uint64_t* __restrict__ seg_off, uint32_t n, uint64_t* __restrict__ rec_first) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= n) rec_first[r] = seg_off[(uint64_t)qann::ANNOT_SEGS * r];
}

// k_part_copy<1> with two source planes: `text` (a batch's text plane) and `tags` (the tag plane), both 16-byte aligned with
// PART_SLACK bytes in front and 32 bytes or more behind their last source byte.  The grid is sized by the output's bound; a
// workgroup behind the output's end leaves at once.
__global__ void __launch_bounds__(256)
k_annot_copy(const uint64_t* __restrict__ dst_off, const uint64_t* __restrict__ src_pos, uint32_t n,
             const uint32_t* __restrict__ chunk_first, const uint8_t* __restrict__ text, const uint8_t* __restrict__ tags,
             uint8_t* __restrict__ dst) {
    __shared__ uint64_t s_off[qpart::PART_LDS_SEGS + 1];
    __shared__ uint64_t s_src[qpart::PART_LDS_SEGS];
    const uint64_t total = dst_off[n];
    const uint64_t c0 = (uint64_t)blockIdx.x * qpart::PART_CHUNK;
    if (c0 >= total) return;                       // (the same for every lane: nobody is left at a barrier)
    const uint64_t cend = c0 + qpart::PART_CHUNK < total ? c0 + qpart::PART_CHUNK : total;
    const auto goff = [&](uint32_t j) { return dst_off[j]; };
    const uint32_t jf = chunk_first[blockIdx.x];
    const uint32_t hi = cend < total ? chunk_first[blockIdx.x + 1] + 1u : n;
    const uint32_t jl = qpart::find_segment(goff, jf, hi, cend - 1);
    const uint32_t m = jl - jf + 1u;
    const bool in_lds = m <= qpart::PART_LDS_SEGS;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i <= m; i += 256u) {
            s_off[i] = dst_off[jf + i];
            if (i < m) s_src[i] = src_pos[jf + i];
        }
        __syncthreads();
    }
    const auto load16 = [&](uint32_t, int64_t a) {
        const uint4 v = *reinterpret_cast<const uint4*>((qann::src_in_tag(a) ? tags : text) + qann::src_plane_off(a));
        qpart::Vec16 o; o.w[0] = v.x; o.w[1] = v.y; o.w[2] = v.z; o.w[3] = v.w;
        return o;
    };
    for (uint32_t it = 0; it < qpart::PART_VECS_PER_LANE; ++it) {
        const uint64_t d0 = c0 + ((uint64_t)it * 256u + threadIdx.x) * qpart::PART_VEC;
        if (d0 >= cend) break;
        qpart::Vec16 v[1];
        if (in_lds)
            qpart::gather_vectors<1>([&](uint32_t j) { return s_off[j]; }, [&](uint32_t j) { return s_src[j]; }, load16, 0u, m, d0, total, v);
        else
            qpart::gather_vectors<1>(goff, [&](uint32_t j) { return src_pos[j]; }, load16, jf, jl + 1u, d0, total, v);
        *reinterpret_cast<uint4*>(dst + d0) = make_uint4(v[0].w[0], v[0].w[1], v[0].w[2], v[0].w[3]);
    }
}

}  // namespace qk

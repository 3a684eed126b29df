// kernels_tsvtext.inc -- the driver's TSV rows of a scanned text batch in device memory (qcat_batch_tsv_text):
//   k_tsv_lengths    one lane per read: the kept slice and the verdict of the minimum-length filter (qpart::slice_of, dev_skipped:
//                    the partition's), the name's length (the title's only scan), the row's fields and their length; a called
//                    read whose (raw_score, score_den) has no slot in the score table raises a flag
//   (k_scan_reduce / _top / _add of kernels_partition.inc: row_first)
//   k_tsv_tiles      the row that holds the first byte of every tile of TSV_TILE bytes of the OUTPUT
//   k_tsv_write      one workgroup per tile: the rows that overlap it, a group of TSV_GROUP lanes per row, assemble their bytes in
//                    the LDS -- a dword per lane from the text plane, the tables and the per-read numbers --; the tile goes out in
//                    aligned 16-byte vectors, the output's last partial vector byte by byte
// No atomic hands out a position and no workgroup waits for another; every byte of the output has one writer.  The arithmetic
// is tsvtext_core.h's.  Included by qcat_hip.hip.
#include "tsvtext_core.h"

namespace qk {

// row_len[r] = bytes of row r (0: dropped), row_len[n] = 0 (the scan turns them into row_first and the total); name_len / keep:
// what the writer needs again
__global__ void __launch_bounds__(256)
k_tsv_lengths(KitPtrs kp, qtsv::Tables T, const qcat_result* __restrict__ results, const uint64_t* __restrict__ offsets,
              const uint8_t* __restrict__ text, const qfq::Rec* __restrict__ recs, uint32_t n, uint64_t* __restrict__ row_len,
              uint32_t* __restrict__ name_len, uint32_t* __restrict__ keep, uint32_t* __restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (r == n) { row_len[r] = 0; return; }
    const DevKit* k = kp.kit;
    const qcat_result res = results[r];
    const int64_t len = (int64_t)(offsets[r + 1] - offsets[r]);
    row_len[r] = 0; name_len[r] = 0; keep[r] = 0;
    if (dev_skipped(k, len, res.trim5p, res.trim3p)) return;
    uint64_t s, l;
    qpart::slice_of(len, res.trim5p, res.trim3p, k->trim_reads && k->ends != QCAT_ENDS_5P, &s, &l);
    const qfq::Rec rec = recs[r];
    const uint32_t nl = qtsv::name_len(text + rec.title_off, rec.title_len, rec.title_blank != 0);
    qtsv::Row row;
    if (!qtsv::row_of(T, rec.title_off, rec.title_len, nl, (uint32_t)l, res.barcode_idx, res.barcode2_idx, res.adapter_idx, res.adapter_end,
                      res.raw_score, res.score_den, &row))
        *bad = 1u;                                 // (every such store writes the same value; the host zeroes the flag before the launch)
    row_len[r] = qtsv::row_len(row);
    name_len[r] = nl; keep[r] = (uint32_t)l;
}

// tile_first[c] = the row that holds the first byte of tile c, for every tile with bytes
__global__ void __launch_bounds__(256)
k_tsv_tiles(const uint64_t* __restrict__ row_first, uint32_t n, uint32_t* __restrict__ tile_first, uint64_t max_tiles) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = row_first[n];
    if (c >= max_tiles || c * qtsv::TSV_TILE >= total) return;
    tile_first[c] = qpart::find_segment([&](uint32_t j) { return row_first[j]; }, 0u, n, c * qtsv::TSV_TILE);
}

// The grid is sized by the output's bound -- its size is known on the device only --, and a workgroup behind the output's
// end leaves at once (all of them when the output is longer than `bound`, which the host reports).  `out` is 16-byte aligned.
__global__ void __launch_bounds__(qtsv::TSV_THREADS)
k_tsv_write(qtsv::Tables T, const qcat_result* __restrict__ results, const uint8_t* __restrict__ text, const qfq::Rec* __restrict__ recs,
            const uint64_t* __restrict__ row_first, const uint32_t* __restrict__ name_len, const uint32_t* __restrict__ keep, uint32_t n,
            const uint32_t* __restrict__ tile_first, uint64_t bound, uint8_t* __restrict__ out) {
    __shared__ uint4 s_tile[qtsv::TSV_TILE / qtsv::TSV_VEC];
    uint8_t* const tile = reinterpret_cast<uint8_t*>(s_tile);
    const uint64_t total = row_first[n];
    const uint64_t c0 = (uint64_t)blockIdx.x * qtsv::TSV_TILE;
    if (c0 >= total || total > bound) return;      // (the same for every lane: nobody is left at the barrier)
    const uint64_t cend = c0 + qtsv::TSV_TILE < total ? c0 + qtsv::TSV_TILE : total;
    uint32_t jf, jl;
    qtsv::tile_rows([&](uint32_t j) { return row_first[j]; }, [&](uint64_t c) { return tile_first[c]; }, n, blockIdx.x, total, &jf, &jl);
    const uint32_t group = threadIdx.x / qtsv::TSV_GROUP, gl = threadIdx.x % qtsv::TSV_GROUP;
    for (uint64_t r = (uint64_t)jf + group; r <= jl; r += qtsv::TSV_GROUPS) {
        const uint64_t b = row_first[r], e = row_first[r + 1];
        if (e == b) continue;                      // (a dropped read)
        const qcat_result res = results[r];
        const qfq::Rec rec = recs[r];
        qtsv::Row row;
        (void)qtsv::row_of(T, rec.title_off, rec.title_len, name_len[r], keep[r], res.barcode_idx, res.barcode2_idx, res.adapter_idx,
                           res.adapter_end, res.raw_score, res.score_den, &row);
        qtsv::tile_put_row(row, b, e, c0, cend, gl, text, T.blob,
                           [&](uint32_t o, uint32_t w) { *reinterpret_cast<uint32_t*>(tile + o) = w; },
                           [&](uint32_t o, uint8_t v) { tile[o] = v; });
    }
    __syncthreads();
    for (uint32_t it = 0; it < qtsv::TSV_VECS_PER_LANE; ++it) {
        const uint32_t v = it * qtsv::TSV_THREADS + threadIdx.x;
        const uint64_t d0 = c0 + (uint64_t)v * qtsv::TSV_VEC;
        if (d0 >= cend) break;
        if (qtsv::vector_whole(d0, total)) *reinterpret_cast<uint4*>(out + d0) = s_tile[v];
        else for (uint64_t d = d0; d < total; ++d) out[d] = tile[d - c0];
    }
}

}  // namespace qk

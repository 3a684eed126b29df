// kernels_partition.inc -- the stable partition of a resident batch by barcode (qcat_batch_partition):
//   k_part_keys      records -> bin and kept slice (source position, length) per read
//   k_part_hist / k_part_scatter   one pass of a least-significant-digit radix sort over 8 bits of the bin: per-workgroup
//                    digit histogram, a scan over (digit, workgroup), a scatter whose rank inside the workgroup comes from wave
//                    ballots and a cross-wave prefix -- no atomic hands out a position, so the order is the input's, run after run
//   k_scan_reduce / k_scan_top / k_scan_add   exclusive prefix sum as a chain of three launches (no workgroup waits for another)
//   k_part_gather    slice lengths and source positions in sorted order
//   k_part_bins      first read of every bin
//   k_part_chunks    first segment of every 32 KiB chunk of the output
//   k_part_copy      the segmented copy: 16-byte aligned stores, one owner per destination vector (partition_core.h), of one
//                    plane (bases) or two (bases and qualities) in one pass
//   k_offsets_check  qcat_batch_from_device: the caller's offsets start at 0 and never decrease
// Included by qcat_hip.hip.
#include "partition_core.h"

namespace qk {

constexpr uint32_t PART_SORT_ROUNDS = 8;                               // a sort workgroup takes 8 rounds of 256 consecutive keys
constexpr uint32_t PART_SORT_TILE = 256 * PART_SORT_ROUNDS;
constexpr uint32_t PART_SCAN_ITEMS = 8;                                // a scan workgroup takes 256 x 8 consecutive elements
constexpr uint32_t PART_SCAN_BLOCK = 256 * PART_SCAN_ITEMS;

// ---------------------------------------------------------------------------------------------
// a. keys: the bin is k_count's barcode bucket (dev_barcode_bucket), the last bin for a read the min-length filter drops
// (dev_skipped); the slice is the one dev_skipped measures
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_part_keys(KitPtrs kp, const qcat_result* __restrict__ results, const uint64_t* __restrict__ offsets, uint32_t n_reads,
            uint32_t* __restrict__ key, uint64_t* __restrict__ start, uint64_t* __restrict__ keep) {
    const DevKit* k = kp.kit;
    const int nb = k->n_barcode_slots;
    const int nbc = (k->mode == QCAT_MODE_DUAL) ? nb * nb : nb;
    const bool trimming = k->trim_reads && k->ends != QCAT_ENDS_5P;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const qcat_result res = results[r];
        const uint64_t o = offsets[r];
        const int64_t len = (int64_t)(offsets[r + 1] - o);
        int slot = dev_barcode_bucket(kp, nb, nbc, res.barcode_idx, res.barcode2_idx, res.adapter_idx);
        if (dev_skipped(k, len, res.trim5p, res.trim3p)) slot = nbc + 1;
        uint64_t s, l;
        qpart::slice_of(len, res.trim5p, res.trim3p, trimming, &s, &l);
        key[r] = (uint32_t)slot; start[r] = o + s; keep[r] = l;
    }
}

// ---------------------------------------------------------------------------------------------
// b. one radix pass.  Workgroup w owns keys [w * PART_SORT_TILE, ...); hist[digit * n_wg + w] is its count of a digit, and
// after the exclusive scan of the whole table the first position of its keys of that digit.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_part_hist(const uint32_t* __restrict__ key, uint32_t n, uint32_t shift, uint32_t* __restrict__ hist, uint32_t n_wg) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PART_SORT_TILE;
    for (uint32_t t = 0; t < PART_SORT_ROUNDS; ++t) {
        const uint64_t i = base + t * 256u + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(key[i] >> shift) & 255u], 1u);      // (a count, not a position: any order gives the same sum)
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_wg + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void __launch_bounds__(256)
k_part_scatter(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ idx_in /* null: the identity */, uint32_t n,
               uint32_t shift, const uint32_t* __restrict__ hist, uint32_t n_wg,
               uint32_t* __restrict__ key_out, uint32_t* __restrict__ idx_out) {
    __shared__ uint32_t pos[256];                 // next free position of every digit
    __shared__ uint32_t wcnt[4][256];             // this round's count per (wave, digit)
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    pos[tid] = hist[(size_t)tid * n_wg + blockIdx.x];
    for (uint32_t w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PART_SORT_TILE;
    for (uint32_t t = 0; t < PART_SORT_ROUNDS; ++t) {
        const uint64_t i = base + t * 256u + tid;
        const bool live = i < n;
        const uint32_t kv = live ? key_in[i] : 0u;
        const uint32_t dg = (kv >> shift) & 255u;
        // lanes of the wave with the same digit: eight ballots
        uint64_t same = __ballot(live);
        for (uint32_t b = 0; b < 8; ++b) {
            const uint64_t bal = __ballot((dg >> b) & 1u);
            same &= ((dg >> b) & 1u) ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (live && rank == 0) wcnt[wave][dg] = (uint32_t)__popcll(same);           // the group's first lane: one writer per (wave, digit)
        __syncthreads();
        if (live) {
            uint32_t p = pos[dg] + rank;
            for (uint32_t w = 0; w < wave; ++w) p += wcnt[w][dg];
            key_out[p] = kv;
            idx_out[p] = idx_in ? idx_in[i] : (uint32_t)i;
        }
        __syncthreads();
        pos[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        for (uint32_t w = 0; w < 4; ++w) wcnt[w][tid] = 0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// c. exclusive prefix sum in place: block sums, their scan by one workgroup, local scan plus block offset
// ---------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T dev_block_excl_scan(T v, T* lds /* 256 */, T* total) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();                               // (the buffer may still be read from the call before)
    lds[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        const T t = tid >= off ? lds[tid - off] : (T)0;
        __syncthreads();
        lds[tid] += t;
        __syncthreads();
    }
    *total = lds[255];
    return lds[tid] - v;
}

template <class T>
__global__ void __launch_bounds__(256)
k_scan_reduce(const T* __restrict__ data, uint64_t n, T* __restrict__ sums) {
    __shared__ T lds[256];
    const uint64_t first = (uint64_t)blockIdx.x * PART_SCAN_BLOCK + (uint64_t)threadIdx.x * PART_SCAN_ITEMS;
    T s = 0;
    for (uint32_t i = 0; i < PART_SCAN_ITEMS; ++i) if (first + i < n) s += data[first + i];
    T total;
    (void)dev_block_excl_scan(s, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

template <class T>
__global__ void __launch_bounds__(256)
k_scan_top(T* __restrict__ sums, uint64_t n_blocks) {
    __shared__ T lds[256];
    T carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += 256u) {
        const uint64_t i = base + threadIdx.x;
        const T v = i < n_blocks ? sums[i] : (T)0;
        T total;
        const T ex = dev_block_excl_scan(v, lds, &total);
        if (i < n_blocks) sums[i] = carry + ex;
        carry += total;
    }
}

template <class T>
__global__ void __launch_bounds__(256)
k_scan_add(T* __restrict__ data, uint64_t n, const T* __restrict__ sums) {
    __shared__ T lds[256];
    const uint64_t first = (uint64_t)blockIdx.x * PART_SCAN_BLOCK + (uint64_t)threadIdx.x * PART_SCAN_ITEMS;
    T v[PART_SCAN_ITEMS];
    T s = 0;
    for (uint32_t i = 0; i < PART_SCAN_ITEMS; ++i) { v[i] = first + i < n ? data[first + i] : (T)0; s += v[i]; }
    T total;
    T run = sums[blockIdx.x] + dev_block_excl_scan(s, lds, &total);
    for (uint32_t i = 0; i < PART_SCAN_ITEMS; ++i) { if (first + i < n) data[first + i] = run; run += v[i]; }
}

template <class T>
static void part_scan_launch(T* data, uint64_t n, T* sums, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)((n + PART_SCAN_BLOCK - 1) / PART_SCAN_BLOCK);
    if (!blocks) return;
    hipLaunchKernelGGL(k_scan_reduce<T>, dim3(blocks), dim3(256), 0, stream, (const T*)data, n, sums);
    hipLaunchKernelGGL(k_scan_top<T>, dim3(1), dim3(256), 0, stream, sums, (uint64_t)blocks);
    hipLaunchKernelGGL(k_scan_add<T>, dim3(blocks), dim3(256), 0, stream, data, n, (const T*)sums);
}
static inline size_t part_scan_sums(uint64_t n) { return (size_t)((n + PART_SCAN_BLOCK - 1) / PART_SCAN_BLOCK) + 1; }

// slice lengths (into the output's offset array, n + 1 entries: the scan turns them into offsets and the total) and
// source positions in sorted order
__global__ void __launch_bounds__(256)
k_part_gather(const uint32_t* __restrict__ source, const uint64_t* __restrict__ start, const uint64_t* __restrict__ keep, uint32_t n,
              uint64_t* __restrict__ dst_off, uint64_t* __restrict__ src_pos) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { dst_off[j] = 0; return; }
    const uint32_t r = source[j];
    dst_off[j] = keep[r];
    src_pos[j] = start[r];
}

// bin_first[b] = reads of the sorted order with a bin below b, b = 0 .. n_bins
__global__ void __launch_bounds__(256)
k_part_bins(const uint32_t* __restrict__ key_sorted, uint32_t n, uint32_t n_bins, uint64_t* __restrict__ bin_first) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_bins) return;
    uint32_t lo = 0, hi = n;                      // first j with key[j] >= b
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_sorted[mid] < b) lo = mid + 1; else hi = mid;
    }
    bin_first[b] = lo;
}

// chunk_first[c] = the segment that holds the first byte of chunk c, for every chunk with bytes
__global__ void __launch_bounds__(256)
k_part_chunks(const uint64_t* __restrict__ dst_off, uint32_t n, uint32_t* __restrict__ chunk_first, uint64_t max_chunks) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = dst_off[n];
    if (c >= max_chunks || c * qpart::PART_CHUNK >= total) return;
    chunk_first[c] = qpart::find_segment([&](uint32_t j) { return dst_off[j]; }, 0u, n, c * qpart::PART_CHUNK);
}

// ---------------------------------------------------------------------------------------------
// d. the copy.  Workgroup c writes bytes [c * PART_CHUNK, (c + 1) * PART_CHUNK) of the output, lane l the vectors
// l, l + 256, ... of the chunk: a wave instruction stores 1 KiB of consecutive 16-byte vectors.  The chunk's segment
// boundaries and source positions go to the LDS; a lane finds a vector's segment there and gathers it from the two aligned
// source vectors around its source position (qpart::gather_vector).  The grid is sized by the INPUT's bases -- the
// output's size is known on the device only -- and a workgroup behind the output's end leaves at once.
// P planes (1: the bases; 2: bases and qualities, one byte per base on the same offsets, both allocations aligned alike):
// the LDS table, the segment search, the source offset, the shift and the byte masks of a destination vector are computed
// once and applied to P loads (or load pairs) and P stores (qpart::gather_vectors).  P = 1 ignores src1 / dst1.
// ---------------------------------------------------------------------------------------------
template <uint32_t P>
__global__ void __launch_bounds__(256)
k_part_copy(const uint64_t* __restrict__ dst_off, const uint64_t* __restrict__ src_pos, uint32_t n,
            const uint32_t* __restrict__ chunk_first, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
            const uint8_t* __restrict__ src1, uint8_t* __restrict__ dst1) {
    static_assert(P == 1 || P == 2, "one or two planes");
    __shared__ uint64_t s_off[qpart::PART_LDS_SEGS + 1];
    __shared__ uint64_t s_src[qpart::PART_LDS_SEGS];
    const uint64_t total = dst_off[n];
    const uint64_t c0 = (uint64_t)blockIdx.x * qpart::PART_CHUNK;
    if (c0 >= total) return;                       // (the same for every lane: nobody is left at a barrier)
    const uint64_t cend = c0 + qpart::PART_CHUNK < total ? c0 + qpart::PART_CHUNK : total;
    const auto goff = [&](uint32_t j) { return dst_off[j]; };
    const uint32_t jf = chunk_first[blockIdx.x];
    // the chunk's last segment lies at or in front of the next chunk's first
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
    const auto load16 = [&](uint32_t k, int64_t a) {           // (k is a constant after unrolling)
        const uint4 v = *reinterpret_cast<const uint4*>((k == 0 ? src : src1) + a);
        qpart::Vec16 o; o.w[0] = v.x; o.w[1] = v.y; o.w[2] = v.z; o.w[3] = v.w;
        return o;
    };
    for (uint32_t it = 0; it < qpart::PART_VECS_PER_LANE; ++it) {
        const uint64_t d0 = c0 + ((uint64_t)it * 256u + threadIdx.x) * qpart::PART_VEC;
        if (d0 >= cend) break;
        qpart::Vec16 v[P];
        if (in_lds)
            qpart::gather_vectors<P>([&](uint32_t j) { return s_off[j]; }, [&](uint32_t j) { return s_src[j]; }, load16, 0u, m, d0, total, v);
        else
            qpart::gather_vectors<P>(goff, [&](uint32_t j) { return src_pos[j]; }, load16, jf, jl + 1u, d0, total, v);
        *reinterpret_cast<uint4*>(dst + d0) = make_uint4(v[0].w[0], v[0].w[1], v[0].w[2], v[0].w[3]);
        if constexpr (P == 2) *reinterpret_cast<uint4*>(dst1 + d0) = make_uint4(v[P - 1].w[0], v[P - 1].w[1], v[P - 1].w[2], v[P - 1].w[3]);
    }
}

// ---------------------------------------------------------------------------------------------
// e. the offsets of a batch made from a caller's device memory (qcat_batch_from_device): offsets[0] == 0 and no entry below
// the one in front of it, n + 1 entries.  A grid-stride compare of neighbours; a lane that finds a fault stores 1 to *bad
// (every such store writes the same value; the host zeroes the flag before the launch).  No workgroup waits for another.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_offsets_check(const uint64_t* __restrict__ offsets, uint32_t n, uint32_t* __restrict__ bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        const bool wrong = i == 0 ? offsets[0] != 0 : offsets[i] < offsets[i - 1];
        if (wrong) *bad = 1u;
    }
}

}  // namespace qk

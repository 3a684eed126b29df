// kernels_filter.inc -- --filter-barcodes on records in device memory (qcat_scan_resident_batches with
// QCAT_RESIDENT_FILTER_BARCODES, qcat_filter_barcodes; the arithmetic: filter_core.h):
//   k_filter_hist    records of a batch -> table[batch][key], integer adds only
//   k_filter_floor   one workgroup per batch: the row's maximum -> floor[batch]
//   k_filter_apply   one thread per record: a called record whose key is not above the floor is stored as the empty record
// A workgroup reads the records of ONE batch (blockIdx.y), so nothing straddles a batch border.  The table and the floors are
// sums and maxima of integers: whatever order the adds arrive in, the bytes are the same run after run, and so are the records.
// Included by qcat_hip.hip.
#include "filter_core.h"

namespace qk {

// the key of a record on the device: filter_core.h's key_of over the kit's id slots -- the same bucket as dev_barcode_bucket
// (kernels_common.inc) gives a record's (barcode_idx, barcode2_idx, adapter_idx), `none` = the last barcode bucket
__device__ __forceinline__ uint32_t dev_filter_key(const KitPtrs& kp, const qcat_result& q) {
    const DevKit* k = kp.kit;
    return qfilt::key_of(q, k->mode == QCAT_MODE_DUAL, k->mode == QCAT_MODE_SIMPLE, (uint32_t)k->n_barcode_slots,
                         [&](int t, int s, int i) { return (uint32_t)kp.ids[k->tpl[t].sets[s].ids_off + i]; });
}

// grid (workgroups per batch, batches of this round); recs / n: the records from the round's first batch to the end of the
// call; table: n_bins counters per batch of the round, zeroed by the fill list in front of the launch.
// Rows of up to FILTER_LDS_BINS bins (every single and simple kit up to 1024 ids): a histogram in the LDS, then one global
// add per non-zero (workgroup, bin).  Longer rows (dual kits: 9 217 bins for the shipped 96 x 96 ids, up to 1024^2 + 1): the
// lanes of a wave that hold the same key are found with ballots -- as k_part_scatter finds equal digits -- and their first
// lane adds the group's size: one global add per distinct key per wave.
__global__ void __launch_bounds__(256)
k_filter_hist(KitPtrs kp, const qcat_result* __restrict__ recs, uint32_t n, uint32_t batch_reads, uint32_t n_bins, uint32_t key_bits,
              uint32_t* __restrict__ table) {
    __shared__ uint32_t hist[qfilt::FILTER_LDS_BINS];
    const bool lds = n_bins <= qfilt::FILTER_LDS_BINS;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x) hist[i] = 0;
        __syncthreads();
    }
    const uint64_t r0 = (uint64_t)blockIdx.y * batch_reads;
    const uint64_t r1 = r0 + batch_reads < (uint64_t)n ? r0 + batch_reads : (uint64_t)n;
    uint32_t* __restrict__ row = table + (size_t)blockIdx.y * n_bins;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = r0 + (uint64_t)blockIdx.x * 256u; base < r1; base += (uint64_t)gridDim.x * 256u) {     // (uniform: the ballots below)
        const uint64_t r = base + threadIdx.x;
        const bool live = r < r1;
        uint32_t key = live ? dev_filter_key(kp, recs[r]) : 0u;
        if (key >= n_bins) key = n_bins - 1u;                  // (a record that indexes outside the kit counts as `none`: nothing is added out of bounds)
        if (lds) {
            if (live) atomicAdd(&hist[key], 1u);
        } else {
            uint64_t same = __ballot(live);
            for (uint32_t b = 0; b < key_bits; ++b) {
                const uint64_t bal = __ballot((key >> b) & 1u);
                same &= ((key >> b) & 1u) ? bal : ~bal;
            }
            if (live && (same & ((1ull << lane) - 1ull)) == 0) atomicAdd(&row[key], (uint32_t)__popcll(same));
        }
    }
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x)
            if (hist[i]) atomicAdd(&row[i], hist[i]);
    }
}

// one workgroup per batch of the round: floor[batch] = int(max(row) * 0.05)
__global__ void __launch_bounds__(256)
k_filter_floor(const uint32_t* __restrict__ table, uint32_t n_bins, uint32_t* __restrict__ floor) {
    __shared__ uint32_t red[256];
    const uint32_t* __restrict__ row = table + (size_t)blockIdx.x * n_bins;
    uint32_t m = 0;
    for (uint32_t i = threadIdx.x; i < n_bins; i += 256u) m = max(m, row[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) floor[blockIdx.x] = (uint32_t)qfilt::floor_of(red[0]);
}

// one thread per record of the round (n records, batches of batch_reads): only the records that change are stored
__global__ void __launch_bounds__(256)
k_filter_apply(KitPtrs kp, qcat_result* __restrict__ recs, uint32_t n, uint32_t batch_reads, uint32_t n_bins,
               const uint32_t* __restrict__ table, const uint32_t* __restrict__ floor) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        qcat_result q = recs[r];
        const uint32_t key = dev_filter_key(kp, q);
        if (key >= n_bins - 1u) continue;                      // no call (or outside the kit): untouched
        const uint32_t batch = (uint32_t)(r / batch_reads);
        if (qfilt::survives(table[(size_t)batch * n_bins + key], floor[batch])) continue;
        qfilt::make_empty(q);
        recs[r] = q;
    }
}

}  // namespace qk

// filter_core.h -- the arithmetic of --filter-barcodes on the device (kernels_filter.inc, filter_host.inc), as pure functions
// that compile for host and device: the key of a record, the floor of a batch and the record a filtered call becomes.
// They restate get_valid(counts, 0.05) and filter_barcodes of the reference driver (qcat/scanner_base.py:690-712), the way
// fq_filter_batch (fastq_host.inc) does for the file loop.  tests/filter_check.cpp runs them on the host against a std::map
// restatement of its own.
//
// Vocabulary.  A batch is a run of consecutive records that is filtered on its own (the driver's 4000 reads).  The KEY of a
// record is its barcode bucket in the count vector -- the slot of the barcode's id, in dual mode slot1 * n_slots + slot2 --
// or `none` (the last bin) for a record without a call; the minimum-length rule plays no part.  Every key of a batch is
// counted, `none` included, and `none` can hold the maximum.  FLOOR = int(max * 0.05).  A called record whose key was counted
// `floor` times or fewer becomes the empty record; records without a call stay as they are.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QF_HD __host__ __device__ __forceinline__
#else
#define QF_HD static inline
#endif

namespace qfilt {

constexpr uint32_t FILTER_LDS_BINS = 2048;                     // bins of the workgroup histogram of k_filter_hist (8 KiB of LDS)

// bins of a batch's row: every key and `none` (= the last bin)
QF_HD uint32_t bins_of(bool dual, uint32_t n_slots) { return (dual ? n_slots * n_slots : n_slots) + 1u; }

// bits that hold a key below n_bins (the ballots of k_filter_hist)
QF_HD uint32_t key_bits(uint32_t n_bins) {
    uint32_t bits = 1;
    while (bits < 32 && (n_bins - 1) >> bits) ++bits;
    return bits;
}

// the key of a record.  slot(template, set, barcode index) is the id slot of a barcode of the kit; a record without an
// adapter has no call, except in simple mode, which has no adapters (its one list belongs to template 0)
template <class Rec, class Slot>
QF_HD uint32_t key_of(const Rec& q, bool dual, bool simple, uint32_t n_slots, const Slot& slot) {
    const uint32_t none = bins_of(dual, n_slots) - 1u;
    if (q.barcode_idx < 0 || (q.adapter_idx < 0 && !simple)) return none;
    const int t = q.adapter_idx < 0 ? 0 : q.adapter_idx;
    uint32_t key = slot(t, 0, (int)q.barcode_idx);
    if (dual) key = key * n_slots + slot(t, 1, (int)q.barcode2_idx);
    return key;
}

// int(max_barcode_count * 0.05): the same IEEE product and truncation as Python's
QF_HD uint64_t floor_of(uint64_t max_count) { return (uint64_t)((double)max_count * 0.05); }

// a key survives when it was counted strictly more often than the floor
QF_HD bool survives(uint64_t count, uint64_t floor) { return count > floor; }

// empty_return_dict() with the trims the driver takes from it
template <class Rec>
QF_HD void make_empty(Rec& q) {
    q.barcode_idx = -1; q.barcode2_idx = -1; q.adapter_idx = -1; q.adapter_end = 0; q.raw_score = 0; q.score_den = 1;
    q.exit_status = 1; q.trim5p = 0; q.trim3p = 0;
}

}  // namespace qfilt

// kernels_eval.inc -- the evaluation of a scanned text batch in device memory (qcat_batch_eval):
//   k_eval_classify   one lane per read and round, or (<EVAL_GROUP>, option EVAL_SHAPE) a group of eight lanes per read: the verdict of the minimum-length filter (dev_skipped: the partition's, as
//                     k_tsv_lengths), the title in aligned 16-byte vectors -- masks of its blanks and its '=', the tokens resolved
//                     from the masks --, the call's text from the id slots, the class byte, the ROC kind and the score bucket of
//                     the read; the (kind, bucket) and class counts of a workgroup in the LDS, then integer adds to global memory;
//                     a read that cannot be evaluated lowers the first-bad-read number
//   k_eval_roc        one workgroup: suffix sums of the counts, then one lane per threshold: the ROC table
// Integer adds only: the result is the same bytes run after run.  The arithmetic is eval_core.h's.  Included by qcat_hip.hip.
#include "eval_core.h"

namespace qk {

// hist: EVAL_HIST counters, zeroed by the host; bad: the smallest 1-based number of a read that cannot be evaluated, EVAL_NO_BAD
// before the launch.  `text` is 16-byte aligned and has the batch's slack on both sides.  from_comment: no kit, record or table
// is looked at.  GROUP = 1: one lane per read and round; GROUP = EVAL_GROUP: that many lanes per read -- they load a title's
// vectors side by side, exchange the masks inside the group (__shfl: a group's lanes share their read and so their control
// flow) and resolve them redundantly; the group's first lane judges and writes.
template <uint32_t GROUP>
__global__ void __launch_bounds__(qev::EVAL_THREADS)
k_eval_classify(KitPtrs kp, qtsv::Tables T, const qcat_result* __restrict__ results, const uint64_t* __restrict__ offsets,
                const uint8_t* __restrict__ text, const qfq::Rec* __restrict__ recs, uint32_t n, uint32_t from_comment,
                uint8_t* __restrict__ cls, uint8_t* __restrict__ kind, uint16_t* __restrict__ bucket, uint32_t* __restrict__ hist,
                uint32_t* __restrict__ bad) {
    static_assert(GROUP == 1 || GROUP == qev::EVAL_GROUP, "one lane or a group per read");
    __shared__ uint32_t s_hist[qev::EVAL_HIST];
    for (uint32_t i = threadIdx.x; i < qev::EVAL_HIST; i += qev::EVAL_THREADS) s_hist[i] = 0;
    __syncthreads();
    const auto load16 = [&](uint64_t a) {
        const uint4 q = *reinterpret_cast<const uint4*>(text + a);
        qpart::Vec16 v; v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
        return v;
    };
    const uint32_t per_block = qev::EVAL_THREADS / GROUP, gl = threadIdx.x % GROUP;
    for (uint64_t r = (uint64_t)blockIdx.x * per_block + threadIdx.x / GROUP; r < n; r += (uint64_t)gridDim.x * per_block) {
        qcat_result res;
        res.barcode_idx = res.barcode2_idx = res.adapter_idx = -1; res.raw_score = 0; res.score_den = 1;
        if (!from_comment) {
            res = results[r];
            const int64_t len = (int64_t)(offsets[r + 1] - offsets[r]);
            if (dev_skipped(kp.kit, len, res.trim5p, res.trim3p)) {
                if (gl == 0) { cls[r] = qev::CLS_DROPPED; kind[r] = 0; bucket[r] = 0; }
                continue;
            }
        }
        const qfq::Rec rec = recs[r];
        qev::Verdict v;
        if (GROUP == 1)
            v = qev::read_verdict(T, text, load16, rec.title_off, rec.title_len, from_comment != 0, res.barcode_idx, res.barcode2_idx,
                                  res.adapter_idx, res.raw_score, res.score_den);
        else
            v = qev::read_verdict_group(T, text, load16, [](uint32_t m, uint32_t k, uint64_t) { return (uint32_t)__shfl((int)m, (int)k, (int)GROUP); },
                                        gl, rec.title_off, rec.title_len, from_comment != 0, res.barcode_idx, res.barcode2_idx,
                                        res.adapter_idx, res.raw_score, res.score_den);
        if (gl != 0) continue;
        cls[r] = v.cls; kind[r] = v.kind; bucket[r] = v.bucket;
        if (v.cls & qev::CLS_BAD) { atomicMin(bad, (uint32_t)r + 1u); continue; }
        atomicAdd(&s_hist[qev::hist_slot(v.kind, v.bucket)], 1u);
        atomicAdd(&s_hist[qev::class_slot(v.cls)], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < qev::EVAL_HIST; i += qev::EVAL_THREADS) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// roc: EVAL_Q rows of EVAL_ROC_COLS.  The counts go to the LDS, one lane per kind turns them into suffix sums in one pass, then
// one lane per threshold reads its row off them.
__global__ void __launch_bounds__(qev::EVAL_ROC_THREADS)
k_eval_roc(const uint32_t* __restrict__ hist, int64_t* __restrict__ roc) {
    __shared__ uint32_t s_hist[qev::EVAL_KINDS * qev::EVAL_BUCKETS];
    __shared__ uint32_t s_suf[qev::EVAL_KINDS][qev::EVAL_BUCKETS + 1];
    for (uint32_t i = threadIdx.x; i < qev::EVAL_KINDS * qev::EVAL_BUCKETS; i += qev::EVAL_ROC_THREADS) s_hist[i] = hist[i];
    __syncthreads();
    if (threadIdx.x < qev::EVAL_KINDS)
        qev::suffix_sums([&](uint32_t i) { return s_hist[i]; }, threadIdx.x, [&](uint32_t b, uint32_t v) { s_suf[threadIdx.x][b] = v; });
    __syncthreads();
    const uint32_t q = threadIdx.x;
    if (q >= qev::EVAL_Q) return;
    int64_t row[qev::EVAL_ROC_COLS];
    qev::roc_row([&](uint32_t k, uint32_t b) { return s_suf[k][b]; }, q, row);
    for (uint32_t i = 0; i < qev::EVAL_ROC_COLS; ++i) roc[(uint64_t)q * qev::EVAL_ROC_COLS + i] = row[i];
}

}  // namespace qk

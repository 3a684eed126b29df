// pipeline.h -- qcat_scan_batch from HOST buffers as a three-stage pipeline over chunks of the
// batch (replaces: the per-read loop of cli.qcat_cli over detect_barcode, qcat/cli.py:504-513, whose
// reads live in host memory):
//
//     host threads : compact chunk k+1 to its scanned windows (head + tail of every read) into pinned memory
//     copy stream  : H2D of chunk k   (windows, offsets, real lengths: <= 300 B + 12 B per read)
//     scan stream  : the kernels of chunk k-1, then D2H of its 24-byte records into pinned memory
//
// so a call costs max(host compaction, PCIe, GPU) instead of their sum.  Everything it needs is owned
// by the context and reused: a persistent worker pool, two pinned staging sets, two device chunk sets,
// their pinned record buffers (all sized by the chunk, not by the batch) -- no hipMalloc / hipFree / thread start per call once warm, and one host
// synchronisation at the end.  The count vector accumulates on the device across the chunks.
// The types are here; the steps that need no device (pool, cuts, sizing, lengths, compaction) in pipeline_core.h, checked on
// the CPU by tests/pipeline_check.cpp; the function itself, scan_batch_pipelined, in pipeline_host.inc.
// Included by qcat_hip.hip.
#pragma once
#include "pipeline_core.h"

namespace qk {

struct PipeStage {                     // one of the two chunk slots
    PinBuf<uint8_t> pin_bases; PinBuf<uint64_t> pin_offsets; PinBuf<uint32_t> pin_len;
    DevBuf<uint8_t> dev_bases_alloc; DevBuf<uint64_t> dev_offsets; DevBuf<uint32_t> dev_len;
    PinBuf<qcat_result> pin_results;                    // the chunk's records on their way to the caller's array
    uint32_t res_first = 0, res_count = 0;              // ... reads [res_first, res_first + res_count), 0: nothing pending
    hipEvent_t copied = nullptr, scanned = nullptr;
};

struct HostPipeline {
    HostPool* pool = nullptr;
    PipeStage st[2];
    hipStream_t copy = nullptr;
};

static inline void pipeline_free(HostPipeline* p) {
    if (!p) return;
    delete p->pool;
    for (PipeStage& s : p->st) {
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.scanned) (void)hipEventDestroy(s.scanned);
    }
    if (p->copy) (void)hipStreamDestroy(p->copy);
    delete p;                          // (the stages' staging buffers free themselves)
}

// one read of a mapped FASTQ / FASTA file (fastq_host.inc, fastq_stream.inc) -- title: offset of the byte after '@'; seq, qual:
// offsets of the sequence / quality lines; title_len after rstrip; seq_len == quality length
struct FqRec { uint64_t title, seq, qual; uint32_t title_len, seq_len; };

}  // namespace qk

// where the reads of a host batch lie: concatenated (bases + offsets, the form of qcat_scan_batch) or scattered through a
// mapped FASTQ file (one FqRec per read, fastq_host.inc) -- the pipeline only ever reads head and tail of a read in place
struct ReadView {
    const uint8_t* bases;
    const uint64_t* offsets;           // concatenated form (recs == nullptr)
    const qk::FqRec* recs;             // FASTQ form: bases = the mapping, read r = recs[r]
    inline uint64_t start(uint32_t r) const { return recs ? recs[r].seq : offsets[r]; }
    inline const uint8_t* src(uint32_t r) const { return bases + start(r); }
    inline uint64_t len(uint32_t r) const { return recs ? (uint64_t)recs[r].seq_len : offsets[r + 1] - offsets[r]; }
    inline bool decreasing(uint32_t r) const { return !recs && offsets[r + 1] < offsets[r]; }     // (the caller's offsets: refused)
};

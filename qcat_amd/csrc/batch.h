// batch.h -- the resident batch (reads in device memory) and what belongs to it on the host (host only, like dev_buf.h): the
// type behind qcat_batch*, its two makers' building blocks -- an owned batch allocates its planes, a view borrows a context's
// staging -- the guard of a batch under construction, and the scratch of the calls over a batch: the partition, the filter, the
// text parse, the three text products (their shared types: text_out.h) and the evaluation.  The functions are in batch_host.inc and the host
// files named at each scratch.  Included by qcat_hip.hip in front of middle_host.inc.
#pragma once
#include <memory>
#include <vector>

#include "../../include/qcat_hip.h"
#include "dev_buf.h"
#include "partition_core.h"
#include "fqtext_core.h"
#include "tsvtext_core.h"
#include "text_out.h"

constexpr size_t BATCH_SLACK = 64;                 // bytes in front of and behind a batch's bases
static_assert(BATCH_SLACK == qpart::PART_SLACK, "the partition's copy kernel relies on the batches' slack");

struct qcat_batch {
    int device = 0;
    uint32_t n_reads = 0;
    uint64_t n_bases = 0;
    uint8_t* bases = nullptr;      // BATCH_SLACK bytes into an allocation of BATCH_SLACK + n_bases + BATCH_SLACK bytes: k_pack_windows
                                   // reads whole aligned dwords up to 19 bytes before / after a read's window
    uint8_t* quals = nullptr;      // the quality plane (null: none): one byte per base on the same offsets, an allocation of its own
                                   // laid out like the bases'; no scan reads it, the partition moves it with the bases
    uint64_t* offsets = nullptr;   // n_reads + 1
    uint32_t* true_len = nullptr;  // window-only batches (batch_upload_windows): the reads' real lengths
    // a batch parsed from FASTQ text on the device (qcat_batch_upload_fastq_text, fqtext_host.inc; null: none): the text plane --
    // BATCH_SLACK bytes into an allocation of BATCH_SLACK + text_bytes + qfq::FQ_CONST_BYTES + BATCH_SLACK bytes, the titles as the
    // writers print them (tabs are blanks), the constants block behind the text -- and the record table, one entry per read
    uint8_t* text = nullptr;
    uint64_t text_bytes = 0;
    qfq::Rec* text_recs = nullptr;
    bool text_fasta = false;       // the text is FASTA (qcat_batch_upload_text): two lines per record, qual_off = 0, no quality part

    // the planes of a batch that owns its memory (fixed size, the caller's: no generation bump); a view -- the device buffers
    // belong to a context (host-buffer calls) or a pipeline stage -- leaves them empty, and destroying it frees the shell only
    struct Store {
        qk::FixedBuf<uint8_t> bases, quals;
        qk::FixedBuf<uint64_t> offsets;
        qk::FixedBuf<uint8_t> text;
        qk::FixedBuf<qfq::Rec> text_recs;
    } store;
    bool owned() const { return store.bases.get() != nullptr; }

    // the device arrays of an owned batch of n_reads reads and n_bases bases; with_quals: a quality plane as well
    bool alloc(bool with_quals) {
        const hipError_t e1 = store.bases.ensure(n_bases + 2 * BATCH_SLACK);
        const hipError_t e2 = store.offsets.ensure((size_t)n_reads + 1);
        const hipError_t e3 = with_quals ? store.quals.ensure(n_bases + 2 * BATCH_SLACK) : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return false;
        bases = store.bases + BATCH_SLACK;
        offsets = store.offsets;
        if (with_quals) quals = store.quals + BATCH_SLACK;
        return true;
    }
};

// a view of memory that is somebody else's: `bases` points BATCH_SLACK bytes into its allocation
static inline qcat_batch batch_view(int device, uint32_t n_reads, uint64_t n_bases, uint8_t* bases, uint64_t* offsets, uint32_t* true_len) {
    qcat_batch v;
    v.device = device; v.n_reads = n_reads; v.n_bases = n_bases;
    v.bases = bases; v.offsets = offsets; v.true_len = true_len;
    return v;
}

extern "C" void qcat_batch_destroy(qcat_batch* b);
// owns a batch under construction, or a call's batch: destroyed on every early return, handed over with release()
struct BatchDeleter { void operator()(qcat_batch* b) const { qcat_batch_destroy(b); } };
using BatchPtr = std::unique_ptr<qcat_batch, BatchDeleter>;

// qcat_batch_partition (kernels_partition.inc): keys, the radix sort's two (key, read index) buffers, histogram table, block
// sums of the scans, slices, the copy's tables; `source` / `bins` belong to the latest partition
struct PartScratch {
    qk::DevBuf<uint32_t> key[2], idx[2], hist, sums32, chunk_first;
    qk::DevBuf<uint64_t> start, keep, src_pos, sums64, bins;
    uint32_t* source = nullptr;                // = idx[passes & 1] of the latest partition
    uint32_t n_reads = 0;
    int32_t n_bins = 0;                        // 0: no partition yet
};
// --filter-barcodes on the device (kernels_filter.inc, filter_host.inc): the key counters of a round of batches, a floor per
// batch of the round, and the records of a caller that holds them on the host (qcat_filter_barcodes)
struct FilterScratch {
    qk::DevBuf<uint32_t> table, floor;
    qk::DevBuf<qcat_result> recs;
};
// FASTQ text on the device (kernels_fqtext.inc, fqtext_host.inc): the parse's block counts, line table, status and copy tables;
// the segment table, the text of the latest qcat_batch_demux_text (text.first: the first byte of every record in sorted order)
// and its arrays of its own (`source`: a copy of the partition scratch's sorted order, which the next partition overwrites)
struct FqTextScratch {
    qk::DevBuf<uint64_t> counts, sums, line_start, seq_src, status;
    qk::DevBuf<uint32_t> chunk_first;
    qk::DevBuf<uint64_t> seg_off, seg_src, bin_bytes;
    qk::DevBuf<uint32_t> source;
    TextOut text;
    int32_t n_bins = 0;                        // bins of `text`
};
// the TSV rows of a text batch (kernels_tsvtext.inc, tsvtext_host.inc), scratch of their own: the latest qcat_batch_tsv_text keeps
// its text (text.first: the rows) beside the latest demultiplexed text.  The tables' blob on the device beside its host copy;
// the score part of the kit with serial `score_kit` (0: none)
struct TsvScratch {
    qk::DevBuf<uint64_t> sums;
    qk::DevBuf<uint32_t> name_len, keep, tile_first, bad;
    MirroredTable tables;
    TextOut text;
    qtsv::ScoreTable scores;
    uint64_t score_kit = 0;
};
// the annotated single stream of a text batch (kernels_textstream.inc, textstream_host.inc), scratch of its own beside the
// demultiplexed text and the TSV text: the segment table and the stream of the latest qcat_batch_annot_text (text.first: the
// records); the tag plane (BATCH_SLACK, the TSV tables' blob, the stream's constants, BATCH_SLACK) on the device beside its host copy
struct AnnotScratch {
    qk::DevBuf<uint64_t> seg_off, seg_src, sums;
    qk::DevBuf<uint32_t> chunk_first;
    MirroredTable tags;
    TextOut text;
};
// the evaluation of a text batch (kernels_eval.inc, eval_host.inc), scratch of its own beside the three texts: the planes, the
// counts and the ROC table of the latest qcat_batch_eval (valid: a failed call leaves none behind); the id slots' blob on the
// device beside its host copy
struct EvalScratch {
    qk::DevBuf<uint8_t> cls, kind;
    qk::DevBuf<uint16_t> bucket;
    qk::DevBuf<uint32_t> hist, bad;
    qk::DevBuf<int64_t> roc;
    MirroredTable tables;
    uint32_t n_reads = 0;
    bool valid = false;
};
// what a context keeps for the batch functions
struct BatchScratch {
    PartScratch part;
    FilterScratch filter;
    FqTextScratch fqtext;
    TsvScratch tsv;
    AnnotScratch annot;
    EvalScratch eval;
    qk::DevBuf<qcat_result> recs;              // records a caller handed over, of whichever call runs (records_on_device, text_out_host.inc)
    qk::DevBuf<uint32_t> offs_bad;             // qcat_batch_from_device: the flag of k_offsets_check
};

// fqtext_host.inc -- FASTQ text in device memory (the kernels: kernels_fqtext.inc; the arithmetic: fqtext_core.h):
//   qcat_batch_upload_fastq_text   the bytes of a FASTQ file go up; a resident batch with bases, offsets, a text plane and a record
//                                  table comes out of four device passes -- count, lines, records, the bases' copy -- with the
//                                  verdict of fq_parse (fastq_host.inc) on every record
//   qcat_batch_upload_text         the driver's dispatch by the first byte: '>' is FASTA -- the same passes with k_fa_records
//                                  (kernels_textstream.inc) and two lines per record --, anything else the call above
//   qcat_batch_demux_text          the per-barcode FASTQ files' bytes of a scanned text batch: the partition's keys and order, a
//                                  segment table of six byte ranges per read (a FASTA batch: k_fa_segments, the .fasta files'
//                                  bytes), the partition's scan chain and copy kernel
//   qcat_ctx_fetch_demux_text / _demux_text_devptr / qcat_batch_fetch_text_records   read-out
// The demultiplexed text's argument check, its tail and its read-out are the text products' shared layer (text_out_host.inc);
// here are its bounds, its own arrays (bin_bytes, source) and its launches.
// Included by qcat_hip.hip behind batch_host.inc and text_out_host.inc: it uses their helpers and the partition's phases.

static int fq_text_refused(uint64_t record) {
    return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_upload_fastq_text: not a plain four-line FASTQ file (record " + std::to_string(record) + ")");
}

static int fa_text_refused(uint64_t record) {
    return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_upload_text: not a plain two-line FASTA file (record " + std::to_string(record) + ")");
}

// the parse of both formats: `fasta` -- two lines per record, k_fa_records and its blame rule (fqtext_core.h) -- or FASTQ; fn: the
// entry point's name in front of the messages
static int text_upload(qcat_ctx* c, const uint8_t* text, uint64_t n_bytes, qcat_batch** out, bool fasta, const std::string& fn) {
    HIPCHK(hipSetDevice(c->device));
    FqTextScratch& T = c->batch.fqtext;
    BatchPtr b(new qcat_batch());
    b->device = c->device;
    int rc;
    // the text plane: slack, text, constants, slack
    if (b->store.text.ensure(n_bytes + qfq::FQ_CONST_BYTES + 2 * BATCH_SLACK) != hipSuccess)
        return set_err(QCAT_ERR_NOMEM, "hipMalloc failed for the text plane");
    b->text = b->store.text + BATCH_SLACK;
    b->text_bytes = n_bytes;
    b->text_fasta = fasta;
    uint8_t tail[qfq::FQ_CONST_BYTES + BATCH_SLACK];
    memset(tail, 0, sizeof tail);
    qfq::fq_constants(tail);
    HIPCHK(hipMemsetAsync(b->store.text, 0, BATCH_SLACK, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->text + n_bytes, tail, sizeof tail, hipMemcpyHostToDevice, c->stream));
    if (n_bytes) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->text, text, n_bytes, hipMemcpyHostToDevice, c->stream));
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    // a. newlines per block, their scan; the host sizes the line table by the total
    const uint64_t n_blocks = qfq::blocks_of(n_bytes);
    if (n_blocks >= (1ull << 31)) { (void)hipStreamSynchronize(c->stream); return set_err(QCAT_ERR_UNSUPPORTED, fn + ": text too large (>= 2^45 bytes)"); }
    uint64_t newlines = 0;
    if (n_blocks) {
        if ((rc = grow(T.counts, (size_t)n_blocks + 1)) || (rc = grow(T.sums, part_scan_sums(n_blocks + 1)))) { (void)hipStreamSynchronize(c->stream); return rc; }
        hipLaunchKernelGGL(k_fq_count, dim3((uint32_t)n_blocks), dim3(256), 0, c->stream, (const uint8_t*)b->text, n_bytes, T.counts.get());
        part_scan_launch<uint64_t>(T.counts, n_blocks + 1, T.sums, c->stream);
        mark(c, "fq_count");
        HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&newlines, T.counts + n_blocks, 8, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = stream_done(c, fn.c_str()))) return rc;
    const uint64_t n_lines = n_bytes ? qfq::lines_of(newlines, text[n_bytes - 1] == '\n') : 0;
    const uint64_t n_rec64 = fasta ? qfq::fa_records_of(n_lines) : qfq::records_of(n_lines);
    if (n_rec64 >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, fn + ": more than 2^31 records in one text");
    const uint32_t n = (uint32_t)n_rec64;
    // b. line table and byte classes; c. records, their lengths' scan = the offsets
    if ((rc = grow(T.line_start, (size_t)newlines + 2)) || (rc = grow(T.status, 1)) || (rc = grow(T.seq_src, n)) ||
        (rc = grow(T.sums, part_scan_sums(std::max<uint64_t>(n_blocks, n) + 1)))) return rc;
    if (b->store.text_recs.ensure(n) != hipSuccess || b->store.offsets.ensure((size_t)n + 1) != hipSuccess)
        return set_err(QCAT_ERR_NOMEM, "hipMalloc failed for batch");
    b->text_recs = b->store.text_recs;
    uint64_t* const offsets = b->store.offsets;
    FqStatus* const status = reinterpret_cast<FqStatus*>(T.status.get());
    HIPCHK(hipMemsetAsync(status, 0xFF, sizeof(FqStatus), c->stream));
    if (n_blocks) hipLaunchKernelGGL(k_fq_lines, dim3((uint32_t)n_blocks), dim3(256), 0, c->stream, (const uint8_t*)b->text, n_bytes,
                                     (const uint64_t*)T.counts.get(), n_blocks, T.line_start.get(), status);
    mark(c, "fq_lines");
    if (fasta) hipLaunchKernelGGL(k_fa_records, dim3(n / 256 + 1), dim3(256), 0, c->stream, b->text, (const uint64_t*)T.line_start.get(), n_lines, n,
                                  b->text_recs, offsets, T.seq_src.get(), status);
    else hipLaunchKernelGGL(k_fq_records, dim3(n / 256 + 1), dim3(256), 0, c->stream, b->text, (const uint64_t*)T.line_start.get(), n_lines, n,
                            b->text_recs, offsets, T.seq_src.get(), status);
    part_scan_launch<uint64_t>(offsets, (uint64_t)n + 1, T.sums, c->stream);
    mark(c, "fq_records");
    uint64_t back[2] = {0, 0};                                 // status, number of bases
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&back[0], status, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&back[1], offsets + n, 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stream_done(c, fn.c_str()))) return rc;
    if (back[0] != qfq::FQ_NO_LINE) return fasta ? fa_text_refused(qfq::fa_record_of_line(back[0])) : fq_text_refused(back[0] / 4 + 1);
    // d. the bases: the partition's copy over the text plane, segment r = the sequence line of read r
    b->n_reads = n; b->n_bases = back[1];
    if (b->n_bases > n_bytes) return set_err(QCAT_ERR_DEVICE, fn + ": more bases than text");
    if (!b->alloc(false)) return set_err(QCAT_ERR_NOMEM, "hipMalloc failed for batch");
    const uint64_t chunks = qpart::chunks_of(b->n_bases);
    if ((rc = grow(T.chunk_first, (size_t)chunks + 1))) return rc;
    if (chunks) {
        hipLaunchKernelGGL(k_part_chunks, dim3((uint32_t)((chunks + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t*)b->offsets, n,
                           T.chunk_first.get(), chunks);
        hipLaunchKernelGGL(k_part_copy<1>, dim3((uint32_t)chunks), dim3(256), 0, c->stream, (const uint64_t*)b->offsets,
                           (const uint64_t*)T.seq_src.get(), n, (const uint32_t*)T.chunk_first.get(), (const uint8_t*)b->text, b->bases,
                           (const uint8_t*)nullptr, (uint8_t*)nullptr);
    }
    mark(c, "fq_bases");
    if ((rc = stream_done(c, fn.c_str()))) return rc;
    *out = b.release();
    return 0;
}

extern "C" int qcat_batch_upload_fastq_text(qcat_ctx* c, const uint8_t* text, uint64_t n_bytes, qcat_batch** out) {
    if (!c || !out || (!text && n_bytes)) return set_err(QCAT_ERR_ARG, "qcat_batch_upload_fastq_text: null argument");
    if (n_bytes && text[0] == '>')
        return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_upload_fastq_text: FASTA text is not supported, the text must be FASTQ (record 1)");
    return text_upload(c, text, n_bytes, out, false, "qcat_batch_upload_fastq_text");
}

// the driver's dispatch (qcat/cli.py:248-262): a first byte '>' is FASTA, anything else goes the FASTQ way
extern "C" int qcat_batch_upload_text(qcat_ctx* c, const uint8_t* text, uint64_t n_bytes, qcat_batch** out) {
    if (!c || !out || (!text && n_bytes)) return set_err(QCAT_ERR_ARG, "qcat_batch_upload_text: null argument");
    if (n_bytes && text[0] == '>') return text_upload(c, text, n_bytes, out, true, "qcat_batch_upload_text");
    return qcat_batch_upload_fastq_text(c, text, n_bytes, out);
}

extern "C" int qcat_batch_text_is_fasta(const qcat_batch* b) {
    if (!b) return set_err(QCAT_ERR_ARG, "qcat_batch_text_is_fasta: null batch");
    if (!b->text) return set_err(QCAT_ERR_ARG, "qcat_batch_text_is_fasta: the batch has no text plane");
    return b->text_fasta ? 1 : 0;
}

extern "C" int qcat_batch_fetch_text_records(qcat_ctx* c, const qcat_batch* b, uint64_t* title_off, uint32_t* title_len,
                                             uint64_t* seq_off, uint32_t* seq_len) {
    if (!c || !b) return set_err(QCAT_ERR_ARG, "qcat_batch_fetch_text_records: null argument");
    if (!b->text) return set_err(QCAT_ERR_ARG, "qcat_batch_fetch_text_records: the batch has no text plane");
    HIPCHK(hipSetDevice(c->device));
    std::vector<qfq::Rec> recs(b->n_reads);
    if (b->n_reads) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(recs.data(), b->text_recs, (size_t)b->n_reads * sizeof(qfq::Rec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t r = 0; r < b->n_reads; ++r) {
        if (title_off) title_off[r] = recs[r].title_off;
        if (title_len) title_len[r] = recs[r].title_len;
        if (seq_off) seq_off[r] = recs[r].seq_off;
        if (seq_len) seq_len[r] = recs[r].seq_len;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// per-barcode FASTQ text of a scanned text batch
// ------------------------------------------------------------------------------------------
static int fq_demux_check(const qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records, uint32_t flags, const uint64_t* n_text_bytes) {
    if (int rc = batch_call_check(c, ckit, b, records, flags, n_text_bytes, "qcat_batch_demux_text", "qcat_batch_upload_fastq_text")) return rc;
    if (records && !part_records_fit(ckit->hk.dk, records, b->n_reads))
        return set_err(QCAT_ERR_ARG, "qcat_batch_demux_text: a record indexes outside the kit's templates / barcode sets or has a negative trim");
    if ((uint64_t)qfq::FQ_SEGS * b->n_reads >= (1ull << 32))
        return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_demux_text: batch too large (6 segments per read, >= 2^32 segments)");
    return 0;
}

extern "C" int qcat_batch_demux_text(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                                     uint32_t flags, uint64_t* n_text_bytes) {
    int rc = fq_demux_check(c, ckit, b, records, flags, n_text_bytes);
    if (rc) return rc;
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return rc;
    PartJob j{};
    j.in = b; j.n = b->n_reads;
    j.kp = KitPtrs{kd->kit, kd->codes, kd->ids, kd->tables};
    j.n_bins = (uint32_t)part_bins_of(kit->hk.dk);
    j.passes = qpart::key_passes(j.n_bins);
    j.n_wg = (j.n + PART_SORT_TILE - 1) / PART_SORT_TILE;
    // the output's size is known on the device only: the grid and the buffer follow an upper bound (qfq::output_bound)
    const uint64_t bound = qfq::output_bound(b->text_bytes, j.n);
    j.max_chunks = qpart::chunks_of(bound);
    if (j.max_chunks >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_demux_text: text too large (>= 2^46 bytes)");
    PartScratch& P = c->batch.part;
    FqTextScratch& T = c->batch.fqtext;
    P.n_bins = 0; P.source = nullptr;                        // (the partition's scratch is taken: no partition is left behind)
    T.text.valid = false;
    const uint32_t n = j.n, n_segs = qfq::FQ_SEGS * n;
    if ((rc = part_size_buffers(c, j, records))) return rc;
    if ((rc = grow(T.seg_off, (size_t)n_segs + 1)) || (rc = grow(T.seg_src, n_segs)) || (rc = grow(T.sums, part_scan_sums((uint64_t)n_segs + 1))) ||
        (rc = grow(T.text.first, (size_t)n + 1)) || (rc = grow(T.bin_bytes, (size_t)j.n_bins + 1)) || (rc = grow(T.text.buf, bound + 2 * BATCH_SLACK)) ||
        (rc = grow(T.source, n))) {
        (void)hipStreamSynchronize(c->stream);               // (the caller's records may be on their way)
        return rc;
    }
    uint8_t* const dst = text_out_ptr(T.text);
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    part_keys(c, j);
    part_order(c, j);
    if (n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(T.source, j.source, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_part_bins, dim3(j.n_bins / 256 + 1), dim3(256), 0, c->stream, j.key_sorted, n, j.n_bins, P.bins.get());
    if (b->text_fasta)
        hipLaunchKernelGGL(k_fa_segments, dim3(n / 256 + 1), dim3(256), 0, c->stream, (const uint32_t*)j.source, j.key_sorted,
                           (const uint64_t*)P.start.get(), (const uint64_t*)P.keep.get(), (const uint64_t*)b->offsets, (const qfq::Rec*)b->text_recs, n,
                           j.n_bins - 1, b->text_bytes, T.seg_off.get(), T.seg_src.get());
    else
    hipLaunchKernelGGL(k_fq_segments, dim3(n / 256 + 1), dim3(256), 0, c->stream, (const uint32_t*)j.source, j.key_sorted,
                       (const uint64_t*)P.start.get(), (const uint64_t*)P.keep.get(), (const uint64_t*)b->offsets, (const qfq::Rec*)b->text_recs, n,
                       j.n_bins - 1, b->text_bytes, T.seg_off.get(), T.seg_src.get());
    part_scan_launch<uint64_t>(T.seg_off, (uint64_t)n_segs + 1, T.sums, c->stream);
    hipLaunchKernelGGL(k_fq_firsts, dim3(std::max(n, j.n_bins) / 256 + 1), dim3(256), 0, c->stream, (const uint64_t*)T.seg_off.get(), n,
                       (const uint64_t*)P.bins.get(), j.n_bins, T.text.first.get(), T.bin_bytes.get());
    hipLaunchKernelGGL(k_part_chunks, dim3((uint32_t)((j.max_chunks + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t*)T.seg_off.get(), n_segs,
                       P.chunk_first.get(), j.max_chunks);
    mark(c, "text_segments");
    hipLaunchKernelGGL(k_part_copy<1>, dim3((uint32_t)j.max_chunks), dim3(256), 0, c->stream, (const uint64_t*)T.seg_off.get(),
                       (const uint64_t*)T.seg_src.get(), n_segs, (const uint32_t*)P.chunk_first.get(), (const uint8_t*)b->text, dst,
                       (const uint8_t*)nullptr, (uint8_t*)nullptr);
    mark(c, "text_copy");
    T.n_bins = (int32_t)j.n_bins;
    return text_out_finish(c, T.text, T.seg_off + n_segs, n, bound, "qcat_batch_demux_text", n_text_bytes);
}

extern "C" int qcat_ctx_fetch_demux_text(qcat_ctx* c, uint8_t* text, uint64_t cap, uint64_t* bin_first_bytes, int32_t n_bins,
                                         uint64_t* rec_first, uint32_t* source) {
    const FqTextScratch* T = c ? &c->batch.fqtext : nullptr;
    int rc = text_out_fetch_check(c, T ? &T->text : nullptr, text, cap, "qcat_ctx_fetch_demux_text", "no demultiplexed text");
    if (rc) return rc;
    if (bin_first_bytes && n_bins != T->n_bins) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_demux_text: bin count does not match the latest text");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = text_out_fetch_copies(c, T->text, text, nullptr))) return rc;                     // (the copies in the order they always had)
    if (bin_first_bytes) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(bin_first_bytes, T->bin_bytes, ((size_t)T->n_bins + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = text_out_fetch_copies(c, T->text, nullptr, rec_first))) return rc;
    if (source && T->text.n_reads) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(source, T->source, (size_t)T->text.n_reads * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" void* qcat_ctx_demux_text_devptr(qcat_ctx* c) { return text_out_devptr(c ? &c->batch.fqtext.text : nullptr); }

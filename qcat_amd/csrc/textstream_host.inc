// textstream_host.inc -- the driver's annotated single stream of a scanned text batch in device memory (the kernels:
// kernels_textstream.inc; the arithmetic and the tag plane's layout: textstream_core.h):
//   qcat_batch_annot_text      every kept read in read order with " barcode=<id>" behind its title, as FqWriter::write_range
//                              (fastq_host.inc, the !to_dir branch) writes it to out_fd: a segment table of ten byte ranges per read,
//                              the partition's scan chain and chunk table, the two-plane copy
//   qcat_ctx_fetch_annot_text / qcat_ctx_annot_text_devptr   read-out
// The id texts are the id slots of the TSV tables' blob (name_tables_build without scores: no score slots); the blob, the
// stream's constants and the copy's slack make the tag plane, which is uploaded when it differs from the one on the device (a
// MirroredTable).
// The argument check, the name tables, the records, the tail and the read-out are the text products' shared layer
// (text_out_host.inc); here are the tag plane's layout, the bound, the stream's own arrays and the launches.
// Included by qcat_hip.hip behind tsvtext_host.inc: it uses the helpers of batch_host.inc.

extern "C" int qcat_batch_annot_text(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                                     const qcat_tsv_names* names, uint32_t flags, uint64_t* n_text_bytes) {
    const std::string fn = "qcat_batch_annot_text";
    int rc = batch_call_check(c, ckit, b, records, flags, n_text_bytes, fn, "qcat_batch_upload_text");
    if (rc) return rc;
    if ((uint64_t)qann::ANNOT_SEGS * b->n_reads >= (1ull << 32))
        return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_annot_text: batch too large (10 segments per read, >= 2^32 segments)");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    AnnotScratch& A = c->batch.annot;
    // the tables: the ids of the caller's name tables, no kit names and no scores (the stream prints neither)
    std::vector<uint8_t> plane;
    qtsv::Tables T;
    uint32_t den_off = 0;
    if ((rc = name_tables_build(kit->hk.dk, names, nullptr, fn, &plane, &T, &den_off))) return rc;
    // the tag plane: slack, blob, constants, slack
    const uint64_t const_off = qann::tag_const_off(plane.size());
    plane.resize((size_t)qann::tag_plane_bytes(plane.size()) + BATCH_SLACK, 0);
    qann::annot_constants(plane.data() + const_off);
    plane.insert(plane.begin(), BATCH_SLACK, 0);
    const uint32_t n = b->n_reads, n_segs = qann::ANNOT_SEGS * n;
    const uint64_t bound = qann::output_bound(b->text_bytes, n, T);
    const uint64_t max_chunks = qpart::chunks_of(bound);
    if (max_chunks >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_annot_text: text too large (>= 2^46 bytes)");
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return rc;
    A.text.valid = false;
    const bool fresh_plane = A.tags.stale(plane);  // (once per kit and name tables)
    if ((rc = grow(A.tags.dev, plane.size())) || (rc = grow(A.seg_off, (size_t)n_segs + 1)) || (rc = grow(A.seg_src, n_segs)) ||
        (rc = grow(A.sums, part_scan_sums((uint64_t)n_segs + 1))) || (rc = grow(A.text.first, (size_t)n + 1)) ||
        (rc = grow(A.chunk_first, (size_t)max_chunks + 1)) || (rc = grow(A.text.buf, bound + 2 * BATCH_SLACK)))
        return rc;
    if (fresh_plane && (rc = mirror_upload(c, A.tags, plane, "the tag plane"))) return rc;
    const uint8_t* const tags = A.tags.dev + BATCH_SLACK;
    tables_at(T, tags, den_off);
    const qcat_result* recs;
    if ((rc = records_on_device(c, records, n, &recs))) return rc;
    const KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
    uint8_t* const dst = text_out_ptr(A.text);
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_annot_segments, dim3(n / 256 + 1), dim3(256), 0, c->stream, kp, T, recs, (const uint64_t*)b->offsets,
                       (const qfq::Rec*)b->text_recs, n, b->text_fasta ? 1u : 0u, const_off, A.seg_off.get(), A.seg_src.get());
    part_scan_launch<uint64_t>(A.seg_off, (uint64_t)n_segs + 1, A.sums, c->stream);
    hipLaunchKernelGGL(k_annot_firsts, dim3(n / 256 + 1), dim3(256), 0, c->stream, (const uint64_t*)A.seg_off.get(), n, A.text.first.get());
    if (max_chunks)
        hipLaunchKernelGGL(k_part_chunks, dim3((uint32_t)((max_chunks + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t*)A.seg_off.get(), n_segs,
                           A.chunk_first.get(), max_chunks);
    mark(c, "annot_segments");
    if (max_chunks)
        hipLaunchKernelGGL(k_annot_copy, dim3((uint32_t)max_chunks), dim3(256), 0, c->stream, (const uint64_t*)A.seg_off.get(),
                           (const uint64_t*)A.seg_src.get(), n_segs, (const uint32_t*)A.chunk_first.get(), (const uint8_t*)b->text, tags, dst);
    mark(c, "annot_copy");
    return text_out_finish(c, A.text, A.seg_off + n_segs, n, bound, fn, n_text_bytes);
}

extern "C" int qcat_ctx_fetch_annot_text(qcat_ctx* c, uint8_t* text, uint64_t cap, uint64_t* rec_first) {
    return text_out_fetch(c, c ? &c->batch.annot.text : nullptr, text, cap, rec_first, "qcat_ctx_fetch_annot_text", "no annotated text");
}
extern "C" void* qcat_ctx_annot_text_devptr(qcat_ctx* c) { return text_out_devptr(c ? &c->batch.annot.text : nullptr); }

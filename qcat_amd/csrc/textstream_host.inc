// textstream_host.inc -- the driver's annotated single stream of a scanned text batch in device memory (the kernels:
// kernels_textstream.inc; the arithmetic and the tag plane's layout: textstream_core.h):
//   qcat_batch_annot_text      every kept read in read order with " barcode=<id>" behind its title, as FqWriter::write_range
//                              (fastq_host.inc, the !to_dir branch) writes it to out_fd: a segment table of ten byte ranges per read,
//                              the partition's scan chain and chunk table, the two-plane copy
//   qcat_ctx_fetch_annot_text / qcat_ctx_annot_text_devptr   read-out
// The id texts are the id slots of the TSV tables' blob (qtsv::tables_build, without score slots); the blob, the stream's constants
// and the copy's slack make the tag plane, which is uploaded when it differs from the one on the device.
// Included by qcat_hip.hip behind tsvtext_host.inc: it uses the helpers of batch_host.inc.

static int annot_check(const qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records, const qcat_tsv_names* names,
                       uint32_t flags, const uint64_t* n_text_bytes) {
    if (!c || !ckit || !b || !n_text_bytes) return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: null argument");
    if (flags != 0) return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: flags are reserved and must be 0");
    if (b->device != c->device) return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: batch lives on another device than the context");
    if (!b->text || !b->owned()) return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: the batch has no text plane (qcat_batch_upload_text makes one)");
    const DevKit& d = ckit->hk.dk;
    if (!names || !names->bc_id || (d.mode == QCAT_MODE_DUAL && !names->bc2_id))
        return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: name tables missing");
    for (int t = 0; t < d.nt; ++t)
        if ((d.tpl[t].sets[0].n > 0 && !names->bc_id[t]) || (d.mode == QCAT_MODE_DUAL && d.tpl[t].sets[1].n > 0 && !names->bc2_id[t]))
            return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: a name table is missing (template " + std::to_string(t) + ")");
    if (!records && (c->last_kit != ckit || c->last_n_reads != b->n_reads))
        return set_err(QCAT_ERR_ARG, "qcat_batch_annot_text: records == NULL needs this context's latest qcat_scan_resident to be a scan of "
                                     "these reads with this kit");
    if ((uint64_t)qann::ANNOT_SEGS * b->n_reads >= (1ull << 32))
        return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_annot_text: batch too large (10 segments per read, >= 2^32 segments)");
    return 0;
}

extern "C" int qcat_batch_annot_text(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                                     const qcat_tsv_names* names, uint32_t flags, uint64_t* n_text_bytes) {
    int rc = annot_check(c, ckit, b, records, names, flags, n_text_bytes);
    if (rc) return rc;
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& d = kit->hk.dk;
    AnnotScratch& A = c->batch.annot;
    // the tables: the ids of the caller's name tables, no kit names and no scores (the stream prints neither)
    uint32_t n_ids[2 * QCAT_MAX_TEMPLATES];
    const int32_t* ids[2 * QCAT_MAX_TEMPLATES];
    const char* no_kit[QCAT_MAX_TEMPLATES];
    const bool dual = d.mode == QCAT_MODE_DUAL, simple = d.mode == QCAT_MODE_SIMPLE;
    for (int t = 0; t < d.nt; ++t) {
        n_ids[2 * t] = (uint32_t)std::max(0, d.tpl[t].sets[0].n); ids[2 * t] = names->bc_id[t];
        n_ids[2 * t + 1] = dual ? (uint32_t)std::max(0, d.tpl[t].sets[1].n) : 0; ids[2 * t + 1] = dual ? names->bc2_id[t] : nullptr;
        no_kit[t] = nullptr;
    }
    qtsv::ScoreTable no_scores;
    for (uint32_t i = 0; i <= qtsv::TSV_MAX_DEN; ++i) no_scores.den_first[i] = no_scores.den_last[i] = -1;
    std::vector<uint8_t> plane;
    qtsv::Tables T;
    uint32_t den_off = 0;
    const std::string err = qtsv::tables_build(simple, dual, (uint32_t)d.nt, n_ids, ids, no_kit, no_scores, &plane, &T, &den_off);
    if (!err.empty()) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_annot_text: " + err);
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
    A.valid = false;
    // A.plane says what A.tags holds: dropped before the device buffer may move, set again once the upload is on its way
    const bool fresh_plane = !A.tags.get() || A.tags.cap() < plane.size() || plane != A.plane;
    if (fresh_plane) A.plane.clear();
    if ((rc = grow(A.tags, plane.size())) || (rc = grow(A.seg_off, (size_t)n_segs + 1)) || (rc = grow(A.seg_src, n_segs)) ||
        (rc = grow(A.sums, part_scan_sums((uint64_t)n_segs + 1))) || (rc = grow(A.rec_first, (size_t)n + 1)) ||
        (rc = grow(A.chunk_first, (size_t)max_chunks + 1)) || (rc = grow(A.out, bound + 2 * BATCH_SLACK)) || (records && (rc = grow(A.recs, n))))
        return rc;
    if (fresh_plane) {                             // (once per kit and name tables; the context keeps the host copy the upload reads)
        A.plane.swap(plane);
        const hipError_t e = hipMemcpyAsync(A.tags, A.plane.data(), A.plane.size(), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            A.plane.clear();
            return set_err(QCAT_ERR_DEVICE, std::string("hipMemcpyAsync of the tag plane: ") + hipGetErrorString(e));
        }
    }
    const uint8_t* const tags = A.tags + BATCH_SLACK;
    T.blob = tags;
    T.den_first = reinterpret_cast<const int32_t*>(tags + den_off);
    T.den_last = T.den_first + (qtsv::TSV_MAX_DEN + 1);
    const qcat_result* recs = c->results;
    if (records) {
        if (n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(A.recs, records, (size_t)n * sizeof(qcat_result), hipMemcpyHostToDevice, c->stream));
        recs = A.recs;
    }
    const KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
    uint8_t* const dst = A.out + BATCH_SLACK;
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_annot_segments, dim3(n / 256 + 1), dim3(256), 0, c->stream, kp, T, recs, (const uint64_t*)b->offsets,
                       (const qfq::Rec*)b->text_recs, n, b->text_fasta ? 1u : 0u, const_off, A.seg_off.get(), A.seg_src.get());
    part_scan_launch<uint64_t>(A.seg_off, (uint64_t)n_segs + 1, A.sums, c->stream);
    hipLaunchKernelGGL(k_annot_firsts, dim3(n / 256 + 1), dim3(256), 0, c->stream, (const uint64_t*)A.seg_off.get(), n, A.rec_first.get());
    if (max_chunks)
        hipLaunchKernelGGL(k_part_chunks, dim3((uint32_t)((max_chunks + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t*)A.seg_off.get(), n_segs,
                           A.chunk_first.get(), max_chunks);
    mark(c, "annot_segments");
    if (max_chunks)
        hipLaunchKernelGGL(k_annot_copy, dim3((uint32_t)max_chunks), dim3(256), 0, c->stream, (const uint64_t*)A.seg_off.get(),
                           (const uint64_t*)A.seg_src.get(), n_segs, (const uint32_t*)A.chunk_first.get(), (const uint8_t*)b->text, tags, dst);
    mark(c, "annot_copy");
    uint64_t total = 0;
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&total, A.seg_off + n_segs, 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stream_done(c, "qcat_batch_annot_text"))) return rc;
    if (total > bound) return set_err(QCAT_ERR_DEVICE, "qcat_batch_annot_text: the text is longer than its bound");
    A.n_reads = n; A.total = total; A.valid = true;
    *n_text_bytes = total;
    return 0;
}

extern "C" int qcat_ctx_fetch_annot_text(qcat_ctx* c, uint8_t* text, uint64_t cap, uint64_t* rec_first) {
    if (!c) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_annot_text: null context");
    const AnnotScratch& A = c->batch.annot;
    if (!A.valid) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_annot_text: no annotated text on this context");
    if (text && cap < A.total) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_annot_text: the buffer is shorter than the text");
    HIPCHK(hipSetDevice(c->device));
    if (text && A.total) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(text, A.out + BATCH_SLACK, A.total, hipMemcpyDeviceToHost, c->stream));
    if (rec_first) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(rec_first, A.rec_first, ((size_t)A.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" void* qcat_ctx_annot_text_devptr(qcat_ctx* c) { return c && c->batch.annot.valid ? (void*)(c->batch.annot.out + BATCH_SLACK) : nullptr; }

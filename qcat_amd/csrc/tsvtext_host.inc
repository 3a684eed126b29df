// tsvtext_host.inc -- the driver's TSV rows of a scanned text batch in device memory (the kernels: kernels_tsvtext.inc; the
// arithmetic and the tables' layout: tsvtext_core.h):
//   qcat_batch_tsv_text      one row per kept read, in read order, as FqWriter::write_range (fastq_host.inc) prints them: a length
//                            pass, the scan chain of the partition, the tile table, the writer
//   qcat_ctx_fetch_tsv_text / qcat_ctx_tsv_text_devptr   read-out
// The strings a row looks up -- Barcode ids, kit names, score texts -- go up as one blob: the score part is built once per kit
// with fq_repr_double and kept on the context, the blob is uploaded when it differs from the one on the device (a MirroredTable).
// The argument check, the name tables, the records, the tail and the read-out are the text products' shared layer
// (text_out_host.inc); here are the score table, the bounds, the rows' own arrays and the launches.
// Included by qcat_hip.hip behind fastq_host.inc: it uses that file's fq_repr_double and the helpers of batch_host.inc.

// the score table of `kit` on this context: every denominator the kit can write to score_den -- every set's tlen, the barcodes'
// own lengths of a ragged simple list -- with the raw scores 0 .. den * (the barcode matrix's largest entry)
static int tsv_score_table(qcat_ctx* c, const qcat_kit* kit) {
    TsvScratch& S = c->batch.tsv;
    if (S.score_kit == kit->serial) return 0;
    const HostKit& h = kit->hk;
    const DevKit& d = h.dk;
    int best = 0;
    for (int i = 0; i < 49; ++i) best = std::max(best, (int)d.bmat[i]);
    std::vector<int32_t> dens, max_raw;
    const int nsets = d.mode == QCAT_MODE_DUAL ? 2 : 1;
    for (int t = 0; t < d.nt; ++t)
        for (int s = 0; s < nsets; ++s) {
            const DevSet& q = d.tpl[t].sets[s];
            if (q.n <= 0) continue;
            dens.push_back(q.tlen);
            if (q.len_off >= 0) for (int b = 0; b < q.n; ++b) dens.push_back(h.ids[(size_t)q.len_off + 3 * (size_t)b]);
        }
    for (int32_t den : dens) max_raw.push_back(den * best);
    S.score_kit = 0;
    const std::string err = qtsv::score_table_build(dens, max_raw, [](double v, char* out) { return fq_repr_double(v, out); }, &S.scores);
    if (!err.empty()) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_tsv_text: " + err);
    S.score_kit = kit->serial;
    return 0;
}

extern "C" int qcat_batch_tsv_text(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                                   const qcat_tsv_names* names, uint32_t flags, uint64_t* n_text_bytes) {
    const std::string fn = "qcat_batch_tsv_text";
    int rc = batch_call_check(c, ckit, b, records, flags, n_text_bytes, fn, "qcat_batch_upload_fastq_text");
    if (rc) return rc;
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    TsvScratch& S = c->batch.tsv;
    // the tables: nothing is enqueued before they stand
    if ((rc = tsv_score_table(c, kit))) return rc;
    std::vector<uint8_t> blob;
    qtsv::Tables T;
    uint32_t den_off = 0;
    if ((rc = name_tables_build(kit->hk.dk, names, &S.scores, fn, &blob, &T, &den_off))) return rc;
    const uint32_t n = b->n_reads;
    const uint64_t titles = b->text_fasta ? qtsv::fa_title_bound(b->text_bytes, b->n_bases, n) : qtsv::title_bound(b->text_bytes, b->n_bases, n);
    const uint64_t bound = qtsv::output_bound(titles, n, T);
    const uint64_t max_tiles = qtsv::tiles_of(bound);
    if (max_tiles >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_tsv_text: text too large (>= 2^45 bytes)");
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return rc;
    S.text.valid = false;
    const bool fresh_blob = S.tables.stale(blob);  // (once per kit and name tables)
    if ((rc = grow(S.tables.dev, blob.size())) || (rc = grow(S.text.first, (size_t)n + 1)) || (rc = grow(S.sums, part_scan_sums((uint64_t)n + 1))) ||
        (rc = grow(S.name_len, n)) || (rc = grow(S.keep, n)) || (rc = grow(S.tile_first, (size_t)max_tiles + 1)) || (rc = grow(S.bad, 1)) ||
        (rc = grow(S.text.buf, bound + 2 * BATCH_SLACK)))
        return rc;
    if (fresh_blob && (rc = mirror_upload(c, S.tables, blob, "the TSV tables"))) return rc;
    tables_at(T, S.tables.dev, den_off);
    const qcat_result* recs;
    if ((rc = records_on_device(c, records, n, &recs))) return rc;
    const KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
    uint8_t* const dst = text_out_ptr(S.text);
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    HIPCHK_DRAIN(c->stream, hipMemsetAsync(S.bad, 0, 4, c->stream));
    hipLaunchKernelGGL(k_tsv_lengths, dim3(n / 256 + 1), dim3(256), 0, c->stream, kp, T, recs, (const uint64_t*)b->offsets, (const uint8_t*)b->text,
                       (const qfq::Rec*)b->text_recs, n, S.text.first.get(), S.name_len.get(), S.keep.get(), S.bad.get());
    mark(c, "tsv_lengths");
    part_scan_launch<uint64_t>(S.text.first, (uint64_t)n + 1, S.sums, c->stream);
    mark(c, "tsv_scan");
    if (max_tiles) {
        hipLaunchKernelGGL(k_tsv_tiles, dim3((uint32_t)((max_tiles + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t*)S.text.first.get(), n,
                           S.tile_first.get(), max_tiles);
        hipLaunchKernelGGL(k_tsv_write, dim3((uint32_t)max_tiles), dim3(qtsv::TSV_THREADS), 0, c->stream, T, recs, (const uint8_t*)b->text,
                           (const qfq::Rec*)b->text_recs, (const uint64_t*)S.text.first.get(), (const uint32_t*)S.name_len.get(),
                           (const uint32_t*)S.keep.get(), n, (const uint32_t*)S.tile_first.get(), bound, dst);
    }
    mark(c, "tsv_write");
    return text_out_finish(c, S.text, S.text.first + n, n, bound, fn, n_text_bytes, S.bad,
                           "a called record's (raw_score, score_den) lies outside the kit's score table");
}

extern "C" int qcat_ctx_fetch_tsv_text(qcat_ctx* c, uint8_t* text, uint64_t cap, uint64_t* row_first) {
    return text_out_fetch(c, c ? &c->batch.tsv.text : nullptr, text, cap, row_first, "qcat_ctx_fetch_tsv_text", "no TSV text");
}
extern "C" void* qcat_ctx_tsv_text_devptr(qcat_ctx* c) { return text_out_devptr(c ? &c->batch.tsv.text : nullptr); }

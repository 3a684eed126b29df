// tsvtext_host.inc -- the driver's TSV rows of a scanned text batch in device memory (the kernels: kernels_tsvtext.inc; the
// arithmetic and the tables' layout: tsvtext_core.h):
//   qcat_batch_tsv_text      one row per kept read, in read order, as FqWriter::write_range (fastq_host.inc) prints them: a length
//                            pass, the scan chain of the partition, the tile table, the writer
//   qcat_ctx_fetch_tsv_text / qcat_ctx_tsv_text_devptr   read-out
// The strings a row looks up -- Barcode ids, kit names, score texts -- go up as one blob: the score part is built once per kit
// with fq_repr_double and kept on the context, the blob is uploaded when it differs from the one on the device.
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

static int tsv_check(const qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records, const qcat_tsv_names* names,
                     uint32_t flags, const uint64_t* n_text_bytes) {
    if (!c || !ckit || !b || !n_text_bytes) return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: null argument");
    if (flags != 0) return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: flags are reserved and must be 0");
    if (b->device != c->device) return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: batch lives on another device than the context");
    if (!b->text || !b->owned()) return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: the batch has no text plane (qcat_batch_upload_fastq_text makes one)");
    const DevKit& d = ckit->hk.dk;
    if (!names || !names->kit_name || !names->bc_id || (d.mode == QCAT_MODE_DUAL && !names->bc2_id))
        return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: name tables missing");
    for (int t = 0; t < d.nt; ++t)
        if ((d.tpl[t].sets[0].n > 0 && !names->bc_id[t]) || (d.mode == QCAT_MODE_DUAL && d.tpl[t].sets[1].n > 0 && !names->bc2_id[t]))
            return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: a name table is missing (template " + std::to_string(t) + ")");
    if (!records && (c->last_kit != ckit || c->last_n_reads != b->n_reads))
        return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: records == NULL needs this context's latest qcat_scan_resident to be a scan of "
                                     "these reads with this kit");
    return 0;
}

extern "C" int qcat_batch_tsv_text(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                                   const qcat_tsv_names* names, uint32_t flags, uint64_t* n_text_bytes) {
    int rc = tsv_check(c, ckit, b, records, names, flags, n_text_bytes);
    if (rc) return rc;
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& d = kit->hk.dk;
    TsvScratch& S = c->batch.tsv;
    // the tables: nothing is enqueued before they stand
    if ((rc = tsv_score_table(c, kit))) return rc;
    uint32_t n_ids[2 * QCAT_MAX_TEMPLATES];
    const int32_t* ids[2 * QCAT_MAX_TEMPLATES];
    const bool dual = d.mode == QCAT_MODE_DUAL, simple = d.mode == QCAT_MODE_SIMPLE;
    for (int t = 0; t < d.nt; ++t) {
        n_ids[2 * t] = (uint32_t)std::max(0, d.tpl[t].sets[0].n); ids[2 * t] = names->bc_id[t];
        n_ids[2 * t + 1] = dual ? (uint32_t)std::max(0, d.tpl[t].sets[1].n) : 0; ids[2 * t + 1] = dual ? names->bc2_id[t] : nullptr;
    }
    std::vector<uint8_t> blob;
    qtsv::Tables T;
    uint32_t den_off = 0;
    const std::string err = qtsv::tables_build(simple, dual, (uint32_t)d.nt, n_ids, ids, names->kit_name, S.scores, &blob, &T, &den_off);
    if (!err.empty()) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_tsv_text: " + err);
    const uint32_t n = b->n_reads;
    const uint64_t titles = b->text_fasta ? qtsv::fa_title_bound(b->text_bytes, b->n_bases, n) : qtsv::title_bound(b->text_bytes, b->n_bases, n);
    const uint64_t bound = qtsv::output_bound(titles, n, T);
    const uint64_t max_tiles = qtsv::tiles_of(bound);
    if (max_tiles >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_tsv_text: text too large (>= 2^45 bytes)");
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return rc;
    S.valid = false;
    // S.blob says what S.tables holds: it is dropped before the device buffer may move and set again once the upload is on its
    // way, so that no early return leaves it vouching for an allocation nobody wrote
    const bool fresh_blob = !S.tables.get() || S.tables.cap() < blob.size() || blob != S.blob;
    if (fresh_blob) S.blob.clear();
    if ((rc = grow(S.tables, blob.size())) || (rc = grow(S.row_first, (size_t)n + 1)) || (rc = grow(S.sums, part_scan_sums((uint64_t)n + 1))) ||
        (rc = grow(S.name_len, n)) || (rc = grow(S.keep, n)) || (rc = grow(S.tile_first, (size_t)max_tiles + 1)) || (rc = grow(S.bad, 1)) ||
        (rc = grow(S.out, bound + 2 * BATCH_SLACK)) || (records && (rc = grow(S.recs, n))))
        return rc;
    if (fresh_blob) {                              // (once per kit and name tables; the context keeps the host copy the upload reads)
        S.blob.swap(blob);
        const hipError_t e = hipMemcpyAsync(S.tables, S.blob.data(), S.blob.size(), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            S.blob.clear();
            return set_err(QCAT_ERR_DEVICE, std::string("hipMemcpyAsync of the TSV tables: ") + hipGetErrorString(e));
        }
    }
    T.blob = S.tables;
    T.den_first = reinterpret_cast<const int32_t*>(S.tables + den_off);
    T.den_last = T.den_first + (qtsv::TSV_MAX_DEN + 1);
    const qcat_result* recs = c->results;
    if (records) {
        if (n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(S.recs, records, (size_t)n * sizeof(qcat_result), hipMemcpyHostToDevice, c->stream));
        recs = S.recs;
    }
    const KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
    uint8_t* const dst = S.out + BATCH_SLACK;
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    HIPCHK_DRAIN(c->stream, hipMemsetAsync(S.bad, 0, 4, c->stream));
    hipLaunchKernelGGL(k_tsv_lengths, dim3(n / 256 + 1), dim3(256), 0, c->stream, kp, T, recs, (const uint64_t*)b->offsets, (const uint8_t*)b->text,
                       (const qfq::Rec*)b->text_recs, n, S.row_first.get(), S.name_len.get(), S.keep.get(), S.bad.get());
    mark(c, "tsv_lengths");
    part_scan_launch<uint64_t>(S.row_first, (uint64_t)n + 1, S.sums, c->stream);
    mark(c, "tsv_scan");
    if (max_tiles) {
        hipLaunchKernelGGL(k_tsv_tiles, dim3((uint32_t)((max_tiles + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t*)S.row_first.get(), n,
                           S.tile_first.get(), max_tiles);
        hipLaunchKernelGGL(k_tsv_write, dim3((uint32_t)max_tiles), dim3(qtsv::TSV_THREADS), 0, c->stream, T, recs, (const uint8_t*)b->text,
                           (const qfq::Rec*)b->text_recs, (const uint64_t*)S.row_first.get(), (const uint32_t*)S.name_len.get(),
                           (const uint32_t*)S.keep.get(), n, (const uint32_t*)S.tile_first.get(), bound, dst);
    }
    mark(c, "tsv_write");
    uint64_t total = 0;
    uint32_t bad = 0;
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&total, S.row_first + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&bad, S.bad, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stream_done(c, "qcat_batch_tsv_text"))) return rc;
    if (bad) return set_err(QCAT_ERR_ARG, "qcat_batch_tsv_text: a called record's (raw_score, score_den) lies outside the kit's score table");
    if (total > bound) return set_err(QCAT_ERR_DEVICE, "qcat_batch_tsv_text: the text is longer than its bound");
    S.n_reads = n; S.total = total; S.valid = true;
    *n_text_bytes = total;
    return 0;
}

extern "C" int qcat_ctx_fetch_tsv_text(qcat_ctx* c, uint8_t* text, uint64_t cap, uint64_t* row_first) {
    if (!c) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_tsv_text: null context");
    const TsvScratch& S = c->batch.tsv;
    if (!S.valid) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_tsv_text: no TSV text on this context");
    if (text && cap < S.total) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_tsv_text: the buffer is shorter than the text");
    HIPCHK(hipSetDevice(c->device));
    if (text && S.total) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(text, S.out + BATCH_SLACK, S.total, hipMemcpyDeviceToHost, c->stream));
    if (row_first) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(row_first, S.row_first, ((size_t)S.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" void* qcat_ctx_tsv_text_devptr(qcat_ctx* c) { return c && c->batch.tsv.valid ? (void*)(c->batch.tsv.out + BATCH_SLACK) : nullptr; }

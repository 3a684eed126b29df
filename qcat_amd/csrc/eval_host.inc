// eval_host.inc -- the evaluation of a scanned text batch in device memory (the kernels: kernels_eval.inc; the contract and the
// arithmetic: eval_core.h):
//   qcat_batch_eval        the reference's qcat-eval classes, its summary counts and the counts of qcat-roc at the 1001 score
//                          thresholds, of the reads that have a TSV row: a classify pass, the ROC table from its histogram
//   qcat_ctx_fetch_eval    read-out of the per-read planes and the table
// The id texts are the id slots of the TSV tables' blob (name_tables_build without scores), uploaded when they differ from the
// ones on the device (a MirroredTable of this product's own).  The argument check, the name tables and the records are the text
// products' shared layer (text_out_host.inc); here are the comment mode's own check, the product's arrays and the launches.
// Included by qcat_hip.hip behind textstream_host.inc: it uses the helpers of batch_host.inc.

// the shape of the classify pass without the option EVAL_SHAPE: one lane per read, the faster of the two (profiles/eval_ab.txt)
constexpr int EVAL_SHAPE_DEFAULT = 0;

extern "C" int qcat_batch_eval(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                               const qcat_tsv_names* names, uint32_t flags, qcat_eval_counts* out) {
    const std::string fn = "qcat_batch_eval";
    const bool from_comment = (flags & QCAT_EVAL_FROM_COMMENT) != 0;
    int rc = 0;
    if (from_comment) {                            // (no kit, no records, no names: the titles alone)
        if (!c || !b || !out) return set_err(QCAT_ERR_ARG, fn + ": null argument");
        if (flags != QCAT_EVAL_FROM_COMMENT) return set_err(QCAT_ERR_ARG, fn + ": flags other than QCAT_EVAL_FROM_COMMENT are reserved and must be 0");
        if (b->device != c->device) return set_err(QCAT_ERR_ARG, fn + ": batch lives on another device than the context");
        if (!b->text || !b->owned()) return set_err(QCAT_ERR_ARG, fn + ": the batch has no text plane (qcat_batch_upload_text makes one)");
    } else if ((rc = batch_call_check(c, ckit, b, records, flags, out, fn, "qcat_batch_upload_text"))) return rc;
    const uint32_t n = b->n_reads;
    if (n == qev::EVAL_NO_BAD) return set_err(QCAT_ERR_UNSUPPORTED, fn + ": batch too large (2^32 - 1 reads)");
    EvalScratch& E = c->batch.eval;
    std::vector<uint8_t> blob;
    qtsv::Tables T;
    memset(&T, 0, sizeof T);
    uint32_t den_off = 0;
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    if (!from_comment && (rc = name_tables_build(kit->hk.dk, names, nullptr, fn, &blob, &T, &den_off))) return rc;
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    if (!from_comment && (rc = kit_on_device(kit, c->device, &kd))) return rc;
    E.valid = false;
    const bool fresh_blob = !from_comment && E.tables.stale(blob);
    if ((!from_comment && (rc = grow(E.tables.dev, blob.size()))) || (rc = grow(E.cls, n)) || (rc = grow(E.kind, n)) || (rc = grow(E.bucket, n)) ||
        (rc = grow(E.hist, qev::EVAL_HIST)) || (rc = grow(E.bad, 1)) || (rc = grow(E.roc, (size_t)qev::EVAL_Q * qev::EVAL_ROC_COLS)))
        return rc;
    if (fresh_blob && (rc = mirror_upload(c, E.tables, blob, "the id tables"))) return rc;
    const qcat_result* recs = nullptr;
    KitPtrs kp{nullptr, nullptr, nullptr, nullptr};
    if (!from_comment) {
        tables_at(T, E.tables.dev, den_off);
        if ((rc = records_on_device(c, records, n, &recs))) return rc;
        kp = KitPtrs{kd->kit, kd->codes, kd->ids, kd->tables};
    }
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));
    HIPCHK_DRAIN(c->stream, hipMemsetAsync(E.hist, 0, qev::EVAL_HIST * sizeof(uint32_t), c->stream));
    HIPCHK_DRAIN(c->stream, hipMemsetAsync(E.bad, 0xFF, 4, c->stream));
    // one lane per read by default, a group of lanes per read with EVAL_SHAPE=1
    const bool group = opt_val(QO_EVAL_SHAPE, EVAL_SHAPE_DEFAULT) != 0;
    hipLaunchKernelGGL(group ? k_eval_classify<qev::EVAL_GROUP> : k_eval_classify<1>,
                       dim3(group ? qev::classify_group_blocks(n) : qev::classify_blocks(n)), dim3(qev::EVAL_THREADS), 0, c->stream, kp, T, recs,
                       (const uint64_t*)b->offsets, (const uint8_t*)b->text, (const qfq::Rec*)b->text_recs, n, from_comment ? 1u : 0u,
                       E.cls.get(), E.kind.get(), E.bucket.get(), E.hist.get(), E.bad.get());
    mark(c, "eval_classify");
    hipLaunchKernelGGL(k_eval_roc, dim3(1), dim3(qev::EVAL_ROC_THREADS), 0, c->stream, (const uint32_t*)E.hist.get(), E.roc.get());
    mark(c, "eval_roc");
    // the call's one synchronisation: the four class counts and the first bad read
    uint32_t counts[4] = {0, 0, 0, 0}, bad = qev::EVAL_NO_BAD;
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(counts, E.hist + qev::class_slot(qev::CLS_CORRECT), sizeof counts, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&bad, E.bad, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stream_done(c, fn.c_str()))) return rc;
    if (bad != qev::EVAL_NO_BAD) {                 // (a refused call alone pays a second copy: why that read is refused)
        uint8_t why = 0;
        HIPCHK(hipMemcpy(&why, E.cls + (bad - 1u), 1, hipMemcpyDeviceToHost));
        return set_err(QCAT_ERR_ARG, fn + ": read " + std::to_string(bad) + " cannot be evaluated: " + qev::bad_text((uint8_t)(why & ~qev::CLS_BAD)));
    }
    out->correct = counts[0]; out->incorrect = counts[1]; out->fn = counts[2]; out->fp = counts[3];
    out->total = out->correct + out->incorrect + out->fn + out->fp;
    E.n_reads = n; E.valid = true;
    return 0;
}

extern "C" int qcat_ctx_fetch_eval(qcat_ctx* c, uint8_t* cls, uint8_t* kind, uint16_t* bucket, int64_t* roc) {
    const std::string fn = "qcat_ctx_fetch_eval";
    if (!c) return set_err(QCAT_ERR_ARG, fn + ": null context");
    const EvalScratch& E = c->batch.eval;
    if (!E.valid) return set_err(QCAT_ERR_ARG, fn + ": no evaluation on this context");
    HIPCHK(hipSetDevice(c->device));
    const size_t n = E.n_reads;
    if (cls && n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(cls, E.cls, n, hipMemcpyDeviceToHost, c->stream));
    if (kind && n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(kind, E.kind, n, hipMemcpyDeviceToHost, c->stream));
    if (bucket && n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(bucket, E.bucket, n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    if (roc) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(roc, E.roc, (size_t)qev::EVAL_Q * qev::EVAL_ROC_COLS * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

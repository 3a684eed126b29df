// text_out_host.inc -- the host layer the calls over a scanned resident batch share (the types: text_out.h): the partition
// (batch_host.inc) takes its argument check and its records from here, the three text products -- the demultiplexed text
// (fqtext_host.inc), the TSV rows (tsvtext_host.inc), the annotated stream (textstream_host.inc) -- everything below:
//   batch_call_check     the arguments every such call refuses
//   records_on_device    the records a call works on: the context's latest scan, or the caller's in the one buffer for them
//   name_tables_build / tables_at   the caller's name tables as the blob of qtsv::tables_build, and its pointers on the device
//   mirror_upload        the upload step of a MirroredTable (text_out.h states the invariant)
//   text_out_finish      the tail of a text call: total, the device's verdict, the bound, valid
//   text_out_fetch / text_out_devptr   behind every qcat_ctx_fetch_*_text / qcat_ctx_*_text_devptr
// Nothing here launches a kernel or touches the partition's scratch.  A product supplies its sizes and bounds (its *_core.h),
// the grow chain of its own arrays, its kernel launches and marks.
// Included by qcat_hip.hip behind batch_host.inc and in front of fqtext_host.inc.

// fn: the entry point's name in front of every message; out: where the call's result goes; text_maker: the upload named behind
// "the batch has no text plane" (null: the call needs none)
static int batch_call_check(const qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records, uint32_t flags,
                            const void* out, const std::string& fn, const char* text_maker) {
    if (!c || !ckit || !b || !out) return set_err(QCAT_ERR_ARG, fn + ": null argument");
    if (flags != 0) return set_err(QCAT_ERR_ARG, fn + ": flags are reserved and must be 0");
    if (b->device != c->device) return set_err(QCAT_ERR_ARG, fn + ": batch lives on another device than the context");
    if (text_maker && (!b->text || !b->owned()))
        return set_err(QCAT_ERR_ARG, fn + ": the batch has no text plane (" + text_maker + " makes one)");
    if (!records && (c->last_kit != ckit || c->last_n_reads != b->n_reads))
        return set_err(QCAT_ERR_ARG, fn + ": records == NULL needs this context's latest qcat_scan_resident to be a scan of "
                                          "these reads with this kit");
    return 0;
}

// *recs: the context's latest scan (records == NULL), or the caller's n records on their way into the context's one buffer for
// them.  One buffer serves every call: each uploads its own records on the stream its kernels run on, and none returns before
// that stream is drained -- stream_done at its end, a drain on every failure behind this point, this function's own included.
static int records_on_device(qcat_ctx* c, const qcat_result* records, uint32_t n, const qcat_result** recs) {
    *recs = c->results;
    if (!records) return 0;
    qk::DevBuf<qcat_result>& buf = c->batch.recs;
    if (int rc = grow(buf, n)) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (n) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(buf, records, (size_t)n * sizeof(qcat_result), hipMemcpyHostToDevice, c->stream));
    *recs = buf;
    return 0;
}

// the caller's name tables for the kit `d`, checked, as the blob of qtsv::tables_build.  scores: the kit's score table, and the
// rows' kit names come from names->kit_name; null: ids alone, neither kit names nor scores (the annotated stream prints
// neither, and names->kit_name is not looked at).  T holds host pointers until tables_at.
static int name_tables_build(const DevKit& d, const qcat_tsv_names* names, const qtsv::ScoreTable* scores, const std::string& fn,
                             std::vector<uint8_t>* blob, qtsv::Tables* T, uint32_t* den_off) {
    const bool dual = d.mode == QCAT_MODE_DUAL, simple = d.mode == QCAT_MODE_SIMPLE;
    if (!names || (scores && !names->kit_name) || !names->bc_id || (dual && !names->bc2_id))
        return set_err(QCAT_ERR_ARG, fn + ": name tables missing");
    for (int t = 0; t < d.nt; ++t)
        if ((d.tpl[t].sets[0].n > 0 && !names->bc_id[t]) || (dual && d.tpl[t].sets[1].n > 0 && !names->bc2_id[t]))
            return set_err(QCAT_ERR_ARG, fn + ": a name table is missing (template " + std::to_string(t) + ")");
    uint32_t n_ids[2 * QCAT_MAX_TEMPLATES];
    const int32_t* ids[2 * QCAT_MAX_TEMPLATES];
    for (int t = 0; t < d.nt; ++t) {
        n_ids[2 * t] = (uint32_t)std::max(0, d.tpl[t].sets[0].n); ids[2 * t] = names->bc_id[t];
        n_ids[2 * t + 1] = dual ? (uint32_t)std::max(0, d.tpl[t].sets[1].n) : 0; ids[2 * t + 1] = dual ? names->bc2_id[t] : nullptr;
    }
    std::string err;
    if (scores) err = qtsv::tables_build(simple, dual, (uint32_t)d.nt, n_ids, ids, names->kit_name, *scores, blob, T, den_off);
    else {
        const char* const no_kit[QCAT_MAX_TEMPLATES] = {};
        qtsv::ScoreTable no_scores;
        for (uint32_t i = 0; i <= qtsv::TSV_MAX_DEN; ++i) no_scores.den_first[i] = no_scores.den_last[i] = -1;
        err = qtsv::tables_build(simple, dual, (uint32_t)d.nt, n_ids, ids, no_kit, no_scores, blob, T, den_off);
    }
    if (!err.empty()) return set_err(QCAT_ERR_UNSUPPORTED, fn + ": " + err);
    return 0;
}

// T's pointers for a blob that stands at the device address `blob`
static void tables_at(qtsv::Tables& T, const uint8_t* blob, uint32_t den_off) {
    T.blob = blob;
    T.den_first = reinterpret_cast<const int32_t*>(blob + den_off);
    T.den_last = T.den_first + (qtsv::TSV_MAX_DEN + 1);
}

// the upload step of a stale table, behind the grow chain: `want` is handed over to t.host; what: the table's name in the message
static int mirror_upload(qcat_ctx* c, MirroredTable& t, std::vector<uint8_t>& want, const char* what) {
    t.host.swap(want);
    const hipError_t e = hipMemcpyAsync(t.dev, t.host.data(), t.host.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) return 0;
    (void)hipStreamSynchronize(c->stream);
    t.host.clear();
    return set_err(QCAT_ERR_DEVICE, std::string("hipMemcpyAsync of ") + what + ": " + hipGetErrorString(e));
}

static uint8_t* text_out_ptr(const TextOut& o) { return o.buf + BATCH_SLACK; }

// the tail of a text call over n reads: the total -- the last entry of the product's scanned lengths, at `d_total` -- comes
// back with the device's verdict on everything queued, is held to `bound`, and the text becomes valid.  d_refused: a flag the
// product's kernels raise (null: none), read back with the total; set, the call fails with `refusal`.
static int text_out_finish(qcat_ctx* c, TextOut& o, const uint64_t* d_total, uint32_t n, uint64_t bound, const std::string& fn,
                           uint64_t* n_text_bytes, const uint32_t* d_refused = nullptr, const char* refusal = nullptr) {
    uint64_t total = 0;
    uint32_t refused = 0;
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    if (d_refused) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&refused, d_refused, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = stream_done(c, fn.c_str())) return rc;
    if (refused) return set_err(QCAT_ERR_ARG, fn + ": " + refusal);
    if (total > bound) return set_err(QCAT_ERR_DEVICE, fn + ": the text is longer than its bound");
    o.n_reads = n; o.total = total; o.valid = true;
    *n_text_bytes = total;
    return 0;
}

// read-out.  o: null with a null context; none: what the context lacks ("no TSV text").  The checks, the two copies (either may
// be left out: a product with arrays of its own to fetch places them between its own), and the whole for a product without.
static int text_out_fetch_check(const qcat_ctx* c, const TextOut* o, const uint8_t* text, uint64_t cap, const std::string& fn, const char* none) {
    if (!c) return set_err(QCAT_ERR_ARG, fn + ": null context");
    if (!o->valid) return set_err(QCAT_ERR_ARG, fn + ": " + none + " on this context");
    if (text && cap < o->total) return set_err(QCAT_ERR_ARG, fn + ": the buffer is shorter than the text");
    return 0;
}
static int text_out_fetch_copies(qcat_ctx* c, const TextOut& o, uint8_t* text, uint64_t* first) {
    if (text && o.total) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(text, text_out_ptr(o), o.total, hipMemcpyDeviceToHost, c->stream));
    if (first) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(first, o.first, ((size_t)o.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    return 0;
}
static int text_out_fetch(qcat_ctx* c, const TextOut* o, uint8_t* text, uint64_t cap, uint64_t* first, const std::string& fn, const char* none) {
    int rc = text_out_fetch_check(c, o, text, cap, fn, none);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = text_out_fetch_copies(c, *o, text, first))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
static void* text_out_devptr(const TextOut* o) { return o && o->valid ? (void*)text_out_ptr(*o) : nullptr; }

// pipeline_host.inc -- scan_batch_pipelined: qcat_scan_batch over host buffers as a chunked pipeline (the picture and the
// types: pipeline.h), in its steps -- qualify, open (pool, priority copy stream, events), plan (chunk, cuts), size the stages,
// then per chunk stage / upload / scan / download, then drain and counts.  Everything that needs no device -- the cuts, the
// sizing rule, the length sums with their refusals, the compaction with its prefetch, the split of the records -- is taken
// from pipeline_core.h, where tests/pipeline_check.cpp checks it on the CPU.
// Included by qcat_hip.hip behind filter_host.inc: it needs the context, scan_resident_impl, batch_view and qcat_ctx_fetch_counts.

// the wall clock of one call (PIPELINE_TRACE prints its figures), and the context's per-kernel timing switched off while the
// chunks run: per-kernel events describe one scan, not a chunk train
struct PipeClock {
    qcat_ctx* c;
    bool timing_was;
    double entry, begin = 0, t0 = 0, loop_end = 0;
    double wait = 0, prefix = 0, compact = 0, enqueue = 0;      // ms per stage of the host's work, over the chunks
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit PipeClock(qcat_ctx* c_) : c(c_), timing_was(c_->timing), entry(now()) {}
    ~PipeClock() { c->timing = timing_was; }
    void chunks_begin() { c->timing = false; begin = now(); }
    void start() { t0 = now(); }
    void lap(double& stage) { const double t = now(); stage += t - t0; t0 = t; }
    void print(uint32_t n_reads, uint32_t n_chunks, unsigned threads) const {
        fprintf(stderr, "[qcat pipeline] %u reads, %u chunks, %u threads: set-up (pool, pinned and device staging) %.2f ms, staging wait %.2f ms, "
                        "prefix %.2f, compaction %.2f, enqueue %.2f, drain %.2f, total so far %.2f ms\n", n_reads, n_chunks, threads,
                begin - entry, wait, prefix, compact, enqueue, now() - loop_end, now() - begin);
    }
};

// the context's pipeline, made on first use
static int pipeline_open(qcat_ctx* c) {
    if (c->pipe) return 0;
    c->pipe = new HostPipeline();
    c->pipe->pool = new HostPool(host_threads() - 1);
    // the copy stream gets the highest priority: the runtime multiplexes streams of one priority onto a few
    // hardware queues, and a copy queued behind a 20 ms persistent barcode kernel of a side stream would
    // not start before that kernel ends (measured: no copy/compute overlap at all on a default stream)
    int prio_low = 0, prio_high = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
    HIPCHK(hipStreamCreateWithPriority(&c->pipe->copy, hipStreamNonBlocking, prio_high));
    for (PipeStage& st : c->pipe->st) {
        HIPCHK(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&st.scanned, hipEventDisableTiming));
    }
    return 0;
}

// staging for the LARGEST chunk of this call, and for the second slot only when there is a second chunk (round 6: a segment of
// the file loop is one chunk of 40-180 k reads -- sizing both slots for 256 k reads pinned 157 MB, 0.2 ms per MiB, in front
// of the first segment's scan: 42 ms of a 160 ms run); a later, bigger call grows them with headroom (qpipe::stage_need)
static int pipeline_size_stages(HostPipeline* p, uint32_t n_chunks, uint32_t largest, uint32_t chunk, uint64_t keep) {
    for (PipeStage& st : p->st) {
        if (&st != &p->st[0] && n_chunks < 2) break;
        // (the arrays of a group grow together: the smallest capacity stands for the group, 0 after an allocation that failed)
        const size_t cap_reads = std::min({st.pin_offsets.cap(), st.pin_len.cap(), st.pin_results.cap(), st.dev_offsets.cap(), st.dev_len.cap()});
        const size_t cap_bases = std::min(st.pin_bases.cap(), st.dev_bases_alloc.cap());
        const qpipe::StageNeed need = qpipe::stage_need(largest, chunk, keep, 2 * BATCH_SLACK, cap_reads, cap_bases);
        HIPCHK(st.pin_offsets.ensure(need.reads));
        HIPCHK(st.pin_len.ensure(need.reads));
        HIPCHK(st.pin_results.ensure(need.reads));
        HIPCHK(st.dev_offsets.ensure(need.reads));
        HIPCHK(st.dev_len.ensure(need.reads));
        HIPCHK(st.pin_bases.ensure(need.bases));
        HIPCHK(st.dev_bases_alloc.ensure(need.bases));
    }
    return 0;
}

// a slot's records go to the caller's array once its scan is known to be done
static void pipeline_flush(HostPipeline* p, PipeStage& st, qcat_result* out) {
    if (!st.res_count) return;
    qpipe::copy_records(*p->pool, out + st.res_first, (const qcat_result*)st.pin_results, st.res_count);
    st.res_count = 0;
}

// the host's half of a chunk, reads [r0, r0 + nr) into the slot's pinned staging: offsets + real lengths of the compacted
// chunk (per-part sums in parallel, a serial scan over the parts), then every part writes its offsets and copies its reads
static int pipeline_stage(HostPipeline* p, PipeStage& st, const ReadView& rv, uint32_t r0, uint32_t nr, const qupload::Keep& k,
                          PipeClock& clk, uint64_t* total) {
    const qpipe::Split parts = qpipe::chunk_parts(nr, p->pool->size());
    qpipe::PartSum sums[qpipe::MAX_PARTS];
    switch (qpipe::stage_lengths(*p->pool, rv, r0, parts, k.keep, sums, total)) {
    case qupload::DECREASING: return set_err(QCAT_ERR_ARG, "offsets must be non-decreasing");
    case qupload::TOO_LONG: return set_err(QCAT_ERR_UNSUPPORTED, "read longer than 4 Gb");
    default: break;
    }
    clk.lap(clk.prefix);
    qpipe::stage_compact(*p->pool, rv, r0, parts, k, sums, st.pin_bases, st.pin_offsets, st.pin_len);
    clk.lap(clk.compact);
    return 0;
}

// the chunk's staging to the slot's device buffers on the copy stream; the scan stream waits for it
static int pipeline_upload(qcat_ctx* c, HostPipeline* p, PipeStage& st, uint32_t nr, uint64_t total) {
    if (total) HIPCHK(hipMemcpyAsync(st.dev_bases_alloc + BATCH_SLACK, st.pin_bases, total, hipMemcpyHostToDevice, p->copy));
    HIPCHK(hipMemcpyAsync(st.dev_offsets, st.pin_offsets, ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, p->copy));
    HIPCHK(hipMemcpyAsync(st.dev_len, st.pin_len, (size_t)nr * 4, hipMemcpyHostToDevice, p->copy));
    HIPCHK(hipEventRecord(st.copied, p->copy));
    HIPCHK(hipStreamWaitEvent(c->stream, st.copied, 0));
    return 0;
}

// the chunk's records into the slot's pinned buffer, behind its scan
static int pipeline_download(qcat_ctx* c, PipeStage& st, uint32_t r0, uint32_t nr) {
    HIPCHK(hipMemcpyAsync(st.pin_results, c->results, (size_t)nr * sizeof(qcat_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(st.scanned, c->stream));
    st.res_first = r0; st.res_count = nr;
    return 0;
}

// Returns 1 when the batch does not qualify (small, --detect-middle, disabled) and the caller should take the one-shot path.
static int scan_batch_pipelined(qcat_ctx* c, qcat_kit* kit, const ReadView& rv,
                                uint32_t n_reads, qcat_result* out, int64_t* counts) {
    const DevKit& hk = kit->hk.dk;
    if (hk.scan_middle || n_reads < 32768 || opt_on(QO_FULL_UPLOAD) || opt_on(QO_NO_PIPELINE)) return 1;
    if (!rv.recs) {
        if (!rv.bases && rv.offsets[n_reads] > 0) return set_err(QCAT_ERR_ARG, "qcat_scan_batch: null argument");
        if (rv.offsets[0] != 0) return set_err(QCAT_ERR_ARG, "offsets[0] must be 0");
    }
    HIPCHK(hipSetDevice(c->device));
    const qupload::Keep k = qupload::keep_of((uint64_t)hk.max_align, hk.ends == QCAT_ENDS_BOTH, false);
    PipeClock clk(c);
    int rc = pipeline_open(c);
    if (rc) return rc;
    HostPipeline* p = c->pipe;
    const QOptVal ce = qopt_get(QO_PIPELINE_CHUNK);
    const uint32_t chunk = qpipe::chunk_reads(n_reads, rv.recs != nullptr, (bool)ce, atoi(ce));
    const std::vector<uint32_t> cuts = qpipe::chunk_cuts(n_reads, chunk, (bool)ce);
    const uint32_t n_chunks = (uint32_t)cuts.size() - 1;
    if ((rc = pipeline_size_stages(p, n_chunks, qpipe::largest_chunk(cuts), chunk, k.keep))) return rc;
    clk.chunks_begin();
    for (PipeStage& st : p->st) st.res_count = 0;
    for (uint32_t ci = 0; ci < n_chunks; ++ci) {
        PipeStage& st = p->st[ci & 1];
        const uint32_t r0 = cuts[ci], nr = cuts[ci + 1] - r0;
        uint64_t total = 0;
        clk.start();
        if (ci >= 2) HIPCHK(hipEventSynchronize(st.copied));          // this slot's pinned staging has been read
        clk.lap(clk.wait);
        if ((rc = pipeline_stage(p, st, rv, r0, nr, k, clk, &total))) break;       // (a refused read: reported behind the drain)
        // this slot's device buffers are free again once the scan of chunk ci - 2 is done: waited for on the HOST, so
        // that the copy stream never holds a barrier packet behind which its copies would queue up
        if (ci >= 2) { HIPCHK(hipEventSynchronize(st.scanned)); pipeline_flush(p, st, out); }
        if ((rc = pipeline_upload(c, p, st, nr, total))) return rc;
        // the chunk as a resident batch (no ownership); its bases begin behind the front slack of the stage's allocation
        const qcat_batch view = batch_view(c->device, nr, total, st.dev_bases_alloc + BATCH_SLACK, st.dev_offsets, st.dev_len);
        if ((rc = scan_resident_impl(c, kit, &view, ScanPass::plain().keeping_counts(ci > 0)))) break;
        if ((rc = pipeline_download(c, st, r0, nr))) return rc;
        clk.lap(clk.enqueue);
    }
    clk.loop_end = PipeClock::now();
    const hipError_t es = hipStreamSynchronize(c->stream);
    const hipError_t ec = hipStreamSynchronize(p->copy);
    if (opt_on(QO_PIPELINE_TRACE)) clk.print(n_reads, n_chunks, p->pool->size());
    c->last_n_reads = 0;                                 // the context's result buffer holds the last chunk only
    c->last_kit = nullptr;
    if (rc) return rc;
    if (es != hipSuccess || ec != hipSuccess)
        return set_err(QCAT_ERR_DEVICE, std::string("qcat_scan_batch: ") + hipGetErrorString(es != hipSuccess ? es : ec));
    for (PipeStage& st : p->st) pipeline_flush(p, st, out);
    if (counts) {
        std::vector<int64_t> tmp((size_t)hk.n_buckets);
        c->last_buckets = hk.n_buckets;
        if ((rc = qcat_ctx_fetch_counts(c, tmp.data(), hk.n_buckets))) return rc;
        for (size_t i = 0; i < tmp.size(); ++i) counts[i] += tmp[i];
    }
    return 0;
}

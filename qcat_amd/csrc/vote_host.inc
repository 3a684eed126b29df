// vote_host.inc -- the kit vote of kit auto (qcat/scanner_base.py:662-678): every read votes for the kit of the adapter template
// that scores best at its better end, per batch of the driver.  ONE place for the vote's block (VoteBuf) and its launches
// (vote_enqueue: the two fills, k_vote, k_pick_kit), and the three entry points that use them: qcat_detect_kit (votes to the
// host, which decides), the kit-auto host-buffer calls (scan_batch_auto_impl: one batch, or consecutive batches of the file
// loop) and qcat_scan_resident_batches (a resident batch in chunks of whole vote batches), with qcat_ctx_fetch_kit_slots.
// Included by qcat_hip.hip behind filter_host.inc: it needs the context, scan_resident_impl, api_graph_run, batch_upload_windows,
// filter_run, grow, mark and stream_done.

// The vote's block for nb batches, as it lies in the context's vote buffer and in a host copy of it: votes [nb][MAX_T], first
// voters [nb][MAX_T], chosen slots [nb] -- one allocation, so that one copy brings all of it back.
struct VoteBuf {
    struct View { unsigned long long* votes; unsigned long long* first; int32_t* chosen; };
    size_t nb;
    size_t bytes;                                  // of the three arrays
    View dev;
    static View over(void* block, size_t nb) {
        unsigned long long* v = reinterpret_cast<unsigned long long*>(block);
        return View{v, v + nb * MAX_T, reinterpret_cast<int32_t*>(v + 2 * nb * MAX_T)};
    }
    View host(void* copy) const { return over(copy, nb); }
};
static int vote_buf(qcat_ctx* c, size_t nb, VoteBuf* v) {
    const size_t bytes = nb * (2 * MAX_T * 8 + 4);
    HIPCHK(c->vote_buf.ensure(bytes + 16));
    *v = VoteBuf{nb, bytes, VoteBuf::over(c->vote_buf.get(), nb)};
    return 0;
}

// The vote over the n_reads reads whose adapter pass lies in c->recs, in stream order behind that pass: the counters cleared,
// k_vote, and -- `chosen` given -- k_pick_kit, which decides every batch's kit slot there.  span_reads > 0: v.nb consecutive
// batches of that many reads, each with counters of its own; 0: one batch.  The caller's FillScope says how the counters are
// cleared: collected into one launch, or a memset each.
static int vote_enqueue(qcat_ctx* c, const KitOnDevice* kd, const VoteBuf& v, uint32_t n_reads, uint32_t span_reads, int32_t* chosen) {
    const uint32_t nb = (uint32_t)v.nb;
    HIPCHK(packed_fill(v.dev.votes, 0, v.nb * MAX_T * 8, c->stream));
    HIPCHK(packed_fill(v.dev.first, 0xFF, v.nb * MAX_T * 8, c->stream));
    HIPCHK(packed_fill_flush(c->stream));
    const uint32_t per = span_reads ? span_reads : n_reads;
    const uint32_t blocks = std::min<uint32_t>((per + 255) / 256, span_reads ? 64 : 1024);
    hipLaunchKernelGGL(k_vote, dim3(blocks, nb), dim3(256), 0, c->stream, kd->kit, c->recs, n_reads, v.dev.votes, v.dev.first, span_reads);
    if (chosen) hipLaunchKernelGGL(k_pick_kit, dim3(nb), dim3(64), 0, c->stream, kd->kit, v.dev.votes, v.dev.first, chosen);
    return 0;
}

// adapter-only pass over a resident batch + k_vote: per-template votes / first voting read (host arrays of MAX_T)
static int vote_resident(qcat_ctx* c, qcat_kit* kit, const qcat_batch* b, unsigned long long* hv, unsigned long long* hf) {
    for (int t = 0; t < MAX_T; ++t) { hv[t] = 0; hf[t] = ~0ull; }
    int rc = scan_resident_impl(c, kit, b, ScanPass::vote());
    // (a failed step drains the stream before it returns: the caller's upload may still be reading the pinned staging)
    auto drained = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    if (rc) return drained(rc);
    if (!b->n_reads) return 0;
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return drained(rc);
    VoteBuf v;
    if ((rc = vote_buf(c, 1, &v))) return drained(rc);
    {
        FillScope fills(false);                                  // (a memset each; the host decides: no k_pick_kit)
        if ((rc = vote_enqueue(c, kd, v, b->n_reads, 0, nullptr))) return rc;
    }
    HIPCHK(hipMemcpyAsync(hv, v.dev.votes, MAX_T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hf, v.dev.first, MAX_T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int qcat_detect_kit(qcat_ctx* c, const qcat_kit* ckit, const uint8_t* bases, const uint64_t* offsets,
                               uint32_t n_reads, int64_t* votes, int64_t* first_read) {
    if (!c || !ckit || !offsets || !votes || !first_read) return set_err(QCAT_ERR_ARG, "null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    if (kit->hk.dk.ends != QCAT_ENDS_BOTH) return set_err(QCAT_ERR_ARG, "qcat_detect_kit needs a kit created with QCAT_ENDS_BOTH");
    const int nt = kit->hk.dk.nt;
    unsigned long long hv[MAX_T], hf[MAX_T];
    qcat_batch* b = nullptr;
    int rc = batch_upload_windows(c, kit, bases, offsets, n_reads, &b);
    if (rc) return rc;
    rc = vote_resident(c, kit, b, hv, hf);
    qcat_batch_destroy(b);
    if (rc) return rc;
    for (int t = 0; t < nt; ++t) {
        votes[t] += (int64_t)hv[t];
        first_read[t] = hf[t] == ~0ull ? (int64_t)n_reads : (int64_t)hf[t];
    }
    return 0;
}

// What a kit-auto host-buffer call brings back, through the context's pinned block: the records, the vote's block as it lies
// on the device (votes, first voting reads, chosen slots: one allocation), the counts -- three DMAs and the call's one host
// synchronisation.  The views point into the pinned block: valid until the context's next call.
struct AutoReturn {
    const qcat_result* records;
    VoteBuf::View vote;
    const int64_t* counts;                         // (null: not asked for)
};
static int auto_fetch(qcat_ctx* c, const VoteBuf& v, uint32_t n_reads, int n_buckets, bool with_counts, AutoReturn* r) {
    const size_t bytes_rec = (size_t)n_reads * sizeof(qcat_result);
    const size_t off_vote = (bytes_rec + 63) / 64 * 64, off_cnt = (off_vote + v.bytes + 63) / 64 * 64;
    const size_t need_ret = off_cnt + (size_t)n_buckets * 8;
    if (need_ret > c->pin_ret.cap()) {
        (void)hipStreamSynchronize(c->stream);
        HIPCHK(c->pin_ret.ensure(need_ret + need_ret / 4));
    }
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(c->pin_ret, c->results, bytes_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(c->pin_ret + off_vote, v.dev.votes, v.bytes, hipMemcpyDeviceToHost, c->stream));
    if (with_counts) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(c->pin_ret + off_cnt, c->counts, (size_t)n_buckets * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    r->records = reinterpret_cast<const qcat_result*>(c->pin_ret.get());
    r->vote = v.host(c->pin_ret + off_vote);
    r->counts = with_counts ? reinterpret_cast<const int64_t*>(c->pin_ret + off_cnt) : nullptr;
    return 0;
}

// the kit-auto scan of one batch.  Round 4: ONE host synchronisation -- the vote is counted AND decided on the device
// (k_vote, k_pick_kit), the second pass reads the voted kit slot there (k_adapter_finish), and votes, choice, records and
// counts come back together.  (Round 3 waited for the upload, for the votes and for the records: three round trips in a call
// whose kernels take 0.3 ms.)
static int scan_batch_auto_impl(qcat_ctx* c, const qcat_kit* ckit, const uint8_t* bases, const uint64_t* offsets,
                                const uint8_t* const* ptrs, const uint64_t* lens,
                                uint32_t n_reads, qcat_result* out, int64_t* counts, int32_t* chosen_kit_slot,
                                int64_t* votes, int64_t* first_read, uint32_t batch_reads = 0) {
    // batch_reads > 0 (round 4, the kit-auto file loop): the reads are consecutive batches of that many reads, each votes for
    // a kit of its own (qcat/cli.py:500 calls detect_barcode_batch per batch) -- one adapter pass over all of them, the votes
    // counted and decided per batch (k_vote / k_pick_kit with a batch dimension), the second pass takes every read's kit slot
    // from its batch (k_adapter_finish: slot_span); chosen_kit_slot then has one entry per batch, votes / first_read are unused
    if (!c || !ckit || (n_reads && !offsets && !ptrs) || !out || !chosen_kit_slot) return set_err(QCAT_ERR_ARG, "qcat_scan_batch_auto: null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& hk = kit->hk.dk;
    if (hk.ends != QCAT_ENDS_BOTH) return set_err(QCAT_ERR_ARG, "qcat_scan_batch_auto needs a kit created with QCAT_ENDS_BOTH");
    const uint32_t nb = batch_reads ? (n_reads + batch_reads - 1) / batch_reads : 1u;
    for (uint32_t q = 0; q < std::max(1u, nb); ++q) chosen_kit_slot[q] = -1;
    if (!n_reads) return 0;                                     // (an empty batch: nobody votes, nothing to scan)
    if (batch_reads && (votes || first_read)) return set_err(QCAT_ERR_ARG, "qcat_scan_batches_auto: the per-template votes are reported for one batch only");
    qcat_batch* b = nullptr;
    int rc = batch_upload_windows(c, kit, bases, offsets, n_reads, &b, ptrs, lens);
    if (rc) return rc;
    BatchPtr guard(b);
    // (a failed step drains the stream before it returns: the upload may still be reading the pinned staging)
    auto drained = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return drained(rc);
    VoteBuf v;
    if ((rc = vote_buf(c, nb, &v))) return drained(rc);
    const uint32_t slot_span = batch_reads ? batch_reads * 2u : 0u;        // read ends per batch (both ends: checked above)
    // the device work of the call, in stream order behind the upload
    auto enqueue = [&]() -> int {
        // pass 1: every template of every kit against both ends (qcat/scanner_base.py:662-678)
        int e = scan_resident_impl(c, kit, b, ScanPass::vote());
        if (e) return e;
        {
            FillScope fills(true);
            if ((e = vote_enqueue(c, kd, v, n_reads, batch_reads, v.dev.chosen))) return e;
        }
        // pass 2: detect_barcode per read with the voted kit's templates (:714-733): the adapter alignments of the vote are
        // still on the device -- only their merge (the kit slot read from v.dev.chosen), the barcode phase and the finalisation run now
        c->packed.kit_slot_dev = v.dev.chosen; c->packed.kit_slot_span = slot_span;
        if (opt_on(QO_DEBUG_VOTE)) {                  // (diagnostics: the choice as the device made it, before the second pass)
            unsigned long long dv[2 * MAX_T]; int32_t dc = -7;
            (void)hipStreamSynchronize(c->stream);
            (void)hipMemcpy(dv, v.dev.votes, sizeof dv, hipMemcpyDeviceToHost);
            (void)hipMemcpy(&dc, v.dev.chosen, 4, hipMemcpyDeviceToHost);
            fprintf(stderr, "[qcat] vote: chosen %d (kit slots %d, templates %d):", dc, hk.n_kit_slots, hk.nt);
            for (int t = 0; t < hk.nt; ++t) fprintf(stderr, " %llu/slot%d", dv[t], hk.tpl[t].kit_slot);
            fprintf(stderr, "\n");
        }
        return scan_resident_impl(c, kit, b, ScanPass::resume(RESUME_KIT_ON_DEVICE));
    };
    if ((rc = api_graph_run(c->stream, c->timing, &c->packed, c->api_graph, kit, kd, b, batch_reads, enqueue,
                            [&] { c->packed.kit_slot_dev = v.dev.chosen; c->packed.kit_slot_span = slot_span; }))) return rc;
    AutoReturn ret;
    if ((rc = auto_fetch(c, v, n_reads, hk.n_buckets, counts != nullptr, &ret))) return rc;
    memcpy(out, ret.records, (size_t)n_reads * sizeof(qcat_result));
    if (!batch_reads)
        for (int t = 0; t < hk.nt; ++t) {
            if (votes) votes[t] += (int64_t)ret.vote.votes[t];
            if (first_read) first_read[t] = ret.vote.first[t] == ~0ull ? (int64_t)n_reads : (int64_t)ret.vote.first[t];
        }
    bool all_voted = true;
    for (uint32_t q = 0; q < nb; ++q) { chosen_kit_slot[q] = ret.vote.chosen[q]; all_voted = all_voted && ret.vote.chosen[q] >= 0; }
    if (!all_voted) return set_err(QCAT_ERR_DEVICE, "qcat_scan_batch_auto: no read voted");
    if (counts)
        for (size_t i = 0; i < (size_t)hk.n_buckets; ++i) counts[i] += ret.counts[i];
    return 0;
}

extern "C" int qcat_scan_batch_auto(qcat_ctx* c, const qcat_kit* ckit, const uint8_t* bases, const uint64_t* offsets,
                                    uint32_t n_reads, qcat_result* out, int64_t* counts, int32_t* chosen_kit_slot,
                                    int64_t* votes, int64_t* first_read) {
    return scan_batch_auto_impl(c, ckit, bases, offsets, nullptr, nullptr, n_reads, out, counts, chosen_kit_slot, votes, first_read);
}

extern "C" int qcat_scan_batch_auto_ptrs(qcat_ctx* c, const qcat_kit* ckit, const uint8_t* const* reads, const uint64_t* lengths,
                                         uint32_t n_reads, qcat_result* out, int64_t* counts, int32_t* chosen_kit_slot,
                                         int64_t* votes, int64_t* first_read) {
    if (n_reads && (!reads || !lengths)) return set_err(QCAT_ERR_ARG, "qcat_scan_batch_auto_ptrs: null argument");
    return scan_batch_auto_impl(c, ckit, nullptr, nullptr, reads, lengths, n_reads, out, counts, chosen_kit_slot, votes, first_read);
}

extern "C" int qcat_scan_batches_auto_ptrs(qcat_ctx* c, const qcat_kit* ckit, const uint8_t* const* reads, const uint64_t* lengths,
                                           uint32_t n_reads, uint32_t batch_reads, qcat_result* out, int64_t* counts, int32_t* chosen_kit_slots) {
    if (n_reads && (!reads || !lengths)) return set_err(QCAT_ERR_ARG, "qcat_scan_batches_auto_ptrs: null argument");
    if (!batch_reads) return set_err(QCAT_ERR_ARG, "qcat_scan_batches_auto_ptrs: batch_reads must be positive");
    if (batch_reads >= n_reads)                                 // one batch: the plain call (small batches upload whole reads)
        return scan_batch_auto_impl(c, ckit, nullptr, nullptr, reads, lengths, n_reads, out, counts, chosen_kit_slots, nullptr, nullptr);
    if ((uint64_t)(n_reads + batch_reads - 1) / batch_reads > 65535u) return set_err(QCAT_ERR_ARG, "qcat_scan_batches_auto_ptrs: more than 65535 batches in one call");
    return scan_batch_auto_impl(c, ckit, nullptr, nullptr, reads, lengths, n_reads, out, counts, chosen_kit_slots, nullptr, nullptr, batch_reads);
}

// ------------------------------------------------------------------------------------------
// the driver's per-batch semantics on a resident batch: kit vote and --filter-barcodes without leaving the device
// ------------------------------------------------------------------------------------------
// what one such scan is: the batches of the vote and of the filter, and the chunks the adapter passes of a vote take them in
struct ResidentBatchesJob {
    uint32_t n, per, n_batches;         // per: reads of a batch (the whole resident batch when the caller gave 0 or more than it holds)
    uint32_t chunk_batches;             // batches per adapter pass of a kit vote
    bool kit_auto, filter;
};

static int resident_batches_check(const qcat_ctx* c, const qcat_kit* kit, const qcat_batch* b, uint32_t flags) {
    if (!c || !kit || !b) return set_err(QCAT_ERR_ARG, "qcat_scan_resident_batches: null argument");
    if (flags & ~(uint32_t)(QCAT_RESIDENT_KIT_AUTO | QCAT_RESIDENT_FILTER_BARCODES))
        return set_err(QCAT_ERR_ARG, "qcat_scan_resident_batches: unknown flag");
    if (b->device != c->device) return set_err(QCAT_ERR_ARG, "batch lives on another device than the context");
    const DevKit& hk = kit->hk.dk;
    if ((flags & QCAT_RESIDENT_KIT_AUTO) && hk.mode == QCAT_MODE_SIMPLE)
        return set_err(QCAT_ERR_ARG, "qcat_scan_resident_batches: simple mode has no kits to vote for (QCAT_RESIDENT_KIT_AUTO)");
    if ((flags & QCAT_RESIDENT_KIT_AUTO) && hk.ends != QCAT_ENDS_BOTH)
        return set_err(QCAT_ERR_ARG, "qcat_scan_resident_batches: QCAT_RESIDENT_KIT_AUTO needs a kit created with QCAT_ENDS_BOTH");
    return 0;
}

// the batches and the chunks; a scan this call could not finish is refused here, before anything is enqueued
static int resident_batches_plan(const DevKit& hk, const qcat_batch* b, uint32_t batch_reads, uint32_t flags, ResidentBatchesJob& j) {
    j.n = b->n_reads;
    j.kit_auto = (flags & QCAT_RESIDENT_KIT_AUTO) != 0; j.filter = (flags & QCAT_RESIDENT_FILTER_BARCODES) != 0;
    j.per = (batch_reads == 0 || batch_reads >= j.n) ? j.n : batch_reads;
    j.n_batches = (j.n + j.per - 1) / j.per;
    // one adapter pass over every template of every kit holds its alignments for the resumed pass: the file loop takes a
    // million reads per call at most (fastq_host.inc), and so does this -- whole vote batches, 65535 of them at most (the
    // grid of k_vote); a single batch larger than that is one pass, as it is for qcat_scan_resident
    const uint64_t chunk_reads = (uint64_t)std::max<int64_t>(1, opt_val(QO_RESIDENT_AUTO_CHUNK, (int64_t)1 << 20));
    j.chunk_batches = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(chunk_reads / j.per, 1), 65535);
    if (!j.kit_auto || j.n_batches <= j.chunk_batches) j.chunk_batches = j.n_batches;
    // the interior scan reads its batch from the first base on (absm_c2, the search of a base's read): it takes no view that
    // starts inside a batch
    if (j.kit_auto && hk.scan_middle && j.n_batches > j.chunk_batches)
        return set_err(QCAT_ERR_UNSUPPORTED, "qcat_scan_resident_batches: a kit vote with scan_middle_adapter takes one adapter pass "
                                             "(QCAT_HIP_RESIDENT_AUTO_CHUNK reads, 65535 batches) at most; scan the batch in parts");
    return 0;
}

// one chunk of a kit vote: the vote pass over every template, the votes counted and decided per batch on the device, the
// resumed pass with every read's kit slot from its batch -- the sequence of scan_batch_auto_impl over a view of the resident
// batch, the slots kept in c->kit_slots, the records from read r0 on in c->results
static int resident_vote_chunk(qcat_ctx* c, qcat_kit* kit, KitOnDevice* kd, const qcat_batch* b, const ResidentBatchesJob& j, uint32_t q0, uint32_t qn) {
    const uint32_t r0 = q0 * j.per, rn = (uint32_t)std::min<uint64_t>(j.n - r0, (uint64_t)qn * j.per);
    const qcat_batch view = batch_view(b->device, rn, b->n_bases, b->bases, b->offsets + r0, nullptr);
    const uint32_t span_reads = j.n_batches > 1 ? j.per : 0u;           // (0: one batch, one slot -- the form of qcat_scan_batch_auto)
    int rc;
    c->res_first = r0;
    if ((rc = scan_resident_impl(c, kit, &view, ScanPass::vote().keeping_counts(q0 > 0)))) return rc;
    VoteBuf v;
    if ((rc = vote_buf(c, qn, &v))) return rc;
    int32_t* chosen = c->kit_slots + q0;
    {
        FillScope fills(true);
        if ((rc = vote_enqueue(c, kd, v, rn, span_reads, chosen))) return rc;
    }
    c->packed.kit_slot_dev = chosen; c->packed.kit_slot_span = span_reads * 2u;
    return scan_resident_impl(c, kit, &view, ScanPass::resume(RESUME_KIT_ON_DEVICE).keeping_counts(q0 > 0).deferring_counts(j.filter));
}

extern "C" int qcat_scan_resident_batches(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, uint32_t batch_reads, uint32_t flags) {
    int rc = resident_batches_check(c, ckit, b, flags);
    if (rc) return rc;
    if (!flags) return qcat_scan_resident(c, ckit, b);                  // the same launches, the same records
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& hk = kit->hk.dk;
    if (!b->n_reads) {                                                  // nobody votes, nothing to filter: zero batches
        if ((rc = scan_resident_impl(c, kit, b, ScanPass::plain()))) return rc;
        if (flags & QCAT_RESIDENT_KIT_AUTO) c->auto_batches = 0;
        return 0;
    }
    if (b->true_len) return set_err(QCAT_ERR_ARG, "qcat_scan_resident_batches: the batch holds read windows, not whole reads");
    ResidentBatchesJob j{};
    if ((rc = resident_batches_plan(hk, b, batch_reads, flags, j))) return rc;
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    if ((rc = kit_on_device(kit, c->device, &kd))) return rc;
    // a failure below leaves no scan behind: no records to fetch or to partition, no slots
    auto failed = [&](int code) { c->res_first = 0; c->last_kit = nullptr; c->last_n_reads = 0; c->auto_batches = -1; return code; };
    if (j.kit_auto) {
        // the records of every chunk in read order in c->results: sized for the whole batch first, so that no chunk's scan moves it
        if ((rc = grow(c->results, (size_t)j.n))) return failed(rc);
        if ((rc = grow(c->kit_slots, (size_t)j.n_batches))) return failed(rc);
        for (uint32_t q0 = 0; q0 < j.n_batches; q0 += j.chunk_batches)
            if ((rc = resident_vote_chunk(c, kit, kd, b, j, q0, std::min(j.chunk_batches, j.n_batches - q0)))) return failed(rc);
        c->res_first = 0;
    } else if ((rc = scan_resident_impl(c, kit, b, ScanPass::plain().deferring_counts(true)))) return failed(rc);
    if (j.filter) {
        // behind k_finalize and the interior scan, in front of the counts: the counts are those of the filtered records
        const KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
        if ((rc = filter_run(c, hk, kp, c->results, j.n, j.per))) return failed(rc);
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((j.n + 255) / 256, hk.n_buckets > 2048 ? 512 : 1024);
        hipLaunchKernelGGL(k_count, dim3(blocks), dim3(256), 0, c->stream, kp, (const qcat_result*)c->results.get(), (const uint64_t*)b->offsets,
                           (const uint32_t*)nullptr, j.n, c->counts.get());
        mark(c, "k_count");
        if (hipGetLastError() != hipSuccess) return failed(set_err(QCAT_ERR_DEVICE, "qcat_scan_resident_batches: launch of k_count failed"));
    }
    c->last_kit = kit; c->last_n_reads = j.n; c->last_buckets = hk.n_buckets;
    c->auto_batches = j.kit_auto ? (int64_t)j.n_batches : -1;
    return 0;
}

extern "C" int qcat_ctx_fetch_kit_slots(qcat_ctx* c, int32_t* slots, uint32_t n_batches) {
    if (!c || (!slots && n_batches)) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_kit_slots: null argument");
    if (c->auto_batches < 0)
        return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_kit_slots: this context's latest scan was no qcat_scan_resident_batches with QCAT_RESIDENT_KIT_AUTO");
    if ((int64_t)n_batches != c->auto_batches) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_kit_slots: n_batches does not match the latest scan");
    HIPCHK(hipSetDevice(c->device));
    if (n_batches) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(slots, c->kit_slots, (size_t)n_batches * 4, hipMemcpyDeviceToHost, c->stream));
    return stream_done(c, "qcat_ctx_fetch_kit_slots");
}

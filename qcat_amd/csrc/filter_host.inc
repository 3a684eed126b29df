// filter_host.inc -- --filter-barcodes on records in device memory: the host steps around kernels_filter.inc (the arithmetic:
// filter_core.h; the scratch: FilterScratch in batch.h) and qcat_filter_barcodes, the filter alone on records a caller holds
// on the host.  qcat_scan_resident_batches (qcat_hip.hip) runs filter_run on the records of its scan.
// Included by qcat_hip.hip behind batch_host.inc: it needs the context, mark, grow, stream_done and part_records_fit.

// what one filter is: the records on the device, their batches, the row of a batch and the rounds the table's budget allows
struct FilterJob {
    KitPtrs kp;
    qcat_result* recs;
    uint32_t n, batch_reads, n_batches;        // batch_reads >= 1: reads [q * batch_reads, (q + 1) * batch_reads) are batch q
    uint32_t n_bins, key_bits;
    uint32_t rows;                             // batches per round
};

// the batches, the row and the rounds; the table and the floors sized for one round
static int filter_plan(qcat_ctx* c, const DevKit& hk, uint32_t n, uint32_t batch_reads, FilterJob& j) {
    j.n = n;
    j.batch_reads = (batch_reads == 0 || batch_reads > n) ? std::max(n, 1u) : batch_reads;
    j.n_batches = (n + j.batch_reads - 1) / j.batch_reads;
    j.n_bins = qfilt::bins_of(hk.mode == QCAT_MODE_DUAL, (uint32_t)hk.n_barcode_slots);
    j.key_bits = qfilt::key_bits(j.n_bins);
    // the table is batches x bins x 4 bytes -- 147 MB for 4000 batches of the shipped dual kit: the batches are taken in rounds
    // whose rows fit the budget (QCAT_HIP_FILTER_TABLE_BYTES, default 64 MiB; one batch at least; 65535: the grid's y limit)
    const uint64_t budget = (uint64_t)std::max<int64_t>(0, opt_val(QO_FILTER_TABLE_BYTES, (int64_t)64 << 20));
    const uint64_t fit = budget / ((uint64_t)j.n_bins * 4);
    j.rows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(fit, 1), std::min<uint32_t>(std::max(j.n_batches, 1u), 65535u));
    FilterScratch& F = c->batch.filter;
    int rc;
    if ((rc = grow(F.table, (size_t)j.rows * j.n_bins))) return rc;
    if ((rc = grow(F.floor, j.rows))) return rc;
    return 0;
}

// one round: batches [q0, q0 + nb) counted, floored and rewritten; the rows are cleared by the fill list
static int filter_round(qcat_ctx* c, const FilterJob& j, uint32_t q0, uint32_t nb) {
    FilterScratch& F = c->batch.filter;
    const uint64_t first = (uint64_t)q0 * j.batch_reads;
    qcat_result* const recs = j.recs + first;
    const uint32_t n_call = (uint32_t)(j.n - first);                                            // records to the end of the call
    const uint32_t n_round = (uint32_t)std::min<uint64_t>(n_call, (uint64_t)nb * j.batch_reads);  // records of this round
    {
        FillScope fills(true);
        HIPCHK(packed_fill(F.table, 0, (size_t)nb * j.n_bins * 4, c->stream));
        HIPCHK(packed_fill_flush(c->stream));
    }
    const uint32_t per_batch = std::min<uint32_t>((j.batch_reads + 255) / 256, 64);
    hipLaunchKernelGGL(k_filter_hist, dim3(per_batch, nb), dim3(256), 0, c->stream, j.kp, (const qcat_result*)recs, n_call, j.batch_reads,
                       j.n_bins, j.key_bits, F.table.get());
    mark(c, "filter_hist");
    hipLaunchKernelGGL(k_filter_floor, dim3(nb), dim3(256), 0, c->stream, (const uint32_t*)F.table.get(), j.n_bins, F.floor.get());
    mark(c, "filter_floor");
    hipLaunchKernelGGL(k_filter_apply, dim3(std::min<uint32_t>((n_round + 255) / 256, 4096)), dim3(256), 0, c->stream, j.kp, recs, n_round,
                       j.batch_reads, j.n_bins, (const uint32_t*)F.table.get(), (const uint32_t*)F.floor.get());
    mark(c, "filter_apply");
    HIPCHK(hipGetLastError());
    return 0;
}

// the filter over n records on the device, batch by batch, in stream order; nothing here waits for the device.  (A scan of
// several rounds repeats the three marks; the timing ring keeps the first MAX_TIMED marks of a call.)
static int filter_run(qcat_ctx* c, const DevKit& hk, KitPtrs kp, qcat_result* recs, uint32_t n, uint32_t batch_reads) {
    if (!n) return 0;
    FilterJob j{};
    j.kp = kp; j.recs = recs;
    if (int rc = filter_plan(c, hk, n, batch_reads, j)) return rc;
    for (uint32_t q0 = 0; q0 < j.n_batches; q0 += j.rows)
        if (int rc = filter_round(c, j, q0, std::min(j.rows, j.n_batches - q0))) return rc;
    return 0;
}

extern "C" int qcat_filter_barcodes(qcat_ctx* c, const qcat_kit* ckit, qcat_result* records, uint32_t n_reads, uint32_t batch_reads) {
    if (!c || !ckit || (!records && n_reads)) return set_err(QCAT_ERR_ARG, "qcat_filter_barcodes: null argument");
    if (!n_reads) return 0;
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& hk = kit->hk.dk;
    if (!part_records_fit(hk, records, n_reads))
        return set_err(QCAT_ERR_ARG, "qcat_filter_barcodes: a record indexes outside the kit's templates / barcode sets or has a negative trim");
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    int rc = kit_on_device(kit, c->device, &kd);
    if (rc) return rc;
    FilterScratch& F = c->batch.filter;
    const size_t bytes = (size_t)n_reads * sizeof(qcat_result);
    if ((rc = grow(F.recs, n_reads))) return rc;
    // the way back: the context's pinned block while the records fit 8 MiB of it (one DMA), else straight to the caller's array
    const bool pinned = bytes <= ((size_t)8 << 20);
    if (pinned && bytes > c->pin_ret.cap()) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(c->pin_ret.ensure(bytes + bytes / 4 + 4096));
    }
    timing_slot(c);
    if (c->timing) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(F.recs, records, bytes, hipMemcpyHostToDevice, c->stream));
    rc = filter_run(c, hk, KitPtrs{kd->kit, kd->codes, kd->ids, kd->tables}, F.recs, n_reads, batch_reads);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(pinned ? (void*)c->pin_ret.get() : (void*)records, F.recs, bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stream_done(c, "qcat_filter_barcodes"))) return rc;
    if (pinned) memcpy(records, c->pin_ret, bytes);
    return 0;
}

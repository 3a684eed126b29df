// batch_host.inc -- the functions of the resident batch (the types: batch.h): upload and download of whole reads, the upload
// of a host-buffer call (batch_upload_windows; its device-free part: upload_core.h), batches from and as device pointers, the
// stable partition by barcode (kernels_partition.inc) and synthetic batches.
// Included by qcat_hip.hip behind mark(): it needs the context, timing_slot and mark, and the error helpers of that file.
#include "upload_core.h"

extern "C" void qcat_batch_destroy(qcat_batch* b) {
    if (!b) return;
    int cur = 0; (void)hipGetDevice(&cur);
    (void)hipSetDevice(b->device);
    delete b;                                      // (an owned batch's planes free themselves; a view has none)
    (void)hipSetDevice(cur);
}

// an owned batch of n_reads reads and n_bases bases on `device` under its guard (with_quals: a quality plane as well), or this
// layer's out-of-memory error with the text `err`
static int batch_make(int device, uint32_t n_reads, uint64_t n_bases, bool with_quals, const char* err, BatchPtr* out) {
    BatchPtr b(new qcat_batch());
    b->device = device; b->n_reads = n_reads; b->n_bases = n_bases;
    if (!b->alloc(with_quals)) return set_err(QCAT_ERR_NOMEM, err);
    *out = std::move(b);
    return 0;
}

// the stream's work is done and nothing went wrong in it, or the device error under the caller's name
static int stream_done(qcat_ctx* c, const char* who) {
    hipError_t es = hipStreamSynchronize(c->stream);
    if (es == hipSuccess) es = hipGetLastError();
    if (es != hipSuccess) return set_err(QCAT_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(es));
    return 0;
}

extern "C" int qcat_batch_info(const qcat_batch* b, uint32_t* n_reads, uint64_t* n_bases) {
    if (!b) return set_err(QCAT_ERR_ARG, "null batch");
    if (n_reads) *n_reads = b->n_reads;
    if (n_bases) *n_bases = b->n_bases;
    return 0;
}

// qcat_batch_upload (with_quals false: `qualities` is not looked at) and qcat_batch_upload_fastq
static int batch_upload_planes(qcat_ctx* c, const uint8_t* bases, const uint8_t* qualities, bool with_quals, const uint64_t* offsets,
                               uint32_t n_reads, qcat_batch** out, const char* null_msg) {
    if (!c || !offsets || !out || (!bases && n_reads && offsets[n_reads] > 0) || (with_quals && !qualities && n_reads && offsets[n_reads] > 0))
        return set_err(QCAT_ERR_ARG, null_msg);
    if (offsets[0] != 0) return set_err(QCAT_ERR_ARG, "offsets[0] must be 0");
    for (uint32_t r = 0; r < n_reads; ++r)
        if (offsets[r + 1] < offsets[r]) return set_err(QCAT_ERR_ARG, "offsets must be non-decreasing");
    HIPCHK(hipSetDevice(c->device));
    BatchPtr b;
    if (int rc = batch_make(c->device, n_reads, offsets[n_reads], with_quals, "hipMalloc failed for batch", &b)) return rc;
    if (b->n_bases) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->bases, bases, b->n_bases, hipMemcpyHostToDevice, c->stream));
    if (with_quals && b->n_bases) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->quals, qualities, b->n_bases, hipMemcpyHostToDevice, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->offsets, offsets, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = b.release();
    return 0;
}

extern "C" int qcat_batch_upload(qcat_ctx* c, const uint8_t* bases, const uint64_t* offsets,
                                 uint32_t n_reads, qcat_batch** out) {
    return batch_upload_planes(c, bases, nullptr, false, offsets, n_reads, out, "qcat_batch_upload: null argument");
}

extern "C" int qcat_batch_upload_fastq(qcat_ctx* c, const uint8_t* bases, const uint8_t* qualities, const uint64_t* offsets,
                                       uint32_t n_reads, qcat_batch** out) {
    return batch_upload_planes(c, bases, qualities, true, offsets, n_reads, out, "qcat_batch_upload_fastq: null argument");
}

extern "C" int qcat_batch_has_qualities(const qcat_batch* b) {
    if (!b) return set_err(QCAT_ERR_ARG, "null batch");
    return b->quals ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// the upload of a host-buffer call: batch_upload_windows and its steps
// ------------------------------------------------------------------------------------------
static int upload_refused(qupload::Refusal why) {
    switch (why) {
        case qupload::NULL_READ: return set_err(QCAT_ERR_ARG, "null read pointer");
        case qupload::DECREASING: return set_err(QCAT_ERR_ARG, "offsets must be non-decreasing");
        case qupload::TOO_LONG: return set_err(QCAT_ERR_UNSUPPORTED, "read longer than 4 Gb");
        default: return 0;
    }
}

// more than a gigabyte of whole reads: the plain upload into a batch of its own (the staging is pinned memory and stays with
// the context); reads that came as pointers are concatenated by this thread first
static int upload_whole_plain(qcat_ctx* c, const qupload::Reads& in, qcat_batch** out) {
    if (!in.ptrs) return qcat_batch_upload(c, in.bases, in.offsets, in.n, out);
    const qupload::Keep all = qupload::keep_of(0, false, true);
    std::vector<uint64_t> cat_off((size_t)in.n + 1);
    uint64_t tot = 0;
    if (int rc = upload_refused(qupload::length_pass(in, all, nullptr, cat_off.data(), &tot))) return rc;
    std::vector<uint8_t> cat((size_t)tot + 1);
    qupload::compact(in, all, cat_off.data(), cat.data(), 0, in.n);
    return qcat_batch_upload(c, cat.data(), cat_off.data(), in.n, out);
}

// room for the lengths and staged offsets of n_reads reads in the pinned staging
static int upload_grow_index(qcat_ctx* c, uint32_t n_reads) {
    if ((size_t)n_reads + 1 > std::min(c->pin_offsets.cap(), c->pin_len.cap())) {
        HIPCHK(c->pin_offsets.ensure((size_t)n_reads + 1));
        HIPCHK(c->pin_len.ensure((size_t)n_reads + 1));
        g_alloc_gen.fetch_add(1);                                      // (kernels of a handful-of-reads call read the staging in place)
    }
    return 0;
}

// room for `total` staged bytes of n_reads reads: the pinned staging, then the context's own device staging (the batch is a
// view of it: one host-buffer call at a time per context)
static int upload_grow_staging(qcat_ctx* c, uint32_t n_reads, uint64_t total) {
    if (total + 1 + 2 * BATCH_SLACK > c->pin_bases.cap()) {
        HIPCHK(c->pin_bases.ensure(total + 1 + 2 * BATCH_SLACK));                        // (slack either side like a device batch)
        memset(c->pin_bases, 0, BATCH_SLACK);
        g_alloc_gen.fetch_add(1);
    }
    if (total + 2 * BATCH_SLACK > c->hb_bases.cap() && c->hb_bases.ensure((total + 2 * BATCH_SLACK) * 5 / 4) != hipSuccess)
        return set_err(QCAT_ERR_NOMEM, "hipMalloc failed for batch");
    if ((size_t)n_reads + 1 > std::min(c->hb_offsets.cap(), c->hb_len.cap())) {
        const size_t want = ((size_t)n_reads + 1) * 5 / 4;
        if (c->hb_offsets.ensure(want) != hipSuccess || c->hb_len.ensure(want) != hipSuccess)
            return set_err(QCAT_ERR_NOMEM, "hipMalloc failed for batch");
    }
    return 0;
}

// the reads into the pinned staging on a few host threads (upload_core.h); *sent: the bases have gone to the device slice by slice
static int upload_compact(qcat_ctx* c, const qupload::Reads& in, const qupload::Keep& k, uint64_t total, bool* sent) {
    uint8_t* const pin_data = c->pin_bases + BATCH_SLACK;
    uint8_t* const dev_data = c->hb_bases + BATCH_SLACK;
    const uint64_t* const off = c->pin_offsets;
    const unsigned nthreads = std::min<unsigned>(host_threads(), (unsigned)std::max<uint64_t>(1u, std::max<uint64_t>(in.n / 16384u, total >> 23)));
    auto work = [&](uint32_t r0, uint32_t r1) { qupload::compact(in, k, off, pin_data, r0, r1); };
    // a big staging (round 6: whole reads of --detect-middle are 130 MB per segment of the file loop) in slices of ~8 MB that
    // the workers draw from a counter: this thread sends every finished run of slices on while the others are still being
    // copied -- the transfer hides behind the compaction instead of following it
    const uint64_t slice_bytes = 8ull << 20;
    *sent = nthreads >= 2 && total >= 4 * slice_bytes;
    if (!*sent) { qupload::run_even(in.n, nthreads, work); return 0; }
    hipError_t ce = hipSuccess;
    qupload::run_sliced(qupload::slice_bounds(off, in.n, total, slice_bytes), off, nthreads, work, [&](uint64_t o0, uint64_t o1) {
        ce = hipMemcpyAsync(dev_data + o0, pin_data + o0, o1 - o0, hipMemcpyHostToDevice, c->stream);
        return ce == hipSuccess;
    });
    if (ce != hipSuccess) { (void)hipStreamSynchronize(c->stream); return set_err(QCAT_ERR_DEVICE, std::string("upload: ") + hipGetErrorString(ce)); }
    return 0;
}

// Host-buffer entry points scan only the first / last max_align_length bases of a read, so that is
// all they send over PCIe: every read is compacted to head + tail (reads up to 2n stay whole, which
// keeps the two windows byte-identical), the real length travels in a separate array for the trims.
// The compaction runs on a few host threads into pinned memory.  --detect-middle needs whole reads.
// `ptrs` / `lens` (both or neither): the reads as one pointer and one length per read instead of the concatenated form
// (qcat_scan_batch_ptrs: a host language that holds a string object per read passes the objects' own buffers)
static int batch_upload_windows(qcat_ctx* c, const qcat_kit* kit, const uint8_t* bases, const uint64_t* offsets,
                                uint32_t n_reads, qcat_batch** out, const uint8_t* const* ptrs = nullptr, const uint64_t* lens = nullptr) {
    const DevKit& hk = kit->hk.dk;
    const qupload::Reads in{bases, offsets, ptrs, lens, n_reads};
    // the paths that take WHOLE reads (--detect-middle: the interior scan; QCAT_HIP_FULL_UPLOAD): round 6 -- through the same pinned
    // staging, host threads and context-owned device buffers as the windows (a read is "compacted" to all of itself).  Before,
    // they were concatenated by one thread into pageable memory and went through qcat_batch_upload: a hipMalloc / hipFree and a
    // pageable copy per call -- 21 ms per 173 000-read segment of the driver's file loop, whose scan takes 1 ms.  Batches
    // of more than a gigabyte keep the plain upload.
    const bool whole = hk.scan_middle || opt_on(QO_FULL_UPLOAD);
    if (whole && c && (ptrs || offsets)) {
        uint64_t tot = 0;
        if (ptrs) for (uint32_t r = 0; r < n_reads; ++r) tot += lens[r];
        else tot = offsets[n_reads];
        if (tot > (1ull << 30)) return upload_whole_plain(c, in, out);
    }
    if (!c || !out || (!ptrs && (!offsets || (!bases && offsets[n_reads] > 0)))) return set_err(QCAT_ERR_ARG, "qcat_scan_batch: null argument");
    if (!ptrs && offsets[0] != 0) return set_err(QCAT_ERR_ARG, "offsets[0] must be 0");
    HIPCHK(hipSetDevice(c->device));
    const qupload::Keep k = qupload::keep_of((uint64_t)hk.max_align, hk.ends == QCAT_ENDS_BOTH, whole);
    int rc;
    uint64_t total = 0;
    bool sent = false;
    if ((rc = upload_grow_index(c, n_reads))) return rc;
    if ((rc = upload_refused(qupload::length_pass(in, k, c->pin_len, c->pin_offsets, &total)))) return rc;
    if ((rc = upload_grow_staging(c, n_reads, total))) return rc;
    if ((rc = upload_compact(c, in, k, total, &sent))) return rc;
    uint8_t* const pin_data = c->pin_bases + BATCH_SLACK;
    // a handful of reads (detect_barcode on one read): the kernels read the pinned staging in place -- host memory the device
    // maps at the same address -- instead of waiting for three copies of a few hundred bytes (~4.5 us each in the call's chain)
    if (n_reads <= 64 && !whole && !sent && !opt_on(QO_NO_ZERO_COPY)) {
        memset(pin_data + total, 0, 1 + BATCH_SLACK);
        *out = new qcat_batch(batch_view(c->device, n_reads, total, pin_data, c->pin_offsets, c->pin_len));
        return 0;
    }
    BatchPtr b(new qcat_batch(batch_view(c->device, n_reads, total, c->hb_bases + BATCH_SLACK, c->hb_offsets, c->hb_len)));
    if (total && !sent) HIPCHK(hipMemcpyAsync(b->bases, pin_data, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b->offsets, c->pin_offsets, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b->true_len, c->pin_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, c->stream));
    // (no synchronisation here: every caller hands results back to the host and drains the stream for that before it returns,
    //  so the pinned staging is free again when the next call fills it -- one round trip less per 4000-read batch)
    *out = b.release();
    return 0;
}

extern "C" int qcat_batch_download(qcat_ctx* c, const qcat_batch* b, uint8_t* bases, uint64_t* offsets) {
    if (!c || !b) return set_err(QCAT_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if (offsets) HIPCHK(hipMemcpyAsync(offsets, b->offsets, ((size_t)b->n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (bases && b->n_bases) HIPCHK(hipMemcpyAsync(bases, b->bases, b->n_bases, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int qcat_batch_download_qualities(qcat_ctx* c, const qcat_batch* b, uint8_t* qualities) {
    if (!c || !b) return set_err(QCAT_ERR_ARG, "qcat_batch_download_qualities: null argument");
    if (!b->quals) return set_err(QCAT_ERR_ARG, "qcat_batch_download_qualities: the batch has no quality plane");
    if (!qualities && b->n_bases) return set_err(QCAT_ERR_ARG, "qcat_batch_download_qualities: null argument");
    HIPCHK(hipSetDevice(c->device));
    if (b->n_bases) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(qualities, b->quals, b->n_bases, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------
// batches from and as device pointers
// ------------------------------------------------------------------------------------------
// `p` is device memory of `device` (not host, not managed) with at least `bytes` bytes of its allocation behind it
static bool devmem_holds(const void* p, int device, uint64_t bytes) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }      // (a plain host pointer: an error, or "unregistered")
    if (at.type != hipMemoryTypeDevice || at.isManaged || at.device != device) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return false; }
    const uintptr_t lo = (uintptr_t)base, at_p = (uintptr_t)p;
    return at_p >= lo && at_p - lo <= size && (uint64_t)(size - (at_p - lo)) >= bytes;
}

extern "C" int qcat_batch_from_device(qcat_ctx* c, const void* d_bases, const void* d_qualities, const void* d_offsets,
                                      uint32_t n_reads, qcat_batch** out) {
    // nothing is trusted: a wrong offset would make a later kernel read out of bounds.  The checks in this order; nothing in
    // front of the final copies touches a byte that has not been checked.
    if (!c || !d_bases || !d_offsets || !out) return set_err(QCAT_ERR_ARG, "qcat_batch_from_device: null argument");
    if ((uintptr_t)d_offsets & 7u) return set_err(QCAT_ERR_ARG, "qcat_batch_from_device: d_offsets is not aligned to 8 bytes");
    HIPCHK(hipSetDevice(c->device));
    const uint64_t off_bytes = ((uint64_t)n_reads + 1) * 8;
    // device memory of this device, every pointer (zero bytes asked for: the attributes alone)
    if (!devmem_holds(d_offsets, c->device, 0) || !devmem_holds(d_bases, c->device, 0) || (d_qualities && !devmem_holds(d_qualities, c->device, 0)))
        return set_err(QCAT_ERR_ARG, "qcat_batch_from_device: a pointer is not device memory of the context's device");
    if (!devmem_holds(d_offsets, c->device, off_bytes))
        return set_err(QCAT_ERR_ARG, "qcat_batch_from_device: the allocation behind d_offsets is shorter than n_reads + 1 offsets");
    const uint64_t* offs = static_cast<const uint64_t*>(d_offsets);
    uint64_t ends[2] = {0, 0};                                 // offsets[0], offsets[n_reads]
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&ends[0], offs, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&ends[1], offs + n_reads, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint64_t total = ends[1];
    if (!devmem_holds(d_bases, c->device, total) || (d_qualities && !devmem_holds(d_qualities, c->device, total)))
        return set_err(QCAT_ERR_ARG, "qcat_batch_from_device: the allocation behind d_bases / d_qualities is shorter than offsets[n_reads] bytes");
    int rc;
    DevBuf<uint32_t>& offs_bad = c->batch.offs_bad;
    if ((rc = grow(offs_bad, 1))) return rc;
    HIPCHK(hipMemsetAsync(offs_bad, 0, 4, c->stream));
    hipLaunchKernelGGL(k_offsets_check, dim3(std::min<uint32_t>(n_reads / 256 + 1, 4096)), dim3(256), 0, c->stream, offs, n_reads, offs_bad.get());
    uint32_t bad = 0;
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&bad, offs_bad, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stream_done(c, "qcat_batch_from_device"))) return rc;
    if (bad || ends[0] != 0) return set_err(QCAT_ERR_ARG, "qcat_batch_from_device: offsets[0] must be 0 and the offsets non-decreasing");
    // an owned batch with the library's slack and alignment (the kernels rely on both): device-to-device on the context's stream
    BatchPtr b;
    if ((rc = batch_make(c->device, n_reads, total, d_qualities != nullptr, "hipMalloc failed for batch", &b))) return rc;
    if (total) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->bases, d_bases, total, hipMemcpyDeviceToDevice, c->stream));
    if (total && d_qualities) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->quals, d_qualities, total, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(b->offsets, d_offsets, off_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = b.release();
    return 0;
}

extern "C" int qcat_batch_devptrs(const qcat_batch* b, const void** bases, const void** qualities, const void** offsets) {
    if (!b) return set_err(QCAT_ERR_ARG, "qcat_batch_devptrs: null batch");
    if (b->true_len || !b->owned())
        return set_err(QCAT_ERR_ARG, "qcat_batch_devptrs: the batch holds read windows or borrowed buffers, not whole reads of its own");
    if (bases) *bases = b->bases;
    if (qualities) *qualities = b->quals;
    if (offsets) *offsets = b->offsets;
    return 0;
}

// ------------------------------------------------------------------------------------------
// stable partition of a resident batch by barcode (kernels_partition.inc)
// ------------------------------------------------------------------------------------------
static int part_bins_of(const DevKit& hk) {
    return (hk.mode == QCAT_MODE_DUAL ? hk.n_barcode_slots * hk.n_barcode_slots : hk.n_barcode_slots) + 2;
}
extern "C" int qcat_kit_partition_bins(const qcat_kit* k) { return k ? part_bins_of(k->hk.dk) : QCAT_ERR_ARG; }

// records of a caller index the kit's tables on the device: every index inside them, as a scan writes them
static bool part_records_fit(const DevKit& hk, const qcat_result* recs, uint32_t n) {
    for (uint32_t r = 0; r < n; ++r) {
        const qcat_result& q = recs[r];
        if (q.adapter_idx < -1 || q.adapter_idx >= hk.nt || q.barcode_idx < -1 || q.trim5p < 0 || q.trim3p < 0) return false;
        if (q.barcode_idx < 0) continue;
        if (q.adapter_idx < 0 && hk.mode != QCAT_MODE_SIMPLE) continue;              // (no call: the indices are not looked at)
        const DevTpl& t = hk.tpl[q.adapter_idx < 0 ? 0 : q.adapter_idx];
        if (q.barcode_idx >= t.sets[0].n) return false;
        if (hk.mode == QCAT_MODE_DUAL && (q.barcode2_idx < 0 || q.barcode2_idx >= t.sets[1].n)) return false;
    }
    return true;
}

// what one partition is: the inputs, the sizes derived from them, and where its sorted keys and read order end up
struct PartJob {
    const qcat_batch* in;
    qcat_batch* out;
    KitPtrs kp;
    const qcat_result* recs;            // on the device: the context's latest scan, or the records a caller handed over
    uint32_t n, n_bins, passes, n_wg;
    uint64_t max_chunks;
    const uint32_t* key_sorted;
    uint32_t* source;
};

// what the partition shares with the text products of a batch (text_out_host.inc)
static int batch_call_check(const qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records, uint32_t flags,
                            const void* out, const std::string& fn, const char* text_maker);
static int records_on_device(qcat_ctx* c, const qcat_result* records, uint32_t n, const qcat_result** recs);

static int part_check(const qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records, uint32_t flags, qcat_batch** out) {
    if (int rc = batch_call_check(c, ckit, b, records, flags, out, "qcat_batch_partition", nullptr)) return rc;
    if (b->true_len || !b->owned())
        return set_err(QCAT_ERR_ARG, "qcat_batch_partition: the batch holds read windows or borrowed buffers, not whole reads of its own");
    if (records && !part_records_fit(ckit->hk.dk, records, b->n_reads))
        return set_err(QCAT_ERR_ARG, "qcat_batch_partition: a record indexes outside the kit's templates / barcode sets or has a negative trim");
    if ((size_t)b->n_reads + 1 >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_partition: batch too large (>= 2^31 reads)");
    return 0;
}

// the scratch of this partition, and the caller's records on their way to the device
static int part_size_buffers(qcat_ctx* c, PartJob& j, const qcat_result* records) {
    PartScratch& P = c->batch.part;
    const uint32_t n = j.n;
    int rc;
    for (int i = 0; i < 2; ++i) { if ((rc = grow(P.key[i], n))) return rc; if ((rc = grow(P.idx[i], n))) return rc; }
    if ((rc = grow(P.hist, (size_t)256 * j.n_wg))) return rc;
    if ((rc = grow(P.sums32, part_scan_sums((uint64_t)256 * j.n_wg)))) return rc;
    if ((rc = grow(P.sums64, part_scan_sums((uint64_t)n + 1)))) return rc;
    if ((rc = grow(P.start, n))) return rc;
    if ((rc = grow(P.keep, n))) return rc;
    if ((rc = grow(P.src_pos, n))) return rc;
    if ((rc = grow(P.bins, (size_t)j.n_bins + 1))) return rc;
    if ((rc = grow(P.chunk_first, (size_t)j.max_chunks + 1))) return rc;
    return records_on_device(c, records, n, &j.recs);
}

// a. keys
static void part_keys(qcat_ctx* c, PartJob& j) {
    PartScratch& P = c->batch.part;
    const uint32_t blocks_n = (j.n + 255) / 256;
    if (j.n) hipLaunchKernelGGL(k_part_keys, dim3(std::min<uint32_t>(blocks_n, 8192)), dim3(256), 0, c->stream, j.kp, j.recs, j.in->offsets, j.n,
                                P.key[0].get(), P.start.get(), P.keep.get());
    mark(c, "part_keys");
}

// b. stable order: one to three passes over 8 bits of the bin
static void part_order(qcat_ctx* c, PartJob& j) {
    PartScratch& P = c->batch.part;
    const uint32_t n = j.n, n_wg = j.n_wg;
    for (uint32_t p = 0; n && p < j.passes; ++p) {
        const uint32_t* kin = P.key[p & 1]; const uint32_t* iin = p ? P.idx[p & 1].get() : nullptr;
        hipLaunchKernelGGL(k_part_hist, dim3(n_wg), dim3(256), 0, c->stream, kin, n, 8 * p, P.hist.get(), n_wg);
        part_scan_launch<uint32_t>(P.hist, (uint64_t)256 * n_wg, P.sums32, c->stream);
        hipLaunchKernelGGL(k_part_scatter, dim3(n_wg), dim3(256), 0, c->stream, kin, iin, n, 8 * p, (const uint32_t*)P.hist.get(), n_wg,
                           P.key[(p + 1) & 1].get(), P.idx[(p + 1) & 1].get());
    }
    j.key_sorted = P.key[j.passes & 1];
    j.source = P.idx[j.passes & 1];
    mark(c, "part_order");
}

// c. output offsets (they are the output batch's offsets), first read of every bin, first segment of every chunk
static void part_offsets(qcat_ctx* c, PartJob& j) {
    PartScratch& P = c->batch.part;
    const uint32_t n = j.n;
    hipLaunchKernelGGL(k_part_gather, dim3(n / 256 + 1), dim3(256), 0, c->stream, (const uint32_t*)j.source, (const uint64_t*)P.start.get(),
                       (const uint64_t*)P.keep.get(), n, j.out->offsets, P.src_pos.get());
    part_scan_launch<uint64_t>(j.out->offsets, (uint64_t)n + 1, P.sums64, c->stream);
    hipLaunchKernelGGL(k_part_bins, dim3(j.n_bins / 256 + 1), dim3(256), 0, c->stream, j.key_sorted, n, j.n_bins, P.bins.get());
    if (j.max_chunks) hipLaunchKernelGGL(k_part_chunks, dim3((uint32_t)((j.max_chunks + 255) / 256)), dim3(256), 0, c->stream,
                                         (const uint64_t*)j.out->offsets, n, P.chunk_first.get(), j.max_chunks);
    mark(c, "part_offsets");
}

// d. the copy: the bases, and a quality plane with them through the same slices in the same launch
template <int PLANES>
static void part_copy_launch(qcat_ctx* c, const PartJob& j, const uint8_t* quals_in, uint8_t* quals_out) {
    PartScratch& P = c->batch.part;
    hipLaunchKernelGGL(k_part_copy<PLANES>, dim3((uint32_t)j.max_chunks), dim3(256), 0, c->stream, (const uint64_t*)j.out->offsets,
                       (const uint64_t*)P.src_pos.get(), j.n, (const uint32_t*)P.chunk_first.get(), (const uint8_t*)j.in->bases, j.out->bases,
                       quals_in, quals_out);
}
static void part_copy(qcat_ctx* c, PartJob& j) {
    if (j.max_chunks && !j.in->quals) part_copy_launch<1>(c, j, nullptr, nullptr);
    else if (j.max_chunks) part_copy_launch<2>(c, j, j.in->quals, j.out->quals);
    mark(c, "part_copy");
}

// the output's real size, and the device's verdict on everything queued above
static int part_read_back(qcat_ctx* c, PartJob& j) {
    uint64_t total = 0;
    HIPCHK_DRAIN(c->stream, hipMemcpyAsync(&total, j.out->offsets + j.n, 8, hipMemcpyDeviceToHost, c->stream));
    if (int rc = stream_done(c, "qcat_batch_partition")) return rc;
    if (total > j.in->n_bases) return set_err(QCAT_ERR_DEVICE, "qcat_batch_partition: the slices are longer than the reads");
    j.out->n_bases = total;
    return 0;
}

extern "C" int qcat_batch_partition(qcat_ctx* c, const qcat_kit* ckit, const qcat_batch* b, const qcat_result* records,
                                    uint32_t flags, qcat_batch** out) {
    int rc = part_check(c, ckit, b, records, flags, out);
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
    j.max_chunks = qpart::chunks_of(b->n_bases);
    if (j.max_chunks >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_batch_partition: batch too large (>= 2^46 bases)");
    // the output: the input's bases are an upper bound, so nothing waits for the device before the copy
    BatchPtr ob;
    if ((rc = batch_make(c->device, j.n, b->n_bases, b->quals != nullptr, "hipMalloc failed for the partitioned batch", &ob))) return rc;
    j.out = ob.get();
    PartScratch& P = c->batch.part;
    P.n_bins = 0; P.source = nullptr;                        // (a failure below leaves no partition behind)
    if ((rc = part_size_buffers(c, j, records))) return rc;
    timing_slot(c);
    if (c->timing) HIPCHK_DRAIN(c->stream, hipEventRecord(c->ev[0], c->stream));     // (the caller's records may be on their way)
    part_keys(c, j);
    part_order(c, j);
    part_offsets(c, j);
    part_copy(c, j);
    if ((rc = part_read_back(c, j))) return rc;
    P.source = j.source; P.n_reads = j.n; P.n_bins = (int32_t)j.n_bins;
    *out = ob.release();
    return 0;
}

extern "C" int qcat_ctx_fetch_partition(qcat_ctx* c, uint64_t* bin_first, int32_t n_bins, uint32_t* source) {
    if (!c || !bin_first) return set_err(QCAT_ERR_ARG, "null argument");
    if (!c->batch.part.n_bins) return set_err(QCAT_ERR_ARG, "qcat_ctx_fetch_partition: no partition on this context");
    if (n_bins != c->batch.part.n_bins) return set_err(QCAT_ERR_ARG, "bin count does not match the latest partition");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(bin_first, c->batch.part.bins, ((size_t)n_bins + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (source && c->batch.part.n_reads)
        HIPCHK_DRAIN(c->stream, hipMemcpyAsync(source, c->batch.part.source, (size_t)c->batch.part.n_reads * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" void* qcat_ctx_partition_bins_devptr(qcat_ctx* c) { return c && c->batch.part.n_bins ? (void*)c->batch.part.bins.get() : nullptr; }
extern "C" void* qcat_ctx_partition_source_devptr(qcat_ctx* c) { return c && c->batch.part.n_bins ? (void*)c->batch.part.source : nullptr; }

// --- synthetic reads ------------------------------------------------------------------------
struct SynthSetup {
    qsynth::Params p;
    qsynth::Tpl t5, t3;
    bool has5 = false, has3 = false;
};

static int synth_setup(const HostKit& hk, const qcat_synth_params* sp, const char* ascii_base, SynthSetup* s, std::string* err) {
    if (!sp) { *err = "null synth params"; return QCAT_ERR_ARG; }
    if (sp->lead_max < sp->lead_min) { *err = "lead_max < lead_min"; return QCAT_ERR_ARG; }
    if (sp->error_rate < 0.f || sp->error_rate > 1.f || sp->no_adapter_fraction < 0.f || sp->no_adapter_fraction > 1.f) {
        *err = "rates must be in [0,1]"; return QCAT_ERR_ARG;
    }
    s->p.seed = sp->seed; s->p.insert_len = sp->insert_len; s->p.lead_min = sp->lead_min; s->p.lead_max = sp->lead_max;
    s->p.thr_err = (uint32_t)(sp->error_rate * 16777216.0f);
    s->p.thr_none = (uint32_t)(sp->no_adapter_fraction * 16777216.0f);
    auto fill = [&](int t, qsynth::Tpl* o) -> bool {
        if (t < 0) return false;
        const DevTpl& p = hk.dk.tpl[t];
        o->seq = ascii_base + hk.ascii_tpl_off[t]; o->len = p.len;
        for (int i = 0; i < 2; ++i) {
            o->bc_start[i] = hk.bc_start[t][i]; o->bc_len[i] = p.sets[i].n > 0 ? p.bc_len[i] : 0;
            o->n[i] = p.sets[i].n;
            o->sets[i] = p.sets[i].n > 0 ? ascii_base + hk.ascii_set_off[t][i] : nullptr;
        }
        return true;
    };
    if (sp->tpl_5p >= hk.dk.nt || sp->tpl_3p >= hk.dk.nt) { *err = "synth template index out of range"; return QCAT_ERR_ARG; }
    s->has5 = fill(sp->tpl_5p, &s->t5);
    s->has3 = fill(sp->tpl_3p, &s->t3);
    return 0;
}

extern "C" int64_t qcat_synth_read(const qcat_kit* kit, const qcat_synth_params* sp, uint64_t index,
                                   uint8_t* buf, uint64_t cap) {
    if (!kit) return set_err(QCAT_ERR_ARG, "null kit");
    SynthSetup s; std::string err;
    int rc = synth_setup(kit->hk, sp, kit->hk.ascii.data(), &s, &err);
    if (rc) return set_err(rc, err);
    qsynth::StoreSink sink(buf, buf ? cap : 0);
    qsynth::generate(s.p, index, s.has5 ? &s.t5 : nullptr, s.has3 ? &s.t3 : nullptr, sink);
    return (int64_t)sink.n;
}

__global__ void k_synth_lengths(qsynth::Params p, qsynth::Tpl t5, qsynth::Tpl t3, int has5, int has3,
                                uint64_t first, uint32_t n, uint64_t* lens) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    qsynth::CountSink sink;
    qsynth::generate(p, first + i, has5 ? &t5 : nullptr, has3 ? &t3 : nullptr, sink);
    lens[i] = sink.n;
}

__global__ void k_synth_write(qsynth::Params p, qsynth::Tpl t5, qsynth::Tpl t3, int has5, int has3,
                              uint64_t first, uint32_t n, const uint64_t* offsets, uint8_t* bases) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    qsynth::StoreSink sink(bases + offsets[i], offsets[i + 1] - offsets[i]);
    qsynth::generate(p, first + i, has5 ? &t5 : nullptr, has3 ? &t3 : nullptr, sink);
}

extern "C" int qcat_batch_synthesize(qcat_ctx* c, const qcat_kit* ckit, const qcat_synth_params* sp, qcat_batch** out) {
    if (!c || !ckit || !sp || !out) return set_err(QCAT_ERR_ARG, "null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    int rc = kit_on_device(kit, c->device, &kd);
    if (rc) return rc;
    SynthSetup s; std::string err;
    if ((rc = synth_setup(kit->hk, sp, kd->ascii, &s, &err))) return set_err(rc, err);
    const uint32_t n = sp->n_reads;
    FixedBuf<uint64_t> lens_buf;
    HIPCHK(lens_buf.ensure((size_t)n + 1));
    uint64_t* d_lens = lens_buf;
    uint32_t blocks = (n + 255) / 256;
    // the read index space is global: `seed` identifies the data set, reads [first, first+n) are
    // produced here (first = 0; shards pass distinct seeds or use qcat_synth_read for offsets)
    if (n) hipLaunchKernelGGL(k_synth_lengths, dim3(blocks), dim3(256), 0, c->stream, s.p, s.t5, s.t3,
                              (int)s.has5, (int)s.has3, (uint64_t)0, n, d_lens);
    std::vector<uint64_t> lens((size_t)n + 1, 0), offs((size_t)n + 1, 0);
    if (n) HIPCHK(hipMemcpyAsync(lens.data(), d_lens, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + lens[i];
    BatchPtr b;
    if ((rc = batch_make(c->device, n, offs[n], false, "hipMalloc failed for synthetic batch", &b))) return rc;
    HIPCHK(hipMemcpyAsync(b->offsets, offs.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n) hipLaunchKernelGGL(k_synth_write, dim3(blocks), dim3(256), 0, c->stream, s.p, s.t5, s.t3,
                              (int)s.has5, (int)s.has3, (uint64_t)0, n, b->offsets, b->bases);
    if ((rc = stream_done(c, "qcat_batch_synthesize"))) return rc;
    *out = b.release();
    return 0;
}

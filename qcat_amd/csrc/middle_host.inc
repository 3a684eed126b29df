// middle_host.inc -- host-side launch sequence of the interior scan of --detect-middle: its scratch buffers, the side stream
// of the packed batch, and the three calls a scan makes (scan_finalize, qcat_hip.hip)
//     absmid_codes_early     (A/B builds: the packed batch beside the read ends' kernels, at the start of the scan)
//     middle_packed          (kernels_middle.inc, kernels_abs_mid.inc: sort of the M-ends -> adapter phase, bit-sliced and
//                             binary16 -> barcode phase of packed_host.inc -> k_mid_finalize)
//     middle_wave_leftovers  (kernels_tiny.inc, k_midw_*: the interiors the packed scan leaves, one wave per alignment)
// and the two diagnostics that read the scratch.  The shared scan buffers (records, byte windows, PackedScratch) stay on the
// context and are passed in.
// Included by qcat_hip.hip after packed_host.inc, kernels_middle.inc and batch.h (qcat_batch), where the error helpers of that
// file (set_err, grow, HIPCHK) are visible: grow sites report QCAT_ERR_NOMEM, HIPCHK sites QCAT_ERR_DEVICE, the packed_* phases
// packed_last_error().

// the bit-sliced interior adapter scan (kernels_abs_mid.inc, abs_mid_kernels.hip)
extern "C" void qcat_absmid_prepare(void* stream, const void* args, uint32_t* win2, uint8_t* wspec, int what);
extern "C" int qcat_absmid_launch(int id, int waves, unsigned grid, void* stream, const void* args);

// the one-wave kernels take up to this many reads of a batch (middle_wave_leftovers)
constexpr uint32_t MIDW_CAP = 2048;

struct MiddleScratch {
    // packed --detect-middle (kernels_middle.inc): M-end sort tables and per-slot arrays
    DevBuf<MidTables> mid_tables;                                 // (allocated once)
    DevBuf<uint8_t> mid_generic;
    DevBuf<uint32_t> mid_slot;
    DevBuf<uint32_t> mid_sorted; DevBuf<int32_t> mid_len, mid_fallback;
    DevBuf<uint32_t> mid_win2; DevBuf<uint8_t> mid_wspec;         // the M-ends' first window at two bits per code + flags (k_mid_windows)
    DevBuf<EndRec> mid_recs; DevBuf<AdapterBest> mid_bests;
    // ... its bit-sliced adapter scan (kernels_abs_mid.inc): the words per big tile of 2048 slots (AbsmTileWords), the per-128
    // flags, letter planes and not-started masks
    DevBuf<uint32_t> absm_tiles;
    DevBuf<uint8_t> absm_need;
    DevBuf<uint2> absm_planes;
    DevBuf<uint32_t> absm_ns;
    DevBuf<uint32_t> absm_c2;                                     // the batch at two bits per base (with ABSM_C2_SLACK dwords on either side)
    DevBuf<uint8_t> absm_rspec;
    DevBuf<uint4> absm_sinfo;                                     // per slot: position / strand, length, special flag
    hipStream_t absm_stream = nullptr; hipEvent_t absm_go = nullptr, absm_done = nullptr;      // the packed batch beside the read ends' kernels
    bool absm_codes_early = false;                                // this scan's k_absmid_codes is in flight on absm_stream
    uint32_t absm_last_big = 0, absm_last_128 = 0;                // big tiles / tiles of 128 slots of the latest scan on that path (0: not taken)
    // the reads the packed interior scan leaves (long interiors) on the one-wave kernels (k_midw_*)
    DevBuf<uint32_t> midw_list; DevBuf<int32_t> midw_tpl; DevBuf<EndRec> midw_recs; DevBuf<int16_t> midw_sc;    // (the first three: allocated once)
    bool midw_ran = false;
};

// (the buffers free themselves with the scratch; the stream and its events go here, on the context's device)
static inline void middle_scratch_free(MiddleScratch* m) {
    if (m->absm_stream) (void)hipStreamDestroy(m->absm_stream);
    if (m->absm_go) (void)hipEventDestroy(m->absm_go);
    if (m->absm_done) (void)hipEventDestroy(m->absm_done);
    m->absm_stream = nullptr; m->absm_go = nullptr; m->absm_done = nullptr;
}

// the words of `absm_tiles` for `big` big tiles: [rows, padding zone, kit, first row: 4 x big] [nonempty, invalid: 2 x 64 x big]
// [cursors: MAX_T]
struct AbsmTileWords {
    int32_t *rows, *pz, *kit;
    uint32_t *first_row, *nonempty, *invalid, *cursor;
    static size_t words(uint32_t big) { return (size_t)big * (4 + 128) + MAX_T; }
    AbsmTileWords(uint32_t* w, uint32_t big)
        : rows((int32_t*)w), pz((int32_t*)(w + big)), kit((int32_t*)(w + 2 * (size_t)big)), first_row(w + 3 * (size_t)big),
          nonempty(w + 4 * (size_t)big), invalid(w + 4 * (size_t)big + 64 * (size_t)big), cursor(w + (size_t)big * (4 + 128)) {}
};

// packed --detect-middle is possible when every template has a generated static-letter adapter
// kernel (all built-in kits) and the kit's slots fit the sort tables
static bool middle_packed_ok(const DevKit& hk) {
    if (!hk.adapter_f16 || hk.n_kit_slots > MID_MAX_KITS || opt_on(QO_MIDDLE_GENERIC)) return false;
    // the interior kernel carries up to PK_ROWS + 63 rows of bias inside a block plus the offset of its
    // last-row keys (kernels_middle.inc): g * ((152 + 63 + 128 + 64) - (160 + 128)) + 1 more than a window
    if (hk.adapter_f16_headroom < hk.gap_open * 119 + 1) return false;
    for (int t = 0; t < hk.nt; ++t) if (hk.tpl[t].static_kernel < 0) return false;
    return true;
}

// kit slots whose templates all have a two-stage bit-sliced plan (the built-in kits' single-template plans)
static uint32_t absmid_kit_mask(const DevKit& hk) {
    if (!hk.abs_ok) return 0u;
    uint32_t mask = 0u, bad = 0u;
    for (int t = 0; t < hk.nt; ++t) {
        const int ks = hk.tpl[t].kit_slot, sk = hk.tpl[t].static_kernel;
        if (ks < 0 || ks >= 32) continue;
        if (sk >= 0 && sk < QCAT_JIT_BASE && qcat_absmid_launch(sk, 2, 0, nullptr, nullptr)) mask |= 1u << ks; else bad |= 1u << ks;
    }
    return mask & ~bad;
}

// slots of the packed interior scan of n reads, and will its adapter scan run bit-sliced (kit mask != 0)?
static size_t middle_slots(const DevKit& hk, uint32_t n) {
    return ((size_t)2 * n + (size_t)hk.n_kit_slots * MID_CLASSES * PK_TILE + PK_TILE - 1) / PK_TILE * PK_TILE;
}
static uint32_t absmid_wanted(const DevKit& hk, uint32_t n) {
    // from 1.25 big tiles of 2048 slots per CU (330 k reads on 256 CUs): below that the binary16 kernel's 3 us per thousand interiors
    // beat a tile's sequential walk (tools/r04_absmid_sizes.sh, profiles/r04_ab_absmid_sizes.txt)
    const size_t min_slots = opt_is_set(QO_MIDDLE_ABS_MIN) ? (size_t)opt_val(QO_MIDDLE_ABS_MIN, 0) : (size_t)abs_cu_count() * 2048 * 5 / 4;
    if (opt_on(QO_MIDDLE_NO_ABS) || middle_slots(hk, n) < min_slots) return 0u;
    return absmid_kit_mask(hk);
}

// QCAT_HIP_MIDDLE_ABS_EARLY=1 (A/B switch, off by default): the batch at two bits per base (k_absmid_codes) at the start of a
// --detect-middle scan on a stream of its own, beside the read ends' kernels -- it needs the reads only; middle_packed waits
// for absm_done.  Measured at 1 M reads: the interior phase loses the kernel's 0.12 ms, k_pack_windows and the plane kernel of
// the read ends -- bound by memory themselves -- gain 0.08 + 0.06 ms: 5.14 ms per step either way.
static int absmid_codes_early(hipStream_t st, MiddleScratch* m, const DevKit& hk, const qcat_batch* b, uint32_t n) {
    m->absm_codes_early = false;
    if (opt_val(QO_MIDDLE_ABS_EARLY, 0) != 1) return 0;
    if (!absmid_wanted(hk, n)) return 0;
    int rc;
    if (!m->absm_stream) {
        HIPCHK(hipStreamCreateWithFlags(&m->absm_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&m->absm_go, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&m->absm_done, hipEventDisableTiming));
    }
    if ((rc = grow(m->absm_c2, (size_t)(b->n_bases / 16) + 4 + 2 * (size_t)ABSM_C2_SLACK))) return rc;
    if ((rc = grow(m->absm_rspec, (size_t)n + 1))) return rc;
    AbsMidArgs am{};
    am.bases = b->bases; am.offsets = b->offsets; am.max_align = hk.max_align; am.n_bases = b->n_bases; am.n_reads = n;
    am.c2 = m->absm_c2 + ABSM_C2_SLACK; am.rspec = m->absm_rspec;
    HIPCHK(hipEventRecord(m->absm_go, st));                        // (after whatever the stream holds: the previous scan's readers of c2)
    HIPCHK(hipStreamWaitEvent(m->absm_stream, m->absm_go, 0));
    HIPCHK(hipMemsetAsync(m->absm_rspec, 0, (size_t)n + 1, m->absm_stream));
    qcat_absmid_prepare(m->absm_stream, &am, nullptr, nullptr, 1);
    HIPCHK(hipEventRecord(m->absm_done, m->absm_stream));
    m->absm_codes_early = true;
    return 0;
}

// the interior scan of every called read on the packed kernels (kernels_middle.inc), on the scan's job tables `sc` and into its
// records `results`; leaves m->mid_generic[r] = 1 for reads it could not take (interior longer than the length classes).
// `win`: the scan's byte windows.
static int middle_packed(hipStream_t st, MiddleScratch* m, PackedScratch* sc, KitPtrs kp, const DevKit& hk, const qcat_batch* b, uint32_t n,
                         qcat_result* results, const uint8_t* win) {
    int rc;
    const size_t slots = middle_slots(hk, n);
    if (slots >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "batch too large for the packed interior scan");
    HIPCHK(m->mid_tables.ensure(1));
    if ((rc = grow(m->mid_generic, (size_t)n))) return rc;
    if ((rc = grow(m->mid_slot, (size_t)n))) return rc;
    HIPCHK(m->mid_win2.ensure(slots * WIN2_WORDS + 64));
    HIPCHK(m->mid_wspec.ensure(slots + 4));
    HIPCHK(m->mid_sorted.ensure(slots));
    HIPCHK(m->mid_len.ensure(slots));
    HIPCHK(m->mid_fallback.ensure(slots));
    HIPCHK(m->mid_recs.ensure(slots));
    if ((rc = grow(m->mid_bests, slots * (size_t)hk.nt))) return rc;
    // the fills of the interior scan leave as two k_fill_multi launches (round 5; thirteen memsets of 5-7 us each before):
    // the slot tables here, the job tables / sorted list / redo count / letter flags / tile cursors before the adapter phase
    const bool merge_fills = !opt_on(QO_NO_FILL_MERGE);
    {
        FillScope fills(merge_fills);
        HIPCHK(packed_fill(m->mid_tables, 0, sizeof(MidTables), st));
        HIPCHK(packed_fill(m->mid_slot, 0xFF, (size_t)n * 4, st));
        HIPCHK(packed_fill(m->mid_sorted, 0xFF, slots * 4, st));
        HIPCHK(packed_fill(m->mid_len, 0, slots * 4, st));
        HIPCHK(packed_fill(m->mid_fallback, 0, slots * 4, st));
        HIPCHK(packed_fill_flush(st));
    }
    const uint32_t rblocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_mid_count, dim3(rblocks), dim3(256), 0, st, kp.kit, b->offsets, n, results, m->mid_tables, m->mid_generic);
    hipLaunchKernelGGL(k_mid_offsets, dim3(1), dim3(1024), 0, st, m->mid_tables);
    hipLaunchKernelGGL(k_mid_scatter, dim3((n + 256 * MID_SCAT - 1) / (256 * MID_SCAT)), dim3(256), 0, st,
                       kp.kit, b->offsets, n, results, m->mid_tables, m->mid_sorted, m->mid_len, m->mid_fallback, m->mid_slot);
    // adapter phase: one launch per template (tiles of other kits record "did not compete"), the
    // launches of a scan run concurrently
    // round 4: the interiors' first window at two bits per code, so that their whole-window barcode jobs -- nearly all of
    // them -- run on the bit-sliced barcode kernels (QCAT_HIP_MIDDLE_NO_BITSLICE=1: binary16 kernels as before)
    const bool mid_bs = !opt_on(QO_MIDDLE_NO_BITSLICE);
    // (with the bit-sliced adapter scan below the windows come from its packed batch instead: k_absmid_windows.  k_mid_windows beside
    //  the adapter kernels was measured and lost: those fill the register files, each of their waves walks ONE tile, and a wave that
    //  starts late is the kernel's tail; beside the preparation chain -- kernels that wait for memory like itself -- it gained 0.02 ms)
    auto launch_mid_windows = [&](hipStream_t q) {
        const uint64_t wthreads = (uint64_t)slots * 16;           // (sixteen lanes per slot; every slot's flag byte is stored, no fill)
        hipLaunchKernelGGL(k_mid_windows, dim3((uint32_t)((wthreads + 255) / 256)), dim3(256), 0, q, b->bases, b->offsets, hk.max_align,
                           m->mid_sorted, (uint32_t)slots, m->mid_win2, m->mid_wspec);
    };
    sc->wspec = mid_bs ? m->mid_wspec : nullptr;          // (null: no letter flags, no bit-sliced classes)
    sc->win2 = mid_bs ? m->mid_win2 : nullptr;
    sc->win = win;                                        // (never read: the job regions come from win2, `lazy`)
    sc->lazy = mid_bs;
    sc->slim = false;                                     // ... and the barcode results stay in the interior's own records
    FillScope fills(merge_fills);                          // (flushed in front of the adapter phase below; every return before drops the list)
    if ((rc = packed_prepare(st, hk, (uint32_t)slots, sc))) return set_err(rc, packed_last_error());
    const uint32_t tiles = (uint32_t)(slots / PK_TILE);
    // round 4: the adapter scan of the interiors in bit-sliced form (kernels_abs_mid.inc) from QCAT_HIP_MIDDLE_ABS_MIN slots
    // (default: one big tile of 2048 slots per CU); QCAT_HIP_MIDDLE_NO_ABS=1: the binary16 kernel for every tile as before.
    // The binary16 kernel then only takes the tiles of 128 slots flagged in absm_need.
    AbsMidArgs am{};
    bool use_absm = false;
    m->absm_last_big = 0; m->absm_last_128 = 0;
    {
        const uint32_t kmask = absmid_wanted(hk, n);
        if (kmask) {
            const uint32_t big = (uint32_t)((slots + 2047) / 2048);
            // rows of all big tiles together: every tile as long as its longest interior -- the mean of the interiors plus
            // the width of the length classes a tile spans; a tile beyond the room falls back to the binary16 kernel
            const bool rcap = opt_is_set(QO_MIDDLE_ABS_ROWS);          // (tests: a plane buffer that is too small)
            size_t rows = rcap ? (size_t)opt_val(QO_MIDDLE_ABS_ROWS, 0)
                               : std::min<size_t>((size_t)1 << 30, (size_t)(2 * b->n_bases / 2048) * 5 / 4 + (size_t)big * 128 + 16384 + 64);
            if (!rcap && rows * 64 > m->absm_planes.cap()) {
                // planes + not-started masks are 768 bytes per row (~0.9 bytes per base of the batch): never more than a quarter
                // of the device memory that is free right now -- the big tiles beyond the room fall back to the binary16 kernel
                // per tile (k_absmid_scan: row_cap), which needs none of it (ADVICE round 4)
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) rows = std::min(rows, std::max<size_t>(16384, free_b / 4 / 768));
            }
            if ((rc = grow(m->absm_tiles, AbsmTileWords::words(big)))) return rc;
            if ((rc = grow(m->absm_need, (size_t)tiles + 16))) return rc;
            if ((rc = grow(m->absm_planes, rows * 64))) return rc;
            if ((rc = grow(m->absm_ns, rows * 64))) return rc;
            const bool early = m->absm_codes_early;                             // (absmid_codes_early: the packed batch is on its way)
            m->absm_codes_early = false;
            if (!early) {
                if ((rc = grow(m->absm_c2, (size_t)(b->n_bases / 16) + 4 + 2 * (size_t)ABSM_C2_SLACK))) return rc;
                if ((rc = grow(m->absm_rspec, (size_t)n + 1))) return rc;
            }
            if ((rc = grow(m->absm_sinfo, slots))) return rc;
            const AbsmTileWords tw(m->absm_tiles, big);
            am.bases = b->bases; am.offsets = b->offsets; am.msorted = m->mid_sorted; am.mlen = m->mid_len; am.mt = m->mid_tables;
            am.max_align = hk.max_align; am.n_tiles = big; am.slot_cap = (uint32_t)slots; am.nt = hk.nt; am.kit_mask = kmask;
            am.t_rows = tw.rows; am.t_pz = tw.pz; am.t_kit = tw.kit; am.t_off = tw.first_row;
            am.nonempty = tw.nonempty; am.invalid = tw.invalid;
            am.cursor = tw.cursor;
            am.c2 = m->absm_c2 + ABSM_C2_SLACK; am.rspec = m->absm_rspec; am.sinfo = m->absm_sinfo; am.n_bases = b->n_bases; am.n_reads = n;
            if (early) HIPCHK(hipStreamWaitEvent(st, m->absm_done, 0));
            else HIPCHK(packed_fill(m->absm_rspec, 0, (size_t)n + 1, st));
            am.need128 = m->absm_need; am.planes = m->absm_planes; am.ns = m->absm_ns; am.row_cap = (uint32_t)rows;
            am.bests = m->mid_bests; am.tpl = -1; am.den = 0; am.kit_slot = -1;
            // issue priority of the row loops rotated every two rows by workgroup parity (abs_setprio; two waves of different
            // launches share a SIMD): 4.79 against 4.91 ms per step at 1 M reads (tools/r04_absmid_prio.sh); QCAT_HIP_MIDDLE_ABS_PRIO
            am.prio = (int32_t)opt_val(QO_MIDDLE_ABS_PRIO, opt_val(QO_ABS_PRIO, 2));
            am.r1_scalar = hk.r1_scalar;
            HIPCHK(packed_fill(am.cursor, 0, MAX_T * 4, st));
            HIPCHK(packed_fill_flush(st));
            // the M-ends' first windows (k_mid_windows) come from the packed batch too: QCAT_HIP_MIDDLE_ABS_WINDOWS=0: from the reads, beside
            const bool c2win = mid_bs && opt_val(QO_MIDDLE_ABS_WINDOWS, 1) != 0;
            fork_join(sc, st, (mid_bs && !c2win) ? 2 : 1, [&](int i, hipStream_t q) {
                if (i == 0) qcat_absmid_prepare(q, &am, c2win ? m->mid_win2.get() : nullptr, c2win ? m->mid_wspec.get() : nullptr, early ? 2 : 3); else launch_mid_windows(q);
            });
            use_absm = true;
            m->absm_last_big = big; m->absm_last_128 = tiles;
        }
    }
    HIPCHK(packed_fill_flush(st));                                 // (no bit-sliced interior scan: the job tables' fills leave here)
    int absm_side = 0;                                             // templates on the bit-sliced path: launches side by side
    if (use_absm) for (int t = 0; t < hk.nt; ++t) if ((am.kit_mask >> hk.tpl[t].kit_slot) & 1u) ++absm_side;
    if (mid_bs && !use_absm) launch_mid_windows(st);
    fork_join(sc, st, hk.nt, [&](int t, hipStream_t q) {
        if (use_absm && ((am.kit_mask >> hk.tpl[t].kit_slot) & 1u)) {
            AbsMidArgs at = am;
            at.bests = m->mid_bests + (size_t)t * slots; at.tpl = t; at.den = hk.tpl[t].den; at.kit_slot = hk.tpl[t].kit_slot;
            at.cursor = am.cursor + t;
            // persistent two-wave workgroups: four per CU (two waves per SIMD) shared by the templates that run side by side --
            // two launches of four per CU each do not fit the register file together, and the second one then runs after
            // the first (1.2 + 0.6 ms at 1 M reads against ~1.0 ms side by side).  QCAT_HIP_MIDDLE_ABS_WGS=<per CU and launch>
            // A template of up to 46 columns walks a tile on ONE wave (k_adapter_mid1: eight per CU); QCAT_HIP_MIDDLE_ABS_ONE_WAVE=0 / 1: pipeline / one wave whatever the size.
            const int sk = hk.tpl[t].static_kernel;
            // one wave per tile from 2.75 big tiles per CU (720 k reads): with fewer tiles than wave slots a tile's walk is the kernel,
            // and the pipeline's two waves halve it (400 k reads: interior phase 1.95 against 2.29 ms; 800 k: 2.96 against 2.87)
            const bool big_enough = slots >= (size_t)abs_cu_count() * 2048 * 11 / 4;
            const bool one = (int)opt_val(QO_MIDDLE_ABS_ONE_WAVE, big_enough ? 1 : 0) != 0 && qcat_absmid_launch(sk, 1, 0, nullptr, nullptr) != 0;
            const int per_cu = (int)opt_val(QO_MIDDLE_ABS_WGS, std::max(1, (one ? 8 : 4) / std::max(1, absm_side)));
            const unsigned grid = (unsigned)std::min<uint32_t>(am.n_tiles, (uint32_t)(abs_cu_count() * per_cu));
            (void)qcat_absmid_launch(sk, one ? 1 : 2, grid, q, &at);
        }
        MiddleAdapterArgs ma{kp, b->bases, b->offsets, m->mid_sorted, m->mid_len, m->mid_tables,
                             m->mid_bests + (size_t)t * slots, t, use_absm ? m->absm_need.get() : nullptr};
        launch_adapter_middle(hk.tpl[t].static_kernel, dim3(tiles), q, ma);
    });
    {
        const uint32_t fblocks = (uint32_t)std::min<uint64_t>((slots + 255) / 256, 2048);
        hipLaunchKernelGGL(k_adapter_finish, dim3(fblocks), dim3(256), 0, st, kp.kit, m->mid_len, (uint32_t)slots,
                           m->mid_bests, hk.nt, m->mid_recs, sc->jt, (const int32_t*)m->mid_fallback, -1, (const uint8_t*)sc->wspec, sc->jobinfo, (int2*)nullptr, (uint32_t*)nullptr);
    }
    const int nsets = hk.mode == QCAT_MODE_DUAL ? 2 : 1;
    rc = packed_barcode(st, kp, hk, (uint32_t)slots, m->mid_recs, sc, [&](uint32_t max_tiles, const BsPlan* taken, hipStream_t gq) {
        const uint64_t gthreads = (uint64_t)max_tiles * 64 * (WIN_STRIDE / 16);
        hipLaunchKernelGGL(k_mid_gather, dim3((uint32_t)((gthreads + 255) / 256)), dim3(256), 0, gq,
                           b->bases, b->offsets, hk.max_align, m->mid_sorted, m->mid_recs, sc->sorted, sc->jt, nsets,
                           sc->tilebuf, sc->tmeta, taken);
    }, (int16_t*)nullptr, 0u, [](const char*) {});
    if (!rc) rc = jit_take_error();
    if (rc) return set_err(rc, packed_last_error());
    hipLaunchKernelGGL(k_mid_finalize, dim3((n + 255) / 256), dim3(256), 0, st, kp.kit, m->mid_recs, m->mid_slot, n, results, m->mid_generic);
    HIPCHK(hipGetLastError());
    return 0;
}

// the reads the packed interior scan left (interiors of more than 16 384 letters ...): on one wave per alignment
// (kernels_tiny.inc: k_midw_*) up to MIDW_CAP of them per batch, the general kernel takes what is left after that.
// `take` false: the path is off for this scan (no packed interior scan in front of it, or a context on the general kernels);
// `maxb`: max_set_barcodes of the kit
static int middle_wave_leftovers(hipStream_t st, MiddleScratch* m, KitPtrs kp, const DevKit& hk, const qcat_batch* b, uint32_t n,
                                 qcat_result* results, int maxb, bool take) {
    m->midw_ran = false;
    if (!take || hk.gap_open != hk.gap_extend || opt_on(QO_NO_TINY)) return 0;
    HIPCHK(m->midw_list.ensure(MIDW_CAP + 1));
    HIPCHK(m->midw_tpl.ensure((size_t)MIDW_CAP * 2 * MAX_T * 2));
    HIPCHK(m->midw_recs.ensure((size_t)MIDW_CAP * 2));
    HIPCHK(m->midw_sc.ensure((size_t)MIDW_CAP * 2 * 2 * (size_t)maxb));
    uint32_t* count = m->midw_list + MIDW_CAP;
    HIPCHK(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
    MidWaveArgs ma{kp, b->bases, b->offsets, n, results, m->mid_generic, m->midw_list, count, MIDW_CAP,
                   m->midw_tpl, m->midw_recs, m->midw_sc, (uint32_t)maxb};
    hipLaunchKernelGGL(k_midw_list, dim3((n + 255) / 256), dim3(256), 0, st, ma);
    hipLaunchKernelGGL(k_midw_adapter, dim3(1024), dim3(64), 0, st, ma);
    hipLaunchKernelGGL(k_midw_decide, dim3(MIDW_CAP * 2 / 64), dim3(64), 0, st, ma);
    hipLaunchKernelGGL(k_midw_barcode, dim3(4096), dim3(64), 0, st, ma);
    hipLaunchKernelGGL(k_midw_finish, dim3(MIDW_CAP / 64), dim3(64), 0, st, ma);
    m->midw_ran = true;
    return 0;
}

// qcat_ctx_middle_wave_reads: reads of the latest scan on the one-wave kernels (the device's count, at most the cap); waits for `st`
static int64_t middle_wave_count(const MiddleScratch& m, int device, hipStream_t st) {
    if (!m.midw_ran || !m.midw_list) return 0;
    if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
    uint32_t cnt = 0;
    if (hipMemcpy(&cnt, m.midw_list + MIDW_CAP, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)std::min<uint32_t>(cnt, MIDW_CAP);
}

// qcat_ctx_middle_bitslice_tiles: the latest scan's big tiles with rows (walked bit-sliced) and its flagged tiles of 128; waits for `st`
static int middle_bitslice_tiles(const MiddleScratch& m, int device, hipStream_t st, uint32_t* out) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!m.absm_last_big) return 0;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int32_t> rows(m.absm_last_big);
    std::vector<uint8_t> need(m.absm_last_128);
    HIPCHK(hipMemcpy(rows.data(), AbsmTileWords(m.absm_tiles, m.absm_last_big).rows, rows.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(need.data(), m.absm_need, need.size(), hipMemcpyDeviceToHost));
    for (int32_t r : rows) if (r > 0) ++out[0];
    out[1] = m.absm_last_big;
    for (uint8_t f : need) if (f) ++out[2];
    out[3] = m.absm_last_128;
    return 0;
}

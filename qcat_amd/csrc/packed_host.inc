// packed_host.inc -- host-side launch sequence of the packed path: scratch buffers, the side
// streams that let independent launches overlap, and the three phases
//     packed_prepare  (job tables) -> packed_adapter (all templates, k_adapter_finish)
//                                  -> packed_barcode (job sort, tile images, barcode kernels, select)
// shared by the main scan (packed_scan) and the interior scan of --detect-middle (middle_host.inc).
// Included by qcat_hip.hip after kernels_packed.inc (and by jit_prelude.inc for the struct layouts).

#include "dev_buf.h"

// the bit-sliced adapter kernels live in a translation unit of their own (abs_kernels.hip, kernels_abs.inc)
extern "C" void qcat_abs_launch_planes(unsigned n_tiles, void* stream, const uint32_t* win2, const int32_t* wlen, const uint8_t* wspec,
                                       uint32_t n_ends, int rows, void* planes, uint32_t* valid, uint8_t* need128, uint32_t* tile_any);
extern "C" unsigned qcat_abs_launch_pack_planes(void* stream, const uint8_t* bases, const uint64_t* offsets, uint32_t n_reads, int ends, int rows,
                                                uint8_t* win, int32_t* wlen, uint8_t* wspec, uint32_t* win2, int lazy_bytes,
                                                void* planes, uint32_t* valid, uint8_t* need128, uint32_t* tile_any);
extern "C" int qcat_abs_launch(int kind, int id, unsigned grid, void* stream, const void* args);

namespace qk {

#ifndef QCAT_ABS_TILE_DEFINED
#define QCAT_ABS_TILE_DEFINED
constexpr int ABS_TILE = 2048;          // read ends per tile of the bit-sliced adapter kernels (kernels_abs.inc)
#endif
constexpr int RESUME_KIT_ON_DEVICE = 1 << 20;      // resume_kit_mask: the voted kit slot is on the device (PackedScratch::kit_slot_dev)

struct PackedScratch {
    DevBuf<JobTables> jt;              // (allocated once)
    DevBuf<int32_t> sorted;
    DevBuf<uint32_t> jobinfo;          // [read end][set] region length | sort bin << 8 | start << 16 (k_adapter_finish), 0: no job
    DevBuf<AdapterBest> bests;
    int n_slices = 0;                  // slices of `bests` the last adapter phase wrote
    bool slices_single = false;        // ... each of exactly one template (kit-mask merges are possible)
    DevBuf<uint8_t> tilebuf;           // [tiles][64 lanes][160 B] LDS images of the barcode tiles
    DevBuf<TileMeta> tmeta;            // [tiles][64]
    DevBuf<uint32_t> raws;             // [tiles][bstride][64] raw barcode scores, two int16 per dword
    DevBuf<uint32_t> part;             // summary mode: [tiles][part_stride][2][64] keys (kernels_packed.inc, barcode_key)
    DevBuf<uint32_t> redo;             // summary mode: [0] = count, [1..] = alignments whose arg-max needs the sequential rule
    // bit-sliced barcode kernels (kernels_bitslice.inc)
    const uint8_t* wspec = nullptr;    // per read end: letters outside A, C, G, T, N (null: no hot classes, e.g. read interiors)
    const uint8_t* win = nullptr;      // the packed windows the flags belong to
    const uint32_t* win2 = nullptr;    // ... at two bits per code (k_pack_windows)
    bool lazy = false;                 // the scan's byte windows exist for the flagged ends only (k_expand_special): readers go through dev_window16
    DevBuf<BsPlan> bsplan;                                 // (allocated once)
    DevBuf<uint32_t> bskeys;                               // [chunk][sorted position]
    bool bs_last = false;                                  // the latest scan planned super-tiles (qcat_ctx_barcode_bitslice_tiles)
    DevBuf<uint2> bsrp;                                    // [launch][workgroup][BS_MAX_ROWS][64]: plane pairs of the trailing columns (bs_trailing_columns)
    // bit-sliced adapter kernels (kernels_abs.inc): letter planes of the tiles, per-lane keep masks, and one zeroed block
    // of flags per scan: [tile cursors: MAX_T u32][tile_any: n_tiles u32][need128: n_tiles * 16 bytes]
    DevBuf<uint2> abs_planes;
    DevBuf<uint32_t> abs_valid;
    DevBuf<uint8_t> abs_flags;
    // round 3: sorted position of every job (k_job_scatter) and the packed barcode results (index, raw score) per job that
    // the select kernels write and k_finalize reads; `slim` = this scan uses them (the main scan outside debug mode)
    DevBuf<uint32_t> posof;
    DevBuf<int2> bcres;
    bool slim = false;
    // ... and one word per read end for k_finalize instead of the record (k_adapter_finish); fin_only = this pass writes it
    // (a slim scan that is not the adapter-only pass of kit auto, whose vote reads the records)
    DevBuf<uint32_t> fin;
    bool fin_only = false;
    uint32_t abs_ready = 0;            // read ends whose planes / flags the fused pack kernel of this scan has already made (0: none)
    uint32_t abs_zeroed = 0;           // read ends whose flag block this scan has sized and zeroed already (packed_abs_buffers ahead of the pack kernel)
    const int32_t* kit_slot_dev = nullptr;     // the voted kit slot of a kit-auto batch (k_pick_kit), read by k_adapter_finish
    uint32_t kit_slot_span = 0;                // > 0: kit_slot_dev holds one slot per this many read ends (several batches in one scan)
    bool prepared = false;             // packed_prepare has run for this scan (ahead of the pack kernel, its fills in the scan's one fill launch)
    bool redo_zeroed = false;          // ... and zeroed the redo count
    // side streams: independent launches (one static kernel per template / per barcode group) run
    // concurrently so that a small group does not cost a whole, mostly idle, launch of its own
    // (seven: the nine adapter launches of a kit-auto scan of a 4000-read batch -- 63 waves each, latency-bound -- run in
    //  two rounds instead of three; big batches queue behind each other whatever the stream count)
    static constexpr int NAUX = 11;    // (round 4: eleven -- the nine launches in ONE round; the adapter pass of such a batch was 270 us of a 730 us call)
    hipStream_t aux[NAUX] = {};
    hipEvent_t ev_fork = nullptr, ev_join[NAUX] = {};
};

static thread_local std::string g_packed_err;
// fills collected while g_fill_defer is set leave as one k_fill_multi launch (packed_fill_flush); otherwise a fill is a
// hipMemsetAsync at once
static thread_local FillList g_fill = {};
static thread_local bool g_fill_defer = false;
static inline hipError_t packed_fill(void* p, int byte, size_t bytes, hipStream_t stream) {
    if (g_fill_defer && g_fill.n < 8 && bytes > 0) {
        const uint32_t b = (uint32_t)(byte & 0xFF);
        g_fill.p[g_fill.n] = p; g_fill.bytes[g_fill.n] = bytes; g_fill.word[g_fill.n] = b * 0x01010101u; ++g_fill.n;
        return hipSuccess;
    }
    return bytes ? hipMemsetAsync(p, byte, bytes, stream) : hipSuccess;
}
static inline hipError_t packed_fill_flush(hipStream_t stream) {
    g_fill_defer = false;
    if (g_fill.n == 0) return hipSuccess;
    unsigned long long most = 0;
    for (int r = 0; r < g_fill.n; ++r) most = std::max(most, g_fill.bytes[r]);
    const unsigned blocks = (unsigned)std::min<unsigned long long>(1024, std::max<unsigned long long>(1, most / (16 * 256 * 4)));
    hipLaunchKernelGGL(k_fill_multi, dim3(blocks), dim3(256), 0, stream, g_fill);
    g_fill.n = 0;
    return hipGetLastError();
}
// the stretch of a function that collects fills (defer: as one launch; else each a memset at once): starts from an empty
// list and leaves an empty list and a cleared flag behind on every way out, so a return between a packed_fill and its
// packed_fill_flush drops the queued fills instead of handing them to the thread's next scan
struct FillScope {
    explicit FillScope(bool defer) { g_fill.n = 0; g_fill_defer = defer; }
    ~FillScope() { g_fill.n = 0; g_fill_defer = false; }
    FillScope(const FillScope&) = delete;
    FillScope& operator=(const FillScope&) = delete;
};
static inline const char* packed_last_error() { return g_packed_err.c_str(); }
// a failed launch of a run-time generated kernel (jit_launch, qcat_hip.hip) is recorded here and turned
// into the scan's status by the phase that issued it
static thread_local int g_jit_rc = 0;
static inline int jit_take_error() { const int rc = g_jit_rc; g_jit_rc = 0; return rc; }

static inline hipError_t packed_streams(PackedScratch* s) {
    if (s->ev_fork) return hipSuccess;
    hipError_t e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
    for (int i = 0; i < PackedScratch::NAUX && e == hipSuccess; ++i) {
        e = hipStreamCreateWithFlags(&s->aux[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join[i], hipEventDisableTiming);
    }
    return e;
}

// launch `n` independent kernels: the first on `stream`, the others round-robin on the side streams,
// all ordered after what `stream` holds now and joined back into `stream`
template <class Launch>
static inline void fork_join(PackedScratch* s, hipStream_t stream, int n, Launch launch) {
    if (n <= 0) return;
    const bool multi = n > 1 && s->ev_fork && !opt_on(QO_ONE_STREAM);
    if (multi) (void)hipEventRecord(s->ev_fork, stream);
    bool used[PackedScratch::NAUX] = {};
    for (int i = 0; i < n; ++i) {
        hipStream_t q = stream;
        if (multi && i > 0) {
            const int a = (i - 1) % PackedScratch::NAUX;
            q = s->aux[a];
            if (!used[a]) { (void)hipStreamWaitEvent(q, s->ev_fork, 0); used[a] = true; }
        }
        launch(i, q);
    }
    for (int a = 0; a < PackedScratch::NAUX; ++a)
        if (used[a]) { (void)hipEventRecord(s->ev_join[a], s->aux[a]); (void)hipStreamWaitEvent(stream, s->ev_join[a], 0); }
}

// drop the side streams and their events (packed_streams makes new ones at the next scan): after a stream capture that did
// not end well nobody knows what state the forked streams are in
static inline void packed_streams_reset(PackedScratch* s) {
    for (int i = 0; i < PackedScratch::NAUX; ++i) {
        if (s->aux[i]) (void)hipStreamDestroy(s->aux[i]);
        if (s->ev_join[i]) (void)hipEventDestroy(s->ev_join[i]);
        s->aux[i] = nullptr; s->ev_join[i] = nullptr;
    }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    s->ev_fork = nullptr;
}

// (the buffers free themselves with the scratch; the streams and events go here, on the context's device)
static inline void packed_scratch_free(PackedScratch* s) { packed_streams_reset(s); }

static inline int packed_max_width(const DevKit& k) {
    int m = 0;
    for (int t = 0; t < k.nt; ++t) m = std::max(m, k.tpl[t].width);
    return m;
}

static inline bool packed_supported(const DevKit& k) {
    if (!k.fast_ok || k.max_align > 150) return false;
    for (int t = 0; t < k.nt; ++t) {
        if (!k.tpl[t].width) return false;
        for (int s = 0; s < 2; ++s) if (k.tpl[t].sets[s].n && !k.tpl[t].sets[s].width) return false;
    }
    return true;
}

static inline int packed_fail(const char* what, hipError_t e) {
    g_packed_err = std::string(what) + ": " + hipGetErrorString(e);
    return (int)QCAT_ERR_DEVICE;
}
// room for n elements in a scratch buffer of the packed path, or this layer's error naming the buffer
template <class T>
static inline int packed_ensure(DevBuf<T>& b, size_t n, const char* what) {
    const hipError_t e = b.ensure(n);
    return e == hipSuccess ? 0 : packed_fail(("hipMalloc(" + std::string(what) + ")").c_str(), e);
}

// ---- bit-sliced adapter kernels: when, and their buffers ------------------------------------------------------------
static inline int abs_cu_count() {
    int cus = 256, dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}
// the bit-sliced plans template t has, as a mask of forms: 1 = two stages (k_adapter_bs), 2 = four stages of <= 13 columns
// (k_adapter_ms: medium batches), 4 = four wide stages (k_adapter_mw: templates too long for two stages) -- generated at
// build time for the built-in kits (abs_generated.inc) or at run time for a custom kit (qcat_amd/jit.py, DevTpl::abs_jit)
static inline int abs_forms(const DevKit& hk, int t) {
    const int sk = hk.tpl[t].static_kernel;
    if (sk < 0) return 0;
    if (sk >= QCAT_JIT_BASE) return hk.tpl[t].abs_jit;
    return (qcat_abs_launch(1, sk, 0, nullptr, nullptr) ? 1 : 0) | (qcat_abs_launch(2, sk, 0, nullptr, nullptr) ? 2 : 0) |
           (qcat_abs_launch(3, sk, 0, nullptr, nullptr) ? 4 : 0);
}
// launch form `form` (1, 2 or 4) of template t's plan
static inline void abs_launch_form(const DevKit& hk, int t, int form, unsigned grid, hipStream_t q, const AbsArgs& aa) {
    const int sk = hk.tpl[t].static_kernel;
    if (sk >= QCAT_JIT_BASE) jit_launch(form == 1 ? QCAT_JIT_ABS2 : (form == 2 ? QCAT_JIT_ABSM : QCAT_JIT_ABSW), t, dim3(grid), q, &aa);
    else (void)qcat_abs_launch(form == 1 ? 1 : (form == 2 ? 2 : 3), sk, grid, q, &aa);
}
// will the bit-sliced adapter kernels take a batch of n_ends read ends of this kit?  A tile occupies two waves for ~0.3 ms,
// so the two-stage plans pay from a few tiles per CU (default 3.5: 1.8 M read ends); below that the binary16 kernels are as
// fast or faster (config 2, 488 tiles: 0.44 ms bit-sliced as two single-template plans side by side, 0.54 ms as one fused
// plan, 0.45 ms binary16; the dual kit at 977 tiles: 1.50 against 1.70 ms) -- unless the templates have plans of four stages.
static inline bool packed_abs_wanted(const DevKit& hk, uint32_t n_ends, bool have_wspec) {
    const bool use_static_a = hk.adapter_f16 && !opt_on(QO_NO_STATIC) && !opt_on(QO_NO_STATIC_ADAPTER);
    const QOptVal amin = qopt_get(QO_ADAPTER_BITSLICE_MIN);                    // (tests: read ends from which the path is taken)
    const size_t abs_min = amin ? (size_t)atoll(amin) : (size_t)abs_cu_count() * 7 * ABS_TILE / 2;
    if (!(hk.abs_ok && have_wspec && use_static_a && !opt_on(QO_NO_ADAPTER_BITSLICE))) return false;
    // medium batches (from 1.5 tiles per CU): only when every template has a plan of four stages (four waves per tile,
    // k_adapter_ms: config 2's 488 tiles 0.39 ms against 0.45 ms binary16 and 0.44 ms on the two-stage plans)
    const size_t abs_min_ms = (size_t)abs_cu_count() * 3 * ABS_TILE / 2;
    const bool medium = n_ends < std::max<size_t>(abs_min, 1);
    if (medium && (amin || n_ends < abs_min_ms)) return false;
    bool any = false;
    for (int t = 0; t < hk.nt; ++t) {                                              // any template with a generated plan?
        const int forms = abs_forms(hk, t);
        if (medium) { if (!(forms & 2)) return false; any = true; continue; }
        if (forms & 5) any = true;
        if (hk.tpl[t].static_kernel >= 0 && hk.tpl[t].static_kernel < QCAT_JIT_BASE && hk.tpl[t].fused_kernel >= 0 &&
            qcat_abs_launch(0, hk.tpl[t].fused_kernel, 0, nullptr, nullptr) != 0) any = true;
    }
    return any;
}
// planes, keep masks and the zeroed flag block [tile cursors: MAX_T u32][tile_any: tiles u32][need128: tiles * 16 bytes]
static inline int packed_abs_buffers(hipStream_t stream, const DevKit& hk, uint32_t n_ends, PackedScratch* sc) {
    hipError_t e;
    int rc;
    const uint32_t abs_tiles = (n_ends + ABS_TILE - 1) / ABS_TILE;
    const size_t need_planes = (size_t)abs_tiles * hk.max_align * 64, need_valid = (size_t)abs_tiles * 64;
    const size_t need_flags = (size_t)MAX_T * 4 + (size_t)abs_tiles * 4 + (size_t)abs_tiles * (ABS_TILE / PK_TILE);
    if ((rc = packed_ensure(sc->abs_planes, need_planes, "adapter letter planes"))) return rc;
    if ((rc = packed_ensure(sc->abs_valid, need_valid, "adapter keep masks"))) return rc;
    if ((rc = packed_ensure(sc->abs_flags, need_flags, "adapter tile flags"))) return rc;
    if ((e = packed_fill(sc->abs_flags, 0, need_flags, stream)) != hipSuccess) return packed_fail("memset(adapter tile flags)", e);
    sc->abs_zeroed = n_ends;
    return 0;
}

// job tables + sorted-job array for `n_ends` read ends (zeroed / invalidated for a new scan)
static inline int packed_prepare(hipStream_t stream, const DevKit& hk, uint32_t n_ends, PackedScratch* sc) {
    auto fail = packed_fail;
    const int nsets = hk.mode == QCAT_MODE_DUAL ? 2 : 1;
    const size_t n_cand = (size_t)n_ends * nsets;
    const size_t need_sorted = n_cand + (size_t)JOB_GROUPS * PK_TILE;
    hipError_t e;
    int rc;
    if ((rc = packed_ensure(sc->jt, 1, "job tables"))) return rc;
    if ((e = packed_streams(sc)) != hipSuccess) return fail("side streams", e);
    if ((rc = packed_ensure(sc->sorted, need_sorted, "sorted jobs"))) return rc;
    if ((rc = packed_ensure(sc->jobinfo, n_cand, "job words"))) return rc;
    if (sc->slim) {
        if ((rc = packed_ensure(sc->posof, n_cand, "job positions"))) return rc;
        if ((rc = packed_ensure(sc->bcres, n_cand, "barcode results"))) return rc;
        if ((rc = packed_ensure(sc->fin, n_ends, "finalize words"))) return rc;
    }
    if ((e = packed_fill(sc->jt, 0, sizeof(JobTables), stream)) != hipSuccess) return fail("memset(job tables)", e);
    if ((e = packed_fill(sc->sorted, 0xFF, need_sorted * 4, stream)) != hipSuccess) return fail("memset(sorted)", e);
    // (the redo count of the summary mode with them: one launch instead of a memset of its own in the barcode phase)
    if (sc->redo && (e = packed_fill(sc->redo, 0, 4, stream)) != hipSuccess) return fail("memset(redo count)", e);
    sc->redo_zeroed = sc->redo != nullptr;

    return 0;
}

// adapter phase: every template against every read-end window, then k_adapter_finish (path choice,
// barcode regions, job histogram)
// k_adapter_finish over the slices the adapter launches left in sc->bests (kit_mask: see the kernel)
static inline int packed_adapter_finish(hipStream_t stream, KitPtrs kp, const uint8_t* /*win*/, const int32_t* wlen,
                                        uint32_t n_ends, EndRec* recs, PackedScratch* sc, int kit_mask) {
    const QOptVal fb_env = qopt_get(QO_FINISH_BLOCKS);                         // (A/B runs)
    // (1024 blocks, not 2048: every block flushes its job histogram with global atomics -- config 2's sort mark 0.100 -> 0.086 ms,
    // config 3 0.728 -> 0.721, the dual kit 0.178 -> 0.168; 512 and 256 lose again; tools/r04_finish.sh)
    const uint32_t fblocks = std::min<uint32_t>((n_ends + 255) / 256, fb_env ? (uint32_t)std::max(1, atoi(fb_env)) : 1024u);
    // kit_mask == RESUME_KIT_ON_DEVICE: the kit slot is read from sc->kit_slot_dev (k_pick_kit wrote it)
    const int32_t* slot_dev = kit_mask == RESUME_KIT_ON_DEVICE ? sc->kit_slot_dev : nullptr;
    hipLaunchKernelGGL(k_adapter_finish, dim3(fblocks), dim3(256), 0, stream, kp.kit, wlen, n_ends, sc->bests, sc->n_slices, recs, sc->jt,
                       (const int32_t*)nullptr, slot_dev ? -1 : kit_mask, sc->wspec, sc->jobinfo, sc->slim ? sc->bcres : nullptr, sc->fin_only ? sc->fin : nullptr,
                       slot_dev, slot_dev ? sc->kit_slot_span : 0u);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return packed_fail("packed kernel launch", e);
    return 0;
}

template <class Mark>
static inline int packed_adapter(hipStream_t stream, KitPtrs kp, const DevKit& hk, const uint8_t* win,
                                 const int32_t* wlen, uint32_t n_ends, EndRec* recs, PackedScratch* sc,
                                 int32_t* dbg_tpl, Mark mark) {
    auto fail = packed_fail;
    hipError_t e;
    int rc;
    // (launches of different width classes are independent; running them on two streams was
    //  measured and gave no overlap benefit on MI355X, so everything stays on the context's stream)
    const int adapter_widths[] = {40, 48, 56, 60, 64, 84, 92, 104, 112, 120, 128};
    // templates with a generated static-letter kernel get one launch (and one slice of `bests`) each;
    // the rest run the table kernel of their width class
    const bool use_static_a = hk.adapter_f16 && !opt_on(QO_NO_STATIC) && !opt_on(QO_NO_STATIC_ADAPTER);
    auto table_tpl = [&](int t, int w) { return hk.tpl[t].width == w && !(use_static_a && hk.tpl[t].static_kernel >= 0); };
    int n_slices = 0, n_static_a = 0;
    for (int w : adapter_widths) { bool present = false; for (int t = 0; t < hk.nt; ++t) present |= table_tpl(t, w); n_slices += present; }
    for (int t = 0; t < hk.nt; ++t) if (use_static_a && hk.tpl[t].static_kernel >= 0) { ++n_slices; ++n_static_a; }
    if ((rc = packed_ensure(sc->bests, (size_t)n_ends * n_slices, "adapter bests"))) return rc;
    const uint32_t tiles = (n_ends + PK_TILE - 1) / PK_TILE;
    const uint32_t blocks = (tiles + PK_WAVES - 1) / PK_WAVES;
    {
        int slice = 0;
#define QK_LAUNCH(WW, TT) do { bool present = false; for (int t = 0; t < hk.nt; ++t) present |= table_tpl(t, WW); \
        if (present) { hipLaunchKernelGGL((k_adapter_packed<WW, TT>), dim3(blocks), dim3(PK_WAVES * 64), 0, stream, kp, win, wlen, n_ends, \
                                          sc->bests + (size_t)slice * n_ends, dbg_tpl, use_static_a ? 1 : 0); ++slice; } } while (0)
        QK_LAUNCH(40, TBL_VGPR); QK_LAUNCH(48, TBL_VGPR); QK_LAUNCH(56, TBL_VGPR); QK_LAUNCH(60, TBL_VGPR); QK_LAUNCH(64, TBL_VGPR);
        QK_LAUNCH(84, TBL_LDS); QK_LAUNCH(92, TBL_LDS); QK_LAUNCH(104, TBL_LDS); QK_LAUNCH(112, TBL_LDS); QK_LAUNCH(120, TBL_LDS); QK_LAUNCH(128, TBL_LDS);
#undef QK_LAUNCH
        if (slice) mark("k_adapter_packed");
        // one launch per static template, or one per two-template kit that has a fused kernel
        const bool use_fused = !opt_on(QO_NO_FUSED_ADAPTER);
        // will the bit-sliced adapter kernels take this batch (packed_abs_wanted)?  A medium batch that is forced onto the
        // path (QCAT_HIP_ADAPTER_BITSLICE_MIN: tests, A/B runs) runs the two templates of a kit as two single-template plans
        // side by side, which doubles the waves
        const uint32_t abs_tiles = (n_ends + ABS_TILE - 1) / ABS_TILE;
        const int abs_cus = abs_cu_count();
        const bool abs_wanted = packed_abs_wanted(hk, n_ends, sc->wspec != nullptr && (sc->win2 != nullptr || sc->abs_ready == n_ends));
        const bool abs_split = abs_wanted && abs_tiles < (uint32_t)abs_cus * 4u && !opt_on(QO_ABS_NO_SPLIT);
        int stpl[MAX_T], sslice[MAX_T], spartner[MAX_T], pslice[MAX_T];
        int ns = 0, nsl = 0;
        bool taken[MAX_T] = {};
        for (int t = 0; t < hk.nt; ++t) {
            if (!(use_static_a && hk.tpl[t].static_kernel >= 0) || taken[t]) continue;
            stpl[ns] = t; sslice[ns] = slice + nsl++; spartner[ns] = -1; pslice[ns] = 0;
            const int p = hk.tpl[t].fused_partner;
            const bool split_pair = abs_split && p > t && hk.tpl[t].static_kernel < QCAT_JIT_BASE &&
                                    (abs_forms(hk, t) & 1) && (abs_forms(hk, p) & 1);
            if (!split_pair && use_fused && hk.tpl[t].fused_kernel >= 0 && hk.tpl[t].static_kernel < QCAT_JIT_BASE && p > t && !taken[p]) {
                spartner[ns] = p; pslice[ns] = slice + nsl++; taken[p] = true;
            }
            ++ns;
        }
        // bit-sliced adapter kernels (kernels_abs.inc) for the units that have a generated plan: full-length windows of
        // plain A/C/G/T (every tile of 2048 read ends is computed whole, `valid` keeps those), the binary16 kernel of the
        // unit then scans only the 128-end tiles that hold some other window.  Big batches only (a tile occupies two
        // waves for ~0.3 ms).
        bool abs_plan[MAX_T] = {};
        bool use_abs = false;
        {
            if (abs_wanted)
                for (int i = 0; i < ns; ++i) {
                    const int t = stpl[i];
                    abs_plan[i] = spartner[i] >= 0 ? qcat_abs_launch(0, hk.tpl[t].fused_kernel, 0, nullptr, nullptr) != 0
                                                   : (abs_forms(hk, t) & 5) != 0;
                    use_abs = use_abs || abs_plan[i];
                }
        }
        uint32_t* abs_cursor = nullptr; uint32_t* abs_tile_any = nullptr; uint8_t* abs_need128 = nullptr;
        if (use_abs) {
            // (the fused pack kernel of this scan may have made planes and flags already: scan_resident_impl)
            const bool ready = sc->abs_ready == n_ends;
            if (!ready && sc->abs_zeroed != n_ends) { const int rc2 = packed_abs_buffers(stream, hk, n_ends, sc); if (rc2) return rc2; }
            sc->abs_zeroed = 0;
            abs_cursor = reinterpret_cast<uint32_t*>(sc->abs_flags.get());
            abs_tile_any = abs_cursor + MAX_T;
            abs_need128 = reinterpret_cast<uint8_t*>(abs_tile_any + abs_tiles);
            if (!ready)
                qcat_abs_launch_planes(abs_tiles, stream, sc->win2, wlen, sc->wspec, n_ends, hk.max_align, sc->abs_planes, sc->abs_valid,
                                       abs_need128, abs_tile_any);
        }
        sc->abs_ready = 0;
        const int abs_prio = (int)opt_val(QO_ABS_PRIO, 0);
        // plans of four stages (four waves per tile, k_adapter_ms) when the tiles alone would leave SIMDs with one wave
        // (QCAT_HIP_ABS_STAGES=2 / 4: one form for every batch -- A/B runs and the tests)
        const QOptVal stages_env = qopt_get(QO_ABS_STAGES);
        const bool abs_ms = stages_env ? atoi(stages_env) == 4 : abs_tiles < (uint32_t)abs_cus * 7u / 2u;
        const bool adapter_reverse = opt_on(QO_ADAPTER_REVERSE);      // (A/B: which of two side-by-side launches goes first)
        const bool adapter_serial = opt_on(QO_ABS_SERIAL) && use_abs;  // (A/B: the units' launches one after the other on the scan's stream)
        auto adapter_unit = [&](int i0, hipStream_t q) {
            const int i = adapter_reverse ? ns - 1 - i0 : i0;
            const int t = stpl[i];
            StaticAdapterArgs sa{kp, win, wlen, n_ends, sc->bests + (size_t)sslice[i] * n_ends, dbg_tpl, t,
                                 spartner[i] >= 0 ? sc->bests + (size_t)pslice[i] * n_ends : nullptr, spartner[i],
                                 abs_plan[i] ? abs_need128 : nullptr, sc->lazy ? sc->win2 : nullptr, sc->wspec};
            if (abs_plan[i]) {
                AbsArgs aa{sc->abs_planes, sc->abs_valid, abs_tile_any, {sa.bests, sa.bests2}, {t, spartner[i]},
                           {hk.tpl[t].den, spartner[i] >= 0 ? hk.tpl[spartner[i]].den : 0}, n_ends, abs_tiles, hk.max_align, abs_cursor + i, dbg_tpl, abs_prio, hk.r1_scalar};
                const unsigned grid = (unsigned)std::min<uint32_t>(abs_tiles, (uint32_t)abs_cus * 4u);   // persistent: four two-wave workgroups per CU
                if (spartner[i] >= 0) (void)qcat_abs_launch(0, hk.tpl[t].fused_kernel, grid, q, &aa);
                else {
                    // the four-stage form for medium batches when the template has one (four four-wave workgroups per CU as
                    // well); else two stages; else -- a template too long for two stages -- four wide stages (two
                    // four-wave workgroups per CU)
                    const int forms = abs_forms(hk, t);
                    if (abs_ms && (forms & 2)) abs_launch_form(hk, t, 2, grid, q, aa);
                    else if (forms & 1) abs_launch_form(hk, t, 1, grid, q, aa);
                    else abs_launch_form(hk, t, 4, (unsigned)std::min<uint32_t>(abs_tiles, (uint32_t)abs_cus * 2u), q, aa);
                }
            }
            if (spartner[i] >= 0) launch_adapter_fused(hk.tpl[t].fused_kernel, dim3(tiles), q, sa);
            else launch_adapter_static(hk.tpl[t].static_kernel, dim3(tiles), q, sa);
        };
        // a small batch (round 6): its units are latency chains -- 63 one-wave workgroups each for the reference driver's 4000
        // reads, 50-110 us -- which launches of their own spread over the runtime's four hardware queues, where they wait for
        // each other (nine launches: 240 us, the longest: 110).  One launch, blockIdx.y = the unit, while the whole batch is
        // at most four waves per SIMD -- two rounds of the merged kernel, which is compiled for the widest chain's registers
        // (kit-auto calls of 8000 / 16 000 / 24 000 reads: 1.04 -> 0.97, 2.0 -> 1.76, 2.7 -> 2.4 ms against a limit of one round).
        bool multi = ns >= 2 && !use_abs && !opt_on(QO_NO_ADAPTER_MULTI) && (uint64_t)tiles * (uint64_t)ns <= (uint64_t)abs_cus * 16u;
        for (int i = 0; i < ns && multi; ++i) multi = hk.tpl[stpl[i]].static_kernel < QCAT_JIT_BASE;
        if (multi) {
            StaticAdapterMulti mm{};
            mm.common = StaticAdapterArgs{kp, win, wlen, n_ends, nullptr, dbg_tpl, 0, nullptr, -1, nullptr, sc->lazy ? sc->win2 : nullptr, sc->wspec};
            for (int i = 0; i < ns; ++i) {
                const int t = stpl[i];
                mm.bests[i] = sc->bests + (size_t)sslice[i] * n_ends;
                mm.bests2[i] = spartner[i] >= 0 ? sc->bests + (size_t)pslice[i] * n_ends : nullptr;
                mm.tpl[i] = (int16_t)t; mm.tpl2[i] = (int16_t)spartner[i];
                mm.fused[i] = spartner[i] >= 0 ? 1 : 0;
                mm.kernel[i] = (int16_t)(spartner[i] >= 0 ? hk.tpl[t].fused_kernel : hk.tpl[t].static_kernel);
            }
            launch_adapter_multi(dim3(tiles, (uint32_t)ns), stream, mm);
        } else if (adapter_serial) for (int i0 = 0; i0 < ns; ++i0) adapter_unit(i0, stream);
        else fork_join(sc, stream, ns, adapter_unit);
        slice += nsl;
        if (n_static_a) mark(use_abs ? "k_adapter_bitslice" : "k_adapter_static");
    }
    sc->n_slices = n_slices;
    sc->slices_single = n_static_a == n_slices;       // every slice holds exactly one template (static-letter kernels)
    if ((e = hipGetLastError()) != hipSuccess) return fail("packed kernel launch", e);
    rc = jit_take_error();
    if (rc) return rc;
    return packed_adapter_finish(stream, kp, win, wlen, n_ends, recs, sc, -1);
}

// barcode phase: counting sort of the jobs in `recs`, tile images (through `gather`, which is given
// the tile capacity), barcode kernels, k_barcode_select
template <class Mark, class Gather>
static inline int packed_barcode(hipStream_t stream, KitPtrs kp, const DevKit& hk, uint32_t n_ends, EndRec* recs,
                                 PackedScratch* sc, Gather gather, int16_t* dbg_rows, uint32_t stride, Mark mark) {
    auto fail = packed_fail;
    hipError_t e;
    int rc;
    const int nsets = hk.mode == QCAT_MODE_DUAL ? 2 : 1;
    const size_t n_cand = (size_t)n_ends * nsets;
    const size_t need_sorted = n_cand + (size_t)JOB_GROUPS * PK_TILE;
    hipLaunchKernelGGL(k_job_offsets, dim3(1), dim3(128), 0, stream, sc->jt);
    {
        const uint32_t per_block = 256u * SCAT_PER_THREAD;
        const uint32_t sblocks = (uint32_t)((n_cand + per_block - 1) / per_block);
        hipLaunchKernelGGL(k_job_scatter, dim3(sblocks), dim3(256), 0, stream, sc->jobinfo, n_ends, nsets, sc->jt, sc->sorted, sc->slim ? sc->posof : nullptr);
    }
    const uint32_t max_tiles = (uint32_t)(need_sorted / PK_TILE);
    if ((rc = packed_ensure(sc->tilebuf, (size_t)max_tiles * 64 * WIN_STRIDE, "tile images"))) return rc;
    if ((rc = packed_ensure(sc->tmeta, (size_t)max_tiles * 64, "tile meta"))) return rc;
    // the tile images are made right before their first reader: the bit-sliced kernels read the hot regions from the
    // windows themselves, and k_bs_plan (which says what they take) has to run before the gather that leaves those tiles out
    bool gathered = false;
    auto ensure_gather = [&](const BsPlan* taken) {
        if (gathered) return;
        gather(max_tiles, taken, stream);
        mark("k_job_sort");
        gathered = true;
    };
    {
        int bstride = 1;                                    // most barcodes any group scans
        for (int t = 0; t < hk.nt; ++t) for (int s = 0; s < nsets; ++s) bstride = std::max(bstride, (int)hk.tpl[t].sets[s].n);
        // summary mode: every group on static-letter kernels and nobody wants the per-barcode rows -> no `raws`
        const bool use_static0 = hk.barcode_f16 && !opt_on(QO_NO_STATIC);
        // (sets of up to 32 barcodes keep the raw scores -- 128 B per alignment are not worth two more launches per
        // scan -- unless the batch is big enough for the bit-sliced kernels, which only produce keys)
        bool bs_sets = false;
        for (int t = 0; t < hk.nt; ++t) for (int s = 0; s < nsets; ++s) bs_sets = bs_sets || hk.tpl[t].sets[s].bs_off >= 0;
        const QOptVal bs_min_env = qopt_get(QO_BITSLICE_MIN);          // (tests: alignments from which the path is taken)
        // default: where the two paths cross.  The bit-sliced launch costs about the same whatever the batch (one workgroup
        // per CU and unit: 0.35 ms + 7 us per barcode of the largest set for up to a unit per CU), the binary16 kernels 0.1 ns
        // per job and barcode: 106 k jobs for a 96-barcode set, 360 k for 12 barcodes (measured, profiles/r03_bs_threshold.txt:
        // config 3 at 250 k reads 49 -> 137 M reads/s; round 2 had one super-tile per CU, 524 288 jobs, for every kit)
        // (round 6, re-measured after rounds 4-6 made both sides faster -- tools/r06_bs_threshold.sh, profiles/r06_bs_threshold.txt:
        // PBC096 crosses at 58 k jobs, a 12-barcode kit at 200 k; round 3's switch sat at 106 k and 361 k and left up to 23 %
        // of a 40-50 k-read scan on the table)
        // (a dual kit -- four groups, four launches, half of its jobs on the small first set -- keeps round 3's switch: at 64 k and
        // 96 k jobs the binary16 kernels are still 25 % ahead there, at 128 k the two are level)
        const size_t bs_min = bs_min_env ? (size_t)atoll(bs_min_env)
                                         : (nsets == 2 ? (size_t)70000 + (size_t)3500000 / (size_t)std::max(1, bstride)
                                                       : (size_t)40000 + (size_t)1900000 / (size_t)std::max(1, bstride));
        // (QCAT_HIP_BS_FROM_TILES=1: the bit-sliced kernels read tile images like the binary16 ones -- A/B runs)
        const bool bs_direct = !opt_on(QO_BS_FROM_TILES) && sc->win != nullptr && sc->win2 != nullptr;
        // Round 4, measured and NOT the default: a small batch of a big barcode set (the reference driver's 4000-read call of a
        // 96-barcode kit: 8000 jobs whose binary16 tiles take 0.2 ms) on the bit-sliced kernels with one PADDED super-tile per
        // hot bin (k_bs_plan: pad_min).  Parity-clean (tests, fuzz sweep), and slower: a unit is 2048 jobs x a chunk of
        // barcodes, so 8000 jobs are a dozen units on a dozen CUs at 8.7 us per barcode and 150 rows -- native call 1.30 against
        // 0.92 ms; 25 k reads: 0.795 against 0.799 ms (tools/r04_pad.sh).  QCAT_HIP_BITSLICE_PAD=<jobs> turns it on (regions
        // read in place only): the tests keep the partly filled super-tiles honest.
        const QOptVal pad_env = qopt_get(QO_BITSLICE_PAD);
        // Round 5: for a batch of at least a super-tile per CU it is the default (128 jobs): the rest of a hot class -- up to 2047
        // jobs per class and group -- rides as one more unit at the end of the queue instead of being the 150-row tiles whose
        // latency was what was left of the binary16 launch (config 3: k_barcode_static 0.36 -> 0.25 ms, tools/r05_short.sh).
        int bs_cus = 256;
        { int dev = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&bs_cus, hipDeviceAttributeMultiprocessorCount, dev); }
        const uint32_t bs_pad_min = !bs_direct ? 0u : (pad_env ? (uint32_t)std::max(0, atoi(pad_env)) / PK_TILE * PK_TILE
                                                               : (n_cand / BS_JOBS >= (size_t)bs_cus ? (uint32_t)PK_TILE : 0u));
        const bool small_big_set = pad_env && bs_pad_min > 0 && bstride >= 48 && n_cand >= 2048 && n_cand < std::max<size_t>(bs_min, BS_JOBS) && !bs_min_env;
        const bool bs_wanted = hk.bs_ok && bs_sets && sc->wspec && !opt_on(QO_NO_BITSLICE) &&
                               (n_cand >= std::max<size_t>(bs_min, BS_JOBS) || (small_big_set && bs_pad_min > 0));
        bool summary = use_static0 && dbg_rows == nullptr && !opt_on(QO_RAWS) &&
                       (bstride > 32 || bs_wanted || opt_on(QO_SUMMARY));
        for (int t = 0; t < hk.nt && summary; ++t)
            for (int s = 0; s < nsets; ++s) if (hk.tpl[t].sets[s].static_kernel < 0) { summary = false; break; }
        const size_t need_raws = summary ? 0 : (size_t)max_tiles * bstride * 64;
        if (need_raws && (rc = packed_ensure(sc->raws, need_raws, "raw barcode scores"))) return rc;
        // barcodes per work unit: ~4 (a unit of 4 x 47 rows still amortises its staging to < 2 %)
        const QOptVal chunk_env = qopt_get(QO_CHUNK_BARCODES);
        const int chunk_b = chunk_env ? std::max(1, atoi(chunk_env)) : 4;
        const int nch = std::max(1, (bstride + chunk_b - 1) / chunk_b);
        const uint32_t bblocks = (uint32_t)(((uint64_t)max_tiles * nch + PK_WAVES - 1) / PK_WAVES);
        const int order = 1;                                 // longest tiles first
        // groups whose targets all have generated static-letter chains run k_barcode_static<G>
        const bool use_static = hk.barcode_f16 && !opt_on(QO_NO_STATIC);   // (env: A/B tests)
        bool have[7] = {false, false, false, false, false, false, false};   // width classes the table kernels must cover
        bool any_table = false, any_static = false;
        for (int t = 0; t < hk.nt; ++t)
            for (int s = 0; s < nsets; ++s) {
                if (use_static && hk.tpl[t].sets[s].static_kernel >= 0) { any_static = true; continue; }
                const int w = hk.tpl[t].sets[s].width;
                have[w == 40 ? 0 : (w == 44 ? 1 : (w == 48 ? 2 : (w == 56 ? 3 : (w == 64 ? 4 : (w == 42 ? 5 : 6)))))] = true;
                any_table = true;
            }
        if (any_table) ensure_gather(nullptr);
#define QK_LAUNCH_B(IDX, WW) if (have[IDX]) { \
            if (hk.barcode_f16) hipLaunchKernelGGL((k_barcode_packed<WW, true>), dim3(bblocks), dim3(PK_WAVES * 64), 0, stream, \
                                                   kp, sc->tilebuf, sc->tmeta, sc->jt, sc->raws, bstride, nch, order, use_static ? 1 : 0); \
            else hipLaunchKernelGGL((k_barcode_packed<WW, false>), dim3(bblocks), dim3(PK_WAVES * 64), 0, stream, \
                                    kp, sc->tilebuf, sc->tmeta, sc->jt, sc->raws, bstride, nch, order, use_static ? 1 : 0); }
        QK_LAUNCH_B(0, 40) QK_LAUNCH_B(5, 42) QK_LAUNCH_B(1, 44) QK_LAUNCH_B(6, 46) QK_LAUNCH_B(2, 48) QK_LAUNCH_B(3, 56) QK_LAUNCH_B(4, 64)
#undef QK_LAUNCH_B
        if (any_table) mark("k_barcode_packed");
        if (any_static) {
            int dev = 0, cus = 256;
            (void)hipGetDevice(&dev);
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            const uint32_t persist = (uint32_t)cus * 16u;       // one-wave workgroups: 4 per SIMD fill the chip
            int sgrp[JOB_GROUPS];
            int ng = 0;
            for (int t = 0; t < hk.nt; ++t)
                for (int s = 0; s < nsets; ++s) if (hk.tpl[t].sets[s].static_kernel >= 0) sgrp[ng++] = t * 2 + s;
            // barcodes per unit: small sets need fine units (one pair) to fill the chip evenly; for big sets 8 per
            // unit halves the re-staging of tile images at the same speed (tools/bench_variants.sh)
            // (even: the static chains take barcodes in pairs)
            // (a small batch -- the reference driver's 4000 reads: 63 tiles -- leaves most of the 4096 wave slots empty with
            // units of eight barcodes: units of four, one quad pass, halve the latency of the phase)
            const bool few_units = (uint64_t)max_tiles * std::max(1, bstride / 8) < (uint64_t)persist / 2;
            // (... and when even units of one pair leave wave slots free, pairs: the phase of such a batch lasts as long as its
            // longest unit -- 185 us for 150 rows x 4 barcodes of the PBC096 group in a 730 us call)
            const bool tiny_units = (uint64_t)max_tiles * std::max(1, bstride / 2) <= (uint64_t)persist;
            auto unit_barcodes = [&](int gidx) {
                return chunk_env ? ((chunk_b + 1) & ~1) : (hk.tpl[gidx >> 1].sets[gidx & 1].n <= 24 || tiny_units ? 2 : (few_units ? 4 : 8));
            };
            NchOfGroup nch_of{};
            int part_stride = 1;
            for (int i = 0; i < ng; ++i) {
                const int gidx = sgrp[i];
                const DevSet& gs = hk.tpl[gidx >> 1].sets[gidx & 1];
                nch_of.v[gidx] = static_units(gs.n_quads, gs.n_pairs, unit_barcodes(gidx));   // as barcode_static_body counts them
                part_stride = std::max(part_stride, nch_of.v[gidx]);
            }
            if (summary) {
                const size_t need_part = (size_t)max_tiles * part_stride * 128, need_redo = (size_t)max_tiles * 128 + 1;
                if ((rc = packed_ensure(sc->part, need_part, "barcode keys"))) return rc;
                if (need_redo > sc->redo.cap()) sc->redo_zeroed = false;                 // (packed_prepare zeroed the count of a buffer that is freed now)
                if ((rc = packed_ensure(sc->redo, need_redo, "redo list"))) return rc;
                if (!sc->redo_zeroed && (e = hipMemsetAsync(sc->redo, 0, 4, stream)) != hipSuccess) return fail("memset(redo count)", e);
                sc->redo_zeroed = false;
            }
            // the static-letter binary16 kernel of group i of `sgrp` (every tile, or the tiles the bit-sliced kernels leave)
            auto static_launch = [&](int i, hipStream_t q, const BsPlan* covered) {
                const int gidx = sgrp[i];
                StaticArgs sa{kp, sc->tilebuf, sc->tmeta, sc->jt, summary ? nullptr : sc->raws, bstride, unit_barcodes(gidx), gidx,
                              opt_on(QO_ONE_QUEUE) ? 0 : 1, summary ? sc->part : nullptr, part_stride, covered};
                launch_barcode_static(hk.tpl[gidx >> 1].sets[gidx & 1].static_kernel, dim3(persist), q, sa);
            };
            bool leftover_beside = false;
            // bit-sliced kernels for the full super-tiles of the hot classes (kernels_bitslice.inc); the launches
            // below skip the tiles those cover
            const BsPlan* bs = nullptr;
            BsNch bsn{};
            sc->bs_last = false;
            const size_t max_super = n_cand / BS_JOBS;
            if (summary && bs_wanted) {
                bool any = false;
                // one launch (and unit cursor) per kernel: a static-letter kernel per target family, else one per
                // number of own columns
                // (small batches stay on the letters-from-memory kernels: one launch for all groups of a width instead of
                // one per target family, each with its own tail)
                // (round 4: the generated kernels at every batch size -- the families of a medium batch on side streams, where the
                // second launch's workgroups take the CUs the first one frees; QCAT_HIP_BS_STATIC_MIN=<super-tiles> moves the
                // switch for A/B runs)
                const QOptVal bs_static_min = qopt_get(QO_BS_STATIC_MIN);
                const int use_static_bs = !opt_on(QO_NO_BS_STATIC) && (max_super >= (size_t)(bs_static_min ? atoll(bs_static_min) : 0) || bs_min_env) ? 1 : 0;
                int owns[8], n_owns = 0;                                      // kernel id + 1 (static) or -(own columns)
                for (int i = 0; i < ng; ++i) {
                    const DevSet& gs = hk.tpl[sgrp[i] >> 1].sets[sgrp[i] & 1];
                    if (gs.bs_off < 0) continue;
                    {
                        const int own = use_static_bs && gs.bs_kernel >= 0 ? gs.bs_kernel + 1 : -(gs.tlen - gs.bs_pre - gs.bs_post);
                        int q = 0;
                        while (q < n_owns && owns[q] != own) ++q;
                        if (q == n_owns) { if (n_owns == 8) continue; owns[n_owns++] = own; }
                    }
                    // barcode chunks per super-tile: one, unless the batch is too small to keep every CU busy (a chunk
                    // repeats the shared columns, and a wave should have two barcodes or more)
                    int want = (int)std::min<size_t>(BS_MAX_CHUNKS, ((size_t)cus * 6 + max_super - 1) / max_super);
                    want = std::max(1, std::min(want, gs.n / (2 * BS_WAVES)));
                    const int per = (gs.n + want - 1) / want;
                    bsn.v[sgrp[i]] = (gs.n + per - 1) / per;
                    any = true;
                }
                if (any) {
                    const size_t need_keys = (size_t)BS_MAX_CHUNKS * need_sorted;
                    if ((rc = packed_ensure(sc->bsplan, 1, "bit-slice plan"))) return rc;
                    if ((rc = packed_ensure(sc->bskeys, need_keys, "bit-slice keys"))) return rc;
                    // a workgroup's unit parks the trailing columns' plane pairs in global memory (8 bytes per row and lane: 77 KB per
                    // workgroup, read back from L2 by its own waves; one workgroup per CU and launch)
                    const size_t need_rp = (size_t)n_owns * (size_t)cus * BS_MAX_ROWS * 64;
                    if ((rc = packed_ensure(sc->bsrp, need_rp, "bit-slice trailing planes"))) return rc;
                    hipLaunchKernelGGL(k_bs_plan, dim3(1), dim3(256), 0, stream, kp.kit, sc->jt, bsn, sc->bsplan,
                                       opt_on(QO_BS_NO_TAIL_SPLIT) ? 0 : cus, bs_pad_min, (bs_direct && !opt_on(QO_BS_NO_SHORT)) ? 1 : 0);
                    // (Round 4, measured and dropped: the tile images of a medium batch made on a side stream beside the bit-sliced
                    // launches -- only the binary16 kernels read them.  Config 2: 1.047 against 1.010 ms in line; the gather's
                    // workgroups and the cross-stream signals delay the first round of units by more than the 22 us they hide;
                    // tools/r04_gather.sh.)
                    const QOptVal lo_env = qopt_get(QO_LEFTOVER_SIDE);
                    // (round 5: every batch size -- with the clipped regions and the classes' rests inside bit-sliced units what is left
                    // for the binary16 kernels is a fraction of a millisecond of latency, which hides beside the long launches:
                    // config 3 -0.2 ms, shipped dual kit -0.05 ms; before, big batches kept them in line: max_super < 4 CUs' worth)
                    leftover_beside = lo_env ? atoi(lo_env) != 0 : true;
                    ensure_gather(bs_direct ? sc->bsplan : nullptr);
                    DevBuf<unsigned long long> bs_trace;
                    const size_t bs_trace_words = (size_t)BS_TRACE_STAMPS + 1 + (size_t)BS_TRACE_LOG * 4;
                    if (opt_on(QO_BS_TRACE) && bs_trace.ensure(bs_trace_words) == hipSuccess) (void)hipMemsetAsync(bs_trace, 0, bs_trace_words * 8, stream);
                    // big batches: the launches (one per target family) go to side streams.  A workgroup holds a whole
                    // CU, so they cannot share one, but the next launch's workgroups take the CUs the previous one's
                    // tail frees (its last units end up to a unit -- 0.3 to 1 ms -- apart): config 3 238.3 -> 239.6 M
                    // reads/s.  Launches of a millisecond or two lose more to the concurrent dispatch than their tails
                    // cost (shipped dual kit at 1 M reads: 195 -> 189 M), so they stay in line.  (Measured and dropped,
                    // tools/ab_bs_streams.sh: the left-over binary16 tiles beside the bit-sliced kernels -- 235 M on
                    // streams of the same priority, 227 M on streams of the lowest.)
                    auto bs_launch = [&](int q, hipStream_t sq) {
                        const BsArgs ba{kp, sc->tilebuf, sc->bsplan, bsn, sc->bskeys, (uint32_t)need_sorted, q, use_static_bs, bs_trace,
                                        bs_direct ? sc->win2 : nullptr, sc->jobinfo, sc->sorted, nsets, !opt_on(QO_BS_NO_SOLO) ? 1 : 0, sc->bsrp,
                                        (int)opt_val(QO_BS_TRACE_WG, 0), (int)opt_val(QO_BS_TRACE_SEQ, 0),
                                        (int)opt_val(QO_BS_DRAW, 1)};
                        if (owns[q] > 0) launch_bs_static(owns[q] - 1, dim3((uint32_t)cus), sq, ba);
                        else launch_bs_barcode(-owns[q], dim3((uint32_t)cus), sq, ba);
                    };
                    // (QCAT_HIP_BS_SERIAL=1 / QCAT_HIP_BS_SIDE=1: one arrangement for every batch size -- A/B runs and the tests)
                    // (a medium batch, up to four super-tiles per CU, has two rounds of units at most: its families side by
                    // side too; in between -- the shipped dual kit at 1 M reads -- the launches stay in line, as measured in round 2)
                    // Round 4: a medium batch also starts the left-over binary16 tiles of every group BESIDE the bit-sliced
                    // launches (they need the tile images and the plan, not the bit-sliced results): the last round of units
                    // leaves most CUs idle -- config 2 has 266 long units for 256 CUs -- and the one-wave workgroups of the
                    // left-over kernels (0.14 ms on their own: a unit's latency, not volume) run there.  QCAT_HIP_LEFTOVER_SIDE=0 / 1.
                    if (leftover_beside) {
                        fork_join(sc, stream, n_owns + ng, [&](int i, hipStream_t sq) {
                            if (i < n_owns) bs_launch(i, sq); else static_launch(i - n_owns, sq, sc->bsplan);
                        });
                    } else if (opt_on(QO_BS_SERIAL) || (max_super < (size_t)cus * 16 && max_super >= (size_t)cus * 4 && !opt_on(QO_BS_SIDE)))
                        for (int q = 0; q < n_owns; ++q) bs_launch(q, stream);
                    else fork_join(sc, stream, n_owns, bs_launch);
                    if (bs_trace) {                           // (diagnostics: phase boundaries of workgroup 0's first units, in shader cycles)
                        std::vector<unsigned long long> ht(bs_trace_words);
                        (void)hipStreamSynchronize(stream);
                        (void)hipMemcpy(ht.data(), bs_trace, ht.size() * 8, hipMemcpyDeviceToHost);
                        for (int q = 0; q < n_owns; ++q)
                            for (int u = 0; u < 8; ++u) {
                                const unsigned long long t0 = ht[((size_t)q * 8 + u) * BS_WAVES * 8];
                                if (!t0 || !ht[((size_t)q * 8 + u) * BS_WAVES * 8 + 7]) continue;
                                for (int w = 0; w < BS_WAVES; ++w) {
                                    fprintf(stderr, "[qcat] bs launch %d unit %d wave %2d:", q, u, w);
                                    for (int ev = 0; ev < 8; ++ev) fprintf(stderr, " %9lld", (long long)(ht[(((size_t)q * 8 + u) * BS_WAVES + w) * 8 + ev] - t0));
                                    fprintf(stderr, "\n");
                                }
                            }
                        {   // the unit log: per (launch, bin, chunks) how many units, their mean duration, first start, last end
                            const unsigned long long* lg = ht.data() + BS_TRACE_STAMPS;
                            const size_t n_log = (size_t)std::min<unsigned long long>(lg[0], BS_TRACE_LOG);
                            unsigned long long tmin = ~0ull;
                            for (size_t i = 0; i < n_log; ++i) tmin = std::min(tmin, lg[1 + i * 4 + 1]);
                            struct Agg { unsigned long long n = 0, dur = 0, first = ~0ull, last = 0; };
                            std::map<unsigned long long, Agg> agg;
                            for (size_t i = 0; i < n_log; ++i) {
                                const unsigned long long* e = lg + 1 + i * 4;
                                Agg& a = agg[e[0] >> 32];
                                a.n++; a.dur += e[2] - e[1]; a.first = std::min(a.first, e[1] - tmin); a.last = std::max(a.last, e[2] - tmin);
                            }
                            for (const auto& kv : agg)
                                fprintf(stderr, "[qcat] bs units: launch %llu bin %3llu chunks %llu: %5llu units, mean %8llu cycles, first start %8llu, last end %8llu\n",
                                        kv.first >> 24, (kv.first >> 8) & 0xFFFF, kv.first & 0xFF, kv.second.n, kv.second.dur / kv.second.n, kv.second.first, kv.second.last);
                            if (opt_on(QO_BS_TRACE_UNITS))
                                for (size_t i = 0; i < n_log; ++i) {
                                    const unsigned long long* e = lg + 1 + i * 4;
                                    fprintf(stderr, "[qcat] bs unit: launch %llu bin %llu chunks %llu chunk %llu wg %llu rows %llu: %llu .. %llu\n", e[0] >> 56, (e[0] >> 40) & 0xFFFF,
                                            (e[0] >> 32) & 0xFF, (e[0] >> 24) & 0xFF, e[0] & 0xFFFFFF, e[3], e[1] - tmin, e[2] - tmin);
                                }
                        }
                    }
                    if (sc->slim)
                        hipLaunchKernelGGL(k_bs_select_ordered, dim3((uint32_t)std::min<size_t>((n_cand + 255) / 256, 65536)), dim3(256), 0, stream,
                                           sc->jobinfo, sc->posof, (uint32_t)n_cand, sc->bsplan, bsn, sc->bskeys, (uint32_t)need_sorted, sc->bcres,
                                           sc->redo + 1, sc->redo);
                    else
                        hipLaunchKernelGGL(k_bs_select, dim3((uint32_t)std::min<size_t>((max_super * BS_JOBS + 255) / 256, 65536)), dim3(256), 0, stream,
                                           kp.kit, recs, sc->sorted, sc->bsplan, bsn, nsets, sc->bskeys, (uint32_t)need_sorted, sc->redo + 1, sc->redo);
                    mark("k_barcode_bitslice");
                    bs = sc->bsplan;
                    sc->bs_last = true;
                }
            }
            ensure_gather(nullptr);
            // a small batch (round 6): one launch, blockIdx.x % groups = the group (static_generated.inc: k_barcode_multi).  The twelve groups
            // of a kit-auto batch were twelve launches on four hardware queues -- nine of them find no tile, and the two or three
            // of the voted kit wait behind those.  The phase of the reference driver's 4000-read call stays what its longest units
            // take (250 us), but the side streams' joins go: a named 12-barcode kit at 2000 .. 64 000 reads 0.28 -> 0.23 ..
            // 0.40 -> 0.35 ms per scan, PBC096 at 8000 reads 0.45 -> 0.39 ms; from ~800 tiles on the two waves per SIMD the merged
            // kernel is compiled for cost more than the joins (tools/r06_multi_sizes.sh).
            bool bmulti = !leftover_beside && bs == nullptr && ng >= 2 && max_tiles <= (uint32_t)cus * 5u / 2u && !opt_on(QO_NO_BARCODE_MULTI);
            for (int i = 0; i < ng && bmulti; ++i) bmulti = hk.tpl[sgrp[i] >> 1].sets[sgrp[i] & 1].static_kernel < QCAT_JIT_BASE;
            if (bmulti) {
                StaticBarcodeMulti bm{};
                bm.common = StaticArgs{kp, sc->tilebuf, sc->tmeta, sc->jt, summary ? nullptr : sc->raws, bstride, 0, 0,
                                       opt_on(QO_ONE_QUEUE) ? 0 : 1, summary ? sc->part : nullptr, part_stride, nullptr};
                for (int i = 0; i < ng; ++i) {
                    bm.gidx[i] = (int16_t)sgrp[i]; bm.chunk_b[i] = (int16_t)unit_barcodes(sgrp[i]);
                    bm.kernel[i] = (int16_t)hk.tpl[sgrp[i] >> 1].sets[sgrp[i] & 1].static_kernel;
                }
                // (the merged kernel is compiled for two waves per SIMD: the widest chains' registers)
                bm.n = ng;
                launch_barcode_multi(dim3(std::min<uint32_t>(persist, (uint32_t)cus * 8u) * (uint32_t)ng), stream, bm);
            } else if (!leftover_beside) fork_join(sc, stream, ng, [&](int i, hipStream_t q) { static_launch(i, q, bs); });
            mark("k_barcode_static");
            if (summary) {
                const uint64_t sthreads = (uint64_t)max_tiles * 64;
                hipLaunchKernelGGL(k_barcode_select_summary, dim3((uint32_t)((sthreads + 255) / 256)), dim3(256), 0, stream,
                                   kp.kit, recs, sc->tmeta, sc->jt, sc->part, part_stride, nch_of, sc->redo + 1, sc->redo, bs, sc->slim ? sc->bcres : nullptr);
                hipLaunchKernelGGL(k_barcode_redo, dim3(1024), dim3(GEN_THREADS), 0, stream,
                                   kp, recs, sc->tilebuf, sc->tmeta, sc->jt, sc->redo + 1, sc->redo, sc->slim ? sc->bcres : nullptr,
                                   (bs && bs_direct) ? bs : nullptr, sc->win, sc->jobinfo, sc->sorted, nsets, sc->lazy ? sc->win2 : nullptr);
                if (opt_on(QO_DEBUG_BINS)) {         // (diagnostics: jobs per (group, length class))
                    JobTables hjt;
                    (void)hipStreamSynchronize(stream);
                    (void)hipMemcpy(&hjt, sc->jt, sizeof hjt, hipMemcpyDeviceToHost);
                    for (int b = 0; b < JOB_BINS; ++b)
                        if (hjt.hist[b]) fprintf(stderr, "[qcat] group %d class %d: %u jobs\n", b / JOB_CLASSES, b % JOB_CLASSES, hjt.hist[b]);
                }
                if (opt_on(QO_DEBUG_REDO)) {         // (diagnostics: how many alignments took the sequential rule)
                    uint32_t cnt = 0;
                    (void)hipStreamSynchronize(stream);
                    (void)hipMemcpy(&cnt, sc->redo, 4, hipMemcpyDeviceToHost);
                    fprintf(stderr, "[qcat] %u of %u alignments redone sequentially (best raw score exactly 0)\n", cnt, n_ends * (uint32_t)nsets);
                }
            }
        }
        ensure_gather(nullptr);
        if (!summary) {
            const uint64_t sthreads = (uint64_t)max_tiles * 64;
            hipLaunchKernelGGL(k_barcode_select, dim3((uint32_t)((sthreads + 255) / 256)), dim3(256), 0, stream,
                               kp.kit, recs, sc->tmeta, sc->jt, sc->raws, bstride, dbg_rows, stride, sc->slim ? sc->bcres : nullptr);
        }
    }
    mark("k_barcode_select");
    if ((e = hipGetLastError()) != hipSuccess) return fail("packed kernel launch", e);
    return jit_take_error();
}

template <class Mark>
static inline int packed_scan(hipStream_t stream, KitPtrs kp, const DevKit& hk, const uint8_t* win,
                              const int32_t* wlen, uint32_t n_ends, EndRec* recs, PackedScratch* sc,
                              int32_t* dbg_tpl, int16_t* dbg_rows, uint32_t stride, Mark mark,
                              bool adapter_only = false, int resume_kit_mask = -1) {
    // resume_kit_mask >= 0: the adapter launches of a previous adapter_only pass over the same windows are
    // still in sc->bests; merge them again for one kit's templates and carry on with the barcode phase
    int rc = sc->prepared ? 0 : packed_prepare(stream, hk, n_ends, sc);
    sc->prepared = false;
    if (rc) return rc;
    sc->fin_only = sc->slim && !adapter_only;
    if (resume_kit_mask >= 0) rc = packed_adapter_finish(stream, kp, win, wlen, n_ends, recs, sc, resume_kit_mask);
    else rc = packed_adapter(stream, kp, hk, win, wlen, n_ends, recs, sc, dbg_tpl, mark);
    if (rc) return rc;
    if (adapter_only) return 0;
    const int nsets = hk.mode == QCAT_MODE_DUAL ? 2 : 1;
    return packed_barcode(stream, kp, hk, n_ends, recs, sc, [&](uint32_t max_tiles, const BsPlan* taken, hipStream_t gq) {
        // (with a plan the workgroups enumerate the uncovered tiles after a prologue over the groups: fewer of them)
        hipLaunchKernelGGL(k_job_gather, dim3(std::min<uint32_t>(max_tiles, taken ? 2048u : 16384u)), dim3(GATHER_THREADS), 0, gq,
                           win, sc->jobinfo, sc->sorted, sc->jt, nsets, sc->tilebuf, sc->tmeta, taken, sc->lazy ? sc->win2 : nullptr, sc->wspec);
    }, dbg_rows, stride, mark);
}

}  // namespace qk

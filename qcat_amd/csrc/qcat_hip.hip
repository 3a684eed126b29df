// qcat_hip.hip -- libqcat_hip.so: C ABI (include/qcat_hip.h) + host orchestration.
// gfx950 only; built by __graft_entry__.build():
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared qcat_hip.hip -o libqcat_hip.so
//
// Per batch the library enqueues on the context's stream:
//   k_pack_windows -> [packed path: k_adapter_packed -> k_job_* -> k_barcode_packed |
//                      generic path: k_scan_generic |
//                      simple mode: k_simple_packed -> k_simple_select (or k_scan_simple)] -> k_finalize
// (see DESIGN.md for the data layout and the roofline of each kernel).
#include <hip/hip_runtime.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kit.h"
#include "synth.h"

#include "kit_prepare.inc"
#include "kernels_common.inc"
#include "kernels_generic.inc"
#include "kernels_tiny.inc"
#include "kernels_packed.inc"
#include "kernels_bitslice.inc"
#include "kernels_simple.inc"
#include "packed_host.inc"
#include "kernels_static.inc"
#include "kernels_middle.inc"
#include "kernels_partition.inc"
#include "kernels_fqtext.inc"
#include "kernels_tsvtext.inc"
#include "kernels_textstream.inc"
#include "kernels_eval.inc"
#include "kernels_filter.inc"
#include "static_registry.inc"
#include "pipeline.h"

using namespace qk;

// ------------------------------------------------------------------------------------------
// error handling
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int set_err(int rc, const std::string& m) { g_err = m; return rc; }

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return set_err(QCAT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
// ... for code with copies in flight to or from memory that dies with the function: the stream is drained before the return
#define HIPCHK_DRAIN(stream, expr)                                                           \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (void)hipStreamSynchronize(stream);                                              \
            return set_err(QCAT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
        }                                                                                    \
    } while (0)

// room for `need` elements in a scratch buffer of the context, or this layer's out-of-memory error
template <class T>
static int grow(DevBuf<T>& buf, size_t need) {
    const hipError_t e = buf.ensure(need);
    return e == hipSuccess ? 0 : set_err(QCAT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
}

extern "C" const char* qcat_last_error(void) { return g_err.c_str(); }
extern "C" int qcat_abi_version(void) { return QCAT_ABI_VERSION; }
extern "C" const char* qcat_backend(void) { return "hip"; }

// ------------------------------------------------------------------------------------------
// options (options.h): the table, its one import from the environment, the ABI around it
// ------------------------------------------------------------------------------------------
std::atomic<int64_t> g_qcat_opt[QO_COUNT];
static const char* const g_qcat_opt_name[QO_COUNT] = {
#define X(N, D) #N,
    QCAT_OPTION_LIST(X)
    QCAT_AB_OPTION_LIST(X)
#undef X
};
static const char* const g_qcat_opt_doc[QO_COUNT] = {
#define X(N, D) D,
    QCAT_OPTION_LIST(X)
    QCAT_AB_OPTION_LIST(X)
#undef X
};
static void qcat_options_from_env() {
    for (int i = 0; i < QO_COUNT; ++i) {
        const std::string env = std::string("QCAT_HIP_") + g_qcat_opt_name[i];
        const char* e = i < QO_SETTABLE ? getenv(env.c_str()) : nullptr;     // (the library's only look at QCAT_HIP_* switches: once, here;
                                                                             //  the A/B switches of dropped variants: -DQCAT_AB builds only)
        g_qcat_opt[i].store(e ? (*e ? (int64_t)atoll(e) : 1) : QOPT_UNSET, std::memory_order_relaxed);
    }
}
// (Round 6, measured and not kept: GPU_MAX_HW_QUEUES = 12 set from here at load -- the runtime's default of four hardware queues
// lets four of a small batch's side-by-side launches run at a time.  With twelve every cross-stream dependency of a call
// becomes a cross-QUEUE signal of 40-50 us where it was an in-queue barrier of 6: the 4000-read kit-auto call 0.81 -> 1.19 ms,
// config 2 0.99 -> 1.66 ms, the dual kit 3.84 -> 5.08 ms, config 3 31.9 -> 32.8 ms; profiles/r06_ab_hw_queues.txt.)
static struct QcatOptInit { QcatOptInit() { qcat_options_from_env(); } } g_qcat_opt_init;
static int qcat_opt_index(const char* name) {
    if (!name) return -1;
    if (strncmp(name, "QCAT_HIP_", 9) == 0) name += 9;
    for (int i = 0; i < QO_SETTABLE; ++i) if (strcmp(name, g_qcat_opt_name[i]) == 0) return i;
    return -1;
}
extern "C" int qcat_option_count(void) { return QO_SETTABLE; }
extern "C" const char* qcat_option_name(int i) { return i >= 0 && i < QO_SETTABLE ? g_qcat_opt_name[i] : nullptr; }
extern "C" const char* qcat_option_doc(int i) { return i >= 0 && i < QO_SETTABLE ? g_qcat_opt_doc[i] : nullptr; }
extern "C" void qcat_reset_options(void) { qcat_options_from_env(); qk::g_alloc_gen.fetch_add(1); }
extern "C" int qcat_set_option(const char* name, int64_t value) {
    const int i = qcat_opt_index(name);
    if (i < 0) return set_err(QCAT_ERR_ARG, std::string("qcat_set_option: no option named ") + (name ? name : "(null)"));
    if (value == QOPT_UNSET) return set_err(QCAT_ERR_ARG, "qcat_set_option: the value INT64_MIN means unset (qcat_clear_option)");
    g_qcat_opt[i].store(value, std::memory_order_relaxed);
    qk::g_alloc_gen.fetch_add(1);                   // (a captured graph holds the launches the old switches chose: dropped, like after a reallocation)
    return 0;
}
extern "C" int qcat_clear_option(const char* name) {
    const int i = qcat_opt_index(name);
    if (i < 0) return set_err(QCAT_ERR_ARG, std::string("qcat_clear_option: no option named ") + (name ? name : "(null)"));
    g_qcat_opt[i].store(QOPT_UNSET, std::memory_order_relaxed);
    qk::g_alloc_gen.fetch_add(1);
    return 0;
}
extern "C" int qcat_get_option(const char* name, int64_t* value) {          // returns 1 when the option is set (*value), 0 when it is not
    const int i = qcat_opt_index(name);
    if (i < 0) return set_err(QCAT_ERR_ARG, std::string("qcat_get_option: no option named ") + (name ? name : "(null)"));
    const int64_t v = g_qcat_opt[i].load(std::memory_order_relaxed);
    if (value) *value = v == QOPT_UNSET ? 0 : v;
    return v == QOPT_UNSET ? 0 : 1;
}
extern "C" int qcat_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// NUMA node of a device's PCI function (sysfs), -1 when unknown: the rank launcher (qcat_amd/parallel.py) keeps a
// rank's host threads -- the compaction pool of pipeline_core.h -- on the node its GPU hangs off
extern "C" int qcat_device_numa_node(int device) {
    char bdf[64] = {0};
    if (device < 0 || device >= qcat_device_count()) return -1;
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) return -1;
    for (char* q = bdf; *q; ++q) *q = (char)tolower((unsigned char)*q);
    const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
    FILE* fh = fopen(path.c_str(), "r");
    if (!fh) return -1;
    int node = -1;
    if (fscanf(fh, "%d", &node) != 1) node = -1;
    fclose(fh);
    return node;
}

// host threads a context may use for compaction / parsing: QCAT_HOST_THREADS (the rank launcher sets it to this
// rank's share of the container's CPU quota), else the CPUs of the affinity mask, at most 16
static inline unsigned host_threads() {
    const char* e = getenv("QCAT_HOST_THREADS");
    if (e && atoi(e) > 0) return (unsigned)std::min(atoi(e), 64);
    unsigned n = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = (unsigned)CPU_COUNT(&set);
    if (!n) n = std::max(1u, std::thread::hardware_concurrency());
    return std::min(n, 16u);
}

// ------------------------------------------------------------------------------------------
// kit
// ------------------------------------------------------------------------------------------
constexpr int MAX_DEVICES = 16;



struct KitOnDevice {
    bool ready = false;
    DevKit* kit = nullptr;
    uint8_t* codes = nullptr;
    int32_t* ids = nullptr;
    uint32_t* tables = nullptr;
    char* ascii = nullptr;
    // static-letter kernels compiled for this kit at run time (qcat_kit_attach_code)
    hipModule_t jit_module = nullptr;
    hipFunction_t jit_ad[MAX_T] = {}, jit_am[MAX_T] = {}, jit_bc[MAX_T * 2] = {}, jit_bs[MAX_T * 2] = {};
    hipFunction_t jit_abs[3][MAX_T] = {};          // bit-sliced adapter plans: qj_abs_<t>, qj_absm_<t>, qj_absw_<t>
};

struct qcat_kit {
    HostKit hk;
    std::mutex mu;
    KitOnDevice dev[MAX_DEVICES];
    std::vector<uint8_t> jit_code;                 // code object (gfx950) with qj_ad_<t>, qj_am_<t>, qj_bc_<t*2+s>, qj_bs_<t*2+s>
    bool jit_tpl[MAX_T] = {}, jit_grp[MAX_T * 2] = {}, jit_bsgrp[MAX_T * 2] = {};
    uint64_t serial = 0;                           // never reused: the key of a context's captured graph (ApiGraph)
};

// launch of a run-time generated kernel (kernel id >= QCAT_JIT_BASE): the scan in progress on this
// thread publishes its kit's function table here
static thread_local const KitOnDevice* g_jit = nullptr;

namespace qk {
static inline void jit_launch(int kind, int index, dim3 grid, hipStream_t stream, const void* args) {
    hipFunction_t f = nullptr;
    if (g_jit) f = kind == QCAT_JIT_ADAPTER ? g_jit->jit_ad[index] : (kind == QCAT_JIT_MIDDLE ? g_jit->jit_am[index] :
                   (kind == QCAT_JIT_BITSLICE ? g_jit->jit_bs[index] :
                    (kind >= QCAT_JIT_ABS2 && kind <= QCAT_JIT_ABSW ? g_jit->jit_abs[kind - QCAT_JIT_ABS2][index] : g_jit->jit_bc[index])));
    if (!f) { g_packed_err = "run-time generated kernel missing from the kit's code object"; g_jit_rc = QCAT_ERR_DEVICE; return; }
    void* params[1] = {const_cast<void*>(args)};
    const unsigned threads = kind == QCAT_JIT_BITSLICE ? BS_WAVES * 64 : (kind == QCAT_JIT_ABS2 ? 128u : (kind == QCAT_JIT_ABSM || kind == QCAT_JIT_ABSW ? 256u : PK_WAVES * 64));
    const hipError_t e = hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, threads, 1, 1, 0, stream, params, nullptr);
    if (e != hipSuccess) { g_packed_err = std::string("launch of a run-time generated kernel: ") + hipGetErrorString(e); g_jit_rc = QCAT_ERR_DEVICE; }
}
}  // namespace qk

extern "C" int qcat_kit_create(const qcat_kit_desc* desc, qcat_kit** out) {
    if (!out) return set_err(QCAT_ERR_ARG, "qcat_kit_create: null output pointer");
    qcat_kit* k = new qcat_kit();
    std::string err;
    int rc = kit_prepare(desc, &k->hk, &err);
    if (rc) { delete k; return set_err(rc, err); }
    static_match(&k->hk);
    static std::atomic<uint64_t> next_serial{1};
    k->serial = next_serial.fetch_add(1);
    *out = k;
    return 0;
}

extern "C" int qcat_kit_attach_code_quads(qcat_kit* k, const void* code, uint64_t size,
                                          const int32_t* template_flags, const int32_t* group_flags,
                                          const int32_t* pair_offsets, const int32_t* pair_entries,
                                          const int32_t* quad_offsets, const int32_t* quad_entries);

extern "C" int qcat_kit_attach_code(qcat_kit* k, const void* code, uint64_t size,
                                    const int32_t* template_flags, const int32_t* group_flags,
                                    const int32_t* pair_offsets, const int32_t* pair_entries) {
    return qcat_kit_attach_code_quads(k, code, size, template_flags, group_flags, pair_offsets, pair_entries, nullptr, nullptr);
}

extern "C" int qcat_kit_attach_code_quads(qcat_kit* k, const void* code, uint64_t size,
                                          const int32_t* template_flags, const int32_t* group_flags,
                                          const int32_t* pair_offsets, const int32_t* pair_entries,
                                          const int32_t* quad_offsets, const int32_t* quad_entries) {
    if (quad_offsets && !quad_entries) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: quad offsets without quad entries");
    if (!k || !code || !size || !template_flags || !group_flags || !pair_offsets || !pair_entries)
        return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: null argument");
    std::lock_guard<std::mutex> lock(k->mu);
    for (int d = 0; d < MAX_DEVICES; ++d)
        if (k->dev[d].ready) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: the kit is already in use on a device");
    if (!k->jit_code.empty()) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: code already attached");
    HostKit& h = k->hk;
    DevKit& d = h.dk;
    const int nsets = d.mode == QCAT_MODE_DUAL ? 2 : 1;
    // validate the pair lists BEFORE anything is bound: the barcode kernel writes its raw scores at the
    // kit barcode indices named here, and k_barcode_select reads one score per barcode of the set
    for (int g = 0; g < 2 * MAX_T; ++g)
        if (pair_offsets[g] < 0 || pair_offsets[g + 1] < pair_offsets[g] ||
            (quad_offsets && (quad_offsets[g] < 0 || quad_offsets[g + 1] < quad_offsets[g])))
            return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: pair / quad offsets must be non-negative and non-decreasing");
    for (int t = 0; t < d.nt; ++t)
        for (int s = 0; s < nsets; ++s) {
            const DevSet& q = d.tpl[t].sets[s];
            if (!group_flags[t * 2 + s] || !d.barcode_f16 || q.static_kernel >= 0 || q.n <= 0) continue;
            const int32_t* ent = pair_entries + (size_t)pair_offsets[t * 2 + s] * 3;
            const int np = pair_offsets[t * 2 + s + 1] - pair_offsets[t * 2 + s];
            const int nqd = quad_offsets ? quad_offsets[t * 2 + s + 1] - quad_offsets[t * 2 + s] : 0;
            if (np <= 0 && nqd <= 0) continue;
            if (np > q.n || nqd > q.n) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: more target pairs than barcodes in a set");
            std::vector<char> seen((size_t)q.n, 0);
            int covered = 0;
            for (int i = 0; i < nqd; ++i) {
                const int32_t* qe = quad_entries + ((size_t)quad_offsets[t * 2 + s] + i) * 5;
                if (qe[0] < 0) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: negative quad case");
                for (int m2 = 1; m2 <= 4; ++m2) {
                    const int32_t b = qe[m2];
                    if (b < 0 || b >= q.n) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: barcode index outside its set");
                    if (seen[(size_t)b]) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: a barcode appears in two target pairs");
                    seen[(size_t)b] = 1; ++covered;
                }
            }
            for (int i = 0; i < np; ++i) {
                if (ent[i * 3] < 0) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: negative pair case");
                for (int half = 1; half <= 2; ++half) {
                    const int32_t b = ent[i * 3 + half];
                    if (b == -1 && half == 2) continue;                      // an unpaired target
                    if (b < 0 || b >= q.n) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: barcode index outside its set");
                    if (seen[(size_t)b]) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: a barcode appears in two target pairs");
                    seen[(size_t)b] = 1; ++covered;
                }
            }
            if (covered != q.n) return set_err(QCAT_ERR_ARG, "qcat_kit_attach_code: the target pairs do not cover every barcode of the set");
        }
    k->jit_code.assign((const uint8_t*)code, (const uint8_t*)code + size);
    for (int t = 0; t < d.nt; ++t) {
        if ((template_flags[t] & 1) && d.adapter_f16 && d.tpl[t].static_kernel < 0) {
            d.tpl[t].static_kernel = QCAT_JIT_BASE + t; k->jit_tpl[t] = true;
            // bits 1..3 of a template flag: the code object also holds bit-sliced adapter plans of this template (qj_abs_<t>
            // two stages, qj_absm_<t> four stages, qj_absw_<t> four wide stages); only kits the path takes at all use them
            if (d.abs_ok) d.tpl[t].abs_jit = (template_flags[t] >> 1) & 7;
        }
        for (int s = 0; s < nsets; ++s) {
            DevSet& q = d.tpl[t].sets[s];
            if (!group_flags[t * 2 + s] || !d.barcode_f16 || q.static_kernel >= 0 || q.n <= 0) continue;
            const int32_t* ent = pair_entries + (size_t)pair_offsets[t * 2 + s] * 3;
            const int np = pair_offsets[t * 2 + s + 1] - pair_offsets[t * 2 + s];
            const int nqd = quad_offsets ? quad_offsets[t * 2 + s + 1] - quad_offsets[t * 2 + s] : 0;
            if (np <= 0 && nqd <= 0) continue;
            q.static_kernel = QCAT_JIT_BASE + t * 2 + s;
            q.n_pairs = np;
            q.case_off = (int32_t)h.ids.size();          // (pair case, barcode of half 0, barcode of half 1) per pair
            h.ids.insert(h.ids.end(), ent, ent + (size_t)np * 3);
            q.n_quads = nqd;
            q.quad_off = (int32_t)h.ids.size();          // (quad case, barcodes a, b, c, d) per quad
            if (nqd > 0) {
                const int32_t* qe = quad_entries + (size_t)quad_offsets[t * 2 + s] * 5;
                h.ids.insert(h.ids.end(), qe, qe + (size_t)nqd * 5);
            }
            k->jit_grp[t * 2 + s] = true;
        }
        // bit 1 of a group flag: the code object also holds qj_bs_<group>, the bit-sliced kernel with this set's
        // letters compiled in (case = barcode index); only sets the bit-sliced path takes at all can use it
        for (int s = 0; s < nsets; ++s) {
            DevSet& q = d.tpl[t].sets[s];
            if (!(group_flags[t * 2 + s] & 2) || q.bs_off < 0 || q.bs_kernel >= 0 || q.n <= 0) continue;
            q.bs_kernel = QCAT_JIT_BASE + t * 2 + s;
            q.bs_case_off = (int32_t)h.ids.size();
            for (int b = 0; b < q.n; ++b) h.ids.push_back(b);
            k->jit_bsgrp[t * 2 + s] = true;
        }
    }
    return 0;
}

extern "C" int qcat_kit_describe(const qcat_kit* k, qcat_kit_info* out) {
    if (!k || !out) return set_err(QCAT_ERR_ARG, "qcat_kit_describe: null argument");
    const DevKit& d = k->hk.dk;
    memset(out, 0, sizeof *out);
    out->packed = ((d.fast_ok && packed_supported(d)) || k->hk.simple_packed) ? 1 : 0;
    out->barcode_f16 = d.barcode_f16; out->adapter_f16 = d.adapter_f16;
    out->n_templates = d.nt;
    const int nsets = d.mode == QCAT_MODE_DUAL ? 2 : 1;
    for (int t = 0; t < d.nt; ++t) {
        if (d.tpl[t].static_kernel >= 0) out->n_static_templates++;
        if (d.abs_ok) {
            const int forms = abs_forms(d, t);
            out->bitslice_templates += (forms & 1 ? 1 : 0) + (forms & 2 ? 0x100 : 0) + (forms & 4 ? 0x10000 : 0);
        }
        for (int s = 0; s < nsets; ++s) {
            out->n_groups++;
            if (d.tpl[t].sets[s].static_kernel >= 0) out->n_static_groups++;
            if (d.bs_ok && d.tpl[t].sets[s].bs_off >= 0) out->bitslice_groups += d.tpl[t].sets[s].bs_kernel >= 0 ? 0x10001 : 1;
        }
    }
    return 0;
}

static void kit_device_release(KitOnDevice& kd);

extern "C" void qcat_kit_destroy(qcat_kit* k) {
    if (!k) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < MAX_DEVICES; ++d) {
        KitOnDevice& kd = k->dev[d];
        if (!kd.ready) continue;
        (void)hipSetDevice(d);
        kit_device_release(kd);
    }
    (void)hipSetDevice(cur);
    delete k;
}

extern "C" int qcat_kit_count_buckets(const qcat_kit* k) { return k ? k->hk.dk.n_buckets : QCAT_ERR_ARG; }

static void kit_device_release(KitOnDevice& kd) {
    (void)hipFree(kd.kit); (void)hipFree(kd.codes); (void)hipFree(kd.ids); (void)hipFree(kd.tables); (void)hipFree(kd.ascii);
    if (kd.jit_module) (void)hipModuleUnload(kd.jit_module);
    kd = KitOnDevice();
}

static int kit_upload(qcat_kit* k, KitOnDevice& kd) {
    const HostKit& h = k->hk;
    HIPCHK(hipMalloc((void**)&kd.kit, sizeof(DevKit)));
    HIPCHK(hipMalloc((void**)&kd.codes, h.codes.size()));
    HIPCHK(hipMalloc((void**)&kd.ids, h.ids.size() * 4));
    HIPCHK(hipMalloc((void**)&kd.tables, h.tables.size() * 4));
    HIPCHK(hipMalloc((void**)&kd.ascii, std::max<size_t>(1, h.ascii.size())));
    HIPCHK(hipMemcpy(kd.kit, &h.dk, sizeof(DevKit), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(kd.codes, h.codes.data(), h.codes.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(kd.ids, h.ids.data(), h.ids.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(kd.tables, h.tables.data(), h.tables.size() * 4, hipMemcpyHostToDevice));
    if (!h.ascii.empty()) HIPCHK(hipMemcpy(kd.ascii, h.ascii.data(), h.ascii.size(), hipMemcpyHostToDevice));
    if (!k->jit_code.empty()) {
        HIPCHK(hipModuleLoadData(&kd.jit_module, k->jit_code.data()));
        char name[32];
        for (int t = 0; t < h.dk.nt; ++t) {
            if (k->jit_tpl[t]) {
                snprintf(name, sizeof name, "qj_ad_%d", t);
                HIPCHK(hipModuleGetFunction(&kd.jit_ad[t], kd.jit_module, name));
                snprintf(name, sizeof name, "qj_am_%d", t);
                HIPCHK(hipModuleGetFunction(&kd.jit_am[t], kd.jit_module, name));
                static const char* const abs_names[3] = {"qj_abs_%d", "qj_absm_%d", "qj_absw_%d"};
                for (int f = 0; f < 3; ++f) if (h.dk.tpl[t].abs_jit & (1 << f)) {
                    snprintf(name, sizeof name, abs_names[f], t);
                    HIPCHK(hipModuleGetFunction(&kd.jit_abs[f][t], kd.jit_module, name));
                }
            }
            for (int s2 = 0; s2 < 2; ++s2) if (k->jit_grp[t * 2 + s2]) {
                snprintf(name, sizeof name, "qj_bc_%d", t * 2 + s2);
                HIPCHK(hipModuleGetFunction(&kd.jit_bc[t * 2 + s2], kd.jit_module, name));
            }
            for (int s2 = 0; s2 < 2; ++s2) if (k->jit_bsgrp[t * 2 + s2]) {
                snprintf(name, sizeof name, "qj_bs_%d", t * 2 + s2);
                HIPCHK(hipModuleGetFunction(&kd.jit_bs[t * 2 + s2], kd.jit_module, name));
            }
        }
    }
    return 0;
}

static int kit_on_device(qcat_kit* k, int device, KitOnDevice** out) {
    if (device < 0 || device >= MAX_DEVICES) return set_err(QCAT_ERR_ARG, "device index out of range");
    std::lock_guard<std::mutex> lock(k->mu);
    KitOnDevice& kd = k->dev[device];
    if (!kd.ready) {
        const int rc = kit_upload(k, kd);
        if (rc) { kit_device_release(kd); return rc; }     // a failed upload leaves nothing behind: a retry starts clean
        kd.ready = true;
    }
    *out = &kd;
    return 0;
}

// ------------------------------------------------------------------------------------------
// batch (reads resident in device memory)
// ------------------------------------------------------------------------------------------
#include "batch.h"

// the interior scan of --detect-middle on a resident batch: its scratch (MiddleScratch) and launch sequence
#include "middle_host.inc"

// the device work of a host-buffer call as a captured graph: ApiGraph, api_graph_run
#include "api_graph.inc"

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
constexpr int MAX_TIMED = 12;

struct qcat_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // per-scan buffers (grown on demand; every buffer owns its memory and knows its capacity: dev_buf.h)
    DevBuf<uint8_t> win;
    DevBuf<int32_t> wlen;
    DevBuf<uint8_t> wspec;                              // per read end: the window holds a letter outside A, C, G, T, N
    DevBuf<uint32_t> win2;                              // the windows at two bits per code (plain windows: the bit-sliced kernels' input)
    bool win2_valid = false;                            // ... written by the pack kernel of the windows in `win`
    DevBuf<EndRec> recs;
    DevBuf<qcat_result> results;
    DevBuf<unsigned long long> counts;
    // pinned staging of window-only uploads (qcat_scan_batch): compact bases, offsets, real lengths
    PinBuf<uint8_t> pin_bases;
    PinBuf<uint64_t> pin_offsets; PinBuf<uint32_t> pin_len;
    PinBuf<uint8_t> pin_ret;                                // what a host-buffer call brings back (records, votes, counts): copies into PINNED
                                                            // memory are one DMA each; into the caller's pageable arrays the runtime stages
                                                            // every one through a copy kernel and a host memcpy (round 6: five of them were
                                                            // 100 us of a 4000-read kit-auto call)
    HostPipeline* pipe = nullptr;                  // chunked host-buffer scans (pipeline.h, pipeline_host.inc), created on first use
    std::vector<qcat_ctx*> helpers;                // contexts of the kit-auto file loop's other workers (fastq_host.inc), created on first use
    PackedScratch packed;
    MiddleScratch middle;                          // the interior scan of --detect-middle (middle_host.inc)
    uint32_t last_n_reads = 0;
    int last_buckets = 0;
    const qcat_kit* last_kit = nullptr;            // the kit of the scan whose records `results` holds (null: none, or a vote only)
    BatchScratch batch;                            // qcat_batch_partition, qcat_batch_from_device and the barcode filter (batch.h)
    // qcat_scan_resident_batches: the first read of the chunk a scan writes its records for (0 outside that call), the voted
    // kit slot of every batch of the latest kit-auto scan and their number (-1: the latest scan voted for nothing)
    uint32_t res_first = 0;
    DevBuf<int32_t> kit_slots;
    int64_t auto_batches = -1;
    // device staging of the host-buffer calls (qcat_scan_batch / _auto / _debug, qcat_detect_kit): grown on demand and
    // reused -- a 4000-read batch of the reference driver's call shape spent a third of its call in six hipMalloc / hipFree
    DevBuf<uint8_t> hb_bases;
    DevBuf<uint64_t> hb_offsets; DevBuf<uint32_t> hb_len;
    DevBuf<uint8_t> vote_buf;                      // the block of a kit vote (vote_host.inc: VoteBuf)
    // the device work of a host-buffer call as a captured graph (api_graph.inc): kit-auto calls (scan_batch_auto_impl); calls
    // with a named kit (qcat_scan_batch, round 5)
    ApiGraph api_graph, scan_graph;
    // the handful-of-reads path (kernels_tiny.inc): per read end the templates' (raw, end) and the barcodes' raw scores
    DevBuf<int32_t> tiny_tpl; DevBuf<int16_t> tiny_sc;
    uint32_t last_tiny_ends = 0;                   // read ends the last scan put on that path (0: another path)
    uint32_t last_fused_ends = 0;                  // read ends whose windows and letter planes the last scan made in one kernel (k_pack_planes)
    DevBuf<int32_t> tiny_simple;                   // simple kits on qcat_scan_sequences: (raw, end_query) per (sequence, barcode) of a piece
    // simple mode on the packed kernels (kernels_simple.inc): one (key, end) per (work unit, read end); the read ends whose best raw
    // score is 0 ([0]: their count); debug scans with rows: (raw, end) of every barcode
    DevBuf<uint2> simple_part;
    DevBuf<uint32_t> simple_redo;
    DevBuf<uint32_t> simple_full;
    // debug buffers
    DevBuf<int32_t> dbg_tpl;
    DevBuf<int16_t> dbg_rows;
    // timing: a ring of event sets, one per scan, so that timed scans need no host synchronisation
    // between them; qcat_ctx_last_timing drains the ring
    bool timing = false;
    int force_generic = 0;
    static constexpr int TIME_RING = 64;
    int n_timed = 0;                               // marks of the scan being recorded
    int ring_used = 0;                             // recorded scans not yet drained (<= TIME_RING)
    int ring_marks[TIME_RING];
    const char* timed_name[TIME_RING][MAX_TIMED];
    hipEvent_t evr[TIME_RING][MAX_TIMED + 1];
    hipEvent_t* ev = nullptr;                      // event set of the scan being recorded
    bool ev_ready = false;
};

extern "C" int qcat_ctx_create(int device, qcat_ctx** out) {
    if (!out) return set_err(QCAT_ERR_ARG, "qcat_ctx_create: null output pointer");
    int n = qcat_device_count();
    if (n <= 0) return set_err(QCAT_ERR_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n || device >= MAX_DEVICES) return set_err(QCAT_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    qcat_ctx* c = new qcat_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return set_err(QCAT_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    const QOptVal fg = qopt_get(QO_FORCE_GENERIC);
    c->force_generic = (fg && fg.v == 1) ? 1 : 0;
    *out = c;
    return 0;
}

extern "C" void qcat_ctx_destroy(qcat_ctx* c) {
    if (!c) return;
    for (qcat_ctx* h : c->helpers) qcat_ctx_destroy(h);
    c->helpers.clear();
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->api_graph.exec) (void)hipGraphExecDestroy(c->api_graph.exec);
    if (c->scan_graph.exec) (void)hipGraphExecDestroy(c->scan_graph.exec);
    packed_scratch_free(&c->packed);
    middle_scratch_free(&c->middle);
    pipeline_free(c->pipe);
    if (c->ev_ready) for (int r = 0; r < qcat_ctx::TIME_RING; ++r) for (int i = 0; i <= MAX_TIMED; ++i) (void)hipEventDestroy(c->evr[r][i]);
    (void)hipStreamDestroy(c->stream);
    delete c;                                      // (every scratch buffer frees itself: dev_buf.h)
}

extern "C" int qcat_ctx_set_timing(qcat_ctx* c, int enabled) {
    if (!c) return set_err(QCAT_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    if (enabled && !c->ev_ready) {
        for (int r = 0; r < qcat_ctx::TIME_RING; ++r) for (int i = 0; i <= MAX_TIMED; ++i) HIPCHK(hipEventCreate(&c->evr[r][i]));
        c->ev_ready = true;
    }
    c->timing = enabled != 0;
    c->ring_used = 0; c->n_timed = 0; c->ev = nullptr;
    return 0;
}

// a timed call begins: the next event set of the ring (the caller records ev[0] where its device work starts)
static void timing_slot(qcat_ctx* c) {
    c->n_timed = 0;
    c->ev = nullptr;
    if (c->timing) {                               // next slot of the ring; a full ring restarts (oldest scans dropped)
        if (c->ring_used >= qcat_ctx::TIME_RING) c->ring_used = 0;
        c->ring_marks[c->ring_used] = 0;
        c->ev = c->evr[c->ring_used++];
    }
}

static void mark(qcat_ctx* c, const char* name) {
    if (!c->timing || !c->ev || c->n_timed >= MAX_TIMED) return;
    c->timed_name[c->ring_used - 1][c->n_timed] = name;
    (void)hipEventRecord(c->ev[c->n_timed + 1], c->stream);
    c->n_timed++;
    c->ring_marks[c->ring_used - 1] = c->n_timed;
}

// barcodes of the kit's largest set; at least 1 as the stride of the one-wave kernels' score arrays
static int max_set_barcodes(const DevKit& hk, int at_least = 1) {
    int maxb = at_least;
    for (int t = 0; t < hk.nt; ++t) for (int s = 0; s < 2; ++s) maxb = std::max(maxb, (int)hk.tpl[t].sets[s].n);
    return maxb;
}

// scratch of the one-wave-per-alignment kernels (kernels_tiny.inc) for `n_ends` queries of a kit whose largest set has `maxb` barcodes
static int tiny_buffers(qcat_ctx* c, size_t n_ends, int maxb) {
    HIPCHK(c->tiny_sc.ensure(std::max<size_t>(n_ends * 2 * (size_t)maxb, (size_t)TINY_MAX_WAVES * 2)));
    HIPCHK(c->tiny_tpl.ensure(std::max<size_t>(n_ends, 4096) * MAX_T * 2));
    return 0;
}

// simple mode on the packed end-tracking kernels (kernels_simple.inc): work units of (tile of 128 read ends, chunk of the list)
template <int W>
static void launch_simple_packed(hipStream_t st, KitPtrs kp, const uint8_t* win, const int32_t* wlen, uint32_t n_ends, uint32_t n_tiles,
                                 int nch, uint2* part, uint32_t* full) {
    hipLaunchKernelGGL(k_simple_packed<W>, dim3(n_tiles * (uint32_t)nch), dim3(64), 0, st, kp, win, wlen, n_ends, n_tiles, nch, part, full);
}

static int simple_packed_scan(qcat_ctx* c, KitPtrs kp, const DevKit& hk, size_t n_ends, int16_t* dbg_rows, uint32_t row_stride) {
    const DevSet& bs = hk.tpl[0].sets[0];
    const uint32_t n_tiles = (uint32_t)((n_ends + PK_TILE - 1) / PK_TILE);
    // units: enough of them to fill the chip's wave slots a few times over while the batch is small (a chunk re-stages its
    // tile's windows, so a big batch takes the list in one piece); `part` holds at most max(tiles, 2 * target) units
    const uint32_t target = 8192;
    int nch = (int)std::min<uint32_t>((target + n_tiles - 1) / n_tiles, (uint32_t)bs.n);
    if (dbg_rows) nch = std::min(nch, 8);
    const int per = (bs.n + nch - 1) / nch;
    nch = (bs.n + per - 1) / per;                   // (every chunk holds a barcode)
    int rc;
    if (dbg_rows) { if ((rc = grow(c->simple_full, (size_t)n_tiles * bs.n * 128))) return rc; }
    else {
        if ((rc = grow(c->simple_part, (size_t)n_tiles * nch * 128))) return rc;
        if ((rc = grow(c->simple_redo, n_ends + 1))) return rc;
        HIPCHK(hipMemsetAsync(c->simple_redo, 0, sizeof(uint32_t), c->stream));
    }
    uint32_t* full = dbg_rows ? c->simple_full : nullptr;
    switch (bs.width) {
        case 24: launch_simple_packed<24>(c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, n_tiles, nch, c->simple_part, full); break;
        case 32: launch_simple_packed<32>(c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, n_tiles, nch, c->simple_part, full); break;
        case 40: launch_simple_packed<40>(c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, n_tiles, nch, c->simple_part, full); break;
        case 48: launch_simple_packed<48>(c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, n_tiles, nch, c->simple_part, full); break;
        case 56: launch_simple_packed<56>(c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, n_tiles, nch, c->simple_part, full); break;
        case 64: launch_simple_packed<64>(c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, n_tiles, nch, c->simple_part, full); break;
        default: return set_err(QCAT_ERR_UNSUPPORTED, "simple kit without a width class on the packed path");
    }
    const uint32_t sblocks = (uint32_t)((n_ends + 255) / 256);
    if (dbg_rows) {
        hipLaunchKernelGGL(k_simple_select_rows, dim3(sblocks), dim3(256), 0, c->stream, kp.kit, c->wlen, (uint32_t)n_ends, c->simple_full,
                           c->recs, dbg_rows, row_stride);
    } else {
        hipLaunchKernelGGL(k_simple_select, dim3(sblocks), dim3(256), 0, c->stream, c->wlen, (uint32_t)n_ends, nch, c->simple_part, c->recs, c->simple_redo);
        const uint32_t rblocks = (uint32_t)std::min<size_t>((n_ends + GEN_THREADS - 1) / GEN_THREADS, 1024);
        hipLaunchKernelGGL(k_simple_redo, dim3(rblocks), dim3(GEN_THREADS), 0, c->stream, kp, c->win, c->wlen, c->recs, c->simple_redo);
    }
    return 0;
}

// the kind of pass a scan of a resident batch is: plain, a debug scan, the vote pass of kit auto or its resumed second pass;
// a later chunk of a pipelined call keeps the count vector
struct ScanPass {
    bool debug_scan = false;            // every end's template scores into dbg_tpl and -- row_stride > 0 -- every barcode's raw score into dbg_rows
    uint32_t row_stride = 0;
    bool adapter_only = false;          // the adapter templates of every kit only: the records the vote reads, no results
    int resume_kit_mask = -1;           // >= 0: the adapter alignments of the vote pass are still on the device; their merge for these kit
                                        // slots (RESUME_KIT_ON_DEVICE: the slot k_pick_kit chose), the barcode phase and the finalisation
    bool keep_counts = false;           // the count vector goes on from the scan before
    bool defer_counts = false;          // the records are not final yet (--filter-barcodes on the device): nothing is counted, the caller runs k_count
    static ScanPass plain() { return ScanPass{}; }
    static ScanPass debug(uint32_t row_stride) { ScanPass p; p.debug_scan = true; p.row_stride = row_stride; return p; }
    static ScanPass vote() { ScanPass p; p.adapter_only = true; return p; }
    static ScanPass resume(int kit_mask) { ScanPass p; p.resume_kit_mask = kit_mask; return p; }
    ScanPass keeping_counts(bool keep = true) const { ScanPass p = *this; p.keep_counts = keep; return p; }
    ScanPass deferring_counts(bool defer = true) const { ScanPass p = *this; p.defer_counts = defer; return p; }
    bool resumed() const { return resume_kit_mask >= 0; }
};

// the kernels a scan takes, decided once from the kit, the batch size, the pass and the options (nothing here touches the
// context's state or the stream)
struct ScanPath {
    bool packed_kit;                    // the kit fits the packed kernels
    bool use_packed;                    // ... and the read ends of this batch take them (not the handful-of-reads path)
    bool packed_pairs;                  // ... through packed_scan -- adapter templates and barcode sets, not simple mode: job tables, lazy windows, slim results
    bool tiny; int tiny_maxb;           // one wave per alignment (kernels_tiny.inc); the stride of its score arrays
    bool lazy;                          // byte windows for the flagged ends only
    bool slim;                          // packed barcode results instead of the records
    bool abs_planes;                    // a scan from the reads whose adapter phase runs bit-sliced: flag block and letter planes ahead of it
    bool fused_front;                   // ... its windows and planes from one kernel (k_pack_planes)
    bool middle_packed;                 // the interiors of --detect-middle on the packed kernels (middle_host.inc)
};

static ScanPath scan_choose_path(bool force_generic, const DevKit& hk, size_t n_ends, const ScanPass& pass) {
    ScanPath p{};
    p.packed_kit = hk.fast_ok && !force_generic && packed_supported(hk);
    // a handful of read ends (detect_barcode on one read, a few reads of a test): one wave per alignment, kernels_tiny.inc
    // (QCAT_HIP_TINY_MAX_ENDS: the largest batch that goes there, 0: none; QCAT_HIP_NO_TINY=1)
    // the path pays while its waves -- one per (read end, template) plus one per (read end, set, barcode) -- fit the chip a few
    // times over: up to TINY_MAX_WAVES of them (tools/tiny_crossover.py: PBC096 wins to ~180 reads, NBD104 to ~700)
    const QOptVal tiny_env = qopt_get(QO_TINY_MAX_ENDS);
    p.tiny_maxb = max_set_barcodes(hk);
    const uint64_t tiny_waves = n_ends * (uint64_t)(hk.nt + p.tiny_maxb * (hk.mode == QCAT_MODE_DUAL ? 2 : 1));
    const bool tiny_fits = tiny_env ? n_ends <= (uint64_t)std::max<long long>(0, atoll(tiny_env)) : tiny_waves <= (uint64_t)TINY_MAX_WAVES;
    p.tiny = n_ends > 0 && n_ends <= 4096 && tiny_fits && !opt_on(QO_NO_TINY) && hk.mode != QCAT_MODE_SIMPLE && !pass.resumed() &&
             !pass.adapter_only && !force_generic && hk.gap_open == hk.gap_extend;
    p.use_packed = p.packed_kit && !p.tiny;        // (no job tables, no lazy windows: the tiny kernels read byte windows)
    p.packed_pairs = p.use_packed && hk.mode != QCAT_MODE_SIMPLE;
    // lazy byte windows (round 4): a kit whose every template runs a generated kernel reads plain windows at two
    // bits per code everywhere (dev_window16), so the byte windows -- 3.3 of the pack kernel's 4.1 GB of stores per
    // 10 M reads -- are written for the flagged ends only (k_expand_special; QCAT_HIP_EAGER_BYTES=1: all of them)
    p.lazy = p.packed_pairs && hk.adapter_f16 && !opt_on(QO_NO_STATIC) && !opt_on(QO_NO_STATIC_ADAPTER) && !opt_on(QO_EAGER_BYTES);
    for (int t = 0; t < hk.nt && p.lazy; ++t) p.lazy = hk.tpl[t].static_kernel >= 0;
    // packed barcode results (kernels_bitslice.inc: k_bs_select_ordered) instead of 8 bytes scattered into every record;
    // debug scans keep the records complete for the traces
    p.slim = p.packed_pairs && !pass.debug_scan && !opt_on(QO_NO_SLIM);
    // a batch the bit-sliced adapter kernels will take: its windows and their letter planes in one pass (kernels_abs.inc:
    // k_pack_planes), so that the windows are not read back from memory.  QCAT_HIP_PACK_PLANES=0 (A/B builds):
    // k_pack_windows here and k_abs_planes in the adapter phase, the route of every other batch and of the vote pass of kit auto
    p.abs_planes = p.packed_pairs && !pass.resumed() && packed_abs_wanted(hk, (uint32_t)n_ends, true);
    p.fused_front = p.abs_planes && !pass.adapter_only && opt_val(QO_PACK_PLANES, 1) != 0;
    p.middle_packed = hk.scan_middle && !pass.adapter_only && p.packed_kit && middle_packed_ok(hk);
    return p;
}

// step 1, size the buffers: room for n reads / n_ends read ends in the context's scan buffers; a debug scan's buffers start cleared
static int scan_size_buffers(qcat_ctx* c, const DevKit& hk, uint32_t n, size_t n_ends, const ScanPass& pass) {
    int rc;
    if ((rc = grow(c->win, n_ends * WIN_STRIDE + 512))) return rc;    // + slack: k_job_gather reads whole dwords, k_bs_barcode 84 bytes from any region start
    if ((rc = grow(c->wlen, n_ends))) return rc;
    if ((rc = grow(c->wspec, n_ends))) return rc;
    // + slack: readers take whole dwords past a region's end -- and, round 5, one dword in FRONT of the first window (a front-padded
    // unit of the bit-sliced barcode kernels fetches from up to BS_PAD_ROWS bases before a region): the windows start WIN2_FRONT words in
    if ((rc = grow(c->win2, n_ends * WIN2_WORDS + 64 + WIN2_FRONT))) return rc;
    if ((rc = grow(c->recs, n_ends))) return rc;
    if ((rc = grow(c->results, (size_t)n))) return rc;
    if ((rc = grow(c->counts, (size_t)hk.n_buckets))) return rc;
    if (pass.debug_scan) {
        const uint32_t row_stride = pass.row_stride;
        if ((rc = grow(c->dbg_tpl, n_ends * 2 * MAX_T))) return rc;
        if (row_stride && (rc = grow(c->dbg_rows, n_ends * 2 * row_stride))) return rc;
        HIPCHK(hipMemsetAsync(c->dbg_tpl, 0, n_ends * 2 * MAX_T * 4, c->stream));
        if (row_stride) HIPCHK(hipMemsetD16Async((hipDeviceptr_t)c->dbg_rows, (unsigned short)0x8000, n_ends * 2 * row_stride, c->stream));
    }
    return 0;
}

// step 3, the front end of a scan that starts from the reads: letter flags, windows at one byte and at two bits per code.
// With the job tables and the adapter tile flags sized here instead of after the pack kernel, their fills leave with the
// count vector's and the letter flags' as ONE launch in front of it (the caller's FillScope)
static int scan_front_end(qcat_ctx* c, const DevKit& hk, const qcat_batch* b, int ends, size_t n_ends, const ScanPath& path) {
    int rc;
    const uint32_t n = b->n_reads;
    HIPCHK(packed_fill(c->wspec, 0, n_ends, c->stream));
    c->packed.abs_ready = 0;
    if (g_fill_defer && path.packed_pairs) {
        if ((rc = packed_prepare(c->stream, hk, (uint32_t)n_ends, &c->packed))) return set_err(rc, packed_last_error());     // (sizes the slim buffers)
        c->packed.prepared = true;
        if (path.abs_planes && (rc = packed_abs_buffers(c->stream, hk, (uint32_t)n_ends, &c->packed))) return set_err(rc, packed_last_error());
    }
    HIPCHK(packed_fill_flush(c->stream));
    c->win2_valid = true;
    c->packed.lazy = path.lazy;
    const int lazy_bytes = path.lazy ? 1 : 0;
    if (path.fused_front) {
        if (c->packed.abs_zeroed != (uint32_t)n_ends && (rc = packed_abs_buffers(c->stream, hk, (uint32_t)n_ends, &c->packed))) return set_err(rc, packed_last_error());
        const uint32_t tiles = ((uint32_t)n_ends + ABS_TILE - 1) / ABS_TILE;
        uint32_t* cursor = reinterpret_cast<uint32_t*>(c->packed.abs_flags.get());
        uint32_t* tile_any = cursor + MAX_T;
        (void)qcat_abs_launch_pack_planes(c->stream, b->bases, b->offsets, n, ends, hk.max_align, c->win, c->wlen, c->wspec, c->win2 + WIN2_FRONT, lazy_bytes,
                                          c->packed.abs_planes, c->packed.abs_valid, reinterpret_cast<uint8_t*>(tile_any + tiles), tile_any);
        c->packed.abs_ready = (uint32_t)n_ends;
        c->last_fused_ends = (uint32_t)n_ends;
    } else {
        const uint32_t pack_blocks = (uint32_t)((n_ends + PACK_WINDOWS - 1) / PACK_WINDOWS);
        if (ends == 2) hipLaunchKernelGGL(k_pack_windows<2>, dim3(pack_blocks), dim3(PACK_THREADS), 0, c->stream,
                                          b->bases, b->offsets, n, hk.max_align, c->win, c->wlen, c->wspec, c->win2 + WIN2_FRONT, lazy_bytes);
        else hipLaunchKernelGGL(k_pack_windows<1>, dim3(pack_blocks), dim3(PACK_THREADS), 0, c->stream,
                                b->bases, b->offsets, n, hk.max_align, c->win, c->wlen, c->wspec, c->win2 + WIN2_FRONT, lazy_bytes);
    }
    if (path.lazy) hipLaunchKernelGGL(k_expand_special, dim3((uint32_t)((n_ends + 255) / 256)), dim3(256), 0, c->stream,
                                      b->bases, b->offsets, n, ends, hk.max_align, c->wspec, c->win);
    mark(c, "k_pack_windows");
    return 0;
}

// step 4, the scan of the read ends: simple mode on the packed end-tracking kernels or on the general one, else the packed
// path, the one-wave kernels or the general kernel
static int scan_read_ends(qcat_ctx* c, const qcat_kit* kit, KitPtrs kp, size_t n_ends, const ScanPass& pass, const ScanPath& path) {
    const DevKit& hk = kit->hk.dk;
    int32_t* dbg_tpl = pass.debug_scan ? c->dbg_tpl.get() : nullptr;
    int16_t* dbg_rows = pass.debug_scan && pass.row_stride ? c->dbg_rows.get() : nullptr;
    const uint32_t row_stride = pass.row_stride;
    int rc;
    if (hk.mode == QCAT_MODE_SIMPLE && kit->hk.simple_packed && !c->force_generic && !opt_on(QO_NO_SIMPLE_PACKED)) {
        // every batch size from one read end up: a chunked packed scan beats one lane walking the whole list
        if ((rc = simple_packed_scan(c, kp, hk, n_ends, dbg_rows, row_stride))) return rc;
        mark(c, "k_simple_packed");
    } else if (hk.mode == QCAT_MODE_SIMPLE) {
        uint32_t blocks = (uint32_t)((n_ends + GEN_THREADS - 1) / GEN_THREADS);
        hipLaunchKernelGGL(k_scan_simple, dim3(blocks), dim3(GEN_THREADS), 0, c->stream, kp, c->win, c->wlen, (uint32_t)n_ends, c->recs,
                           dbg_rows, row_stride);
        mark(c, "k_scan_simple");
    } else if (path.use_packed) {
        rc = packed_scan(c->stream, kp, hk, c->win, c->wlen, (uint32_t)n_ends, c->recs, &c->packed, dbg_tpl, dbg_rows, row_stride,
                         [&](const char* nm) { mark(c, nm); }, pass.adapter_only, pass.resume_kit_mask);
        if (rc) return set_err(rc, packed_last_error());
    } else if (path.tiny) {
        TinyArgs ta{kp, c->win, c->wlen, nullptr, nullptr, (uint32_t)n_ends, c->recs, c->tiny_tpl, c->tiny_sc, (uint32_t)path.tiny_maxb,
                    dbg_tpl, dbg_rows, row_stride, 0};
        hipLaunchKernelGGL(k_tiny_adapter, dim3((uint32_t)n_ends * (uint32_t)hk.nt), dim3(64), 0, c->stream, ta);
        hipLaunchKernelGGL(k_tiny_decide, dim3((uint32_t)((n_ends + 63) / 64)), dim3(64), 0, c->stream, ta);
        hipLaunchKernelGGL(k_tiny_barcode, dim3((uint32_t)path.tiny_maxb, (uint32_t)n_ends * 2), dim3(64), 0, c->stream, ta);
        hipLaunchKernelGGL(k_tiny_select, dim3((uint32_t)n_ends * 2), dim3(64), 0, c->stream, ta);
        mark(c, "k_scan_tiny");
    } else {
        uint32_t blocks = (uint32_t)((n_ends + GEN_THREADS - 1) / GEN_THREADS);
        hipLaunchKernelGGL(k_scan_generic, dim3(blocks), dim3(GEN_THREADS), 0, c->stream,
                           kp, c->win, c->wlen, (uint32_t)n_ends, c->recs, dbg_tpl, dbg_rows, row_stride, pass.adapter_only ? 1 : 0);
        mark(c, "k_scan_generic");
    }
    return 0;
}

// step 5, finalise (every pass but the vote): the records of the reads and their counts; --detect-middle kits scan the
// interiors of the called reads in between (middle_host.inc, k_scan_middle for what that leaves) and count afterwards
// (`counting` false: the caller counts -- the records still change behind this step, qcat_scan_resident_batches' filter; the
// records go to c->results from read c->res_first on: a chunk of a resident batch)
static int scan_finalize(qcat_ctx* c, const DevKit& hk, KitPtrs kp, const qcat_batch* b, const ScanPath& path, bool counting = true) {
    const uint32_t n = b->n_reads;
    qcat_result* const results = c->results + c->res_first;
    // every block zeroes and flushes an LDS histogram of n_buckets entries with global atomics on the same few counters:
    // fewer, fatter blocks -- 1024 (measured, tools/r04_fin.sh: config 2 0.059 -> 0.028 ms against 4096 blocks, config 3
    // 0.235 -> 0.207 ms), 512 when the bucket vector is long (dual kits: 0.052 against 0.072 ms)
    const QOptVal fb_env = qopt_get(QO_FIN_BLOCKS);                          // (A/B runs)
    uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, fb_env ? (uint64_t)std::max(1, atoi(fb_env)) : (hk.n_buckets > 2048 ? 512 : 1024));
    const bool middle = hk.scan_middle != 0;
    hipLaunchKernelGGL(k_finalize, dim3(blocks), dim3(256), fin_lds_bytes(hk.n_buckets, !middle && counting), c->stream,
                       kp, c->recs, b->offsets, b->true_len, n, results, (middle || !counting) ? nullptr : c->counts.get(),
                       path.slim ? c->packed.bcres : nullptr, path.slim ? c->packed.fin : nullptr);
    mark(c, "k_finalize");
    if (!middle) return 0;
    int rc;
    const uint8_t* only = nullptr;
    if (path.middle_packed) {                              // (also after the tiny kernels: the interiors are no handful of cells)
        if ((rc = middle_packed(c->stream, &c->middle, &c->packed, kp, hk, b, n, results, c->win))) return rc;
        only = c->middle.mid_generic;                      // interiors beyond the packed path's length classes
        mark(c, "k_middle_packed");
    }
    if ((rc = middle_wave_leftovers(c->stream, &c->middle, kp, hk, b, n, results, path.tiny_maxb, only && !c->force_generic))) return rc;
    hipLaunchKernelGGL(k_scan_middle, dim3((n + GEN_THREADS - 1) / GEN_THREADS), dim3(GEN_THREADS), 0, c->stream,
                       kp, b->bases, b->offsets, n, results, only);
    if (counting) hipLaunchKernelGGL(k_count, dim3(blocks), dim3(256), 0, c->stream, kp, results, b->offsets, b->true_len, n, c->counts);
    mark(c, "k_scan_middle");
    return 0;
}

// core: scan a resident batch
static int scan_resident_impl(qcat_ctx* c, qcat_kit* kit, const qcat_batch* b, const ScanPass& pass) {
    if (!c || !kit || !b) return set_err(QCAT_ERR_ARG, "null argument");
    if (b->device != c->device) return set_err(QCAT_ERR_ARG, "batch lives on another device than the context");
    HIPCHK(hipSetDevice(c->device));
    KitOnDevice* kd = nullptr;
    int rc = kit_on_device(kit, c->device, &kd);
    if (rc) return rc;
    const DevKit& hk = kit->hk.dk;
    const int ends = hk.ends == QCAT_ENDS_5P ? 1 : 2;
    const uint32_t n = b->n_reads;
    const size_t n_ends = (size_t)n * ends;
    if (n_ends >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "batch too large (>= 2^31 read ends)");

    // 1. size the buffers, 2. choose the path
    if ((rc = scan_size_buffers(c, hk, n, n_ends, pass))) return rc;
    c->last_n_reads = n;
    c->last_buckets = hk.n_buckets;
    c->last_kit = pass.adapter_only ? nullptr : kit;
    c->auto_batches = -1;                          // (the voted slots of an earlier qcat_scan_resident_batches belong to other records)
    timing_slot(c);
    const ScanPath path = scan_choose_path(c->force_generic != 0, hk, n_ends, pass);
    c->last_tiny_ends = path.tiny ? (uint32_t)n_ends : 0;
    c->last_fused_ends = 0;
    if (path.tiny && (rc = tiny_buffers(c, n_ends, path.tiny_maxb))) return rc;

    // the fills of a scan leave as ONE launch in front of the pack kernel (k_fill_multi): the count vector's here, the front end's
    FillScope fills(n != 0 && !opt_on(QO_NO_FILL_MERGE));      // (every return before a flush drops what was queued)
    if (!pass.keep_counts) HIPCHK(packed_fill(c->counts, 0, (size_t)hk.n_buckets * 8, c->stream));
    if (n == 0) { HIPCHK(packed_fill_flush(c->stream)); return 0; }
    if (c->timing) HIPCHK(hipEventRecord(c->ev[0], c->stream));   // (an empty batch returned above: its slot holds no marks)
    c->middle.absm_codes_early = false;
    if (path.middle_packed && (rc = absmid_codes_early(c->stream, &c->middle, hk, b, n))) return rc;

    KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
    g_jit = kd;
    c->packed.prepared = false; c->packed.abs_zeroed = 0; c->packed.redo_zeroed = false;
    c->packed.slim = path.slim;
    // 3. front end -- or, a resumed scan (the second pass of a kit-auto batch): its job tables' fills with the count vector's, one launch
    if (!pass.resumed()) {
        if ((rc = scan_front_end(c, hk, b, ends, n_ends, path))) return rc;
    } else if (g_fill_defer && path.packed_pairs && c->packed.slices_single) {
        if ((rc = packed_prepare(c->stream, hk, (uint32_t)n_ends, &c->packed))) return set_err(rc, packed_last_error());
        c->packed.prepared = true;
    }
    HIPCHK(packed_fill_flush(c->stream));               // (a resumed scan: the count vector's fill)
    if (hk.mode == QCAT_MODE_SIMPLE && pass.adapter_only) return set_err(QCAT_ERR_ARG, "simple mode has no adapter templates to vote with");
    if (pass.resumed() && !(path.use_packed && c->packed.slices_single))
        return set_err(QCAT_ERR_UNSUPPORTED, "the adapter pass of this kit cannot be resumed per kit (table or general kernels)");
    c->packed.wspec = c->wspec; c->packed.win = c->win; c->packed.win2 = c->win2_valid ? c->win2 + WIN2_FRONT : nullptr;

    // 4. the read ends, 5. finalise
    if ((rc = scan_read_ends(c, kit, kp, n_ends, pass, path))) return rc;
    if (!pass.adapter_only && (rc = scan_finalize(c, hk, kp, b, path, !pass.defer_counts))) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int qcat_scan_resident(qcat_ctx* c, const qcat_kit* kit, const qcat_batch* b) {
    return scan_resident_impl(c, const_cast<qcat_kit*>(kit), b, ScanPass::plain());
}

extern "C" int qcat_ctx_synchronize(qcat_ctx* c) {
    if (!c) return set_err(QCAT_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int qcat_ctx_fetch_results(qcat_ctx* c, qcat_result* out, uint32_t n_reads) {
    if (!c || !out) return set_err(QCAT_ERR_ARG, "null argument");
    if (n_reads != c->last_n_reads) return set_err(QCAT_ERR_ARG, "n_reads does not match the last scan");
    HIPCHK(hipSetDevice(c->device));
    if (n_reads) HIPCHK(hipMemcpyAsync(out, c->results, (size_t)n_reads * sizeof(qcat_result), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int qcat_ctx_fetch_counts(qcat_ctx* c, int64_t* counts, int32_t n_buckets) {
    if (!c || !counts) return set_err(QCAT_ERR_ARG, "null argument");
    if (n_buckets != c->last_buckets) return set_err(QCAT_ERR_ARG, "bucket count does not match the last scan");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(counts, c->counts, (size_t)n_buckets * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// records and counts of the last scan back to a host-buffer caller: through the context's pinned block while that stays small
// (a call of the reference's own shape: 4000 reads = 96 KB) -- one DMA each and ONE wait -- else straight to the caller's arrays
static int fetch_back(qcat_ctx* c, qcat_result* out, uint32_t n_reads, int64_t* counts_add, int32_t n_buckets) {
    const size_t bytes_rec = (size_t)n_reads * sizeof(qcat_result), off_cnt = (bytes_rec + 63) / 64 * 64;
    const size_t need = off_cnt + (counts_add ? (size_t)n_buckets * 8 : 0);
    if (need > (8u << 20)) {
        int rc = qcat_ctx_fetch_results(c, out, n_reads);
        if (!rc && counts_add) {
            std::vector<int64_t> tmp((size_t)n_buckets);
            rc = qcat_ctx_fetch_counts(c, tmp.data(), n_buckets);
            if (!rc) for (size_t i = 0; i < tmp.size(); ++i) counts_add[i] += tmp[i];
        }
        return rc;
    }
    if (n_reads != c->last_n_reads || (counts_add && n_buckets != c->last_buckets)) return set_err(QCAT_ERR_ARG, "sizes do not match the last scan");
    HIPCHK(hipSetDevice(c->device));
    if (need > c->pin_ret.cap()) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(c->pin_ret.ensure(need + need / 4 + 4096));
    }
    if (n_reads) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(c->pin_ret, c->results, bytes_rec, hipMemcpyDeviceToHost, c->stream));
    if (counts_add) HIPCHK_DRAIN(c->stream, hipMemcpyAsync(c->pin_ret + off_cnt, c->counts, (size_t)n_buckets * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_reads) memcpy(out, c->pin_ret, bytes_rec);
    if (counts_add) {
        const int64_t* tmp = reinterpret_cast<const int64_t*>(c->pin_ret + off_cnt);
        for (int32_t i = 0; i < n_buckets; ++i) counts_add[i] += tmp[i];
    }
    return 0;
}

extern "C" void* qcat_ctx_stream(qcat_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int64_t qcat_ctx_tiny_ends(const qcat_ctx* c) { return c ? (int64_t)c->last_tiny_ends : -1; }
// diagnostics of the latest scan's front end: out[0] = read ends whose windows and letter planes came from the one kernel
// (k_pack_planes; 0: k_pack_windows, and k_abs_planes where the bit-sliced adapter scan ran), out[1] = read ends per workgroup of that kernel
extern "C" int qcat_ctx_fused_front(const qcat_ctx* c, uint32_t* out) {
    if (!c || !out) return set_err(QCAT_ERR_ARG, "null argument");
    out[0] = c->last_fused_ends;
    out[1] = qcat_abs_launch_pack_planes(nullptr, nullptr, nullptr, 0, 1, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    return 0;
}
// reads whose interior the latest --detect-middle scan put on the one-wave kernels (k_midw_*: interiors the packed interior scan
// does not take); synchronises the stream; -1: null context, 0: none / the path did not run
extern "C" int64_t qcat_ctx_middle_wave_reads(qcat_ctx* c) {
    return c ? middle_wave_count(c->middle, c->device, c->stream) : -1;
}
extern "C" int64_t qcat_ctx_graph_replays(const qcat_ctx* c) { return c ? (int64_t)(c->api_graph.replays + c->scan_graph.replays) : -1; }
// diagnostics of the latest scan of the read ends: super-tiles (2048 barcode alignments each) its bit-sliced barcode kernels took, per
// hot class summed over the (template, set) groups -- out[0] regions a few bases short of nominal (front-padded units), out[1]
// nominal regions, out[2] full windows; all 0 when the path was not taken
extern "C" int qcat_ctx_barcode_bitslice_tiles(qcat_ctx* c, uint32_t* out) {
    if (!c || !out) return set_err(QCAT_ERR_ARG, "null argument");
    out[0] = out[1] = out[2] = 0;
    if (!c->packed.bsplan || !c->packed.bs_last) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    BsPlan hp;
    HIPCHK(hipMemcpy(&hp, c->packed.bsplan, sizeof hp, hipMemcpyDeviceToHost));
    for (int b = 0; b < JOB_BINS; ++b) {
        const int cls = b % JOB_CLASSES - (JOB_CLASSES - JOB_HOT);
        if (cls >= 0) out[cls] += hp.count[b];
    }
    return 0;
}
// diagnostics of the latest --detect-middle scan: out[0] = big tiles (2048 interiors) its bit-sliced adapter scan walked, out[1] = big
// tiles in all, out[2] = tiles of 128 interiors left to the binary16 kernel, out[3] = tiles of 128 in all (all 0: path not taken)
extern "C" int qcat_ctx_middle_bitslice_tiles(qcat_ctx* c, uint32_t* out) {
    if (!c || !out) return set_err(QCAT_ERR_ARG, "null argument");
    return middle_bitslice_tiles(c->middle, c->device, c->stream, out);
}
extern "C" void* qcat_ctx_counts_devptr(qcat_ctx* c) { return c ? c->counts : nullptr; }
extern "C" void* qcat_ctx_results_devptr(qcat_ctx* c) { return c ? c->results : nullptr; }

extern "C" int qcat_ctx_last_timing(qcat_ctx* c, const char** names, float* ms, int cap) {
    if (!c) return set_err(QCAT_ERR_ARG, "null context");
    if (!c->timing) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    // average per mark over the recorded scans that have the same mark list as the newest one
    const int last = c->ring_used - 1;
    if (last < 0) return 0;
    const int n = std::min(cap, c->ring_marks[last]);
    for (int i = 0; i < n; ++i) { names[i] = c->timed_name[last][i]; ms[i] = 0.f; }
    int scans = 0;
    for (int r = 0; r <= last; ++r) {
        if (c->ring_marks[r] != c->ring_marks[last]) continue;
        bool same = true;
        for (int i = 0; i < n; ++i) same = same && c->timed_name[r][i] == c->timed_name[last][i];
        if (!same) continue;
        for (int i = 0; i < n; ++i) { float t = 0.f; HIPCHK(hipEventElapsedTime(&t, c->evr[r][i], c->evr[r][i + 1])); ms[i] += t; }
        ++scans;
    }
    for (int i = 0; i < n; ++i) ms[i] /= (float)scans;
    c->ring_used = 0; c->n_timed = 0; c->ev = nullptr;
    return n;
}

// ------------------------------------------------------------------------------------------
// batches: upload / download / from and as device pointers / partition / synthetic (the types: batch.h)
// ------------------------------------------------------------------------------------------
#include "batch_host.inc"
// --filter-barcodes on the device: filter_run for the records of a scan, qcat_filter_barcodes for records of a caller
#include "filter_host.inc"
// what the calls over a scanned batch share: argument check, records, name tables, mirrored tables, the finished text
#include "text_out_host.inc"
// FASTQ text in device memory: the parse into a resident batch, per-barcode FASTQ text out of one (kernels_fqtext.inc)
#include "fqtext_host.inc"
// the kit vote: VoteBuf and vote_enqueue, and the entry points that vote -- qcat_detect_kit, the kit-auto host-buffer calls,
// qcat_scan_resident_batches
#include "vote_host.inc"

// ------------------------------------------------------------------------------------------
// host-buffer entry points
// ------------------------------------------------------------------------------------------
static void fill_trace(const HostKit& hk, const EndRec& r, const int32_t* tplraw, const int32_t* tplend, qcat_end_trace* t) {
    memset(t, 0, sizeof *t);
    t->window_len = r.window_len;
    for (int i = 0; i < MAX_T; ++i) { t->tpl_raw[i] = tplraw[i]; t->tpl_end[i] = tplend[i]; }
    t->best_tpl = r.best_tpl; t->best_end = r.best_end; t->best_raw = r.best_raw; t->used_tpl = r.used_tpl;
    t->region_path = r.region_path;
    for (int s = 0; s < 2; ++s) {
        t->region_start[s] = r.region_start[s]; t->region_len[s] = r.region_len[s];
        t->bc_idx[s] = r.bc_idx[s]; t->bc_raw[s] = r.bc_raw[s];
    }
    const DevTpl& p = hk.dk.tpl[r.used_tpl];
    if (hk.dk.mode == QCAT_MODE_EPI2ME) {
        int ae = r.best_end + p.trim_offset;
        t->adapter_end = ae > r.window_len ? r.window_len : ae;
    } else if (hk.dk.mode == QCAT_MODE_SIMPLE) {
        t->adapter_end = (r.bc_idx[0] >= 0 && r.bc_raw[0] >= p.sets[0].min_raw_pass) ? r.best_end : 0;
    } else {
        t->adapter_end = (r.bc_idx[0] >= 0 && r.bc_idx[1] >= 0) ? r.best_end : 0;
    }
}

// qcat_scan_batch over host buffers as a chunked pipeline (pipeline.h): scan_batch_pipelined
#include "pipeline_host.inc"

// (ptrs / lens: the reads as one pointer and one length each instead of bases / offsets -- the file loops' one-shot path)
static int scan_debug_impl(qcat_ctx* c, const qcat_kit* ckit,
                           const uint8_t* bases, const uint64_t* offsets, const uint8_t* const* ptrs, const uint64_t* lens, uint32_t n_reads,
                           qcat_result* out, int64_t* counts,
                           qcat_end_trace* traces, int16_t* bc_rows, uint32_t row_stride) {
    if (!c || !ckit || (!offsets && !ptrs) || !out) return set_err(QCAT_ERR_ARG, "null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    if (bc_rows && (int)row_stride < max_set_barcodes(kit->hk.dk, 0))
        return set_err(QCAT_ERR_ARG, "row_stride smaller than the largest barcode set");
    qcat_batch* b = nullptr;
    int rc = batch_upload_windows(c, kit, bases, offsets, n_reads, &b, ptrs, lens);
    if (rc) return rc;
    const bool debug = traces != nullptr || bc_rows != nullptr;
    // (whole reads -- --detect-middle -- never replay a graph: the interior scan sizes buffers from the batch)
    if (!debug && !b->owned() && n_reads && n_reads <= 65536 && !kit->hk.dk.scan_middle && !opt_on(QO_FULL_UPLOAD)) {
        // the reference's library entry -- detect_barcode / detect_barcode_batch with a named kit, down to ONE read per call
        // (qcat/test/test_barcode.py:84, cli.py:504-509) -- is a dozen launches of a few microseconds each: calls of one shape
        // replay them as a graph, like the kit-auto calls (api_graph_run)
        KitOnDevice* kd = nullptr;
        rc = kit_on_device(kit, c->device, &kd);
        if (!rc) rc = api_graph_run(c->stream, c->timing, &c->packed, c->scan_graph, kit, kd, b, 0,
                                    [&] { return scan_resident_impl(c, kit, b, ScanPass::plain()); }, [] {});
        else (void)hipStreamSynchronize(c->stream);
        if (!rc) { c->last_n_reads = n_reads; c->last_buckets = kit->hk.dk.n_buckets; }      // (a replay does not pass through scan_resident_impl)
    } else rc = scan_resident_impl(c, kit, b, debug ? ScanPass::debug(bc_rows ? row_stride : 0) : ScanPass::plain());
    if (rc) (void)hipStreamSynchronize(c->stream);          // (the upload may still be reading the context's pinned staging)
    if (!rc) rc = fetch_back(c, out, n_reads, counts, kit->hk.dk.n_buckets);
    if (!rc && debug && n_reads) {
        const int ends = kit->hk.dk.ends == QCAT_ENDS_5P ? 1 : 2;
        const size_t n_ends = (size_t)n_reads * ends;
        std::vector<EndRec> recs(n_ends);
        std::vector<int32_t> tpl(n_ends * 2 * MAX_T);
        hipError_t e = hipMemcpy(recs.data(), c->recs, n_ends * sizeof(EndRec), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(tpl.data(), c->dbg_tpl, tpl.size() * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && bc_rows) e = hipMemcpy(bc_rows, c->dbg_rows, n_ends * 2 * row_stride * 2, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(QCAT_ERR_DEVICE, std::string("debug download: ") + hipGetErrorString(e));
        else if (traces)
            for (size_t i = 0; i < n_ends; ++i)
                fill_trace(kit->hk, recs[i], &tpl[(i * 2 + 0) * MAX_T], &tpl[(i * 2 + 1) * MAX_T], &traces[i]);
    }
    qcat_batch_destroy(b);
    return rc;
}

extern "C" int qcat_scan_debug(qcat_ctx* c, const qcat_kit* ckit,
                               const uint8_t* bases, const uint64_t* offsets, uint32_t n_reads,
                               qcat_result* out, int64_t* counts,
                               qcat_end_trace* traces, int16_t* bc_rows, uint32_t row_stride) {
    if (!offsets) return set_err(QCAT_ERR_ARG, "null argument");
    return scan_debug_impl(c, ckit, bases, offsets, nullptr, nullptr, n_reads, out, counts, traces, bc_rows, row_stride);
}

extern "C" int qcat_scan_batch(qcat_ctx* c, const qcat_kit* kit,
                               const uint8_t* bases, const uint64_t* offsets, uint32_t n_reads,
                               qcat_result* out, int64_t* counts) {
    if (!c || !kit || !offsets || !out) return set_err(QCAT_ERR_ARG, "null argument");
    const ReadView rv{bases, offsets, nullptr};
    const int rc = scan_batch_pipelined(c, const_cast<qcat_kit*>(kit), rv, n_reads, out, counts);
    if (rc <= 0) return rc;                           // done (0) or failed (< 0); 1 = take the one-shot path
    return qcat_scan_debug(c, kit, bases, offsets, n_reads, out, counts, nullptr, nullptr, 0);
}

extern "C" int qcat_scan_sequences(qcat_ctx* c, const qcat_kit* ckit, const uint8_t* bases, const uint64_t* offsets,
                                   uint32_t n_seqs, qcat_result* out) {
    if (!c || !ckit || !offsets || !out) return set_err(QCAT_ERR_ARG, "qcat_scan_sequences: null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    for (uint32_t r = 0; r < n_seqs; ++r)
        if (offsets[r + 1] >= offsets[r] && offsets[r + 1] - offsets[r] >= (1ull << 31))
            return set_err(QCAT_ERR_UNSUPPORTED, "qcat_scan_sequences: sequence longer than 2^31 - 1 bases");
    qcat_batch* b = nullptr;
    int rc = qcat_batch_upload(c, bases, offsets, n_seqs, &b);
    if (rc) return rc;
    KitOnDevice* kd = nullptr;
    rc = kit_on_device(kit, c->device, &kd);
    if (!rc) rc = grow(c->results, (size_t)n_seqs);
    if (!rc && n_seqs) {
        KitPtrs kp{kd->kit, kd->codes, kd->ids, kd->tables};
        const DevKit& hk = kit->hk.dk;
        // one wave per alignment along its anti-diagonals (kernels_tiny.inc; round 5): L + M steps per alignment and every
        // template and barcode of a sequence side by side, where the general kernel walks L x M cells of everything on one
        // lane -- every mode: the adapter modes with linear or affine gap costs (k_tiny_adapter / k_tiny_adapter_affine; the
        // barcode waves are linear 1/1 always), simple mode on k_tiny_simple_*.  QCAT_HIP_NO_TINY=1, the generic switch and gap
        // costs beyond WAVE_GAP_MAX: the general kernel, as are calls beyond the size limits of kernels_tiny.inc (option WAVE_MAX)
        const int maxb = max_set_barcodes(hk);
        const bool affine = hk.gap_open != hk.gap_extend, simple = hk.mode == QCAT_MODE_SIMPLE;
        const bool gaps_fit = !affine || (hk.gap_open >= 0 && hk.gap_extend >= 0 && hk.gap_open <= WAVE_GAP_MAX && hk.gap_extend <= WAVE_GAP_MAX);
        // (linear gaps in the adapter modes: every call, as before; the configurations that came later: up to a number of waves)
        const uint64_t n_waves = simple ? (uint64_t)n_seqs * (uint64_t)std::max(1, (int)hk.tpl[0].sets[0].n)
                                        : (uint64_t)n_seqs;
        const bool size_fits = simple ? n_waves <= (uint64_t)opt_val(QO_WAVE_MAX, (int64_t)WAVE_SIMPLE_MAX)
                                      : !affine || n_waves <= (uint64_t)opt_val(QO_WAVE_MAX, (int64_t)WAVE_AFFINE_MAX);
        const bool waves = (simple || gaps_fit) && size_fits && !opt_on(QO_NO_TINY) && !c->force_generic;
        if (waves && simple) {
            // the scores of a piece: piece x B x 8 bytes, 64 MiB at most (and the grid's y limit as below)
            const uint32_t nb = (uint32_t)std::max(1, (int)hk.tpl[0].sets[0].n);
            const uint32_t PIECE = std::max<uint32_t>(1u, std::min<uint32_t>(32767u, (uint32_t)(((size_t)64 << 20) / ((size_t)nb * 8))));
            const uint32_t piece = std::min(n_seqs, PIECE);
            rc = grow(c->recs, (size_t)piece);
            if (!rc) rc = grow(c->tiny_simple, (size_t)piece * nb * 2);
            for (uint32_t s0 = 0; !rc && s0 < n_seqs; s0 += PIECE) {
                const uint32_t ns = std::min(PIECE, n_seqs - s0);
                TinyArgs ta{kp, nullptr, nullptr, b->bases, b->offsets + s0, ns, c->recs, nullptr, nullptr, 0, nullptr, nullptr, 0, 0};
                if (hk.tpl[0].sets[0].n > 0)
                    hipLaunchKernelGGL(k_tiny_simple_barcode, dim3(nb, ns), dim3(64), 0, c->stream, ta, c->tiny_simple);
                hipLaunchKernelGGL(k_tiny_simple_select, dim3(ns), dim3(64), 0, c->stream, ta, (const int32_t*)c->tiny_simple);
                hipLaunchKernelGGL(k_tiny_store_sequences, dim3((ns + 63) / 64), dim3(64), 0, c->stream, ta, c->results + s0);
            }
        } else if (waves) {
            constexpr uint32_t PIECE = 32767;          // (the barcode kernel's grid has (sequence, set) in y: 65535 at most)
            const uint32_t piece = std::min(n_seqs, PIECE);
            rc = grow(c->recs, (size_t)piece);
            if (!rc) rc = tiny_buffers(c, (size_t)piece, maxb);
            for (uint32_t s0 = 0; !rc && s0 < n_seqs; s0 += PIECE) {
                const uint32_t ns = std::min(PIECE, n_seqs - s0);
                TinyArgs ta{kp, nullptr, nullptr, b->bases, b->offsets + s0, ns, c->recs, c->tiny_tpl, c->tiny_sc, (uint32_t)maxb, nullptr, nullptr, 0, 0};
                if (affine) hipLaunchKernelGGL(k_tiny_adapter_affine, dim3(ns * (uint32_t)hk.nt), dim3(64), 0, c->stream, ta);
                else hipLaunchKernelGGL(k_tiny_adapter, dim3(ns * (uint32_t)hk.nt), dim3(64), 0, c->stream, ta);
                hipLaunchKernelGGL(k_tiny_decide, dim3((ns + 63) / 64), dim3(64), 0, c->stream, ta);
                hipLaunchKernelGGL(k_tiny_barcode, dim3((uint32_t)maxb, ns * 2), dim3(64), 0, c->stream, ta);
                hipLaunchKernelGGL(k_tiny_select, dim3(ns * 2), dim3(64), 0, c->stream, ta);
                hipLaunchKernelGGL(k_tiny_store_sequences, dim3((ns + 63) / 64), dim3(64), 0, c->stream, ta, c->results + s0);
            }
        } else
        hipLaunchKernelGGL(k_scan_sequences, dim3((n_seqs + GEN_THREADS - 1) / GEN_THREADS), dim3(GEN_THREADS), 0, c->stream,
                           kp, b->bases, b->offsets, n_seqs, c->results);
        c->last_tiny_ends = (waves && !rc) ? n_seqs : 0;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out, c->results, (size_t)n_seqs * sizeof(qcat_result), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = set_err(QCAT_ERR_DEVICE, std::string("qcat_scan_sequences: ") + hipGetErrorString(e));
    }
    c->last_n_reads = 0;                               // the context's result buffer no longer holds a batch scan
    c->last_kit = nullptr;
    qcat_batch_destroy(b);
    return rc;
}

extern "C" int qcat_sg_align(qcat_ctx* c, const uint8_t* queries, const uint64_t* q_offsets, const uint8_t* targets,
                             const uint64_t* t_offsets, uint32_t n, int32_t gap_open, int32_t gap_extend, const int8_t* matrix,
                             int32_t with_stats_and_rule, qcat_alignment* out) {
    const int32_t r1_flag = with_stats_and_rule & QCAT_SG_R1_SCALAR, with_stats = with_stats_and_rule & ~QCAT_SG_R1_SCALAR;
    if (!c || !q_offsets || !t_offsets || !matrix || !out) return set_err(QCAT_ERR_ARG, "qcat_sg_align: null argument");
    if (n == 0) return 0;
    if (gap_open < 0 || gap_extend < 0) return set_err(QCAT_ERR_ARG, "qcat_sg_align: negative gap cost");
    if (with_stats != QCAT_STATS_NONE && with_stats != QCAT_STATS_PARASAIL6 && with_stats != QCAT_STATS_PARASAIL5 && with_stats != QCAT_STATS_ROUND3)
        return set_err(QCAT_ERR_ARG, "qcat_sg_align: with_stats must be one of QCAT_STATS_* (optionally | QCAT_SG_R1_SCALAR)");
    for (uint32_t i = 0; i < n; ++i) {
        if (q_offsets[i + 1] < q_offsets[i] || t_offsets[i + 1] < t_offsets[i]) return set_err(QCAT_ERR_ARG, "offsets must be non-decreasing");
        if (t_offsets[i + 1] - t_offsets[i] > (uint64_t)MAX_TLEN) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_sg_align: target longer than QCAT_MAX_TEMPLATE_LEN");
        if (q_offsets[i + 1] - q_offsets[i] >= (1ull << 31)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_sg_align: query longer than 2^31 - 1");
    }
    HIPCHK(hipSetDevice(c->device));
    const uint64_t qb = q_offsets[n], tb = t_offsets[n];
    if ((qb && !queries) || (tb && !targets)) return set_err(QCAT_ERR_ARG, "qcat_sg_align: null sequence buffer");
    // without statistics: one wave per pair along its anti-diagonals (kernels_tiny.inc: k_sg_wave), no scratch; the statistics
    // need the matrices of the traceback and stay on k_sg_align, as do QCAT_HIP_NO_TINY=1, the generic switch and gap costs
    // beyond WAVE_GAP_MAX and calls of more than WAVE_SG_MAX pairs (option WAVE_MAX)
    const bool waves = with_stats == QCAT_STATS_NONE && !opt_on(QO_NO_TINY) && !c->force_generic &&
                       gap_open <= WAVE_GAP_MAX && gap_extend <= WAVE_GAP_MAX && (uint64_t)n <= (uint64_t)opt_val(QO_WAVE_MAX, (int64_t)WAVE_SG_MAX);
    c->last_tiny_ends = 0;
    const uint32_t blocks = (n + GEN_THREADS - 1) / GEN_THREADS;
    const size_t threads = (size_t)blocks * GEN_THREADS;
    FixedBuf<uint8_t> dq, dt;                          // (temporaries of this call: released on every exit path)
    FixedBuf<uint64_t> dqo, dto;
    FixedBuf<int32_t> dscr;
    FixedBuf<qcat_alignment> dout;
    HIPCHK(dq.ensure(qb + 1)); HIPCHK(dqo.ensure((size_t)n + 1)); HIPCHK(dt.ensure(tb + 1)); HIPCHK(dto.ensure((size_t)n + 1));
    if (!waves) HIPCHK(dscr.ensure((with_stats ? 6 : 2) * (size_t)(MAX_TLEN + 1) * threads));
    HIPCHK(dout.ensure(n));
    if (qb) HIPCHK(hipMemcpyAsync(dq, queries, qb, hipMemcpyHostToDevice, c->stream));
    if (tb) HIPCHK(hipMemcpyAsync(dt, targets, tb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dqo, q_offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dto, t_offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    SgMatrix m;
    memcpy(m.m, matrix, 49);
    if (waves)
        hipLaunchKernelGGL(k_sg_wave, dim3(n), dim3(64), 0, c->stream, dq.get(), dqo.get(), dt.get(),
                           dto.get(), n, (int)gap_open, (int)gap_extend, m, (int)(r1_flag != 0), dout.get());
    else
    hipLaunchKernelGGL(k_sg_align, dim3(blocks), dim3(GEN_THREADS), 0, c->stream, dq.get(), dqo.get(), dt.get(),
                       dto.get(), n, (int)gap_open, (int)gap_extend, m, (int)(with_stats | r1_flag), dscr.get(), dout.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * sizeof(qcat_alignment), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->last_tiny_ends = waves ? n : 0;
    return 0;
}

// ------------------------------------------------------------------------------------------
// native FASTQ ingest and egress
// ------------------------------------------------------------------------------------------
#include "fastq_host.inc"
#include "fastq_stream.inc"
// the driver's TSV rows of a scanned text batch, formatted in device memory (the score texts: fq_repr_double of fastq_host.inc)
#include "tsvtext_host.inc"
// the driver's annotated single stream of a scanned text batch (the id texts: the id slots of the TSV tables)
#include "textstream_host.inc"
// the evaluation of a scanned text batch: qcat-eval's classes and summary, qcat-roc's table (the id texts: the id slots again)
#include "eval_host.inc"

// ------------------------------------------------------------------------------------------
// multi-GPU count reduction (RCCL)
// ------------------------------------------------------------------------------------------
#include "comm.inc"

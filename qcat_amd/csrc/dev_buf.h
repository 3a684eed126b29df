// dev_buf.h -- owners of the scan path's grow-on-demand scratch (host only): DevBuf<T> over device memory, PinBuf<T> over
// pinned host memory.  A context, its PackedScratch and its pipeline stages hold their buffers as these types, so a buffer is
// freed exactly once -- by its owner's destructor -- and every reallocation of device scratch goes through q_malloc.
// FixedBuf<T> owns device memory outside that rule: the planes of a resident batch (batch.h) and the temporaries of one call.
// Included by packed_host.inc (qcat_hip.hip, and jit_prelude.inc for the struct layouts).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace qk {

// every device allocation of the scan path bumps this counter: a captured graph of a host-buffer call (qcat_hip.hip:
// api_graph_run) holds the buffers' addresses and is dropped when anything was reallocated since its capture
// (process-wide, not per thread: the workers of the kit-auto file loop are new threads at every call, and a counter that
// starts at zero in each of them could match a graph captured by an earlier thread although another thread moved the buffers
// in between; an allocation of ANY context drops every context's graph -- spurious, and safe)
static std::atomic<uint64_t> g_alloc_gen{0};
static inline hipError_t q_malloc(void** p, size_t bytes) { g_alloc_gen.fetch_add(1); return hipMalloc(p, bytes); }

struct DevMem {
    static hipError_t alloc(void** p, size_t bytes) { return q_malloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinMem {                                // (no generation bump: the one pinned buffer kernels read in place bumps at its site)
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void release(void* p) { (void)hipHostFree(p); }
};
struct FixedMem {                              // (device memory of a fixed size that is the caller's -- the planes of a resident batch,
                                               //  the temporaries of one call: no scan buffer moves, so no generation bump)
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};

// a pointer and its capacity in elements; move-only.  Contents are never preserved across a reallocation.
template <class T, class Mem>
class ScratchBuf {
public:
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf&) = delete;
    ScratchBuf& operator=(const ScratchBuf&) = delete;
    ScratchBuf(ScratchBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    ScratchBuf& operator=(ScratchBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~ScratchBuf() { reset(); }
    // room for n elements (at least one): nothing when the buffer has it, else free and allocate exactly that.  A failure
    // leaves a null pointer and capacity 0.
    hipError_t ensure(size_t n) {
        if (n <= cap_ && p_) return hipSuccess;
        reset();
        if (n < 1) n = 1;
        const hipError_t e = Mem::alloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr; else cap_ = n;
        return e;
    }
    void reset() { if (p_) Mem::release(p_); p_ = nullptr; cap_ = 0; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    operator T*() const { return p_; }         // (kernel arguments, pointer arithmetic and null tests read like the raw pointer did)

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T> using DevBuf = ScratchBuf<T, DevMem>;
template <class T> using PinBuf = ScratchBuf<T, PinMem>;
template <class T> using FixedBuf = ScratchBuf<T, FixedMem>;

}  // namespace qk

// host_pipeline.inc -- qcat_scan_batch from HOST buffers as a three-stage pipeline over chunks of the
// batch (replaces: the per-read loop of cli.qcat_cli over detect_barcode, qcat/cli.py:504-513, whose
// reads live in host memory):
//
//     host threads : compact chunk k+1 to its scanned windows (head + tail of every read) into pinned memory
//     copy stream  : H2D of chunk k   (windows, offsets, real lengths: <= 300 B + 12 B per read)
//     scan stream  : the kernels of chunk k-1, then D2H of its 24-byte records into pinned memory
//
// so a call costs max(host compaction, PCIe, GPU) instead of their sum.  Everything it needs is owned
// by the context and reused: a persistent worker pool, two pinned staging sets, two device chunk sets,
// their pinned record buffers (all sized by the chunk, not by the batch) -- no hipMalloc / hipFree / thread start per call once warm, and one host
// synchronisation at the end.  The count vector accumulates on the device across the chunks.
// Included by qcat_hip.hip.
#include <condition_variable>
#include <atomic>
#include <ctime>
#include <functional>

namespace qk {

// CPU nanoseconds the pools' parts have taken in this process (compaction of the scanned windows into the staging buffers;
// PIPELINE_TRACE prints it beside the file loop's other stages)
static std::atomic<uint64_t> g_host_pool_cpu_ns{0};
static inline uint64_t host_thread_cpu_ns() {
    struct timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec : 0;
}

// persistent pool: run(n, fn) executes fn(part) for part = 0..n-1 on the workers + the caller
class HostPool {
public:
    explicit HostPool(unsigned workers) {
        for (unsigned i = 0; i < workers; ++i) {
            try { threads_.emplace_back([this] { loop(); }); }
            catch (const std::exception&) { break; }               // fewer threads: the caller takes the rest
        }
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; ++gen_; }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    unsigned size() const { return (unsigned)threads_.size() + 1; }
    void run(int parts, const std::function<void(int)>& fn) {
        if (parts <= 0) return;
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn; parts_ = parts; next_ = 0; left_ = parts; ++gen_;
        }
        cv_.notify_all();
        work();                                                    // the caller works too
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return left_ == 0; });
        fn_ = nullptr;
    }

private:
    void work() {
        for (;;) {
            int p;
            const std::function<void(int)>* fn;
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (!fn_ || next_ >= parts_) return;
                p = next_++; fn = fn_;
            }
            const uint64_t c0 = host_thread_cpu_ns();
            (*fn)(p);
            g_host_pool_cpu_ns.fetch_add(host_thread_cpu_ns() - c0, std::memory_order_relaxed);
            std::lock_guard<std::mutex> lk(mu_);
            if (--left_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
            }
            work();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    int parts_ = 0, next_ = 0, left_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

struct PipeStage {                     // one of the two chunk slots
    PinBuf<uint8_t> pin_bases; PinBuf<uint64_t> pin_offsets; PinBuf<uint32_t> pin_len;
    DevBuf<uint8_t> dev_bases_alloc; DevBuf<uint64_t> dev_offsets; DevBuf<uint32_t> dev_len;
    PinBuf<qcat_result> pin_results;                    // the chunk's records on their way to the caller's array
    uint32_t res_first = 0, res_count = 0;              // ... reads [res_first, res_first + res_count), 0: nothing pending
    hipEvent_t copied = nullptr, scanned = nullptr;
};

struct HostPipeline {
    HostPool* pool = nullptr;
    PipeStage st[2];
    hipStream_t copy = nullptr;
};

static inline void pipeline_free(HostPipeline* p) {
    if (!p) return;
    delete p->pool;
    for (PipeStage& s : p->st) {
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.scanned) (void)hipEventDestroy(s.scanned);
    }
    if (p->copy) (void)hipStreamDestroy(p->copy);
    delete p;                          // (the stages' staging buffers free themselves)
}

}  // namespace qk

// api_graph.inc -- the device work of a host-buffer call as a captured graph: what a context keeps per family of calls
// (ApiGraph: kit-auto calls, calls with a named kit) and api_graph_run, which launches, captures or replays.
// Included by qcat_hip.hip in front of the context, which holds two ApiGraph: it needs the kits, qcat_batch, FillScope,
// packed_streams_reset and HIPCHK_DRAIN.

// two dozen launches (round 5: ~45 on twelve streams) replayed by one hipGraphLaunch when a call has the shape of the one before it
struct ApiGraph {
    struct Shape {                                 // what a call's launches depend on besides the data
        uint64_t kit = 0, n_bases = 0, gen = 0;    // the kit's serial, the compacted bases, the allocation generation (dev_buf.h)
        uint32_t n_reads = 0, batch_reads = 0;
        bool operator==(const Shape& o) const { return kit == o.kit && n_bases == o.n_bases && gen == o.gen && n_reads == o.n_reads && batch_reads == o.batch_reads; }
    };
    hipGraphExec_t exec = nullptr;
    Shape captured;                                // what `exec` was captured for
    Shape previous;                                // the shape of the last call
    int failures = 0;                              // captures that did not work out (two: never again)
    uint64_t replays = 0;
};

// The device work of a host-buffer call -- everything between the upload and the download -- launched kernel by kernel
// (`enqueue`) or replayed as ONE graph.  A call shaped like the one before it (same kit, read count, compacted bases; nothing
// reallocated in between) replays: the launches take no arguments from the host but buffer addresses and sizes, every
// decision that depends on the data (kit vote, job plan, cursors) is made on the device.  The second such call captures
// (hipStreamBeginCapture, thread-local mode; the side streams join the capture through fork_join's events), later ones
// replay (`prep`: host-side state a replay needs as well).  QCAT_HIP_NO_GRAPH=1: always launch kernel by kernel.  Timed
// contexts and the diagnostic switches (they synchronise inside the scan) never capture.  A failure drains the stream before
// it returns (the upload may still be reading the pinned staging).
// (stream, timed, packed: the context's stream, whether it times its kernels, its packed scratch with the side streams)
template <class Enqueue, class Prep>
static int api_graph_run(hipStream_t stream, bool timed, PackedScratch* packed, ApiGraph& G, qcat_kit* kit, KitOnDevice* kd,
                         const qcat_batch* b, uint32_t batch_reads, Enqueue enqueue, Prep prep) {
    auto drained = [&](int code) { (void)hipStreamSynchronize(stream); return code; };
    static const QcatOpt no_capture[] = {QO_NO_GRAPH, QO_DEBUG_VOTE, QO_BS_TRACE, QO_DEBUG_BINS, QO_DEBUG_REDO};
    bool graph_ok = !timed && G.failures < 2 && !b->owned() && !kit->hk.dk.scan_middle && !opt_on(QO_FULL_UPLOAD);      // (whole reads -- --detect-middle -- never replay)
    for (QcatOpt o : no_capture) if (opt_on(o)) graph_ok = false;
    const uint64_t gen_before = g_alloc_gen.load();
    const ApiGraph::Shape shape{kit->serial, b->n_bases, gen_before, b->n_reads, batch_reads};
    bool done = false;
    int rc = 0;
    if (graph_ok && G.exec && G.captured == shape) {
        prep();
        g_jit = kd;
        HIPCHK_DRAIN(stream, hipGraphLaunch(G.exec, stream));
        ++G.replays;
        done = true;
    } else if (graph_ok && G.previous == shape) {
        if (G.exec) { (void)hipGraphExecDestroy(G.exec); G.exec = nullptr; }
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int erc = enqueue();
            const hipError_t ee = hipStreamEndCapture(stream, &graph);
            const bool captured = erc == 0 && ee == hipSuccess && graph != nullptr;
            const bool moved = g_alloc_gen.load() != gen_before;     // (some context allocated meanwhile: not this call's failure)
            if (captured && !moved && hipGraphInstantiate(&G.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                G.captured = shape;
                if (hipGraphLaunch(G.exec, stream) == hipSuccess) done = true;
            }
            if (graph) (void)hipGraphDestroy(graph);
            if (!done && !(captured && moved)) {
                ++G.failures;
                (void)hipGetLastError();
                (void)hipStreamSynchronize(stream);
                packed_streams_reset(packed);                    // (fresh side streams: the old ones may still think they capture)
            }
        } else ++G.failures;
        if (!done) {                                             // (nothing of the capture ran: the plain launches below do the work)
            (void)hipGetLastError();
            if (G.exec) { (void)hipGraphExecDestroy(G.exec); G.exec = nullptr; }
            FillScope drop(false);                                 // (whatever the capture queued and did not flush)
        }
    }
    if (!done && (rc = enqueue())) return drained(rc);
    G.previous = shape;
    G.previous.gen = g_alloc_gen.load();                         // (as it is now: the launches above may have allocated)
    return 0;
}

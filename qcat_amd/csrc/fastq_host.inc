// fastq_host.inc -- native FASTQ ingest and egress around the scan (SURVEY.md 8f rank 2, at speed).
//
// The reference driver (qcat/cli.py:445-563) reads a FASTQ file with Biopython's FastqGeneralIterator in batches of 4000
// (:235-306, :500), calls detect_barcode_batch per batch (:506-513), optionally trims (:521-526), applies the
// minimum-length filter (:527-530), and writes TSV rows (:408-442, header :486-487) or FASTQ records with a
// `barcode=<id>` tag into one stream or one file per barcode (:309-358).  qcat_amd/cli.py does the same in Python at
// ~0.2 M reads/s -- three orders of magnitude below the kernels.  This file is the same flow behind the C ABI:
//
//   qcat_fastq_open    mmap the file, split it into records on all host threads (every thread finds a record start in
//                      its byte range by the four-line pattern, parses to the end of its range, and the pieces must
//                      meet exactly -- otherwise the file is split again by one thread), and keep one 32-byte entry
//                      per read: where title, sequence and quality lie in the mapping.  ONLY plain four-line ASCII
//                      records qualify (what ONT base callers write); anything Biopython would treat differently --
//                      wrapped lines, blank lines, '\r', trailing blanks, bytes >= 0x80, a '+' line that repeats a
//                      different title -- makes the call return QCAT_ERR_UNSUPPORTED and the Python parser, which
//                      restates Biopython's rules, takes the file.
//   qcat_fastq_demux   the reads go to the device straight from the mapping (the chunked pipeline of qcat_scan_batch
//                      reads heads and tails of the sequences in place: no intermediate copy, no Python strings), with a
//                      fixed kit in chunks of up to 4 M reads, under kit auto per batch of `batch_size` reads through the
//                      vote-and-resume pass of qcat_scan_batch_auto; then the writers run on the host threads -- a
//                      block of reads is formatted into per-file buffers in parallel, the buffers are appended in
//                      file order -- byte for byte what qcat_amd/cli.py writes (tests/test_cli_gpu.py runs both).
//
// Included by qcat_hip.hip (host code only).

#include <atomic>
#include <charconv>
#include <condition_variable>
#include <functional>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

// (struct qk::FqRec, one record of the file, is declared in pipeline.h beside ReadView, the pipeline's view of the reads)

struct qcat_fastq {
    int fd = -1;
    const uint8_t* data = nullptr;
    uint64_t size = 0;
    std::vector<qk::FqRec> recs;
    double parse_s = 0;
    bool fasta = false;                // plain two-line FASTA records ('>' title, one sequence line; FqRec::qual unused)
};

namespace qk {

// CPU seconds of the file loop's worker threads by stage (PIPELINE_TRACE prints them: the loop is bound by host CPU time
// under a container's CPU quota, not by any one stage's wall time)
static std::atomic<uint64_t> g_fq_cpu_split_ns{0}, g_fq_cpu_format_ns{0};
static inline uint64_t fq_thread_cpu_ns() {
    struct timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec : 0;
}
struct FqCpuScope {
    std::atomic<uint64_t>& sum; uint64_t t0;
    explicit FqCpuScope(std::atomic<uint64_t>& s) : sum(s), t0(fq_thread_cpu_ns()) {}
    ~FqCpuScope() { sum.fetch_add(fq_thread_cpu_ns() - t0, std::memory_order_relaxed); }
};

static inline const uint8_t* fq_nl(const uint8_t* p, const uint8_t* end) {
    return p < end ? static_cast<const uint8_t*>(memchr(p, '\n', (size_t)(end - p))) : nullptr;
}

// any byte a plain record line must not hold: blanks / control characters (<= ' ', which covers '\r' and '\t') or
// non-ASCII.  (a loop the compiler vectorises)
static inline bool fq_has_odd_byte(const uint8_t* p, size_t n) {
    unsigned acc = 0;
    for (size_t i = 0; i < n; ++i) acc |= (unsigned)(p[i] <= 0x20) | (unsigned)(p[i] >= 0x80);
    return acc != 0;
}
// title lines may hold blanks and tabs (name, comment), but no other control character and nothing non-ASCII
static inline bool fq_title_odd(const uint8_t* p, size_t n) {
    unsigned acc = 0;
    for (size_t i = 0; i < n; ++i) acc |= (unsigned)(p[i] < 0x20 && p[i] != '\t') | (unsigned)(p[i] >= 0x80);
    return acc != 0;
}

// the first byte of [p, end) that a sequence / quality line must not hold (<= ' ' or non-ASCII; the line's own '\n' is one);
// `end` when there is none.  One pass finds the end of the line AND proves the line plain (round 5: memchr + a second pass
// over the same bytes before; the splitter is a third of the file loop's CPU time).
#if defined(__x86_64__)
__attribute__((target("avx2"))) static const uint8_t* fq_first_odd_avx2(const uint8_t* p, const uint8_t* end) {
    const __m256i lim = _mm256_set1_epi8(0x20);
    while (p + 64 <= end) {
        // (signed compare: 0x21..0x7F are greater than 0x20, bytes from 0x80 are negative)
        const unsigned ok0 = (unsigned)_mm256_movemask_epi8(_mm256_cmpgt_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(p)), lim));
        const unsigned ok1 = (unsigned)_mm256_movemask_epi8(_mm256_cmpgt_epi8(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(p + 32)), lim));
        const uint64_t bad = ~(((uint64_t)ok1 << 32) | ok0);
        if (bad) return p + __builtin_ctzll(bad);
        p += 64;
    }
    for (; p < end; ++p) if (*p <= 0x20 || *p >= 0x80) return p;
    return end;
}
#endif
static inline const uint8_t* fq_first_odd(const uint8_t* p, const uint8_t* end) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return fq_first_odd_avx2(p, end);
#endif
    for (; p < end; ++p) if (*p <= 0x20 || *p >= 0x80) return p;
    return end;
}

// one plain record at p: fills r and returns the start of the next record (== end after the last one); nullptr when the
// record is not a plain four-line record
static inline const uint8_t* fq_parse(const uint8_t* base, const uint8_t* p, const uint8_t* end, FqRec* r) {
    if (p >= end || *p != '@') return nullptr;
    const uint8_t* l1 = fq_nl(p, end);
    if (!l1) return nullptr;
    const uint8_t* s = l1 + 1;
    const uint8_t* l2 = fq_first_odd(s, end);                            // the sequence line ends at its first odd byte: '\n' or not plain
    if (l2 >= end || *l2 != '\n') return nullptr;
    const uint8_t* pl = l2 + 1;
    if (pl >= end || *pl != '+') return nullptr;
    const uint8_t* l3 = fq_nl(pl, end);
    if (!l3) return nullptr;
    const uint8_t* q = l3 + 1;
    const size_t sl = (size_t)(l2 - s);
    if (sl == 0 || sl > 0x7FFFFFFFull || (size_t)(end - q) < sl) return nullptr;
    // as many quality bytes as bases, all plain, then the newline (or the end of the file)
    const uint8_t* qe = fq_first_odd(q, end);
    if (qe != q + sl || (qe < end && *qe != '\n')) return nullptr;
    const uint8_t* l4 = qe < end ? qe : nullptr;
    size_t tl = (size_t)(l1 - (p + 1));
    if (fq_title_odd(p + 1, tl)) return nullptr;
    while (tl && (p[tl] == ' ' || p[tl] == '\t')) --tl;                 // rstrip (p[tl] = last title byte)
    if (tl > 0xFFFFFFFFull) return nullptr;
    // the '+' line: alone, or followed by blanks, or by the same title
    size_t pll = (size_t)(l3 - (pl + 1));
    if (pll) {
        if (fq_title_odd(pl + 1, pll)) return nullptr;
        while (pll && (pl[pll] == ' ' || pl[pll] == '\t')) --pll;
        if (pll && (pll != tl || memcmp(pl + 1, p + 1, tl) != 0)) return nullptr;
    }
    r->title = (uint64_t)(p + 1 - base); r->title_len = (uint32_t)tl;
    r->seq = (uint64_t)(s - base); r->qual = (uint64_t)(q - base); r->seq_len = (uint32_t)sl;
    return l4 ? l4 + 1 : end;
}

// one plain FASTA record at p ('>' title line + ONE sequence line, round 4): fills r (qual = 0) and returns the start of the
// next record; nullptr for anything else -- a wrapped sequence, a blank line, an empty sequence, odd bytes -- which
// Biopython's SimpleFastaParser (qcat/cli.py:235-306) joins or strips in its own way: the Python parser takes the file
static inline const uint8_t* fa_parse(const uint8_t* base, const uint8_t* p, const uint8_t* end, FqRec* r) {
    if (p >= end || *p != '>') return nullptr;
    const uint8_t* l1 = fq_nl(p, end);
    if (!l1) return nullptr;
    const uint8_t* s = l1 + 1;
    const uint8_t* l2 = fq_nl(s, end);
    const uint8_t* se = l2 ? l2 : end;
    const size_t sl = (size_t)(se - s);
    if (sl == 0 || sl > 0x7FFFFFFFull || fq_has_odd_byte(s, sl)) return nullptr;
    const uint8_t* next = l2 ? l2 + 1 : end;
    if (next < end && *next != '>') return nullptr;                      // a second sequence line (or a blank one)
    size_t tl = (size_t)(l1 - (p + 1));
    if (fq_title_odd(p + 1, tl)) return nullptr;
    while (tl && (p[tl] == ' ' || p[tl] == '\t')) --tl;
    if (tl > 0xFFFFFFFFull) return nullptr;
    r->title = (uint64_t)(p + 1 - base); r->title_len = (uint32_t)tl;
    r->seq = (uint64_t)(s - base); r->qual = 0; r->seq_len = (uint32_t)sl;
    return next;
}
static inline const uint8_t* fa_find_start(const uint8_t* base, const uint8_t* from, const uint8_t* end) {
    const uint8_t* p = from;
    if (p != base) {
        const uint8_t* nl = fq_nl(p - 1, end);
        if (!nl) return end;
        p = nl + 1;
    }
    for (int tries = 0; p < end && tries < 64; ++tries) {
        FqRec a;
        if (*p == '>' && fa_parse(base, p, end, &a)) return p;
        const uint8_t* nl = fq_nl(p, end);
        if (!nl) return end;
        p = nl + 1;
    }
    return nullptr;
}

// a record start at or after `from`: a line that begins with '@', whose third line begins with '+', and whose successor
// (when there is one) is a record too.  A quality line may begin with '@' -- then its "third line" is a sequence or
// title line and does not begin with '+' unless the data is adversarial; the pieces' meeting points are checked anyway.
static inline const uint8_t* fq_find_start(const uint8_t* base, const uint8_t* from, const uint8_t* end) {
    const uint8_t* p = from;
    if (p != base) {                                                     // a line start: after the next newline
        const uint8_t* nl = fq_nl(p - 1, end);
        if (!nl) return end;
        p = nl + 1;
    }
    for (int tries = 0; p < end && tries < 64; ++tries) {
        FqRec a, b;
        const uint8_t* n1 = *p == '@' ? fq_parse(base, p, end, &a) : nullptr;
        if (n1 && (n1 >= end || fq_parse(base, n1, end, &b))) return p;
        const uint8_t* nl = fq_nl(p, end);
        if (!nl) return end;
        p = nl + 1;
    }
    return nullptr;                                                      // nothing that looks like a record nearby
}

static int fq_index(qcat_fastq* f, std::string* err) {
    const uint8_t* base = f->data;
    const uint8_t* end = base + f->size;
    f->recs.clear();
    if (f->size == 0) return 0;
    const bool fasta = base[0] == '>';                                   // (the driver decides by the first byte too, qcat/cli.py:248-262)
    f->fasta = fasta;
    auto parse = [&](const uint8_t* p, FqRec* r) { return fasta ? fa_parse(base, p, end, r) : fq_parse(base, p, end, r); };
    auto find_start = [&](const uint8_t* from) { return fasta ? fa_find_start(base, from, end) : fq_find_start(base, from, end); };
    const unsigned nt = std::max(1u, std::min<unsigned>(host_threads(), (unsigned)(f->size / (4u << 20)) + 1));
    std::vector<std::vector<FqRec>> part(nt);
    std::vector<const uint8_t*> first(nt, nullptr), last(nt, nullptr);
    std::vector<int> bad(nt, 0);
    auto work = [&](unsigned t) {
        const uint8_t* from = base + f->size * t / nt;
        const uint8_t* upto = base + f->size * (t + 1) / nt;
        const uint8_t* p = t == 0 ? base : find_start(from);
        if (!p) { bad[t] = 1; return; }
        first[t] = p;
        part[t].reserve((size_t)((upto - from) / 1200 + 16));
        while (p < upto && p < end) {
            FqRec r;
            const uint8_t* n = parse(p, &r);
            if (!n) { bad[t] = 1; return; }
            part[t].push_back(r);
            p = n;
        }
        last[t] = p;
    };
    {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
    bool ok = true;
    for (unsigned t = 0; t < nt && ok; ++t) ok = !bad[t] && (t + 1 == nt ? last[t] == end : last[t] == first[t + 1]);
    if (!ok) {
        // the pieces did not meet (or a record is not plain): one thread walks the file; a record that is not a plain
        // four-line record ends the attempt
        std::vector<FqRec> all;
        const uint8_t* p = base;
        while (p < end) {
            FqRec r;
            const uint8_t* n = parse(p, &r);
            if (!n) { *err = std::string(fasta ? "not a plain two-line FASTA file (record " : "not a plain four-line FASTQ file (record ") + std::to_string(all.size() + 1) + ")"; return QCAT_ERR_UNSUPPORTED; }
            all.push_back(r);
            p = n;
        }
        f->recs.swap(all);
        return 0;
    }
    size_t total = 0;
    for (auto& v : part) total += v.size();
    if (total > 0xFFFFFFF0ull) { *err = "more than 2^32 reads in one file"; return QCAT_ERR_UNSUPPORTED; }
    f->recs.reserve(total);
    for (auto& v : part) f->recs.insert(f->recs.end(), v.begin(), v.end());
    return 0;
}

// ---- writers -----------------------------------------------------------------------------------------------------------
// Python's repr(float) for the finite, non-negative doubles a barcode score can be: the shortest digits that round-trip,
// fixed notation with at least one decimal (scores lie in [0, 100]: never the exponent form)
static inline size_t fq_repr_double(double v, char* out) {
    auto r = std::to_chars(out, out + 40, v, std::chars_format::fixed);
    size_t n = (size_t)(r.ptr - out);
    bool dot = false;
    for (size_t i = 0; i < n; ++i) dot = dot || out[i] == '.';
    if (!dot) { out[n++] = '.'; out[n++] = '0'; }
    return n;
}

}  // namespace qk

extern "C" int qcat_fastq_open(const char* path, qcat_fastq** out, uint64_t* n_reads, uint64_t* n_bytes) {
    using namespace qk;
    if (!path || !out || !n_reads) return set_err(QCAT_ERR_ARG, "qcat_fastq_open: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    qcat_fastq* f = new qcat_fastq();
    f->fd = open(path, O_RDONLY);
    if (f->fd < 0) { delete f; return set_err(QCAT_ERR_ARG, std::string("qcat_fastq_open: cannot open ") + path); }
    struct stat st;
    if (fstat(f->fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(f->fd); delete f; return set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_open: not a regular file"); }
    f->size = (uint64_t)st.st_size;
    if (f->size) {
        void* m = mmap(nullptr, f->size, PROT_READ, MAP_PRIVATE, f->fd, 0);
        if (m == MAP_FAILED) { close(f->fd); delete f; return set_err(QCAT_ERR_NOMEM, "qcat_fastq_open: mmap failed"); }
        f->data = static_cast<const uint8_t*>(m);
        (void)madvise(m, f->size, MADV_SEQUENTIAL);
    }
    std::string err;
    const int rc = fq_index(f, &err);
    if (rc) {
        if (f->data) munmap(const_cast<uint8_t*>(f->data), f->size);
        close(f->fd);
        delete f;
        return set_err(rc, "qcat_fastq_open: " + err);
    }
    f->parse_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *out = f;
    *n_reads = f->recs.size();
    if (n_bytes) *n_bytes = f->size;
    return 0;
}

extern "C" void qcat_fastq_close(qcat_fastq* f) {
    if (!f) return;
    if (f->data) munmap(const_cast<uint8_t*>(f->data), f->size);
    if (f->fd >= 0) close(f->fd);
    delete f;
}

// (name offset, name length, sequence length) of read r -- for callers that want to look at the index (tests)
extern "C" int qcat_fastq_read_info(const qcat_fastq* f, uint64_t r, uint64_t* title_off, uint32_t* title_len, uint64_t* seq_off, uint32_t* seq_len) {
    if (!f || r >= f->recs.size()) return set_err(QCAT_ERR_ARG, "qcat_fastq_read_info: bad read index");
    const qk::FqRec& x = f->recs[r];
    if (title_off) *title_off = x.title;
    if (title_len) *title_len = x.title_len;
    if (seq_off) *seq_off = x.seq;
    if (seq_len) *seq_len = x.seq_len;
    return 0;
}

// ---- demultiplexing a mapped file -------------------------------------------------------------------------------------
namespace qk {

static inline bool fq_write_all(int fd, const char* p, size_t n) {
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= (size_t)w;
    }
    return true;
}

static inline void fq_append_uint(std::string& s, uint64_t v) {
    char buf[24];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    s.append(buf, (size_t)(r.ptr - buf));
}
static inline void fq_append_int(std::string& s, int64_t v) {
    char buf[24];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    s.append(buf, (size_t)(r.ptr - buf));
}

}  // namespace qk

namespace qk {

// ---- the writers of a demux call: blocks of reads formatted on the host threads, appended in file order ---------------------
// (qcat/cli.py:309-358, :408-442, :521-530).  One object per call; write_range() takes consecutive runs of reads -- whole
// files' blocks from qcat_fastq_demux, one segment at a time from qcat_fastq_demux_stream -- and the outputs continue where
// the previous run ended.
struct FqWriter {
    const DevKit& hk;
    const qcat_demux_opts* o;
    bool dual, simple, fasta, to_dir, write_reads;
    const std::string none_kit = "None";
    std::vector<std::string> kit_name;
    std::vector<std::vector<std::string>> bname, bid, bid2;
    std::vector<std::vector<int>> bnum, bnum2;
    // per-barcode files: every call's file is known by an INTEGER (round 6: a std::string key per read and a linear search over
    // the block's ~100 files with string compares was most of the writer's time -- 0.21 s per million reads where the box takes
    // the bytes in 0.04 s, tools/pagecache_write_probe.py).  file_names: the distinct file names ("none" first); key_of[t]:
    // (barcode[, second barcode]) of template t -> its file; descriptors and positions per file, opened at first use
    std::vector<std::string> file_names;
    std::vector<std::vector<int>> key_of;
    std::vector<int> file_fds;
    std::vector<off_t> file_pos;
    static constexpr uint32_t max_block = 16384;
    unsigned nthreads;
    // the bytes of a block: the TSV rows, the one-stream records, and per file of the per-barcode form a buffer that KEEPS its
    // memory from block to block (round 6: fresh strings per block grew by doubling through glibc's mmap threshold -- every block
    // paid page faults and zeroing for its 25 MB again; with an integer per file instead of a string key and a search, the
    // writer's 0.21 s per million reads -- the box takes the bytes in 0.04 s, tools/pagecache_write_probe.py -- are 0.0x s)
    struct BlockOut { std::string tsv, stream; std::vector<std::string> fbuf; std::vector<int> used; };
    std::vector<BlockOut> outs;
    struct Piece { int fd; const char* p; size_t n; off_t off; unsigned owner; };     // off < 0: no position, write() in order
    std::vector<Piece> pieces;
    std::vector<int> fresh_files;                                // descriptors opened in this round: emptied before anything is written
    off_t tsv_pos = -1, out_pos = -1;
    std::atomic<bool> io_ok{true};
    int io_errno = 0;                                            // (errno is per thread: the writer's is kept here)
    double t_write = 0, t_format = 0;                            // busy time of the writers; of which formatting (the rest: write calls)
    size_t max_id_len = 4, max_kit_len = 4;                      // longest barcode id / kit name of the tables ("none" / "None" at least)

    FqWriter(const DevKit& k, const qcat_demux_opts* opts, bool fasta_) : hk(k), o(opts), dual(k.mode == QCAT_MODE_DUAL), simple(k.mode == QCAT_MODE_SIMPLE), fasta(fasta_) {
        to_dir = o->out_dir != nullptr && o->out_dir[0];
        write_reads = to_dir || !o->tsv;                         // qcat/cli.py:553: `if out or not tsv`
        nthreads = std::max(1u, host_threads());
        outs.resize(nthreads);
    }
    static off_t position_of(int fd) {                           // where pwrite may go: the descriptor's offset, or -1
        if (fd < 0) return -1;
        if (fd <= 2) return -1;                                  // an inherited std stream may share its file description with another one
                                                                 // (`> f 2>&1`): explicit offsets would overwrite what that one logs
        const int fl = fcntl(fd, F_GETFL);
        if (fl < 0 || (fl & O_APPEND)) return -1;
        return lseek(fd, 0, SEEK_CUR);
    }
    int init() {
        if (!o->kit_name || !o->bc_name || !o->bc_id || (dual && !o->bc2_id)) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux: name tables missing");
        if (o->tsv && o->tsv_fd < 0) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux: tsv without a descriptor");
        if (write_reads && !to_dir && o->out_fd < 0) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux: no output descriptor");
        kit_name.resize((size_t)hk.nt); bname.resize((size_t)hk.nt); bid.resize((size_t)hk.nt); bid2.resize((size_t)hk.nt);
        bnum.resize((size_t)hk.nt); bnum2.resize((size_t)hk.nt);
        for (int t = 0; t < hk.nt; ++t) {
            kit_name[(size_t)t] = o->kit_name[t] ? o->kit_name[t] : "None";
            for (int b = 0; b < hk.tpl[t].sets[0].n; ++b) {
                bname[(size_t)t].push_back(o->bc_name[t][b]);
                bnum[(size_t)t].push_back(o->bc_id[t][b]);
                bid[(size_t)t].push_back(std::to_string(o->bc_id[t][b]));
            }
            if (dual) for (int b = 0; b < hk.tpl[t].sets[1].n; ++b) { bnum2[(size_t)t].push_back(o->bc2_id[t][b]); bid2[(size_t)t].push_back(std::to_string(o->bc2_id[t][b])); }
        }
        for (int t = 0; t < hk.nt; ++t) {
            max_kit_len = std::max(max_kit_len, kit_name[(size_t)t].size());
            size_t m1 = 0, m2 = 0;
            for (const std::string& v : bid[(size_t)t]) m1 = std::max(m1, v.size());
            for (const std::string& v : bid2[(size_t)t]) m2 = std::max(m2, v.size());
            max_id_len = std::max(max_id_len, m1 + 1 + m2);      // (dual: "<id>/<id2>")
        }
        tsv_pos = o->tsv ? position_of(o->tsv_fd) : -1;
        out_pos = (write_reads && !to_dir) ? position_of(o->out_fd) : -1;
        if (to_dir) {
            // the file of every possible call: "<barcode name>" (dual: "barcodeAA_BB", '/' is no file name), "none" for the rest
            std::map<std::string, int> ids;
            file_names.assign(1, "none"); ids["none"] = 0;
            key_of.resize((size_t)hk.nt);
            char num[48];
            for (int t = 0; t < hk.nt; ++t) {
                const size_t n0 = bnum[(size_t)t].size(), n1 = dual ? bnum2[(size_t)t].size() : 1;
                key_of[(size_t)t].assign(n0 * n1, 0);
                for (size_t b = 0; b < n0; ++b)
                    for (size_t b2 = 0; b2 < n1; ++b2) {
                        std::string key;
                        if (dual) { snprintf(num, sizeof num, "barcode%02d/%02d", bnum[(size_t)t][b], bnum2[(size_t)t][b2]); key = num; }
                        else key = bname[(size_t)t][b];
                        for (char& ch : key) if (ch == '/') ch = '_';
                        auto it = ids.find(key);
                        if (it == ids.end()) { it = ids.emplace(key, (int)file_names.size()).first; file_names.push_back(key); }
                        key_of[(size_t)t][b * n1 + b2] = it->second;
                    }
            }
            file_fds.assign(file_names.size(), -1);
            file_pos.assign(file_names.size(), 0);
            for (BlockOut& bo : outs) bo.fbuf.resize(file_names.size());
        }
        return 0;
    }
    // a call needs every index inside the caller's tables (k_finalize never writes a first barcode without the second in dual
    // mode; an index outside a table is treated as "not called" rather than read past the table)
    // (simple mode: no adapter -- a record is called when it names a barcode with adapter_idx == -1; names and ids come from
    // template 0, the one list, and the TSV kit column reads "None" as cli.tsv_row prints `result["adapter"] is None`)
    inline size_t tpl_of(const qcat_result& q) const { return simple ? 0 : (size_t)q.adapter_idx; }
    inline bool called(const qcat_result& q) const {
        if (simple ? !(q.barcode_idx >= 0 && q.adapter_idx == -1) : !(q.barcode_idx >= 0 && q.adapter_idx >= 0 && q.adapter_idx < hk.nt)) return false;
        const size_t t = tpl_of(q);
        return (size_t)q.barcode_idx < bnum[t].size() && (!dual || (q.barcode2_idx >= 0 && (size_t)q.barcode2_idx < bnum2[t].size()));
    }
    // formats and writes `cnt` consecutive reads (records x[], results res[], flags skipped[], bytes at `data`): `nthreads`
    // blocks at a time in parallel, appended in file order
    void write_range(const uint8_t* data, const FqRec* xs, const qcat_result* res, uint8_t* skipped, uint64_t cnt) {
      const auto t_w0 = std::chrono::steady_clock::now();
      // blocks of at most 16384 reads, small enough that a run of reads (a segment of the streamed loop: ~125 k reads) keeps every
      // host thread busy (round 6: eight blocks per segment left half of the 16 threads idle through the formatting)
      const uint32_t block = (uint32_t)std::min<uint64_t>(max_block, std::max<uint64_t>(1024, ((cnt + nthreads - 1) / nthreads + 1023) / 1024 * 1024));
      const uint64_t n_blocks = (cnt + block - 1) / block;
      for (uint64_t b0 = 0; b0 < n_blocks && io_ok; b0 += nthreads) {
        const unsigned nb = (unsigned)std::min<uint64_t>(nthreads, n_blocks - b0);
        auto work = [&](unsigned k) {
          FqCpuScope cpu(g_fq_cpu_format_ns);
          try {
            BlockOut& bo = outs[k];
            bo.tsv.clear(); bo.stream.clear();
            for (int fidx : bo.used) bo.fbuf[(size_t)fidx].clear();          // (clear() keeps the capacity)
            bo.used.clear();
            const uint64_t r0 = (b0 + k) * block, r1 = std::min<uint64_t>(cnt, r0 + block);
            std::string dual_name, dual_id;
            char num[48];
            // TSV rows go through a raw cursor into a buffer sized for the longest rows this block can have: the title, two
            // numbers of at most 20 digits, the longest barcode id and kit name, a score of at most 40 characters, separators
            char* tsv_w = nullptr;
            constexpr uint32_t SCORE_CACHE = 256;
            struct ScoreText { uint32_t key = 0; uint8_t len = 0; char text[43]; };
            ScoreText score_cache[SCORE_CACHE];
            if (o->tsv) {
                size_t bound = 0;
                for (uint64_t r = r0; r < r1; ++r) bound += xs[r].title_len;
                bound += (size_t)(r1 - r0) * (size_t)(20 + 20 + 40 + 16 + max_id_len + max_kit_len);
                bo.tsv.resize(bound);
                tsv_w = bo.tsv.data();
            }
            for (uint64_t r = r0; r < r1; ++r) {
                const FqRec& x = xs[r];
                const qcat_result& q = res[r];
                const char* title = reinterpret_cast<const char*>(data + x.title);
                // (the records lie ~1.5 KB apart in the mapped file: each title is a cache miss the prefetcher does not see)
                if (r + 8 < r1) __builtin_prefetch(data + xs[r + 8].title);
                // name / comment: split at the first blank, tabs count as blanks (cli.py:200-214)
                uint32_t nl = 0;
                while (nl < x.title_len && title[nl] != ' ' && title[nl] != '\t') ++nl;
                const bool has_comment = nl < x.title_len;
                uint64_t s0 = 0, s1 = x.seq_len;
                if (o->trim) {                                   // Python slice semantics of sequence[trim5p:trim3p]
                    s0 = std::min<uint64_t>((uint64_t)std::max(q.trim5p, 0), x.seq_len);
                    s1 = std::min<uint64_t>((uint64_t)std::max(q.trim3p, 0), x.seq_len);
                    if (s1 < s0) s1 = s0;
                }
                const uint64_t slen = s1 - s0;
                if ((int64_t)slen < (int64_t)o->min_read_length) { skipped[r] = 1; continue; }
                skipped[r] = 0;
                const bool called = this->called(q);
                const std::string* name_s = nullptr; const std::string* id_s = nullptr;
                if (called) {
                    const size_t t = tpl_of(q);
                    if (dual) {
                        const int a = bnum[t][(size_t)q.barcode_idx], b2 = bnum2[t][(size_t)q.barcode2_idx];
                        snprintf(num, sizeof num, "barcode%02d/%02d", a, b2);
                        dual_name = num;
                        dual_id = bid[t][(size_t)q.barcode_idx] + "/" + bid2[t][(size_t)q.barcode2_idx];
                        name_s = &dual_name; id_s = &dual_id;
                    } else {
                        name_s = &bname[t][(size_t)q.barcode_idx]; id_s = &bid[t][(size_t)q.barcode_idx];
                    }
                }
                auto append_comment = [&](std::string& s) {      // tabs of the title's comment part become blanks
                    const size_t at = s.size();
                    s.append(title + nl + 1, x.title_len - nl - 1);
                    for (size_t i = at; i < s.size(); ++i) if (s[i] == '\t') s[i] = ' ';
                };
                if (o->tsv) {
                    // one row through a raw cursor: the block's buffer was sized for its longest possible rows above
                    char* w = tsv_w;
                    memcpy(w, title, nl); w += nl; *w++ = '\t';
                    w = std::to_chars(w, w + 20, slen).ptr; *w++ = '\t';
                    if (called) {
                        memcpy(w, id_s->data(), id_s->size()); w += id_s->size(); *w++ = '\t';
                        // repr(float) of raw * 100.0 / (1.0 * den): a few dozen distinct (raw, den) pairs per kit -- their text is kept
                        const uint32_t key = ((uint32_t)(uint16_t)q.raw_score << 16) | (uint16_t)q.score_den;
                        ScoreText& st = score_cache[(key ^ (key >> 13)) & (SCORE_CACHE - 1)];
                        if (st.key != key || !st.len) {
                            const double score = (double)(int)q.raw_score * 100.0 / (1.0 * (double)(int)q.score_den);
                            st.len = (uint8_t)fq_repr_double(score, st.text); st.key = key;
                        }
                        memcpy(w, st.text, st.len); w += st.len; *w++ = '\t';
                        const std::string& kn = simple ? none_kit : kit_name[(size_t)q.adapter_idx];
                        memcpy(w, kn.data(), kn.size()); w += kn.size(); *w++ = '\t';
                        w = std::to_chars(w, w + 20, (int64_t)q.adapter_end).ptr; *w++ = '\t';
                    } else {
                        memcpy(w, "none\t-1\tnone\t-1\t", 16); w += 16;
                    }
                    if (has_comment) {
                        const uint32_t cl = x.title_len - nl - 1;
                        const char* cs = title + nl + 1;
                        for (uint32_t i = 0; i < cl; ++i) w[i] = cs[i] == '\t' ? ' ' : cs[i];       // tabs of the comment become blanks
                        w += cl;
                    } else { memcpy(w, "None", 4); w += 4; }
                    *w++ = '\n';
                    tsv_w = w;
                }
                if (write_reads) {
                    std::string* dst;
                    if (to_dir) {
                        const int file = !called ? 0 : key_of[tpl_of(q)][(size_t)q.barcode_idx * (dual ? bnum2[(size_t)q.adapter_idx].size() : 1)
                                                                                     + (size_t)(dual ? q.barcode2_idx : 0)];
                        dst = &bo.fbuf[(size_t)file];
                        if (dst->empty()) bo.used.push_back(file);
                    } else dst = &bo.stream;
                    std::string& s = *dst;
                    s.push_back(fasta ? '>' : '@'); s.append(title, nl); s.push_back(' ');
                    if (has_comment) append_comment(s);
                    if (!to_dir) { s.append(" barcode="); if (called) s.append(*id_s); else s.append("none"); }
                    s.push_back('\n');
                    s.append(reinterpret_cast<const char*>(data + x.seq + s0), slen);
                    if (!fasta) {                                 // (FASTA in, FASTA out: qcat/cli.py:340-346)
                        s.append("\n+\n");
                        s.append(reinterpret_cast<const char*>(data + x.qual + s0), slen);
                    }
                    s.push_back('\n');
                }
            }
            if (o->tsv) bo.tsv.resize((size_t)(tsv_w - bo.tsv.data()));
          } catch (const std::exception&) { io_errno = ENOMEM; io_ok = false; }      // (a thread must not let an exception escape)
        };
        const auto t_f0 = std::chrono::steady_clock::now();
        {
            std::vector<std::thread> th;
            for (unsigned k = 1; k < nb; ++k) th.emplace_back(work, k);
            work(0);
            for (auto& x : th) x.join();
        }
        t_format += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_f0).count();
        // every piece gets its place in its file in block order; pieces of positionable files are then written side by side
        // (pwrite), the rest -- a pipe, a terminal, an O_APPEND descriptor -- in order
        pieces.clear();
        fresh_files.clear();
        for (unsigned k = 0; k < nb && io_ok; ++k) {
            BlockOut& bo = outs[k];
            if (!bo.tsv.empty()) { pieces.push_back(Piece{o->tsv_fd, bo.tsv.data(), bo.tsv.size(), tsv_pos, k}); if (tsv_pos >= 0) tsv_pos += (off_t)bo.tsv.size(); }
            if (!bo.stream.empty()) { pieces.push_back(Piece{o->out_fd, bo.stream.data(), bo.stream.size(), out_pos, k}); if (out_pos >= 0) out_pos += (off_t)bo.stream.size(); }
            for (int fidx : bo.used) {
                const size_t i = (size_t)fidx;
                const std::string& buf = bo.fbuf[i];
                if (file_fds[i] < 0) {
                    // (opened here, emptied below on the host threads: a file left by an earlier run holds page cache whose
                    // release is the kernel's work in whoever truncates it -- 1.5 GB of it were 130 ms of this one thread)
                    const std::string path = std::string(o->out_dir) + "/" + file_names[i] + (fasta ? ".fasta" : ".fastq");
                    const int fd = open(path.c_str(), O_WRONLY | O_CREAT, 0666);
                    if (fd < 0) { io_ok = false; io_errno = errno; break; }
                    file_fds[i] = fd;
                    fresh_files.push_back(fd);
                }
                pieces.push_back(Piece{file_fds[i], buf.data(), buf.size(), file_pos[i], k});
                file_pos[i] += (off_t)buf.size();
            }
        }
        if (io_ok && !fresh_files.empty()) {
            std::atomic<size_t> next{0};
            std::atomic<int> bad{0};
            auto empty_them = [&] {
                for (size_t i = next.fetch_add(1); i < fresh_files.size(); i = next.fetch_add(1)) {
                    // (only a file that holds something: ext4 marks EVERY file truncated to zero for allocation and write-back at
                    // close -- "replace via truncate", auto_da_alloc -- the newly created ones included)
                    struct stat fst;
                    if (fstat(fresh_files[i], &fst) == 0 && fst.st_size == 0) continue;
                    if (ftruncate(fresh_files[i], 0) != 0) { int z = 0; bad.compare_exchange_strong(z, errno ? errno : EIO); }
                }
            };
            std::vector<std::thread> th;
            for (unsigned k = 1; k < std::min<size_t>(nthreads, fresh_files.size()); ++k) th.emplace_back(empty_them);
            empty_them();
            for (auto& x : th) x.join();
            if (bad.load()) { io_ok = false; io_errno = bad.load(); }
        }
        if (io_ok) {
            for (const Piece& pc : pieces)                          // in order first: the descriptors without positions
                if (pc.off < 0 && io_ok) { io_ok = fq_write_all(pc.fd, pc.p, pc.n); if (!io_ok) io_errno = errno; }
            std::atomic<int> bad{0};
            // (every block holds its files in much the same order: thread k starts a k-th of the way through its pieces, or all
            // threads would queue at the same file's inode lock, one file after the other)
            std::vector<size_t> first_of(nb + 1, pieces.size());
            for (size_t i = pieces.size(); i-- > 0;) first_of[pieces[i].owner] = i;
            auto put = [&](unsigned k) {
                size_t lo = first_of[k], hi = lo;
                while (hi < pieces.size() && pieces[hi].owner == k) ++hi;
                const size_t cnt_k = hi - lo, start = cnt_k ? (size_t)k * cnt_k / nb : 0;
                for (size_t q = 0; q < cnt_k; ++q) {
                    const Piece& pc = pieces[lo + (start + q) % cnt_k];
                    if (pc.off < 0) continue;
                    size_t done = 0;
                    while (done < pc.n) {
                        const ssize_t w = pwrite(pc.fd, pc.p + done, pc.n - done, pc.off + (off_t)done);
                        if (w < 0) { if (errno == EINTR) continue; int z = 0; bad.compare_exchange_strong(z, errno ? errno : EIO); return; }
                        done += (size_t)w;
                    }
                }
            };
            std::vector<std::thread> th;
            for (unsigned k = 1; k < nb; ++k) th.emplace_back(put, k);
            put(0);
            for (auto& x : th) x.join();
            if (bad.load()) { io_ok = false; io_errno = bad.load(); }
        }
      }
      t_write += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_w0).count();
    }
    void finish() {
        if (opt_on(QO_PIPELINE_TRACE))
            fprintf(stderr, "[qcat] writers: %.1f ms busy, %.1f ms of it formatting; CPU seconds of the worker threads so far in this process: splitting %.3f, formatting %.3f, compaction %.3f\n",
                    t_write * 1e3, t_format * 1e3, (double)g_fq_cpu_split_ns.load() * 1e-9, (double)g_fq_cpu_format_ns.load() * 1e-9,
                    (double)g_host_pool_cpu_ns.load() * 1e-9);
        // the per-barcode files are closed BEHIND the call, on a thread of their own: every byte is in the page cache when the call
        // returns, close() only gives the descriptors back -- but a file that existed before the run was emptied and rewritten, and
        // ext4 allocates and starts writing such a file back at close ("replace via truncate", auto_da_alloc): 1.5 ms per file,
        // 100-150 ms behind a million reads (round 6 timeline, tools/pagecache_write_probe.py).  Nothing of the writer is touched
        // by that thread; a process that exits first has its descriptors closed by the kernel.
        {
            std::vector<int> open_fds;
            for (int& fd : file_fds) if (fd >= 0) { open_fds.push_back(fd); fd = -1; }
            if (!open_fds.empty()) {
                try { std::thread([fds = std::move(open_fds)] { for (int fd : fds) (void)close(fd); }).detach(); }
                catch (const std::exception&) { for (int fd : open_fds) (void)close(fd); }
            }
        }
        if (tsv_pos >= 0) (void)lseek(o->tsv_fd, tsv_pos, SEEK_SET);    // the caller's descriptors go on after what was written
        if (out_pos >= 0) (void)lseek(o->out_fd, out_pos, SEEK_SET);
    }
};

// --filter-barcodes (qcat/scanner_base.py:690-712, :730-731): per batch of the driver's loop (cli.py:500-513) the calls are
// counted by Barcode.id -- a read without a barcode counts under "0" --, a barcode is valid when its count exceeds
// int(0.05 * the largest count), and a result whose barcode is not valid becomes empty_return_dict() (:393-407: no barcode,
// no adapter, exit status 1, trim5p = trim3p = 0).  res[0 .. cnt) = ONE batch.
static inline void fq_filter_batch(const FqWriter& w, qcat_result* res, uint64_t cnt) {
    std::map<uint64_t, uint64_t> count;                          // key: id (dual: both ids); ~0: none
    auto key_of = [&](const qcat_result& q) -> uint64_t {
        if (!w.called(q)) return ~0ull;
        const size_t t = w.tpl_of(q);
        const uint64_t a = (uint32_t)w.bnum[t][(size_t)q.barcode_idx];
        return w.dual ? (a << 32) | (uint32_t)w.bnum2[t][(size_t)q.barcode2_idx] : a;
    };
    for (uint64_t r = 0; r < cnt; ++r) ++count[key_of(res[r])];
    uint64_t mx = 0;
    for (const auto& kv : count) mx = std::max(mx, kv.second);
    const uint64_t min_count = (uint64_t)((double)mx * 0.05);     // int(max_barcode_count * min_perc)
    for (uint64_t r = 0; r < cnt; ++r) {
        qcat_result& q = res[r];
        const uint64_t k = key_of(q);
        if (k == ~0ull || count[k] > min_count) continue;
        q.barcode_idx = -1; q.barcode2_idx = -1; q.adapter_idx = -1; q.adapter_end = 0; q.raw_score = 0; q.score_den = 1;
        q.exit_status = 1; q.trim5p = 0; q.trim3p = 0;
    }
}

}  // namespace qk

extern "C" int qcat_fastq_demux(qcat_fastq* f, qcat_ctx* c, const qcat_kit* ckit, const qcat_demux_opts* o,
                                qcat_result* recs, uint8_t* skipped, qcat_demux_stats* stats) {
    using namespace qk;
    if (!f || !c || !ckit || !o || !recs || !skipped) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux: null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& hk = kit->hk.dk;
    if (hk.mode == QCAT_MODE_SIMPLE && o->kit_auto) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux: simple mode has no kits to vote for (kit_auto must be 0)");
    if (hk.ends != QCAT_ENDS_BOTH) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux needs a kit created with QCAT_ENDS_BOTH");
    const uint64_t n = f->recs.size();
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    FqWriter w(hk, o, f->fasta);
    if (int wrc = w.init()) return wrc;
    std::atomic<bool>& io_ok = w.io_ok;
    const uint32_t block = FqWriter::max_block;
    const uint64_t n_blocks = (n + block - 1) / block;
    auto write_blocks = [&](uint64_t blk0, uint64_t blk1) {
        const uint64_t r0 = blk0 * block, r1 = std::min<uint64_t>(n, blk1 * block);
        if (r1 > r0) w.write_range(f->data, f->recs.data() + r0, recs + r0, skipped + r0, r1 - r0);
    };
    // --filter-barcodes works on whole batches of the driver's loop: the reads up to the last complete batch of what has been
    // scanned are filtered (once) and may then go to the writer
    const uint64_t fbatch = (uint64_t)std::max(1, o->batch_size);
    uint64_t filtered = 0;
    auto filter_upto = [&](uint64_t upto) -> uint64_t {
        if (!o->filter_barcodes) return upto;
        while (filtered < upto) {
            const uint64_t end = std::min<uint64_t>(n, filtered + fbatch);
            if (end > upto) break;
            fq_filter_batch(w, recs + filtered, end - filtered);
            filtered = end;
        }
        return filtered;
    };
    // ---- the writer runs beside the scan: it takes whole blocks of scanned reads as the scan publishes them -------------
    std::mutex wmu;
    std::condition_variable wcv;
    uint64_t scanned = 0;                                        // reads [0, scanned) have their records
    bool scan_over = false;
    auto publish = [&](uint64_t upto, bool over) {
        { std::lock_guard<std::mutex> lk(wmu); if (over) scan_over = true; else scanned = filter_upto(upto); }
        wcv.notify_all();
    };
    std::thread writer([&] {
        uint64_t done_blocks = 0;
        try {
        for (;;) {
            uint64_t upto; bool over;
            {
                std::unique_lock<std::mutex> lk(wmu);
                wcv.wait(lk, [&] { return scan_over || scanned / block > done_blocks; });
                upto = scanned; over = scan_over;
            }
            const uint64_t end_blocks = over && upto == n ? n_blocks : upto / block;     // (a scan that failed leaves the tail unwritten)
            if (end_blocks > done_blocks) { write_blocks(done_blocks, end_blocks); done_blocks = end_blocks; }
            if (over) break;
        }
        } catch (const std::exception&) { w.io_errno = ENOMEM; io_ok = false; }     // (bad_alloc while formatting: reported as a failed write)
    });
    // the writer is joined on EVERY way out of this function (an exception of the scan side -- the vectors below can throw
    // bad_alloc -- would otherwise unwind past a joinable thread: std::terminate)
    struct JoinWriter {
        std::thread& t; std::function<void()> stop;
        ~JoinWriter() { if (t.joinable()) { stop(); t.join(); } }
    } join_writer{writer, [&] { publish(0, true); }};
    const double t_scan0 = now();
    // ---- scan --------------------------------------------------------------------------------------------------------
    int rc = 0;
    try {
    std::vector<const uint8_t*> one_ptrs;                        // the one-shot path: the reads where they lie in the mapping
    std::vector<uint64_t> one_lens;
    if (o->kit_auto) {
        // the reference votes per batch of `batch_size` reads in file order (qcat/cli.py:500, scanner_base.py:714-733).  Round 3
        // made one call per batch -- 0.9 ms for 4000 reads whose kernels are latency-bound: 4.5 M reads/s whatever the
        // device.  Round 4: CHUNKS of up to 64 batches per call (qcat_scan_batches_auto_ptrs: one adapter pass over the
        // chunk, the votes counted and decided per batch on the device, every read scanned with its own batch's kit), the
        // reads handed over as pointers into the mapping, and -- for big files -- two workers with a context each (stream, staging,
        // captured graph) so that one chunk is compacted on the host while another is on the device; the records land in
        // file order and are published to the writer as the prefix of finished chunks grows.
        // QCAT_HIP_AUTO_WORKERS=<n>, QCAT_HIP_AUTO_CHUNK=<batches per call> (1 + 1: the loop of round 3).
        const uint32_t bs = (uint32_t)std::max(1, o->batch_size);
        const QOptVal cenv = qopt_get(QO_AUTO_CHUNK);
        uint64_t chunk_batches = cenv ? (uint64_t)std::max(1, atoi(cenv)) : 64;
        chunk_batches = std::min<uint64_t>(chunk_batches, std::max<uint64_t>(1, (1u << 20) / bs));   // (a million reads per call at most)
        const uint64_t chunk_reads = chunk_batches * bs;
        const uint64_t n_chunks = (n + chunk_reads - 1) / chunk_reads;
        const QOptVal wenv = qopt_get(QO_AUTO_WORKERS);
        // (a helper context costs ~80 ms of set-up -- pinned staging and device buffers for a 256 k-read chunk -- and a second
        // worker saves ~7 ms per million reads: one worker below 8 M reads, two from there; tools/bench_auto_file.py)
        unsigned workers = wenv ? (unsigned)std::max(1, atoi(wenv)) : (n >= (8u << 20) && host_threads() > 1 ? 2u : 1u);
        workers = (unsigned)std::min<uint64_t>(workers, std::max<uint64_t>(1, n_chunks));
        while (c->helpers.size() + 1 < workers) {
            qcat_ctx* h = nullptr;
            if (qcat_ctx_create(c->device, &h) != 0) { workers = (unsigned)c->helpers.size() + 1; break; }
            c->helpers.push_back(h);
        }
        std::atomic<uint64_t> next_chunk{0};
        std::atomic<int> first_rc{0};
        std::mutex pmu;                                          // the published prefix, the first error's text
        std::vector<uint8_t> finished((size_t)n_chunks, 0);
        uint64_t prefix = 0;
        std::string first_err;
        auto work = [&](qcat_ctx* wc) {
            std::vector<const uint8_t*> ptrs;
            std::vector<uint64_t> lens;
            std::vector<int32_t> slots;
            try {
                const size_t cap = (size_t)std::min<uint64_t>(chunk_reads, n);
                ptrs.resize(cap); lens.resize(cap); slots.resize((size_t)chunk_batches);
                for (;;) {
                    if (first_rc.load() != 0 || !io_ok) return;  // (a failed scan or write ends the other workers too)
                    const uint64_t ch = next_chunk.fetch_add(1);
                    if (ch >= n_chunks) return;
                    const uint64_t first = ch * chunk_reads;
                    const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk_reads, n - first);
                    for (uint32_t r = 0; r < cnt; ++r) {
                        const auto& x = f->recs[first + r];
                        ptrs[r] = f->data + x.seq; lens[r] = x.seq_len;
                    }
                    const int wrc = qcat_scan_batches_auto_ptrs(wc, kit, ptrs.data(), lens.data(), cnt, bs, recs + first, nullptr, slots.data());
                    std::lock_guard<std::mutex> lk(pmu);
                    if (wrc) {
                        int expected = 0;
                        if (first_rc.compare_exchange_strong(expected, wrc)) first_err = qcat_last_error();
                        return;
                    }
                    finished[(size_t)ch] = 1;
                    const uint64_t before = prefix;
                    while (prefix < n_chunks && finished[(size_t)prefix]) ++prefix;
                    if (prefix > before) publish(std::min<uint64_t>(n, prefix * chunk_reads), false);
                }
            } catch (const std::bad_alloc&) {
                std::lock_guard<std::mutex> lk(pmu);
                int expected = 0;
                if (first_rc.compare_exchange_strong(expected, (int)QCAT_ERR_NOMEM)) first_err = "qcat_fastq_demux: out of host memory";
            }
        };
        {
            std::vector<std::thread> pool;
            struct JoinPool { std::vector<std::thread>& p; ~JoinPool() { for (auto& t : p) if (t.joinable()) t.join(); } } join_pool{pool};
            for (unsigned w = 1; w < workers; ++w) {
                try { pool.emplace_back(work, c->helpers[w - 1]); }
                catch (const std::exception&) { break; }          // no more threads: fewer workers
            }
            work(c);
        }
        if ((rc = first_rc.load())) (void)set_err(rc, first_err);
    } else {
        // segments of about a million reads (whole writer blocks): the writers format segment k while segment k + 1 is scanned
        const uint64_t n_seg = std::max<uint64_t>(1, (n + (1u << 20) - 1) >> 20);
        const uint32_t chunk = (uint32_t)(((n + n_seg - 1) / n_seg + block - 1) / block * block);
        for (uint64_t first = 0; first < n && !rc && io_ok; first += chunk) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, n - first);
            const ReadView rv{f->data, nullptr, f->recs.data() + first};
            rc = scan_batch_pipelined(c, kit, rv, cnt, recs + first, nullptr);
            if (rc == 1) {                                       // small batch / --detect-middle: the one-shot path
                one_ptrs.resize(cnt); one_lens.resize(cnt);
                for (uint32_t r = 0; r < cnt; ++r) { one_ptrs[r] = f->data + f->recs[first + r].seq; one_lens[r] = f->recs[first + r].seq_len; }
                rc = scan_debug_impl(c, kit, nullptr, nullptr, one_ptrs.data(), one_lens.data(), cnt, recs + first, nullptr, nullptr, nullptr, 0);
            }
            if (!rc) publish(first + cnt, false);
        }
    }
    } catch (const std::bad_alloc&) { rc = set_err(QCAT_ERR_NOMEM, "qcat_fastq_demux: out of host memory"); }
    const double t_scan1 = now();
    publish(0, true);                                            // (the last published count stands)
    writer.join();
    w.finish();
    if (rc) return rc;
    if (!io_ok) return set_err(QCAT_ERR_IO, std::string("qcat_fastq_demux: write failed: ") + strerror(w.io_errno));
    if (stats) {
        stats->n_reads = n; stats->file_bytes = f->size; stats->next_offset = f->size; stats->incomplete = 0; stats->segments = 1;
        stats->parse_s = f->parse_s; stats->scan_s = t_scan1 - t_scan0; stats->write_s = w.t_write; stats->total_s = now() - t_scan0;
        uint64_t sk = 0;
        for (uint64_t r = 0; r < n; ++r) sk += skipped[r];
        stats->n_skipped = sk;
    }
    return 0;
}

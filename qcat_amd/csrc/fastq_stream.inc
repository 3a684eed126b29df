// fastq_stream.inc -- the driver's per-file loop over a file of ANY size in bounded memory (round 5).
//
// The reference streams: iter_fastx yields one batch of 4000 reads at a time (qcat/cli.py:235-306), the loop scans it and
// writes it (:500-552), and nothing of a batch outlives its iteration.  qcat_fastq_open / qcat_fastq_demux (fastq_host.inc)
// index the WHOLE file first -- 57 bytes of host memory per read and no scan before the last record is split.  This is the
// same flow as a three-stage pipeline over SEGMENTS of the file:
//
//   reader   (own thread + the host threads)  maps the next ~256 MB of the file (a window that is unmapped again once the
//            segment is written: nothing grows with the file; MADV_POPULATE_READ per splitting thread instead of a fault per
//            64 KB; pread() into reused buffers is the other reader, measured slower), splits it
//            into plain records on all host threads (the parser of fastq_host.inc), cuts the segment at the last whole
//            BATCH of the driver's loop (kit vote and --filter-barcodes work on batches counted from the start of the file;
//            the bytes behind the cut are carried into the next segment)
//   scan     (the caller's thread)            the chunked pipeline of qcat_scan_batch reading heads and tails in place in the
//            segment buffer (fixed kit), or qcat_scan_batches_auto_ptrs over chunks of 64 batches (kit auto), whole reads
//            for --detect-middle; then the per-batch barcode filter
//   writer   (own thread + the host threads)  the writers of fastq_host.inc (FqWriter), then the histogram of the kept reads
//
// segment k + 1 is read and split while segment k is scanned and segment k - 1 is written.  Host memory: three segment
// buffers with their indices and records, whatever the size of the file.
// A record that is not a plain four-line FASTQ / two-line FASTA record ends the native loop at the start of ITS segment (a
// batch boundary): everything before has been written, the caller gets the file offset and carries on with its own parser
// (in the first segment: QCAT_ERR_UNSUPPORTED before anything is written, as qcat_fastq_open answers).
// Included by qcat_hip.hip after fastq_host.inc (host code only).

namespace qk {

enum { FQ_OK = 0, FQ_INCOMPLETE = 1, FQ_BAD = 2 };
constexpr int FQ_DEFAULT_READER = 2;          // 1: pread into reused buffers, 2: a mapped window per segment (qcat_demux_opts.stream_reader).
                                              // Measured on the GPU box (16 host threads, 1.5 GB file in the page cache, tools/bench_stream.py,
                                              // profiles/r05_bench_stream.json): reader stage alone 43 ms with windows of 256 MB (35 GB/s: what
                                              // qcat_fastq_open takes for its whole-file index) against 108-148 ms through pread (the kernel's
                                              // copy is the slower way to touch the page cache), 58 / 50 ms with windows of 64 / 128 MB

// fq_parse / fa_parse with the reason of a failure: FQ_INCOMPLETE when the record runs into `end` and `end` is not the end
// of the file (more bytes will follow), FQ_BAD when it is not a plain record
static inline const uint8_t* fq_parse_st(bool fasta, const uint8_t* base, const uint8_t* p, const uint8_t* end, bool at_eof, FqRec* r, int* st) {
    *st = FQ_OK;
    const uint8_t* n = fasta ? fa_parse(base, p, end, r) : fq_parse(base, p, end, r);
    if (n) {
        if (at_eof || n < end) return n;
        // the record ends exactly at `end`: without its newline it is complete only at the end of the file, and a FASTA record
        // needs the first byte of the next line as well
        if (!fasta && end[-1] == '\n') return n;
        *st = FQ_INCOMPLETE;
        return nullptr;
    }
    if (at_eof) { *st = FQ_BAD; return nullptr; }
    // fewer newlines than a record has before `end`: incomplete; otherwise the lines are all there and the record is bad
    const int need = fasta ? 2 : 4;
    const uint8_t* q = p;
    int lines = 0;
    while (lines < need) {
        const uint8_t* nl = fq_nl(q, end);
        if (!nl) break;
        ++lines; q = nl + 1;
    }
    if (lines < need || (fasta && q >= end)) { *st = FQ_INCOMPLETE; return nullptr; }
    *st = FQ_BAD;
    return nullptr;
}

struct FqSeg {
    uint8_t* buf = nullptr;
    size_t cap = 0, len = 0;            // bytes [0, len) of buf = the file's bytes [file_off, file_off + len)
    uint64_t file_off = 0;
    std::vector<FqRec> recs;            // the complete plain records of the buffer (offsets into buf)
    uint64_t n_use = 0;                 // the reads of this round: whole batches, or all of them at the end of the file
    size_t used_bytes = 0;              // ... and their bytes; [used_bytes, len) is carried into the next segment
    uint64_t first_read = 0;            // index of recs[0] in the file
    bool eof = false, bad = false;
    std::vector<qcat_result> res;
    std::vector<uint8_t> skipped;
    int state = 0;                      // 0 free, 1 loaded, 2 scanned
    // round 6: a segment whose records are not all plain -- wrapped sequence / quality lines, \r\n, blank lines, trailing blanks --
    // is rewritten into `norm` as plain records (fq_seg_normalize: Biopython's rules, qcat/cli.py:235-306) and `recs` points into
    // THAT; data() is what the scan and the writers read.  buf / len / used_bytes keep describing the file's own bytes (the carry).
    std::vector<uint8_t> norm;
    std::vector<uint64_t> norm_end;     // per record of a normalised segment: the offset in buf right behind it
    const uint8_t* data() const { return norm.empty() ? buf : norm.data(); }
    bool mapped = false;                // mapped reader: buf points into the reader's mapping of the file (else buf is malloc'd)
    // a mapped segment that has been written gives its pages back: MADV_DONTNEED takes the address-space lock for reading only,
    // so the page faults of the splitting and writing threads go on beside it -- a munmap() per window held it exclusively for
    // 5-9 ms in a process with much device-registered memory (bench.py), and every fault of every thread waited.
    // The zap itself costs the same 5-9 ms per 256 MB there: it runs on a thread of its own (FqSegReader::give_back), not on
    // the reader's -- the reader is the loop's critical path.
    bool release_range(void** addr, size_t* bytes) {
        if (!mapped || !buf) return false;
        const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
        const uintptr_t a = ((uintptr_t)buf + pg - 1) & ~(pg - 1), b = ((uintptr_t)buf + used_bytes) & ~(pg - 1);
        buf = nullptr; cap = 0;
        if (b <= a) return false;
        *addr = (void*)a; *bytes = (size_t)(b - a);
        return true;
    }
    ~FqSeg() { if (!mapped) free(buf); }
    bool reserve(size_t n) {
        if (n <= cap) return true;
        const size_t want = n + (n >> 3) + 4096;
        uint8_t* p = static_cast<uint8_t*>(realloc(buf, want));
        if (!p) return false;
        buf = p; cap = want;
        return true;
    }
};

// splits buf[0, len) into records on `nt` threads (the first byte is a record start); returns 0, or FQ_BAD with *bad_at = the
// offset of the first record that is not plain.  The trailing incomplete record (when !at_eof) is left out.
static int fq_seg_split(FqSeg& s, bool fasta, bool at_eof, unsigned nt, size_t* bad_at) {
    const uint8_t* base = s.buf;
    const uint8_t* end = base + s.len;
    s.recs.clear();
    if (s.len == 0) return 0;
    nt = std::max(1u, std::min<unsigned>(nt, (unsigned)(s.len / (2u << 20)) + 1));
    std::vector<std::vector<FqRec>> part(nt);
    std::vector<const uint8_t*> first(nt, nullptr), last(nt, nullptr);
    std::vector<int> status(nt, FQ_OK);
    auto find_start = [&](const uint8_t* from) { return fasta ? fa_find_start(base, from, end) : fq_find_start(base, from, end); };
    auto work = [&](unsigned t) {
        FqCpuScope cpu(g_fq_cpu_split_ns);
        const uint8_t* from = base + s.len * t / nt;
        const uint8_t* upto = base + s.len * (t + 1) / nt;
#ifdef MADV_POPULATE_READ
        if (s.mapped) {                                                      // this piece's pages in one go instead of a fault per 64 KB
            const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
            const uintptr_t a = (uintptr_t)from & ~(pg - 1), b = ((uintptr_t)upto + pg - 1) & ~(pg - 1);
            const auto tp0 = std::chrono::steady_clock::now();
            (void)madvise((void*)a, (size_t)(b - a), MADV_POPULATE_READ);     // (beyond the file's last page: an error that is ignored)
            if (t == 0 && opt_on(QO_PIPELINE_TRACE))
                fprintf(stderr, "[qcat] stream reader: populate of piece 0 (%zu MB) %.2f ms\n", (size_t)(b - a) >> 20,
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count() * 1e3);
        }
#endif
        const uint8_t* p = t == 0 ? base : find_start(from);
        if (!p) { status[t] = FQ_BAD; return; }
        first[t] = p;
        part[t].reserve((size_t)((upto - from) / 1200 + 16));
        while (p < upto && p < end) {
            FqRec r;
            int st;
            const uint8_t* n = fq_parse_st(fasta, base, p, end, at_eof, &r, &st);
            if (!n) { status[t] = st; break; }
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
    // the pieces must meet; an incomplete record is fine in the last piece that has one (everything behind it is carried)
    bool ok = true;
    for (unsigned t = 0; t < nt && ok; ++t) {
        if (status[t] == FQ_BAD) ok = false;
        else if (status[t] == FQ_INCOMPLETE) { for (unsigned u = t + 1; u < nt; ++u) if (!part[u].empty() || status[u] == FQ_BAD) ok = false; break; }
        else if (t + 1 < nt && last[t] != first[t + 1]) ok = false;
    }
    if (ok) {
        size_t total = 0;
        for (auto& v : part) total += v.size();
        s.recs.reserve(total);
        for (unsigned t = 0; t < nt; ++t) {
            s.recs.insert(s.recs.end(), part[t].begin(), part[t].end());
            if (status[t] == FQ_INCOMPLETE) break;
        }
        return 0;
    }
    // the pieces did not meet (or a record is not plain): one thread walks the buffer
    const uint8_t* p = base;
    while (p < end) {
        FqRec r;
        int st;
        const uint8_t* n = fq_parse_st(fasta, base, p, end, at_eof, &r, &st);
        if (!n) {
            if (st == FQ_INCOMPLETE) break;
            *bad_at = (size_t)(p - base);
            return FQ_BAD;
        }
        s.recs.push_back(r);
        p = n;
    }
    return 0;
}

// ---- a segment that is not all plain records, rewritten as plain ones (round 6) ---------------------------------------------
// The reference reads FASTQ with Biopython's FastqGeneralIterator and FASTA with SimpleFastaParser (qcat/cli.py:235-306;
// restated in qcat_amd/cli.py: _fastq_records_general, _fasta_records): blank lines between records are skipped, titles and
// lines lose trailing whitespace, sequence and quality may be wrapped over several lines (quality lines are collected until
// they are as long as the sequence: a quality line may start with '@'), FASTA sequence lines are joined with blanks and
// carriage returns dropped.  One thread walks buf[0, len) by those rules and writes "@title\nseq\n+\nqual\n" / ">title\nseq\n"
// into s.norm; a record counts only when its end is inside the buffer (FASTA: the next '>' line or the end of the file).
// Returns 0; FQ_BAD for anything the Python parser must see itself -- its error cases (so that message and exit status stay
// the reference's), an empty sequence, a byte outside printable ASCII and \t \r \n \v \f, a lone \r (a line break to Python's
// text mode), a tab or blank inside a FASTQ sequence, a tab inside a FASTA sequence.
static inline bool fq_is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f' || c == '\n'; }
static int fq_seg_normalize(FqSeg& s, bool fasta, bool at_eof, bool at_file_start) {
    const uint8_t* base = s.buf;
    const uint8_t* end = base + s.len;
    s.recs.clear(); s.norm.clear(); s.norm_end.clear();
    s.norm.reserve(s.len + 64);
    // allowed bytes, and no carriage return that is not followed by a newline
    for (const uint8_t* p = base; p < end; ++p) {
        const uint8_t c = *p;
        if (c >= 0x80 || (c < 0x20 && c != '\t' && c != '\n' && c != '\v' && c != '\f' && c != '\r')) return FQ_BAD;
        if (c == '\r' && (p + 1 >= end ? at_eof : p[1] != '\n')) return FQ_BAD;
    }
    struct Line { const uint8_t* b; const uint8_t* e; const uint8_t* next; bool whole; };     // [b, e) without the newline; whole: it ended in '\n' (or at the end of the file)
    auto line_at = [&](const uint8_t* p) {
        const uint8_t* nl = p < end ? static_cast<const uint8_t*>(memchr(p, '\n', (size_t)(end - p))) : nullptr;
        if (nl) return Line{p, nl, nl + 1, true};
        return Line{p, end, end, at_eof};
    };
    auto rstrip = [](const uint8_t* b, const uint8_t* e) { while (e > b && fq_is_space(e[-1])) --e; return e; };
    auto blank = [&](const Line& l) { return rstrip(l.b, l.e) == l.b && [&] { for (const uint8_t* q = l.b; q < l.e; ++q) if (!fq_is_space(*q)) return false; return true; }(); };
    auto put = [&](const uint8_t* b, const uint8_t* e) { s.norm.insert(s.norm.end(), b, e); };
    const uint8_t* p = base;
    if (fasta) {
        if (at_file_start) {                                                 // text before the first '>' is ignored
            while (p < end && *p != '>') { const Line l = line_at(p); if (!l.whole) return FQ_BAD; p = l.next; }
        }
        while (p < end) {
            if (*p != '>') return FQ_BAD;                                    // (a segment starts at a record)
            const Line t = line_at(p);
            if (!t.whole) break;
            const uint8_t* te = rstrip(t.b + 1, t.e);
            // sequence lines up to the next '>' line; the record is complete when that line (or the end of the file) is in sight
            const size_t at = s.norm.size();
            s.norm.push_back('>'); put(t.b + 1, te); s.norm.push_back('\n');
            const size_t seq_at = s.norm.size();
            const uint8_t* q = t.next;
            bool closed = false;
            while (true) {
                if (q >= end) { closed = at_eof; break; }
                if (*q == '>') { closed = true; break; }
                const Line l = line_at(q);
                if (!l.whole) break;
                const uint8_t* le = rstrip(l.b, l.e);
                for (const uint8_t* c = l.b; c < le; ++c) {
                    if (*c == ' ' || *c == '\r') continue;
                    if (*c == '\t' || *c == '\v' || *c == '\f') return FQ_BAD;
                    s.norm.push_back(*c);
                }
                q = l.next;
            }
            if (!closed) { s.norm.resize(at); break; }
            const size_t sl = s.norm.size() - seq_at;
            if (sl == 0 || sl > 0x7FFFFFFFull || (size_t)(te - (t.b + 1)) > 0xFFFFFFFFull) return FQ_BAD;
            s.norm.push_back('\n');
            FqRec r;
            r.title = at + 1; r.title_len = (uint32_t)(te - (t.b + 1)); r.seq = seq_at; r.qual = 0; r.seq_len = (uint32_t)sl;
            s.recs.push_back(r);
            s.norm_end.push_back((uint64_t)(q - base));
            p = q;
        }
        return 0;
    }
    while (p < end) {
        Line l = line_at(p);
        if (!l.whole) break;
        if (blank(l)) { p = l.next; if (!s.norm_end.empty()) s.norm_end.back() = (uint64_t)(p - base); continue; }     // (blank lines between / after records)
        if (*l.b != '@') return FQ_BAD;
        const uint8_t* tb = l.b + 1;
        const uint8_t* te = rstrip(tb, l.e);
        const size_t at = s.norm.size();
        s.norm.push_back('@'); put(tb, te); s.norm.push_back('\n');
        const size_t seq_at = s.norm.size();
        const uint8_t* q = l.next;
        bool complete = false, bad = false;
        // sequence lines up to the '+' line
        Line pl{};
        bool have_plus = false;
        while (q < end) {
            const Line x = line_at(q);
            if (!x.whole) break;
            if (x.b < x.e && *x.b == '+') { pl = x; have_plus = true; break; }
            const uint8_t* xe = rstrip(x.b, x.e);
            for (const uint8_t* c = x.b; c < xe; ++c) { if (*c == ' ' || *c == '\t' || fq_is_space(*c)) { bad = true; break; } s.norm.push_back(*c); }
            if (bad) break;
            q = x.next;
        }
        if (bad) return FQ_BAD;
        if (!have_plus) { if (q >= end && at_eof) return FQ_BAD; s.norm.resize(at); break; }      // ("End of file without quality information": Python's to report)
        const size_t sl = s.norm.size() - seq_at;
        {   // the caption of the '+' line: empty or the title
            const uint8_t* cb = pl.b + 1;
            const uint8_t* ce = rstrip(cb, pl.e);
            if (ce > cb && ((size_t)(ce - cb) != (size_t)(te - tb) || memcmp(cb, tb, (size_t)(te - tb)) != 0)) return FQ_BAD;
        }
        if (sl == 0 || sl > 0x7FFFFFFFull || (size_t)(te - tb) > 0xFFFFFFFFull) return FQ_BAD;
        s.norm.push_back('\n'); s.norm.push_back('+'); s.norm.push_back('\n');
        const size_t qual_at = s.norm.size();
        // quality lines: the first one always, then more while they are shorter than the sequence
        q = pl.next;
        size_t ql = 0;
        bool first_line = true;
        while (first_line || ql < sl) {
            if (q >= end) { if (!at_eof) q = nullptr; break; }
            const Line x = line_at(q);
            if (!x.whole) { q = nullptr; break; }
            const uint8_t* xe = rstrip(x.b, x.e);
            put(x.b, xe); ql += (size_t)(xe - x.b);
            q = x.next;
            first_line = false;
        }
        if (!q) { s.norm.resize(at); break; }                                 // the buffer ends inside the record
        if (ql != sl) return FQ_BAD;                                          // ("Lengths of sequence and quality values differs": Python's to report)
        for (size_t i = 0; i < ql; ++i) if (fq_is_space(s.norm[qual_at + i])) return FQ_BAD;
        complete = true;
        (void)complete;
        s.norm.push_back('\n');
        FqRec r;
        r.title = at + 1; r.title_len = (uint32_t)(te - tb); r.seq = seq_at; r.qual = qual_at; r.seq_len = (uint32_t)sl;
        s.recs.push_back(r);
        s.norm_end.push_back((uint64_t)(q - base));
        p = q;
    }
    return 0;
}

static inline bool fq_pread_all(int fd, uint8_t* dst, size_t n, uint64_t off) {
    while (n) {
        const ssize_t k = pread(fd, dst, n, (off_t)off);
        if (k < 0) { if (errno == EINTR) continue; return false; }
        if (k == 0) return false;                                            // (the file shrank under us)
        dst += k; n -= (size_t)k; off += (uint64_t)k;
    }
    return true;
}


// the reader stage: consecutive segments of a file.  load() fills `s` with the bytes carried over from the previous segment
// plus the next `seg_bytes` of the file (more when that holds no whole batch), splits them, and cuts the round at the last
// whole batch.  The previous segment's buffer must still be alive (its tail is the carry).
struct FqSegReader {
    int fd = -1;
    uint64_t file_size = 0, pos = 0, first_read = 0;
    bool streaming = false;                                  // the input is a pipe: read() in order, the size is known at its end
    bool no_normalize = false;                               // qcat_fastq_batch_offsets: plain records only (offsets into the file)
    uint64_t real_size = 0, range_begin = 0;                 // the file's own size (file_size may be a shard's end); where the shard starts
    bool fasta = false, batches = false, use_mmap = false;
    uint64_t bs = 1;
    size_t seg_bytes = 0;
    unsigned nthreads = 1;
    const uint8_t* carry = nullptr;
    size_t carry_len = 0;
    uint64_t carry_off = 0;                                                  // file offset of the carried bytes
    uint8_t* map_base = nullptr;                                             // mapped reader: the whole file
    std::thread zapper;                                                      // at most one release in flight
    ~FqSegReader() {
        if (zapper.joinable()) zapper.join();
        if (map_base) munmap(map_base, (size_t)file_size);
    }
    std::mutex zap_mu;                                                       // (the writer gives a written segment back, the reader a reused slot)
    void give_back(FqSeg& s) {
        std::lock_guard<std::mutex> lk(zap_mu);
        void* a = nullptr; size_t n = 0;
        if (!s.release_range(&a, &n)) return;
        if (zapper.joinable()) zapper.join();
        if (opt_on(QO_STREAM_SYNC_RELEASE)) { (void)madvise(a, n, MADV_DONTNEED); return; }
        try { zapper = std::thread([a, n] { (void)madvise(a, n, MADV_DONTNEED); }); }
        catch (const std::exception&) { (void)madvise(a, n, MADV_DONTNEED); }
    }
    // 0: s is loaded (s.eof: it is the last one); QCAT_ERR_*: failure (msg); 1: a record that is not plain -- s.file_off says
    // where the segment starts
    unsigned n_loaded = 0;                                                   // segments handed out so far
    int load(FqSeg& s, std::string* msg) {
        // the first two segments are a quarter and a half of the others: the scan and the writer start after a quarter of a
        // segment's splitting time instead of a whole one (the loop's fill is a tenth of a 1.5 GB file's run otherwise)
        size_t want = n_loaded >= 2 ? seg_bytes : std::max<size_t>(std::min<size_t>(seg_bytes, 16u << 20), seg_bytes >> (2 - n_loaded));
        ++n_loaded;
        s.file_off = carry_len ? carry_off : pos;
        s.len = 0;
        bool first_fill = true;
        for (;;) {                                                           // (again with more bytes while the buffer holds no whole batch)
            size_t fresh = (size_t)std::min<uint64_t>(want, file_size - pos);
            const size_t base_len = first_fill ? carry_len : s.len;
            if (streaming) {
                // a pipe: the carried bytes, then up to `fresh` bytes as they come; fewer than asked for = the end of the stream
                if (!s.reserve(base_len + fresh + 1)) { *msg = "out of host memory"; return QCAT_ERR_NOMEM; }
                if (first_fill && carry_len) memmove(s.buf, carry, carry_len);
                s.mapped = false;
                size_t got = 0;
                while (got < fresh) {
                    const ssize_t k = read(fd, s.buf + base_len + got, fresh - got);
                    if (k < 0) { if (errno == EINTR) continue; *msg = std::string("read failed: ") + strerror(errno); return QCAT_ERR_IO; }
                    if (k == 0) break;
                    got += (size_t)k;
                }
                if (got < fresh) file_size = pos + got;                       // the end of the stream
                fresh = got;
            } else if (use_mmap) {
                {   // (ADVICE r5) the pread reader notices a file that shrank by its short read; the mapping would fault instead
                    struct stat now_st;
                    if (fstat(fd, &now_st) != 0 || (uint64_t)now_st.st_size != (real_size ? real_size : file_size)) { *msg = "the file changed size during the run"; return QCAT_ERR_IO; }
                }
                // a window of the file instead of a copy: [the carried bytes' offset, the end of the fresh bytes) of ONE mapping of
                // the whole file (address space only; a written segment's pages are given back, FqSeg::release) -- the pages are
                // touched by the splitting threads (MADV_POPULATE_READ per piece)
                if (!map_base) {
                    void* m = mmap(nullptr, (size_t)file_size, PROT_READ, MAP_PRIVATE, fd, 0);
                    if (m == MAP_FAILED) { *msg = "mmap failed"; return QCAT_ERR_NOMEM; }
                    map_base = static_cast<uint8_t*>(m);
                }
                if (first_fill) give_back(s);
                s.mapped = true;
                s.buf = map_base + s.file_off;
                s.cap = (size_t)(file_size - s.file_off);
            } else {
            if (!s.reserve(base_len + fresh + 1)) { *msg = "out of host memory"; return QCAT_ERR_NOMEM; }
            if (first_fill && carry_len) memcpy(s.buf, carry, carry_len);
            {   // the fresh bytes on all threads (page cache -> buffer: a memory copy per thread, no page faults on a mapping)
                const unsigned nt = std::max(1u, std::min<unsigned>(nthreads, (unsigned)(fresh / (4u << 20)) + 1));
                std::atomic<bool> ok{true};
                auto rd = [&](unsigned t) {
                    const size_t a = fresh * t / nt, b = fresh * (t + 1) / nt;
                    if (b > a && !fq_pread_all(fd, s.buf + base_len + a, b - a, pos + a)) ok = false;
                };
                std::vector<std::thread> th;
                for (unsigned t = 1; t < nt; ++t) th.emplace_back(rd, t);
                rd(0);
                for (auto& x : th) x.join();
                if (!ok) { *msg = "read failed"; return QCAT_ERR_IO; }
            }
            }
            pos += fresh;
            s.len = base_len + fresh;
            s.eof = pos >= file_size;
            first_fill = false;
            size_t bad_at = 0;
            const auto ts0 = std::chrono::steady_clock::now();
            const int split_rc = fq_seg_split(s, fasta, s.eof, nthreads, &bad_at);
            if (opt_on(QO_PIPELINE_TRACE))
                fprintf(stderr, "[qcat] stream reader: split of %zu MB %.2f ms\n", s.len >> 20, std::chrono::duration<double>(std::chrono::steady_clock::now() - ts0).count() * 1e3);
            s.norm.clear(); s.norm_end.clear();
            if (split_rc == FQ_BAD) {
                // not all plain: Biopython's rules on one thread (wrapped lines, \r\n, blank lines ...); what even those do not
                // take goes to the caller's own parser, in front of this segment
                const auto tn0 = std::chrono::steady_clock::now();
                const int nrc = no_normalize ? FQ_BAD : fq_seg_normalize(s, fasta, s.eof, s.file_off == range_begin);
                if (opt_on(QO_PIPELINE_TRACE))
                    fprintf(stderr, "[qcat] stream reader: segment at %llu rewritten as plain records (%s) in %.2f ms\n", (unsigned long long)s.file_off,
                            nrc == 0 ? "ok" : "not taken", std::chrono::duration<double>(std::chrono::steady_clock::now() - tn0).count() * 1e3);
                if (nrc != 0 || (s.recs.empty() && s.eof && s.len)) { s.norm.clear(); s.norm_end.clear(); s.bad = true; return 1; }
            }
            s.bad = false;
            const uint64_t nrec = s.recs.size();
            s.n_use = (s.eof || !batches) ? nrec : nrec / bs * bs;
            if (s.n_use > 0 || s.eof) break;
            want = std::max<size_t>(want, s.len);                            // not one whole batch (or record) yet: double the buffer
        }
        if (s.eof) s.used_bytes = s.len;
        else if (!s.norm_end.empty() || !s.norm.empty()) s.used_bytes = s.n_use ? (size_t)s.norm_end[(size_t)s.n_use - 1] : 0;
        else if (s.n_use < s.recs.size()) s.used_bytes = (size_t)(s.recs[s.n_use].title - 1);
        else {
            const FqRec& l = s.recs.back();                                  // everything behind the last whole record (and its newline)
            s.used_bytes = (size_t)((fasta ? l.seq : l.qual) + l.seq_len) + 1;
        }
        s.first_read = first_read;
        first_read += s.n_use;
        carry = s.buf + s.used_bytes; carry_len = s.len - s.used_bytes; carry_off = s.file_off + s.used_bytes;
        s.recs.resize((size_t)s.n_use);
        return 0;
    }
};

}  // namespace qk

extern "C" int qcat_fastq_demux_stream(const char* path, qcat_ctx* c, const qcat_kit* ckit, const qcat_demux_opts* o,
                                       qcat_demux_hist* hist, qcat_demux_stats* stats) {
    using namespace qk;
    if ((!path && !(o && o->input_fd > 0)) || !c || !ckit || !o || !hist || !stats) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: null argument");
    qcat_kit* kit = const_cast<qcat_kit*>(ckit);
    const DevKit& hk = kit->hk.dk;
    if (hk.mode == QCAT_MODE_SIMPLE && o->kit_auto) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: simple mode has no kits to vote for (kit_auto must be 0)");
    if (hk.ends != QCAT_ENDS_BOTH) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream needs a kit created with QCAT_ENDS_BOTH");
    const bool dual = hk.mode == QCAT_MODE_DUAL;
    if (hist->w0 < 1 || hist->w1 < 1 || !hist->barcode || !hist->adapter) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: histogram arrays missing");
    for (int t = 0; t < hk.nt; ++t)
        if (hk.tpl[t].sets[0].n > hist->w0 || (dual && hk.tpl[t].sets[1].n > hist->w1)) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: histogram rows narrower than a barcode set");
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_call0 = now();
    const bool trace_stages = opt_on(QO_PIPELINE_TRACE);                    // (diagnostics: when every stage held every segment)
    struct Fd { int fd = -1; ~Fd() { if (fd >= 0) close(fd); } } file;
    // the input: a path, or the caller's descriptor (input_fd - 1: the driver's stdin, qcat/cli.py:256-257) -- duplicated, the
    // caller's stays open
    file.fd = o->input_fd > 0 ? dup(o->input_fd - 1) : open(path, O_RDONLY);
    if (file.fd < 0) return set_err(QCAT_ERR_ARG, o->input_fd > 0 ? std::string("qcat_fastq_demux_stream: bad input descriptor") : std::string("qcat_fastq_demux_stream: cannot open ") + path);
    struct stat st;
    if (fstat(file.fd, &st) != 0) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: cannot stat the input");
    const bool streaming = !S_ISREG(st.st_mode);                            // a pipe (or a terminal, a socket): read in order
    if (streaming && o->input_fd <= 0) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_demux_stream: not a regular file");
    if (streaming && (o->rest_fd <= 0 || o->range_begin || o->range_end)) return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: a stream needs rest_fd and takes no byte range");
    uint64_t start_pos = 0;
    if (!streaming && o->input_fd > 0) {                                    // `qcat < file`: from where the descriptor stands
        const off_t at = lseek(file.fd, 0, SEEK_CUR);
        if (at > 0) start_pos = (uint64_t)at;
    }
    const uint64_t real_size = streaming ? ~0ull : (uint64_t)st.st_size;
    // a shard of the file (ABI 6): the records in [range_begin, range_end); the reader treats range_end as the end of the file
    if (o->range_begin > real_size || (o->range_end && (o->range_end > real_size || o->range_end < o->range_begin)))
        return set_err(QCAT_ERR_ARG, "qcat_fastq_demux_stream: byte range outside the file");
    const uint64_t file_size = o->range_end ? o->range_end : real_size;
    const uint64_t begin = o->range_begin ? o->range_begin : start_pos;     // where this call starts in the input
    if (!streaming) (void)posix_fadvise(file.fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    memset(stats, 0, sizeof *stats);
    stats->file_bytes = streaming ? 0 : file_size - begin;
    memset(hist->barcode, 0, sizeof(int64_t) * (size_t)hk.nt * (size_t)hist->w0 * (size_t)hist->w1);
    memset(hist->adapter, 0, sizeof(int64_t) * (size_t)hk.nt);
    hist->n_none = 0; hist->n_adapter_none = 0;
    if (file_size <= begin) return 0;
    uint8_t first_byte = '@';                                                // (a stream is assumed to be FASTQ, qcat/cli.py:219, :256)
    if (!streaming && !fq_pread_all(file.fd, &first_byte, 1, (off_t)begin)) return set_err(QCAT_ERR_IO, "qcat_fastq_demux_stream: read failed");
    const bool fasta = first_byte == '>';                                    // (the driver decides by the first byte too, qcat/cli.py:248-262)
    FqWriter w(hk, o, fasta);
    if (int wrc = w.init()) return wrc;
    const unsigned nthreads = std::max(1u, host_threads());
    const uint64_t bs = (uint64_t)std::max(1, o->batch_size);
    const bool batches = o->kit_auto || o->filter_barcodes;                  // the reads of a round must be whole batches of the driver's loop
    const size_t seg_bytes = (size_t)std::max<uint64_t>(o->segment_bytes ? o->segment_bytes : (256ull << 20), 64);

    // ---- the three segments and who holds them -----------------------------------------------------------------------------
    constexpr int NSEG = 3;
    FqSeg seg[NSEG];
    std::mutex mu;
    std::condition_variable cv;
    int fail_rc = 0;                                                         // first failure of any stage (under mu)
    std::string fail_msg;
    bool reader_done = false;                                                // no more segments will be loaded
    uint64_t n_loaded = 0;                                                   // segments loaded so far
    auto fail = [&](int rc, const std::string& msg) {
        { std::lock_guard<std::mutex> lk(mu); if (!fail_rc) { fail_rc = rc; fail_msg = msg; } }
        cv.notify_all();
    };
    uint64_t stop_offset = file_size;                                        // where the native loop ended (a record that is not plain)
    bool stopped = false;
    double t_parse = 0;

    // ---- reader ---------------------------------------------------------------------------------------------------------
    FqSegReader rdr;
    rdr.fd = file.fd; rdr.file_size = file_size; rdr.real_size = streaming ? 0 : real_size; rdr.pos = begin; rdr.range_begin = begin;
    rdr.streaming = streaming;
    rdr.fasta = fasta; rdr.batches = batches; rdr.bs = bs; rdr.seg_bytes = seg_bytes; rdr.nthreads = nthreads;
    rdr.use_mmap = !streaming && (o->stream_reader ? o->stream_reader : FQ_DEFAULT_READER) == 2;
    std::atomic<int> rest_errno{0};
    std::thread reader([&] {
        try {
            for (uint64_t k = 0;; ++k) {
                FqSeg& s = seg[k % NSEG];
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return fail_rc || s.state == 0; });
                    if (fail_rc) break;
                }
                const double t0 = now();
                std::string msg;
                const int lrc = rdr.load(s, &msg);
                t_parse += now() - t0;
                if (trace_stages) fprintf(stderr, "[qcat stream] segment %llu read   %8.2f .. %8.2f ms (%llu reads)\n", (unsigned long long)k, (t0 - t_call0) * 1e3, (now() - t_call0) * 1e3, (unsigned long long)s.n_use);
                if (lrc < 0) { fail(lrc, "qcat_fastq_demux_stream: " + msg); return; }
                if (lrc == 1) {
                    // a record that is not plain: the native loop ends in front of this segment
                    if (streaming) {
                        // ... whose bytes have left the pipe: they go to the caller's rest descriptor, in front of what the
                        // caller's parser will read from the stream itself
                        size_t done = 0;
                        while (done < s.len) {
                            const ssize_t k = write(o->rest_fd - 1, s.buf + done, s.len - done);
                            if (k < 0) { if (errno == EINTR) continue; rest_errno = errno ? errno : EIO; break; }
                            done += (size_t)k;
                        }
                    }
                    std::lock_guard<std::mutex> lk(mu);
                    stopped = true; stop_offset = s.file_off;
                    reader_done = true;
                    cv.notify_all();
                    return;
                }
                s.res.resize((size_t)s.n_use);
                s.skipped.assign((size_t)s.n_use, 0);
                const bool last = s.eof;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    s.state = 1; ++n_loaded;
                    if (last) reader_done = true;
                }
                cv.notify_all();
                if (last) return;
            }
        } catch (const std::exception&) { fail(QCAT_ERR_NOMEM, "qcat_fastq_demux_stream: out of host memory"); }
    });
    // ---- writer ---------------------------------------------------------------------------------------------------------
    uint64_t n_written = 0, n_skipped = 0;
    std::thread writer([&] {
        try {
            for (uint64_t k = 0;; ++k) {
                FqSeg& s = seg[k % NSEG];
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return fail_rc || s.state == 2 || (reader_done && k >= n_loaded); });
                    if (fail_rc || s.state != 2) break;
                }
                const double tw0 = now();
                if (s.n_use) w.write_range(s.data(), s.recs.data(), s.res.data(), s.skipped.data(), s.n_use);
                if (trace_stages) fprintf(stderr, "[qcat stream] segment %llu write  %8.2f .. %8.2f ms\n", (unsigned long long)k, (tw0 - t_call0) * 1e3, (now() - t_call0) * 1e3);
                if (!w.io_ok) { fail(QCAT_ERR_IO, std::string("qcat_fastq_demux_stream: write failed: ") + strerror(w.io_errno)); break; }
                // the histogram of the kept reads (qcat/cli.py:366-383, :531-534)
                for (uint64_t r = 0; r < s.n_use; ++r) {
                    if (s.skipped[r]) { ++n_skipped; continue; }
                    const qcat_result& q = s.res[r];
                    if (q.adapter_idx >= 0 && q.adapter_idx < hk.nt) ++hist->adapter[q.adapter_idx]; else ++hist->n_adapter_none;
                    if (w.called(q)) ++hist->barcode[(w.tpl_of(q) * (size_t)hist->w0 + (size_t)q.barcode_idx) * (size_t)hist->w1 + (size_t)(dual ? q.barcode2_idx : 0)];
                    else ++hist->n_none;
                }
                n_written += s.n_use;
                rdr.give_back(s);                                            // its pages go back now, not when the slot is loaded again: at the
                                                                             // end of the file only the last segment is still mapped
                { std::lock_guard<std::mutex> lk(mu); s.state = 0; }
                cv.notify_all();
            }
        } catch (const std::exception&) { fail(QCAT_ERR_NOMEM, "qcat_fastq_demux_stream: out of host memory"); }
    });
    struct Join {
        std::thread &a, &b; std::function<void()> stop;
        ~Join() { stop(); if (a.joinable()) a.join(); if (b.joinable()) b.join(); }
    } join{reader, writer, [&] { fail(QCAT_ERR_ARG, "qcat_fastq_demux_stream: interrupted"); }};
    // ---- scan (this thread) ------------------------------------------------------------------------------------------------
    double t_scan = 0;
    uint64_t n_segments = 0;
    int rc = 0;
    try {
        std::vector<uint64_t> lens;
        std::vector<const uint8_t*> ptrs;
        std::vector<int32_t> slots;
        for (uint64_t k = 0; !rc; ++k) {
            FqSeg& s = seg[k % NSEG];
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return fail_rc || s.state == 1 || (reader_done && k >= n_loaded); });
                if (fail_rc || s.state != 1) break;
            }
            const double t0 = now();
            const uint64_t cnt = s.n_use;
            if (cnt > 0xFFFFFFF0ull) { rc = set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_demux_stream: more than 2^32 reads in one segment"); break; }
            if (o->kit_auto) {
                // chunks of up to 64 batches per call: one adapter pass, one vote per batch on the device (fastq_host.inc)
                const uint64_t chunk = std::min<uint64_t>(64, std::max<uint64_t>(1, (1u << 20) / bs)) * bs;
                ptrs.resize((size_t)std::min(chunk, cnt)); lens.resize(ptrs.size()); slots.resize((size_t)(chunk / bs) + 1);
                for (uint64_t first = 0; first < cnt && !rc; first += chunk) {
                    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, cnt - first);
                    for (uint32_t r = 0; r < m; ++r) { const FqRec& x = s.recs[first + r]; ptrs[r] = s.data() + x.seq; lens[r] = x.seq_len; }
                    rc = qcat_scan_batches_auto_ptrs(c, kit, ptrs.data(), lens.data(), m, (uint32_t)bs, s.res.data() + first, nullptr, slots.data());
                }
            } else if (cnt) {
                const ReadView rv{s.data(), nullptr, s.recs.data()};
                rc = scan_batch_pipelined(c, kit, rv, (uint32_t)cnt, s.res.data(), nullptr);
                if (rc == 1) {                                               // a small segment / --detect-middle: the one-shot path over whole reads
                    // (round 6: the reads where they lie in the segment -- the upload's host threads copy them into the pinned staging)
                    ptrs.resize((size_t)cnt); lens.resize((size_t)cnt);
                    for (uint64_t r = 0; r < cnt; ++r) { ptrs[r] = s.data() + s.recs[r].seq; lens[r] = s.recs[r].seq_len; }
                    rc = scan_debug_impl(c, kit, nullptr, nullptr, ptrs.data(), lens.data(), (uint32_t)cnt, s.res.data(), nullptr, nullptr, nullptr, 0);
                }
            }
            if (rc) break;
            if (o->filter_barcodes)
                for (uint64_t first = 0; first < cnt; first += bs) fq_filter_batch(w, s.res.data() + first, std::min<uint64_t>(bs, cnt - first));
            t_scan += now() - t0;
            if (trace_stages) fprintf(stderr, "[qcat stream] segment %llu scan   %8.2f .. %8.2f ms\n", (unsigned long long)k, (t0 - t_call0) * 1e3, (now() - t_call0) * 1e3);
            ++n_segments;
            { std::lock_guard<std::mutex> lk(mu); s.state = 2; }
            cv.notify_all();
        }
    } catch (const std::bad_alloc&) { rc = set_err(QCAT_ERR_NOMEM, "qcat_fastq_demux_stream: out of host memory"); }
    // (ADVICE r5: the scan calls start threads and size vectors -- std::system_error, std::length_error must not unwind through
    // the extern "C" entry into the host process' std::terminate)
    catch (const std::exception& e) { rc = set_err(QCAT_ERR_DEVICE, std::string("qcat_fastq_demux_stream: ") + e.what()); }
    catch (...) { rc = set_err(QCAT_ERR_DEVICE, "qcat_fastq_demux_stream: unknown failure in the scan stage"); }
    std::string scan_err = rc ? std::string(qcat_last_error()) : std::string();
    if (rc) fail(rc, scan_err);
    // the writer drains what was scanned; then both threads end
    join.stop = [] {};
    if (reader.joinable()) reader.join();
    if (writer.joinable()) writer.join();
    const double t_fin0 = now();
    w.finish();
    if (trace_stages) fprintf(stderr, "[qcat stream] threads joined at %8.2f ms, outputs closed at %8.2f ms\n", (t_fin0 - t_call0) * 1e3, (now() - t_call0) * 1e3);
    // (also on failure: a caller tells "not for this loop, nothing written" from an error behind written segments by these two)
    stats->n_reads = n_written; stats->segments = (int32_t)n_segments;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (fail_rc) return set_err(fail_rc, fail_msg);
    }
    if (rest_errno.load()) return set_err(QCAT_ERR_IO, std::string("qcat_fastq_demux_stream: writing the unread bytes of the stream back failed: ") + strerror(rest_errno.load()));
    if (stopped && stop_offset == begin && !streaming) return set_err(QCAT_ERR_UNSUPPORTED, fasta ? "qcat_fastq_demux_stream: not a plain two-line FASTA file" : "qcat_fastq_demux_stream: not a plain four-line FASTQ file");
    stats->n_reads = n_written; stats->n_skipped = n_skipped;
    stats->parse_s = t_parse; stats->scan_s = t_scan; stats->write_s = w.t_write; stats->total_s = now() - t_call0;
    stats->next_offset = stopped ? stop_offset : (streaming ? rdr.pos : file_size);
    stats->incomplete = stopped ? 1 : 0;
    stats->segments = (int32_t)n_segments;
    return 0;
}

// the reader stage alone: how many plain records and sequence letters the file holds, streamed in segments like
// qcat_fastq_demux_stream does (bounded memory; also what the CPU tests drive the segment logic with)
extern "C" int qcat_fastq_stream_count(const char* path, uint64_t segment_bytes, uint32_t batch_size, int32_t stream_reader, uint64_t* n_reads,
                                       uint64_t* n_bases, uint64_t* next_offset, uint32_t* n_segments) {
    using namespace qk;
    if (!path || !n_reads) return set_err(QCAT_ERR_ARG, "qcat_fastq_stream_count: null argument");
    struct Fd { int fd = -1; ~Fd() { if (fd >= 0) close(fd); } } file;
    file.fd = open(path, O_RDONLY);
    if (file.fd < 0) return set_err(QCAT_ERR_ARG, std::string("qcat_fastq_stream_count: cannot open ") + path);
    struct stat st;
    if (fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_stream_count: not a regular file");
    uint64_t reads = 0, bases = 0;
    uint32_t segs = 0;
    *n_reads = 0;
    if (n_bases) *n_bases = 0;
    if (next_offset) *next_offset = (uint64_t)st.st_size;
    if (n_segments) *n_segments = 0;
    if (st.st_size == 0) return 0;
    uint8_t first_byte = 0;
    if (!fq_pread_all(file.fd, &first_byte, 1, 0)) return set_err(QCAT_ERR_IO, "qcat_fastq_stream_count: read failed");
    FqSegReader rdr;
    rdr.fd = file.fd; rdr.file_size = (uint64_t)st.st_size; rdr.fasta = first_byte == '>'; rdr.batches = batch_size > 0;
    rdr.bs = std::max<uint32_t>(1, batch_size); rdr.seg_bytes = (size_t)std::max<uint64_t>(segment_bytes ? segment_bytes : (256ull << 20), 64);
    rdr.nthreads = std::max(1u, host_threads());
    rdr.use_mmap = (stream_reader ? stream_reader : FQ_DEFAULT_READER) == 2;
    FqSeg seg[2];
    for (uint32_t k = 0;; ++k) {
        FqSeg& s = seg[k & 1];
        std::string msg;
        const int rc = rdr.load(s, &msg);
        if (rc < 0) return set_err(rc, "qcat_fastq_stream_count: " + msg);
        if (rc == 1) {
            if (next_offset) *next_offset = s.file_off;
            if (s.file_off == 0) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_stream_count: not a plain FASTQ / FASTA file");
            break;
        }
        reads += s.n_use;
        for (uint64_t r = 0; r < s.n_use; ++r) bases += s.recs[r].seq_len;
        ++segs;
        if (s.eof) break;
    }
    *n_reads = reads;
    if (n_bases) *n_bases = bases;
    if (n_segments) *n_segments = segs;
    return 0;
}

// where every batch of the driver's loop starts in the file (include/qcat_hip.h: what ranks need to share ONE file)
extern "C" int qcat_fastq_batch_offsets(const char* path, uint32_t batch_size, uint64_t segment_bytes, uint64_t** offsets,
                                        uint64_t* n_batches, uint64_t* n_reads, uint64_t* next_offset) {
    using namespace qk;
    if (!path || !offsets || !n_batches || !batch_size) return set_err(QCAT_ERR_ARG, "qcat_fastq_batch_offsets: null argument");
    *offsets = nullptr; *n_batches = 0;
    if (n_reads) *n_reads = 0;
    struct Fd { int fd = -1; ~Fd() { if (fd >= 0) close(fd); } } file;
    file.fd = open(path, O_RDONLY);
    if (file.fd < 0) return set_err(QCAT_ERR_ARG, std::string("qcat_fastq_batch_offsets: cannot open ") + path);
    struct stat st;
    if (fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_batch_offsets: not a regular file");
    if (next_offset) *next_offset = (uint64_t)st.st_size;
    std::vector<uint64_t> starts;
    uint64_t reads = 0, end_off = (uint64_t)st.st_size;
    try {
        if (st.st_size > 0) {
            uint8_t first_byte = 0;
            if (!fq_pread_all(file.fd, &first_byte, 1, 0)) return set_err(QCAT_ERR_IO, "qcat_fastq_batch_offsets: read failed");
            FqSegReader rdr;
            rdr.fd = file.fd; rdr.file_size = (uint64_t)st.st_size; rdr.real_size = rdr.file_size; rdr.fasta = first_byte == '>'; rdr.batches = true;
            rdr.bs = batch_size; rdr.seg_bytes = (size_t)std::max<uint64_t>(segment_bytes ? segment_bytes : (256ull << 20), 64);
            rdr.nthreads = std::max(1u, host_threads());
            rdr.use_mmap = FQ_DEFAULT_READER == 2;
            rdr.no_normalize = true;
            FqSeg seg[2];
            for (uint32_t k = 0;; ++k) {
                FqSeg& s = seg[k & 1];
                std::string msg;
                const int rc = rdr.load(s, &msg);
                if (rc < 0) return set_err(rc, "qcat_fastq_batch_offsets: " + msg);
                if (rc == 1) {
                    if (s.file_off == 0) return set_err(QCAT_ERR_UNSUPPORTED, "qcat_fastq_batch_offsets: not a plain FASTQ / FASTA file");
                    end_off = s.file_off;
                    break;
                }
                // (segments are cut at whole batches counted from the start of the file: record r of a segment starts a batch when
                // r is a multiple of the batch size)
                for (uint64_t r = 0; r < s.n_use; r += batch_size) starts.push_back(s.file_off + s.recs[(size_t)r].title - 1);
                reads += s.n_use;
                rdr.give_back(s);
                if (s.eof) break;
            }
        }
        uint64_t* out = static_cast<uint64_t*>(malloc((starts.size() + 1) * sizeof(uint64_t)));
        if (!out) return set_err(QCAT_ERR_NOMEM, "qcat_fastq_batch_offsets: out of host memory");
        for (size_t i = 0; i < starts.size(); ++i) out[i] = starts[i];
        out[starts.size()] = end_off;
        *offsets = out; *n_batches = starts.size();
        if (n_reads) *n_reads = reads;
        if (next_offset) *next_offset = end_off;
    } catch (const std::exception& e) { return set_err(QCAT_ERR_NOMEM, std::string("qcat_fastq_batch_offsets: ") + e.what()); }
    return 0;
}

extern "C" void qcat_free(void* p) { free(p); }

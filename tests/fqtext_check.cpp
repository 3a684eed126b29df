// fqtext_check.cpp -- the passes of qcat_batch_upload_fastq_text and qcat_batch_demux_text (qcat_amd/csrc/kernels_fqtext.inc)
// run on the host, block by block, wave by wave and lane by lane, through the functions of qcat_amd/csrc/fqtext_core.h that the
// kernels themselves call: the newline and byte-class masks of a vector, the rank of a newline from the wave's ballots, the
// record checks against the line table, the six segments of an output record -- and the segment tables through the chunk and
// lane schedule of k_part_chunks / k_part_copy (qcat_amd/csrc/partition_core.h), as tests/partition_check.cpp does.  The text
// plane is allocated with exactly the device's slack and constants block; every load is checked against it, every table index
// against its size.  Expected values: a plain sequential parser written here, and plain concatenation.
// Built twice by tests/test_fqtext_host.py: plain, and with -fsanitize=address,undefined.
//   usage: fqtext_check <seed>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fqtext_core.h"
#include "check_common.h"

using namespace qfq;
using qpart::Vec16;

// ---- the expected values: a sequential parser (the rules of fq_parse, restated byte by byte) ----------------------------------------
struct Want { std::vector<Rec> recs; uint64_t bad_record = 0; };     // bad_record: 1-based, 0 = the text is plain
static bool title_class(uint8_t c) { return !((c < 0x20 && c != '\t') || c >= 0x80); }
static bool seq_class(uint8_t c) { return c > 0x20 && c < 0x80; }
static Want sequential(const std::string& t) {
    Want w;
    size_t p = 0;
    const size_t end = t.size();
    auto fail = [&]() { w.bad_record = w.recs.size() + 1; return w; };
    while (p < end) {
        if (t[p] != '@') return fail();
        size_t l1 = t.find('\n', p);
        if (l1 == std::string::npos) return fail();
        size_t s = l1 + 1, l2 = s;
        while (l2 < end && seq_class((uint8_t)t[l2])) ++l2;
        if (l2 >= end || t[l2] != '\n' || l2 == s) return fail();
        size_t pl = l2 + 1;
        if (pl >= end || t[pl] != '+') return fail();
        size_t l3 = t.find('\n', pl);
        if (l3 == std::string::npos) return fail();
        size_t q = l3 + 1, qe = q;
        while (qe < end && seq_class((uint8_t)t[qe])) ++qe;
        if (qe - q != l2 - s || (qe < end && t[qe] != '\n')) return fail();
        std::string title = t.substr(p + 1, l1 - p - 1), plus = t.substr(pl + 1, l3 - pl - 1);
        for (char c : title) if (!title_class((uint8_t)c)) return fail();
        for (char c : plus) if (!title_class((uint8_t)c)) return fail();
        while (!title.empty() && is_blank((uint8_t)title.back())) title.pop_back();
        while (!plus.empty() && is_blank((uint8_t)plus.back())) plus.pop_back();
        if (!plus.empty() && plus != title) return fail();
        Rec r{};
        r.title_off = p + 1; r.title_len = (uint32_t)title.size(); r.seq_off = s; r.seq_len = (uint32_t)(l2 - s); r.qual_off = q;
        r.title_blank = title.find_first_of(" \t") != std::string::npos;
        w.recs.push_back(r);
        p = qe < end ? qe + 1 : end;
    }
    return w;
}

// ---- the text plane as the device holds it: slack, text, constants, slack ----------------------------------------------------------
struct TextPlane : Plane {
    uint64_t n_bytes;
    static std::vector<uint8_t> payload(const std::string& t) {
        std::vector<uint8_t> p(t.size() + FQ_CONST_BYTES, 0);
        if (!t.empty()) memcpy(p.data(), t.data(), t.size());
        fq_constants(p.data() + t.size());
        return p;
    }
    explicit TextPlane(const std::string& t) : Plane(payload(t)), n_bytes(t.size()) {}
    uint8_t* text() { return at0(); }
};
static uint32_t valid_of(uint64_t off, uint64_t n_bytes) { return off >= n_bytes ? 0u : (n_bytes - off >= FQ_VEC ? 0xFFFFu : below((uint32_t)(n_bytes - off))); }

struct Parsed { std::vector<Rec> recs; std::vector<uint64_t> offsets, seq_src; uint64_t bad_line = FQ_NO_LINE; uint64_t faults = 0; uint64_t n_lines = 0; };

// k_fq_count, the scan, k_fq_lines, k_fq_records and the scan of the lengths
static Parsed device_parse(TextPlane& pl) {
    Parsed out;
    const uint64_t n_bytes = pl.n_bytes, n_blocks = blocks_of(n_bytes);
    std::vector<uint64_t> first(n_blocks + 1, 0);
    for (uint64_t blk = 0; blk < n_blocks; ++blk) {                        // k_fq_count
        uint64_t total = 0;
        for (uint32_t tid = 0; tid < FQ_THREADS; ++tid)
            for (uint32_t t = 0; t < FQ_ROUNDS; ++t) {
                const uint64_t off = blk * FQ_BLOCK + (uint64_t)t * FQ_ROUND + (uint64_t)tid * FQ_VEC;
                const uint32_t valid = valid_of(off, n_bytes);
                if (valid) total += popc32(nl_mask16(pl.load16((int64_t)off)) & valid);
            }
        first[blk] = total;
    }
    uint64_t run = 0;                                                       // the exclusive scan, the total behind it
    for (uint64_t blk = 0; blk <= n_blocks; ++blk) { const uint64_t c = first[blk]; first[blk] = run; run += c; }
    const uint64_t newlines = first[n_blocks];
    const uint64_t n_lines = n_bytes ? lines_of(newlines, pl.text()[n_bytes - 1] == '\n') : 0;
    out.n_lines = n_lines;
    std::vector<uint64_t> line_start(newlines + 2, ~0ull);
    std::vector<uint32_t> written(newlines + 2, 0);
    auto put = [&](uint64_t k, uint64_t v) { if (k >= line_start.size()) { ++out.faults; return; } line_start[k] = v; ++written[k]; };
    for (uint64_t blk = 0; blk < n_blocks; ++blk) {                        // k_fq_lines
        uint64_t line = first[blk];
        if (blk == 0) put(0, 0);
        for (uint32_t t = 0; t < FQ_ROUNDS; ++t) {
            uint32_t nl[FQ_THREADS], valid[FQ_THREADS], rank[FQ_THREADS], wtot[4];
            Vec16 v[FQ_THREADS];
            for (uint32_t tid = 0; tid < FQ_THREADS; ++tid) {
                const uint64_t off = blk * FQ_BLOCK + (uint64_t)t * FQ_ROUND + (uint64_t)tid * FQ_VEC;
                valid[tid] = valid_of(off, n_bytes);
                v[tid].w[0] = v[tid].w[1] = v[tid].w[2] = v[tid].w[3] = 0;
                if (valid[tid]) v[tid] = pl.load16((int64_t)off);
                nl[tid] = nl_mask16(v[tid]) & valid[tid];
            }
            for (uint32_t wave = 0; wave < 4; ++wave) {                     // the wave's ballots
                uint64_t bal[FQ_VEC];
                for (uint32_t b = 0; b < FQ_VEC; ++b) {
                    bal[b] = 0;
                    for (uint32_t lane = 0; lane < 64; ++lane) bal[b] |= (uint64_t)((nl[wave * 64 + lane] >> b) & 1u) << lane;
                }
                for (uint32_t lane = 0; lane < 64; ++lane) rank[wave * 64 + lane] = wave_rank(bal, lane);
                wtot[wave] = wave_total(bal);
            }
            for (uint32_t tid = 0; tid < FQ_THREADS; ++tid) {
                const uint64_t off = blk * FQ_BLOCK + (uint64_t)t * FQ_ROUND + (uint64_t)tid * FQ_VEC;
                uint64_t mine = line + rank[tid];
                for (uint32_t w = 0; w < tid / 64; ++w) mine += wtot[w];
                if (!valid[tid]) continue;
                const uint32_t bad = lines_bad(nl[tid], odd_title16(v[tid]) & valid[tid], odd_seq16(v[tid]) & valid[tid], (uint32_t)(mine & 3u));
                if (bad) {
                    const uint32_t b = (uint32_t)__builtin_ctz(bad);
                    out.bad_line = std::min(out.bad_line, mine + popc32(nl[tid] & below(b)));
                }
                uint32_t rest = nl[tid];
                uint64_t k = mine;
                while (rest) { const uint32_t b = (uint32_t)__builtin_ctz(rest); put(++k, off + b + 1); rest &= rest - 1u; }
                if (off + FQ_VEC >= n_bytes && !((nl[tid] >> (uint32_t)(n_bytes - 1 - off)) & 1u)) put(first[n_blocks] + 1, n_bytes + 1);
            }
            line += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        }
    }
    // every entry 0 .. n_lines written once (an empty text has no table)
    if (n_bytes) for (uint64_t k = 0; k <= n_lines; ++k) if (written[k] != 1) ++out.faults;
    const uint64_t n_rec = records_of(n_lines);
    out.recs.assign(n_rec, Rec{});
    out.offsets.assign(n_rec + 1, 0);
    out.seq_src.assign(n_rec, 0);
    uint8_t* text = pl.text();
    for (uint64_t r = 0; r < n_rec; ++r) {                                  // k_fq_records
        if (4 * r + 4 > n_lines) { out.bad_line = std::min(out.bad_line, 4 * r); continue; }
        uint64_t ls[5];
        for (uint32_t i = 0; i < 5; ++i) ls[i] = line_start.at(4 * r + i);
        Rec rec;
        const auto at = [&](uint64_t i) { if (i >= n_bytes) { ++out.faults; return (uint8_t)0; } return text[i]; };
        if (!record_of(at, ls, &rec)) { out.bad_line = std::min(out.bad_line, 4 * r); continue; }
        out.recs[r] = rec; out.offsets[r] = rec.seq_len; out.seq_src[r] = rec.seq_off;
        if (rec.title_blank) for (uint64_t i = 0; i < rec.title_len; ++i) if (text[rec.title_off + i] == '\t') text[rec.title_off + i] = ' ';
    }
    run = 0;
    for (uint64_t r = 0; r <= n_rec; ++r) { const uint64_t c = out.offsets[r]; out.offsets[r] = run; run += c; }
    out.faults += pl.stray;
    return out;
}

// k_part_chunks / k_part_copy over a segment table whose sources lie anywhere in the plane; `bound`: the bytes the destination
// was sized for (the grid follows it).  Returns the faults; the output in *dst_out.
static uint64_t device_copy(Plane& pl, const std::vector<uint64_t>& dst_off, const std::vector<uint64_t>& src_pos, uint64_t bound, std::string* dst_out) {
    const CopyRun r = copy_schedule(dst_off, src_pos, bound, [&](uint32_t, int64_t a) { return pl.load16(a); });
    dst_out->assign(reinterpret_cast<const char*>(r.out.data()), std::min<size_t>(dst_off.back(), r.out.size()));
    return r.bad + pl.stray;
}

// ---- texts -----------------------------------------------------------------------------------------------------------------------
struct Read { std::string title, seq, qual, plus; };
static const char* TITLE_FORMS[] = {"r%u", "r%u ch=3", "r%u\tch=3\tx=y", "r%u  two", "r%u ", ""};
static Read make_read(uint32_t i, uint64_t len) {
    Read r;
    char buf[64];
    snprintf(buf, sizeof buf, TITLE_FORMS[i % 6], i);
    r.title = buf;
    for (uint64_t k = 0; k < len; ++k) { r.seq.push_back("ACGTN"[rnd_below(5)]); r.qual.push_back((char)(0x21 + rnd_below(0x5F))); }
    std::string stripped = r.title;
    while (!stripped.empty() && is_blank((uint8_t)stripped.back())) stripped.pop_back();
    r.plus = (i % 3 == 0) ? "" : (i % 3 == 1) ? " \t" : stripped + ((i & 4) ? " " : "");
    return r;
}
static std::string record_text(const Read& r) { return "@" + r.title + "\n" + r.seq + "\n+" + r.plus + "\n" + r.qual + "\n"; }
static std::string join(const std::vector<Read>& reads, bool final_newline) {
    std::string t;
    for (const Read& r : reads) t += record_text(r);
    if (!final_newline && !t.empty()) t.pop_back();
    return t;
}

// one text through the device schedule against the sequential parser: records, offsets, first bad record, tabs; returns faults
static uint64_t check_parse(const std::string& t, Parsed* keep = nullptr, TextPlane** keep_plane = nullptr) {
    const Want w = sequential(t);
    TextPlane* pl = new TextPlane(t);
    Parsed p = device_parse(*pl);
    uint64_t bad = p.faults;
    const uint64_t got_bad = p.bad_line == FQ_NO_LINE ? 0 : p.bad_line / 4 + 1;
    if (got_bad != w.bad_record) ++bad;
    if (!w.bad_record) {
        if (p.recs.size() != w.recs.size()) ++bad;
        else {
            uint64_t o = 0;
            for (size_t r = 0; r < w.recs.size(); ++r) {
                const Rec &a = p.recs[r], &b = w.recs[r];
                if (a.title_off != b.title_off || a.title_len != b.title_len || a.seq_off != b.seq_off || a.seq_len != b.seq_len ||
                    a.qual_off != b.qual_off || a.title_blank != b.title_blank) ++bad;
                if (p.offsets[r] != o || p.seq_src[r] != b.seq_off) ++bad;
                o += b.seq_len;
                // the plane's titles: the text's with blanks for tabs; every other byte of the text unchanged
                for (uint32_t i = 0; i < b.title_len; ++i) {
                    const char c = t[b.title_off + i];
                    if (pl->text()[b.title_off + i] != (uint8_t)(c == '\t' ? ' ' : c)) ++bad;
                }
            }
            if (p.offsets[w.recs.size()] != o) ++bad;
        }
    }
    if (keep) *keep = p;
    if (keep_plane) *keep_plane = pl; else delete pl;
    return bad;
}

// a text in which the newline of a line of kind `kind` lies at byte `at`: filler records, then a record stretched to fit
static std::string text_with_newline_at(uint64_t at, uint32_t kind, bool final_newline, uint32_t tail_reads) {
    std::vector<Read> reads;
    std::string t;
    uint32_t i = 0;
    while (t.size() + 2600 < at) { reads.push_back(make_read(i++, 300 + rnd_below(500))); t += record_text(reads.back()); }
    // the record under test begins at t.size(); its lines: '@' title '\n' seq '\n' '+' plus '\n' qual '\n'
    Read r = make_read(i++, 1);
    const uint64_t fixed0 = t.size() + 1 + r.title.size();                  // the title's newline with the title as it is
    uint64_t len = 1;
    if (kind == 0) { if (fixed0 >= at) return ""; r.title = std::string("x") + std::string(at - fixed0 - 1, 'y') + r.title; if (!r.plus.empty() && !is_blank((uint8_t)r.plus[0])) r.plus = ""; }
    if (kind == 1) { if (fixed0 + 2 > at) return ""; len = at - fixed0 - 1; }
    if (kind == 2) { const uint64_t need = fixed0 + 1 + 1 + 1 + r.plus.size(); if (need + 1 > at) return ""; len = at - need; }
    if (kind == 3) {                                                        // two lines of one length: the rest must be even
        r.plus = "";
        if ((at - (fixed0 + 4)) % 2) r.title += "z";
        const uint64_t need = t.size() + 1 + r.title.size() + 4;
        if (need + 2 > at) return "";
        len = (at - need) / 2;
    }
    const Read shaped = make_read(i, len);
    r.seq = shaped.seq; r.qual = shaped.qual;
    reads.push_back(r);
    for (uint32_t k = 0; k < tail_reads; ++k) reads.push_back(make_read(i++ + 7, 1 + rnd_below(40)));
    return join(reads, final_newline);
}

int main(int argc, char** argv) {
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    uint64_t failed = 0;

    {   // the masks of a vector against their definitions, byte by byte
        Section s{"masks"};
        const uint8_t pool[] = {'\n', '\n', '\t', ' ', 'A', '@', '+', 0x1F, 0x20, 0x21, 0x7F, 0x80, 0xFF, 0x00, '\r', 0x0B, 0x09, 0x8A, 0x89};
        for (int k = 0; k < 4000; ++k) {
            uint8_t b[16];
            for (auto& x : b) x = (k & 1) ? pool[rnd_below(sizeof pool)] : (uint8_t)rnd();
            Vec16 v; memcpy(v.w, b, 16);
            uint32_t nl = 0, ot = 0, os = 0;
            for (uint32_t i = 0; i < 16; ++i) { nl |= (uint32_t)(b[i] == '\n') << i; ot |= (uint32_t)!title_class(b[i]) << i; os |= (uint32_t)!seq_class(b[i]) << i; }
            ++s.cases; if (nl_mask16(v) != nl || odd_title16(v) != ot || odd_seq16(v) != os) ++s.bad;
            const uint32_t valid = k % 5 == 0 ? below(1 + (uint32_t)rnd_below(16)) : 0xFFFFu;
            for (uint32_t kind = 0; kind < 4; ++kind) {
                uint32_t want = 0, kd = kind;
                for (uint32_t i = 0; i < 16; ++i) {
                    if (!((valid >> i) & 1u)) break;
                    if (b[i] == '\n') { kd = (kd + 1) & 3; continue; }
                    if ((kd & 1) ? !seq_class(b[i]) : !title_class(b[i])) want |= 1u << i;
                }
                ++s.cases; if (lines_bad(nl & valid, ot & valid, os & valid, kind) != want) ++s.bad;
            }
        }
        report(s); failed += s.bad;
    }
    {   // a newline of every kind of line (kind 3: the next byte starts a record) at the last byte of a block, the first byte of the
        // next, and around wave, round and lane edges; with and without the final newline
        Section s{"newlines at block edges"};
        const uint64_t edges[] = {1024, FQ_ROUND, FQ_BLOCK, 2ull * FQ_BLOCK};
        for (uint64_t edge : edges) for (int d = -2; d <= 1; ++d) for (uint32_t kind = 0; kind < 4; ++kind) for (int fin = 0; fin < 2; ++fin)
            for (uint32_t tail = 0; tail < 2; ++tail) {
                const std::string t = text_with_newline_at(edge + d, kind, fin != 0, tail * 3);
                // (without a tail and without the final newline the newline under test is cut off: the text then ends at the edge)
                ++s.cases; if (t.empty() || check_parse(t)) ++s.bad;
                if (!t.empty() && (tail || fin) && t[edge + d] != '\n') ++s.bad;
            }
        report(s); failed += s.bad;
    }
    {   // lines longer than two blocks, one record, reads of length 1, every count of reads around a lane's 16 bytes
        Section s{"shapes"};
        for (int fin = 0; fin < 2; ++fin) {
            for (uint32_t which = 0; which < 3; ++which) {
                std::vector<Read> reads;
                for (uint32_t i = 0; i < 5; ++i) reads.push_back(make_read(i, i == 2 && which == 0 ? 2 * FQ_BLOCK + 777 : 1 + rnd_below(30)));
                if (which == 1) reads[3].title = std::string(2 * FQ_BLOCK + 99, 't') + " c";
                if (which == 1) reads[3].plus = "";
                if (which == 2) reads[1].plus = reads[1].title = std::string(2 * FQ_BLOCK + 5, 'u');
                ++s.cases; if (check_parse(join(reads, fin != 0))) ++s.bad;
            }
            for (uint32_t form = 0; form < 6; ++form) for (uint64_t len : {1ull, 2ull, 15ull, 16ull, 17ull, 4000ull, (unsigned long long)FQ_BLOCK}) {
                ++s.cases; if (check_parse(join({make_read(form, len)}, fin != 0))) ++s.bad;
            }
            for (uint32_t n = 1; n <= 40; ++n) {
                std::vector<Read> reads;
                for (uint32_t i = 0; i < n; ++i) reads.push_back(make_read(i + n, 1));
                ++s.cases; if (check_parse(join(reads, fin != 0))) ++s.bad;
            }
        }
        ++s.cases; if (check_parse("")) ++s.bad;
        report(s); failed += s.bad;
    }
    {   // texts that are not plain: the first bad record is the sequential parser's, wherever the fault lies
        Section s{"refusals"};
        uint64_t refused = 0;
        for (uint32_t form = 0; form < 17; ++form) for (uint32_t where = 0; where < 3; ++where) for (int big = 0; big < 2; ++big) {
            std::vector<Read> reads;
            const uint32_t n = big ? 60 : 5;
            for (uint32_t i = 0; i < n; ++i) reads.push_back(make_read(i, big ? 500 + rnd_below(300) : 20 + rnd_below(30)));
            const uint32_t at = where == 0 ? 0 : where == 1 ? n / 2 : n - 1;
            std::vector<std::string> rec;
            for (const Read& r : reads) rec.push_back(record_text(r));
            Read& r = reads[at];
            std::string& x = rec[at];
            switch (form) {
                case 0: x = "@" + r.title + "\n" + r.seq.substr(0, r.seq.size() / 2) + "\n" + r.seq.substr(r.seq.size() / 2) + "\n+\n" + r.qual + "\n"; break;
                case 1: for (size_t p = 0; (p = x.find('\n', p)) != std::string::npos; p += 2) x.insert(p, "\r"); break;
                case 2: x = "\n" + x; break;
                case 3: x += "\n"; break;
                case 16: x.pop_back(); x.pop_back(); break;                            // (the last record: a quality byte short, no newline)
                case 4: r.seq[r.seq.size() / 2] = ' '; x = record_text(r); break;
                case 5: r.title = "a" + std::string(1, (char)0x80) + r.title; r.plus = ""; x = record_text(r); break;
                case 6: r.title = "a" + std::string(1, (char)0x07) + r.title; r.plus = ""; x = record_text(r); break;
                case 7: r.qual.pop_back(); x = record_text(r); break;
                case 8: r.qual.push_back('I'); x = record_text(r); break;
                case 9: r.plus = "other"; x = record_text(r); break;
                case 10: x = x.substr(0, x.size() - r.qual.size() - 1); break;                      // no quality line
                case 11: r.seq = ""; r.qual = ""; x = record_text(r); break;
                case 12: x[0] = '>'; break;
                case 13: r.qual[0] = (char)0x9A; x = record_text(r); break;
                case 14: x = "@" + r.title + "\n" + r.seq + "\n-\n" + r.qual + "\n"; break;
                default: r.plus = std::string(1, (char)0x01); x = record_text(r); break;
            }
            std::string t;
            for (const std::string& y : rec) t += y;
            ++s.cases; if (check_parse(t)) ++s.bad;
            if (sequential(t).bad_record) ++refused;
        }
        if (refused != 17 * 3 * 2) ++s.bad;                                   // (every form is one the sequential parser refuses)
        report(s); failed += s.bad;
    }
    {   // the output text: random trims, empty kept slices and skipped reads, the segment table through the copy schedule against
        // plain concatenation; the bases plane the same way
        Section s{"output text"};
        for (int k = 0; k < 60; ++k) {
            std::vector<Read> reads;
            const uint32_t n = k < 8 ? 1 + (uint32_t)k : 20 + (uint32_t)rnd_below(k < 50 ? 80 : 700);
            for (uint32_t i = 0; i < n; ++i) reads.push_back(make_read(i + k, k % 7 == 0 ? 1 + rnd_below(3) : 1 + rnd_below(k % 3 ? 300 : 1500)));
            const std::string t = join(reads, k % 2 == 0);
            Parsed p; TextPlane* pl = nullptr;
            uint64_t bad = check_parse(t, &p, &pl);
            // bases: segment r = the sequence line of read r
            std::string bases, want_bases;
            for (const Read& r : reads) want_bases += r.seq;
            bad += device_copy(*pl, p.offsets, p.seq_src, p.offsets[n], &bases);
            if (bases != want_bases) ++bad;
            // a sorted order, slices and skips
            std::vector<uint32_t> order(n);
            for (uint32_t i = 0; i < n; ++i) order[i] = i;
            for (uint32_t i = n; i > 1; --i) std::swap(order[i - 1], order[rnd_below(i)]);
            std::vector<uint64_t> seg_off((size_t)FQ_SEGS * n + 1, 0), seg_src((size_t)FQ_SEGS * n, 0);
            std::string want;
            for (uint32_t j = 0; j < n; ++j) {
                const Read& r = reads[order[j]];
                const uint64_t len = r.seq.size();
                const bool skipped = rnd_below(10) == 0;
                const bool trimming = rnd_below(4) != 0;
                const int64_t t5 = (int64_t)rnd_below(len + 3), t3 = rnd_below(6) == 0 ? t5 : (int64_t)rnd_below(len + 3);
                uint64_t a, keep;
                qpart::slice_of((int64_t)len, t5, t3, trimming, &a, &keep);
                record_segments(p.recs[order[j]], a, keep, skipped, pl->n_bytes, &seg_off[(size_t)FQ_SEGS * j], &seg_src[(size_t)FQ_SEGS * j]);
                if (skipped) continue;
                std::string title = r.title;
                while (!title.empty() && is_blank((uint8_t)title.back())) title.pop_back();
                std::replace(title.begin(), title.end(), '\t', ' ');
                if (title.find(' ') == std::string::npos) title += " ";
                want += "@" + title + "\n" + r.seq.substr(a, keep) + "\n+\n" + r.qual.substr(a, keep) + "\n";
            }
            uint64_t run = 0;
            for (size_t i = 0; i < seg_off.size(); ++i) { const uint64_t c = seg_off[i]; seg_off[i] = run; run += c; }
            std::string got;
            const uint64_t bound = output_bound(pl->n_bytes, n);
            bad += device_copy(*pl, seg_off, seg_src, bound, &got);
            if (got != want || run > bound) ++bad;
            delete pl;
            ++s.cases; if (bad) ++s.bad;
        }
        {   // the bound is reached within 2 n + 1 bytes by the shortest records without a final newline
            std::vector<Read> reads;
            for (uint32_t i = 0; i < 9; ++i) { Read r = make_read(5, 1); r.title = ""; r.plus = ""; reads.push_back(r); }
            const std::string t = join(reads, false);
            uint64_t out = 0;
            for (const Read& r : reads) out += 1 + 1 + 1 + r.seq.size() + 3 + r.qual.size() + 1;
            ++s.cases; if (out > output_bound(t.size(), reads.size())) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    return failed ? 1 : 0;
}

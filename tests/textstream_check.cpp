// textstream_check.cpp -- the new passes of qcat_batch_upload_text and qcat_batch_annot_text (qcat_amd/csrc/kernels_textstream.inc)
// run on the host through the functions the kernels themselves call:
//   * the FASTA record pass -- k_fq_lines' byte classes by the parity of a line's kind, then one lane per two-line record with
//     the blame rule of qcat_amd/csrc/fqtext_core.h (fa_record_of, fa_blamed_line) -- against a sequential restatement of
//     fa_parse (qcat_amd/csrc/fastq_host.inc);
//   * the stream's segment tables (qcat_amd/csrc/textstream_core.h: record_segments over the id slots of qtsv::tables_build)
//     through the chunk and lane schedule of k_annot_copy -- qpart::gather_vectors<1> with a load that picks one of TWO planes --
//     against plain concatenation.
// Both planes are allocated with exactly the device's slack; every load is checked against its plane, every store against the
// output's allocation and its one owner.
// Built twice by tests/test_textstream_host.py: plain, and with -fsanitize=address,undefined.
//   usage: textstream_check <seed>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "textstream_core.h"
#include "check_common.h"

using namespace qfq;
using qpart::Vec16;

// the text plane of a text: the text, the constants block
static Plane text_plane(const std::string& t) {
    std::vector<uint8_t> p(t.size() + FQ_CONST_BYTES, 0);
    if (!t.empty()) memcpy(p.data(), t.data(), t.size());
    fq_constants(p.data() + t.size());
    return Plane(p);
}

// ---- FASTA: the expected values, fa_parse restated byte by byte ---------------------------------------------------------------------
struct Want { std::vector<Rec> recs; uint64_t bad_record = 0; };     // bad_record: 1-based, 0 = the text is plain
static bool title_class(uint8_t c) { return !((c < 0x20 && c != '\t') || c >= 0x80); }
static bool seq_class(uint8_t c) { return c > 0x20 && c < 0x80; }
static Want fa_sequential(const std::string& t) {
    Want w;
    size_t p = 0;
    const size_t end = t.size();
    auto fail = [&]() { w.bad_record = w.recs.size() + 1; return w; };
    while (p < end) {
        if (t[p] != '>') return fail();
        const size_t l1 = t.find('\n', p);
        if (l1 == std::string::npos) return fail();
        const size_t s = l1 + 1;
        size_t l2 = t.find('\n', s);
        const size_t se = l2 == std::string::npos ? end : l2;
        if (se == s) return fail();
        for (size_t i = s; i < se; ++i) if (!seq_class((uint8_t)t[i])) return fail();
        const size_t next = l2 == std::string::npos ? end : l2 + 1;
        if (next < end && t[next] != '>') return fail();
        std::string title = t.substr(p + 1, l1 - p - 1);
        for (char c : title) if (!title_class((uint8_t)c)) return fail();
        while (!title.empty() && is_blank((uint8_t)title.back())) title.pop_back();
        Rec r{};
        r.title_off = p + 1; r.title_len = (uint32_t)title.size(); r.seq_off = s; r.seq_len = (uint32_t)(se - s); r.qual_off = 0;
        r.title_blank = title.find_first_of(" \t") != std::string::npos;
        w.recs.push_back(r);
        p = next;
    }
    return w;
}

struct Parsed { std::vector<Rec> recs; std::vector<uint64_t> lens; uint64_t bad_line = FQ_NO_LINE; uint64_t faults = 0; };
// the line table (as k_fq_count / k_fq_lines leave it: fqtext_check.cpp holds their schedule to it), the byte classes of every
// vector by the kind of its first byte's line, k_fa_records
static Parsed fa_device_parse(Plane& pl, uint64_t n_bytes) {
    Parsed out;
    const uint8_t* text = pl.at0();
    std::vector<uint64_t> line_start(1, 0);
    for (uint64_t i = 0; i < n_bytes; ++i) if (text[i] == '\n') line_start.push_back(i + 1);
    const uint64_t newlines = line_start.size() - 1;
    const uint64_t n_lines = n_bytes ? lines_of(newlines, text[n_bytes - 1] == '\n') : 0;
    if (n_lines > newlines) line_start.push_back(n_bytes + 1);
    uint64_t line = 0;
    for (uint64_t off = 0; off < n_bytes; off += FQ_VEC) {
        const uint32_t valid = n_bytes - off >= FQ_VEC ? 0xFFFFu : below((uint32_t)(n_bytes - off));
        const Vec16 v = pl.load16((int64_t)off);
        const uint32_t nl = nl_mask16(v) & valid;
        const uint32_t bad = lines_bad(nl, odd_title16(v) & valid, odd_seq16(v) & valid, (uint32_t)(line & 3u));
        if (bad) out.bad_line = std::min(out.bad_line, line + popc32(nl & below((uint32_t)__builtin_ctz(bad))));
        line += popc32(nl);
    }
    const uint64_t n_rec = fa_records_of(n_lines);
    out.recs.assign(n_rec, Rec{});
    out.lens.assign(n_rec, 0);
    for (uint64_t r = 0; r < n_rec; ++r) {                                  // k_fa_records
        const uint32_t lines = 2 * r + 2 <= n_lines ? 2u : 1u;
        uint64_t ls[3] = {0, 0, 0};
        for (uint32_t i = 0; i <= lines; ++i) ls[i] = line_start.at(2 * r + i);
        Rec rec;
        const auto at = [&](uint64_t i) { if (i >= n_bytes) { ++out.faults; return (uint8_t)0; } return text[i]; };
        const uint32_t verdict = fa_record_of(at, ls, lines, &rec);
        if (verdict != FA_OK) { out.bad_line = std::min(out.bad_line, fa_blamed_line(r, verdict)); continue; }
        out.recs[r] = rec; out.lens[r] = rec.seq_len;
    }
    out.faults += pl.stray;
    return out;
}

static uint64_t fa_check(const std::string& t) {
    const Want w = fa_sequential(t);
    Plane pl = text_plane(t);
    const Parsed p = fa_device_parse(pl, t.size());
    uint64_t bad = p.faults;
    const uint64_t got_bad = p.bad_line == FQ_NO_LINE ? 0 : fa_record_of_line(p.bad_line);
    if (got_bad != w.bad_record) ++bad;
    if (!w.bad_record) {
        if (p.recs.size() != w.recs.size()) ++bad;
        else for (size_t r = 0; r < w.recs.size(); ++r) {
            const Rec &a = p.recs[r], &b = w.recs[r];
            if (a.title_off != b.title_off || a.title_len != b.title_len || a.seq_off != b.seq_off || a.seq_len != b.seq_len ||
                a.qual_off != 0 || a.title_blank != b.title_blank || p.lens[r] != b.seq_len) ++bad;
        }
    }
    return bad;
}

static const char* TITLE_FORMS[] = {"r%u", "r%u ch=3", "r%u\tch=3\tx=y", "r%u  two", "r%u ", ""};
static std::string title_of(uint32_t i) {
    char buf[64];
    snprintf(buf, sizeof buf, TITLE_FORMS[i % 6], i);
    return buf;
}
static std::string bases_of(uint64_t len) {
    std::string s;
    for (uint64_t k = 0; k < len; ++k) s.push_back("ACGTN"[rnd_below(5)]);
    return s;
}
static std::string quals_of(uint64_t len) {
    std::string s;
    for (uint64_t k = 0; k < len; ++k) s.push_back((char)(0x21 + rnd_below(0x5F)));
    return s;
}

// ---- the stream: k_annot_segments' table through k_part_chunks / k_annot_copy --------------------------------------------------------
// Returns the faults; the output in *dst_out; *global: a chunk searched the global arrays (more than PART_LDS_SEGS segments)
static uint64_t stream_copy(Plane& text, Plane& tags, const std::vector<uint64_t>& dst_off, const std::vector<uint64_t>& src_pos, uint64_t bound,
                            std::string* dst_out, bool* global) {
    const CopyRun r = copy_schedule(dst_off, src_pos, bound,
                                    [&](uint32_t, int64_t a) { return (qann::src_in_tag(a) ? tags : text).load16(qann::src_plane_off(a)); });
    if (r.global_chunks && global) *global = true;
    dst_out->assign(reinterpret_cast<const char*>(r.out.data()), std::min<size_t>(dst_off.back(), r.out.size()));
    return r.bad + text.stray + tags.stray;
}

// the id tables of the check: two templates, ids of 1 to 11 characters
static const int32_t IDS_A[] = {1, 12, 123, 1234, 12345, 123456, 1234567, 12345678, 123456789, 1234567890, -2147483647 - 1, 7};
static const int32_t IDS_B[] = {-1, 96, 5, 2147483647, 40};
static const int32_t IDS_A2[] = {3, -77, 100000};
static const int32_t IDS_B2[] = {9, 88, -2147483647 - 1, 12};
struct Tags {
    qtsv::Tables T;
    uint64_t const_off;
    Plane plane;
    uint32_t n_ids[4];
};
static Tags* make_tags(bool simple, bool dual) {
    const uint32_t n_ids[4] = {12, dual ? 3u : 0u, 5, dual ? 4u : 0u};
    const int32_t* ids[4] = {IDS_A, dual ? IDS_A2 : nullptr, IDS_B, dual ? IDS_B2 : nullptr};
    const char* kits[2] = {nullptr, nullptr};
    qtsv::ScoreTable none;
    for (uint32_t i = 0; i <= qtsv::TSV_MAX_DEN; ++i) none.den_first[i] = none.den_last[i] = -1;
    std::vector<uint8_t> blob;
    qtsv::Tables T;
    uint32_t den_off = 0;
    if (!qtsv::tables_build(simple, dual, simple ? 1u : 2u, n_ids, ids, kits, none, &blob, &T, &den_off).empty()) return nullptr;
    const uint64_t const_off = qann::tag_const_off(blob.size());
    blob.resize((size_t)qann::tag_plane_bytes(blob.size()), 0);
    qann::annot_constants(blob.data() + const_off);
    Tags* t = new Tags{T, const_off, Plane(blob), {n_ids[0], n_ids[1], n_ids[2], n_ids[3]}};
    t->T.blob = t->plane.at0();
    t->T.den_first = reinterpret_cast<const int32_t*>(t->plane.at0() + den_off);
    t->T.den_last = t->T.den_first + (qtsv::TSV_MAX_DEN + 1);
    return t;
}

struct Read { std::string title, seq, qual; int32_t bc, bc2, adapter; bool skipped; uint64_t a, keep; };
// the stored title of a read, as the plane holds it after the parse
static std::string stored_title(const std::string& title) {
    std::string s = title;
    while (!s.empty() && is_blank((uint8_t)s.back())) s.pop_back();
    std::replace(s.begin(), s.end(), '\t', ' ');
    return s;
}
static std::string id_text(const Tags& g, const Read& r) {
    if (!qtsv::called(g.T, r.bc, r.bc2, r.adapter)) return "none";
    const uint32_t t = g.T.simple ? 0u : (uint32_t)r.adapter;
    const int32_t* const first[2] = {IDS_A, IDS_B}; const int32_t* const second[2] = {IDS_A2, IDS_B2};
    std::string s = std::to_string(first[t][r.bc]);
    if (g.T.dual) s += "/" + std::to_string(second[t][r.bc2]);
    return s;
}
static std::string want_record(const Tags& g, const Read& r, bool fasta) {
    if (r.skipped) return "";
    const std::string title = stored_title(r.title);
    std::string s = (fasta ? ">" : "@") + title + (title.find(' ') == std::string::npos ? "  " : " ") + "barcode=" + id_text(g, r) + "\n" +
                    r.seq.substr(r.a, r.keep);
    if (!fasta) s += "\n+\n" + r.qual.substr(r.a, r.keep);
    return s + "\n";
}
// the text of the reads, its record table and text plane (stored titles: tabs as blanks), the segment table, the copy; faults
static uint64_t stream_check(const Tags& g0, std::vector<Read>& reads, bool fasta, bool final_newline, bool* global = nullptr, uint64_t* total_out = nullptr) {
    Tags& g = const_cast<Tags&>(g0);
    std::string t;
    std::vector<Rec> recs;
    for (const Read& r : reads) {
        Rec rec{};
        const std::string st = stored_title(r.title);
        rec.title_off = t.size() + 1; rec.title_len = (uint32_t)st.size(); rec.title_blank = st.find(' ') != std::string::npos;
        t += (fasta ? ">" : "@") + r.title + "\n";
        rec.seq_off = t.size(); rec.seq_len = (uint32_t)r.seq.size();
        t += r.seq + "\n";
        if (!fasta) { t += "+\n"; rec.qual_off = t.size(); t += r.qual + "\n"; }
        recs.push_back(rec);
    }
    if (!final_newline && !t.empty()) t.pop_back();
    Plane text = text_plane(t);
    for (const Rec& rec : recs) for (uint32_t i = 0; i < rec.title_len; ++i) if (text.at0()[rec.title_off + i] == '\t') text.at0()[rec.title_off + i] = ' ';
    const size_t n = reads.size();
    std::vector<uint64_t> seg_off(qann::ANNOT_SEGS * n + 1, 0), seg_src(qann::ANNOT_SEGS * n, 0);
    std::string want;
    for (size_t r = 0; r < n; ++r) {
        const Read& x = reads[r];
        qann::record_segments(g.T, recs[r], fasta, x.a, x.keep, x.skipped, x.bc, x.bc2, x.adapter, g.const_off, &seg_off[qann::ANNOT_SEGS * r],
                              &seg_src[qann::ANNOT_SEGS * r]);
        want += want_record(g, x, fasta);
    }
    uint64_t run = 0;
    for (size_t i = 0; i < seg_off.size(); ++i) { const uint64_t c = seg_off[i]; seg_off[i] = run; run += c; }
    const uint64_t bound = qann::output_bound(t.size(), n, g.T);
    std::string got;
    uint64_t bad = stream_copy(text, g.plane, seg_off, seg_src, bound, &got, global);
    g.plane.stray = 0;
    if (got != want || run > bound) ++bad;
    if (total_out) *total_out = run;
    return bad;
}
static Read make_read(const Tags& g, uint32_t i, uint64_t len) {
    Read r;
    r.title = title_of(i); r.seq = bases_of(len); r.qual = quals_of(len);
    const uint32_t t = g.T.simple ? 0u : (uint32_t)rnd_below(2);
    r.adapter = g.T.simple ? -1 : (int32_t)t;
    r.bc = (int32_t)rnd_below(g.n_ids[2 * t]); r.bc2 = g.T.dual ? (int32_t)rnd_below(g.n_ids[2 * t + 1]) : -1;
    switch (rnd_below(8)) {                                                 // reads without a call, in every way the writer knows
        case 0: r.bc = -1; break;
        case 1: if (!g.T.simple) r.adapter = -1; else r.adapter = 0; break;
        case 2: if (g.T.dual) r.bc2 = -1; break;
        default: break;
    }
    r.skipped = false; r.a = 0; r.keep = len;
    return r;
}
static void random_slice(Read& r) {
    const uint64_t len = r.seq.size();
    const int64_t t5 = (int64_t)rnd_below(len + 3), t3 = rnd_below(5) == 0 ? t5 : (int64_t)rnd_below(len + 3);
    qpart::slice_of((int64_t)len, t5, t3, rnd_below(4) != 0, &r.a, &r.keep);
    r.skipped = rnd_below(10) == 0;
}

int main(int argc, char** argv) {
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    uint64_t failed = 0;

    {   // plain FASTA texts: counts of records around a lane's 16 bytes, reads of length 1, long lines, every title form
        Section s{"fasta shapes"};
        for (int fin = 0; fin < 2; ++fin) {
            for (uint32_t n = 0; n <= 40; ++n) {
                std::string t;
                for (uint32_t i = 0; i < n; ++i) t += ">" + title_of(i + n) + "\n" + bases_of(n % 3 ? 1 : 1 + rnd_below(50)) + "\n";
                if (!fin && !t.empty()) t.pop_back();
                ++s.cases; if (fa_check(t) || fa_sequential(t).bad_record) ++s.bad;
            }
            for (uint32_t which = 0; which < 2; ++which) {
                std::string t;
                for (uint32_t i = 0; i < 5; ++i)
                    t += ">" + (which == 1 && i == 3 ? std::string(2 * FQ_BLOCK + 99, 't') + " c" : title_of(i)) + "\n" +
                         bases_of(which == 0 && i == 2 ? 2 * FQ_BLOCK + 777 : 1 + rnd_below(30)) + "\n";
                if (!fin) t.pop_back();
                ++s.cases; if (fa_check(t) || fa_sequential(t).bad_record) ++s.bad;
            }
        }
        report(s); failed += s.bad;
    }
    {   // texts that are not plain: the record named is fa_parse's -- the one in FRONT of a line that should begin with '>'
        Section s{"fasta refusals"};
        uint64_t refused = 0, front = 0;
        const uint32_t forms = 14;
        for (uint32_t form = 0; form < forms; ++form) for (uint32_t where = 0; where < 3; ++where) for (int fin = 0; fin < 2; ++fin) for (int big = 0; big < 2; ++big) {
            const uint32_t n = big ? 61 : 9;
            std::vector<std::string> titles, seqs, rec;
            for (uint32_t i = 0; i < n; ++i) {
                titles.push_back(title_of(i)); seqs.push_back(bases_of(big ? 500 + rnd_below(300) : 20 + rnd_below(30)));
                rec.push_back(">" + titles[i] + "\n" + seqs[i] + "\n");
            }
            const uint32_t at = where == 0 ? 0 : where == 1 ? n / 2 : n - 1;
            std::string& x = rec[at];
            const std::string& q = seqs[at];
            switch (form) {
                case 0: x = ">" + titles[at] + "\n" + q.substr(0, q.size() / 2) + "\n" + q.substr(q.size() / 2) + "\n"; break;   // wrapped
                case 1: for (size_t p = 0; (p = x.find('\n', p)) != std::string::npos; p += 2) x.insert(p, "\r"); break;        // CRLF
                case 2: x = "\n" + x; break;                                                // a blank line in front (at 0: no '>' first)
                case 3: x += "\n"; break;                                                   // a blank line behind (the last: trailing)
                case 4: x = ">" + titles[at] + "\n" + q.substr(0, q.size() / 2) + " " + q.substr(q.size() / 2) + "\n"; break;
                case 5: x = ">a" + std::string(1, (char)0x80) + titles[at] + "\n" + q + "\n"; break;
                case 6: x = ">a" + std::string(1, (char)0x07) + titles[at] + "\n" + q + "\n"; break;
                case 7: x = ">" + titles[at] + "\n\n"; break;                               // an empty sequence
                case 8: x = ">" + titles[at] + "\n"; break;                                 // a title line without a sequence
                case 9: x = "@" + titles[at] + "\n" + q + "\n+\n" + quals_of(q.size()) + "\n"; break;   // a four-line FASTQ record
                case 10: x = ">" + titles[at] + "\n" + q.substr(0, q.size() / 2) + "\n" + std::string(1, (char)0x80) + q.substr(q.size() / 2) + "\n"; break;
                case 11: x = ">" + titles[at] + "\n" + q.substr(0, q.size() / 2) + std::string(1, (char)0x9A) + q.substr(q.size() / 2) + "\n"; break;
                case 12: x = ">" + titles[at] + "\n" + q + "\n\t\n"; break;                 // a line of a tab behind the sequence
                default: x = ">" + titles[at]; break;                                       // a title line without its newline
            }
            std::string t;
            for (const std::string& y : rec) t += y;
            if (!fin && !t.empty() && t.back() == '\n') t.pop_back();
            if (t.empty() || t[0] != '>') continue;                                         // (the dispatch sends such a text the FASTQ way)
            ++s.cases; if (fa_check(t)) ++s.bad;
            const uint64_t named = fa_sequential(t).bad_record;
            if (named) ++refused;
            if (named && named == at) ++front;                                              // the record in front of the changed one
        }
        // plain after all: a title line without its newline in front of another record (its title grows), and a blank line
        // behind the last record without the final newline; a blank line or a FASTQ record in the middle name the record in front
        if (refused != s.cases - (2 * 2 * 2 + 2) || front != 2 * (2 * 2 * 2)) ++s.bad;
        printf("fasta refusals: %llu refused, %llu name the record in front\n", (unsigned long long)refused, (unsigned long long)front);
        report(s); failed += s.bad;
    }
    Tags* kits[3] = {make_tags(false, false), make_tags(false, true), make_tags(true, false)};
    if (!kits[0] || !kits[1] || !kits[2]) { printf("tables_build failed\n"); return 1; }
    {   // every id of the tables, dual ids, none; titles with and without a blank and empty; FASTQ and FASTA
        Section s{"stream records"};
        for (uint32_t kit = 0; kit < 3; ++kit) for (int fasta = 0; fasta < 2; ++fasta) for (int fin = 0; fin < 2; ++fin) {
            const Tags& g = *kits[kit];
            std::vector<Read> reads;
            uint32_t i = 0;
            for (uint32_t t = 0; t < (g.T.simple ? 1u : 2u); ++t) for (uint32_t b = 0; b < g.n_ids[2 * t]; ++b) for (uint32_t form = 0; form < 6; ++form) {
                Read r = make_read(g, form, 1 + rnd_below(60));
                r.adapter = g.T.simple ? -1 : (int32_t)t; r.bc = (int32_t)b; r.bc2 = g.T.dual ? (int32_t)((b + form) % g.n_ids[2 * t + 1]) : -1;
                if (form == 5 && b % 3 == 0) r.bc = -1;
                reads.push_back(r); ++i;
            }
            ++s.cases; if (stream_check(g, reads, fasta != 0, fin != 0)) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // random trims, empty kept slices, dropped reads -- at either end too --, one read, no read
        Section s{"stream slices"};
        for (int k = 0; k < 60; ++k) {
            const Tags& g = *kits[k % 3];
            std::vector<Read> reads;
            const uint32_t n = k < 6 ? (uint32_t)k / 2 : 20 + (uint32_t)rnd_below(k < 50 ? 80 : 500);
            for (uint32_t i = 0; i < n; ++i) { reads.push_back(make_read(g, i + k, k % 7 == 0 ? 1 + rnd_below(3) : 1 + rnd_below(k % 3 ? 300 : 1500))); random_slice(reads.back()); }
            if (n > 2 && k % 2) reads[0].skipped = reads[n - 1].skipped = true;
            if (n > 2 && k % 4 == 2) { reads[0].skipped = true; reads[1].skipped = true; reads[n - 1].keep = 0; }
            ++s.cases; if (stream_check(g, reads, (k / 3) % 2 != 0, k % 5 != 0)) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // a record that ends one byte before, at and one byte behind a chunk edge, stretched by its sequence (FASTA) or its title
        Section s{"stream chunk edges"};
        for (int d = -1; d <= 1; ++d) for (int fasta = 0; fasta < 2; ++fasta) for (uint32_t kit = 0; kit < 3; ++kit) for (uint32_t edge = 1; edge <= 2; ++edge) {
            const Tags& g = *kits[kit];
            std::vector<Read> reads;
            for (uint32_t i = 0; i < 40 * edge; ++i) reads.push_back(make_read(g, i, 200 + rnd_below(300)));
            uint64_t front = 0;
            for (const Read& r : reads) front += want_record(g, r, fasta != 0).size();
            Read r = make_read(g, 1, 10);                                       // ("r1 ch=3": a title with a blank)
            const uint64_t base = want_record(g, r, fasta != 0).size(), target = (uint64_t)edge * qpart::PART_CHUNK + (uint64_t)(int64_t)d;
            if (front + base > target) { ++s.cases; ++s.bad; continue; }
            const uint64_t pad = target - front - base;
            if (fasta) { r.seq += bases_of(pad); r.keep = r.seq.size(); } else r.title += std::string(pad, 'x');
            reads.push_back(r);
            uint64_t upto = 0;
            for (const Read& x : reads) upto += want_record(g, x, fasta != 0).size();
            for (uint32_t i = 0; i < 5; ++i) reads.push_back(make_read(g, i + 3, 100 + rnd_below(100)));
            ++s.cases; if (upto != target || stream_check(g, reads, fasta != 0, true)) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // more than PART_LDS_SEGS segments in a chunk: short records and runs of dropped reads; the global-array path is taken
        Section s{"stream beyond the LDS table"};
        for (int k = 0; k < 6; ++k) {
            const Tags& g = *kits[k % 3];
            std::vector<Read> reads;
            for (uint32_t i = 0; i < 3000; ++i) {
                reads.push_back(make_read(g, i, 1 + rnd_below(40)));
                if (k >= 3) random_slice(reads.back());
                if (k == 5 && i > 200 && i < 1400) reads.back().skipped = true;
            }
            bool global = false;
            uint64_t total = 0;
            ++s.cases; if (stream_check(g, reads, k % 2 != 0, true, &global, &total) || !global || total <= qpart::PART_CHUNK) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // a tag-plane segment and a text-plane segment that start at every offset mod 16, land at every offset mod 16 and have
        // every length from 0 to 40, side by side in one table
        Section s{"two planes at every alignment"};
        Tags& g = *kits[1];
        const std::string t = ">" + bases_of(300) + "\n" + bases_of(700) + "\n";
        Plane text = text_plane(t);
        const uint64_t tag_bytes = g.plane.mem.size() - 2 * qpart::PART_SLACK;
        for (uint32_t lead = 0; lead < 16; ++lead) for (uint32_t so = 0; so < 16; ++so) {
            std::vector<uint64_t> seg_off(1, 0), seg_src;
            std::string want;
            auto add = [&](bool tag, uint64_t src, uint64_t len) {
                seg_src.push_back(tag ? qann::ANNOT_TAG | src : src);
                seg_off.push_back(seg_off.back() + len);
                want.append(reinterpret_cast<const char*>((tag ? g.plane.at0() : text.at0()) + src), len);
            };
            add(false, 1, lead);                                                // moves the next segment's destination
            for (uint32_t len = 0; len <= 40; ++len) {
                add(true, so + 16 * (len % 5), len);
                add(false, so + len, len);
                add(true, tag_bytes - len, len);                                // the plane's last bytes (the constants' padding)
                add(true, 0, len % 3);                                          // the plane's first bytes
            }
            std::string got;
            const uint64_t bad = stream_copy(text, g.plane, seg_off, seg_src, seg_off.back() + 5, &got, nullptr);
            g.plane.stray = 0; text.stray = 0;
            ++s.cases; if (bad || got != want) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    {   // the bound is reached within n (11 + id) + 1 bytes by the shortest records without a final newline
        Section s{"bound"};
        for (int fasta = 0; fasta < 2; ++fasta) for (uint32_t kit = 0; kit < 3; ++kit) {
            const Tags& g = *kits[kit];
            std::vector<Read> reads;
            for (uint32_t i = 0; i < 9; ++i) {
                Read r = make_read(g, 5, 1);
                r.adapter = g.T.simple ? -1 : 0; r.bc = 10; r.bc2 = g.T.dual ? 2 : -1;       // the longest ids of template 0
                reads.push_back(r);
            }
            uint64_t total = 0;
            ++s.cases; if (stream_check(g, reads, fasta != 0, false, nullptr, &total)) ++s.bad;
        }
        report(s); failed += s.bad;
    }
    for (Tags* g : kits) delete g;
    return failed ? 1 : 0;
}

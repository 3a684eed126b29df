// tsvtext_check.cpp -- the passes of qcat_batch_tsv_text (qcat_amd/csrc/kernels_tsvtext.inc) run on the host, tile by tile, group
// by group and lane by lane, through the functions of qcat_amd/csrc/tsvtext_core.h that the kernels themselves call: the
// decimal digits, the name of a title, the `called` predicate, the fields of a row, its length and bytes, the rows of a tile,
// what a lane writes of a row into the tile, and which vectors are stored whole -- with the tables built by the header's own
// builder.  Every byte of a tile must be written exactly once before it is stored, every store must lie inside the output.
// Expected values: snprintf, a plain split of the title, and plain sequential concatenation written here.
// Built twice by tests/test_tsvtext_host.py: plain, and with -fsanitize=address,undefined.
//   usage: tsvtext_check <seed>          the sections below
//          tsvtext_check --scores        "den raw text" of the score table for denominators 1..200, raw 0..den
#include <algorithm>
#include <charconv>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tsvtext_core.h"
#include "check_common.h"

using namespace qtsv;

// Python's repr(float) for the doubles a score can be, as the library's fq_repr_double (fastq_host.inc) writes it: the shortest
// digits that round-trip in fixed notation, ".0" behind an integer
static size_t repr_double(double v, char* out) {
    auto r = std::to_chars(out, out + 40, v, std::chars_format::fixed);
    size_t n = (size_t)(r.ptr - out);
    bool dot = false;
    for (size_t i = 0; i < n; ++i) dot = dot || out[i] == '.';
    if (!dot) { out[n++] = '.'; out[n++] = '0'; }
    return n;
}

// ---- decimal digits against snprintf -----------------------------------------------------------------------------------------------
static void decimal_u(Section& s, uint32_t v) {
    char want[16];
    const int n = snprintf(want, sizeof want, "%u", v);
    std::string got;
    const uint32_t len = dec_len_u32(v);
    for (uint32_t k = 0; k < len; ++k) got.push_back((char)dec_char_u32(v, len, k));
    s.cases++; if ((int)len != n || got != want) s.bad++;
}
static void decimal_i(Section& s, int32_t v) {
    char want[16];
    const int n = snprintf(want, sizeof want, "%d", v);
    std::string got;
    const uint32_t len = dec_len_i32(v);
    for (uint32_t k = 0; k < len; ++k) got.push_back((char)dec_char_i32(v, len, k));
    s.cases++; if ((int)len != n || got != want) s.bad++;
}
static void test_decimal() {
    Section s{"decimal"};
    decimal_u(s, 0); decimal_i(s, 0);
    uint32_t p = 1;
    for (int k = 1; k <= 9; ++k) {
        p *= 10;
        for (int d = -1; d <= 1; ++d) { decimal_u(s, p + (uint32_t)d); decimal_i(s, (int32_t)p + d); decimal_i(s, -((int32_t)p + d)); }
    }
    decimal_u(s, UINT32_MAX); decimal_i(s, INT32_MAX); decimal_i(s, INT32_MIN); decimal_i(s, INT32_MIN + 1); decimal_i(s, -1);
    for (int i = 0; i < 2000; ++i) {
        const uint32_t bits = (uint32_t)rnd_below(33);
        const uint32_t v = bits >= 32 ? (uint32_t)rnd() : (uint32_t)rnd() & ((1u << bits) - 1u);
        decimal_u(s, v); decimal_i(s, (int32_t)(uint32_t)rnd() >> (int)rnd_below(32));
    }
    report(s);
}

// ---- a batch as the device holds it ------------------------------------------------------------------------------------------------
struct Read {
    std::string title;                                     // as stored: right-stripped, tabs as blanks
    uint32_t keep = 0;
    bool dropped = false;
    int32_t bc = -1, bc2 = -1, adapter = -1, adapter_end = 0, raw = 0, den = 1;
};
struct Kit {
    bool simple = false, dual = false;
    uint32_t nt = 0;
    std::vector<std::vector<int32_t>> ids, ids2;           // per template
    std::vector<std::string> kit_name;                     // "" : NULL
    std::vector<int32_t> dens, max_raw;
};
struct Built {
    std::vector<uint8_t> blob;
    Tables T;
    ScoreTable scores;
};
static bool build_tables(const Kit& k, Built* b) {
    if (!score_table_build(k.dens, k.max_raw, repr_double, &b->scores).empty()) return false;
    std::vector<uint32_t> n_ids(2 * k.nt);
    std::vector<const int32_t*> ids(2 * k.nt);
    std::vector<const char*> names(k.nt);
    for (uint32_t t = 0; t < k.nt; ++t) {
        n_ids[2 * t] = (uint32_t)k.ids[t].size(); ids[2 * t] = k.ids[t].data();
        n_ids[2 * t + 1] = k.dual ? (uint32_t)k.ids2[t].size() : 0; ids[2 * t + 1] = k.dual ? k.ids2[t].data() : nullptr;
        names[t] = k.kit_name[t].empty() ? nullptr : k.kit_name[t].c_str();
    }
    uint32_t den_off = 0;
    return tables_build(k.simple, k.dual, k.nt, n_ids.data(), ids.data(), names.data(), b->scores, &b->blob, &b->T, &den_off).empty();
}

// the expected row: FqWriter::write_range restated with printf
static std::string want_row(const Kit& k, const Read& r) {
    if (r.dropped) return std::string();
    const size_t sp = r.title.find_first_of(" \t");
    const std::string name = r.title.substr(0, sp), comment = sp == std::string::npos ? "None" : r.title.substr(sp + 1);
    std::string row = name + "\t" + std::to_string(r.keep) + "\t";
    bool call = k.simple ? (r.bc >= 0 && r.adapter == -1) : (r.bc >= 0 && r.adapter >= 0 && r.adapter < (int32_t)k.nt);
    const size_t t = k.simple ? 0 : (size_t)r.adapter;
    if (call) call = (size_t)r.bc < k.ids[t].size() && (!k.dual || (r.bc2 >= 0 && (size_t)r.bc2 < k.ids2[t].size()));
    if (call) {
        char score[48];
        const size_t sl = repr_double((double)r.raw * 100.0 / (1.0 * (double)r.den), score);
        row += std::to_string(k.ids[t][(size_t)r.bc]);
        if (k.dual) row += "/" + std::to_string(k.ids2[t][(size_t)r.bc2]);
        row += "\t" + std::string(score, sl) + "\t" + (k.simple || k.kit_name[t].empty() ? std::string("None") : k.kit_name[t]) + "\t" +
               std::to_string(r.adapter_end) + "\t";
    } else row += "none\t-1\tnone\t-1\t";
    return row + comment + "\n";
}

// the passes: lengths, scan, tiles, writer.  Returns mismatches (0 or 1).
static uint64_t run_batch(const Kit& k, const std::vector<Read>& reads) {
    Built B;
    if (!build_tables(k, &B)) return 1;
    const uint32_t n = (uint32_t)reads.size();
    // the text plane: the titles one behind the other with a byte between them (the sequences are not looked at)
    std::vector<uint8_t> text;
    std::vector<uint64_t> title_off(n);
    for (uint32_t r = 0; r < n; ++r) {
        text.push_back('@');
        title_off[r] = text.size();
        text.insert(text.end(), reads[r].title.begin(), reads[r].title.end());
    }
    text.push_back('\n');
    std::string want;
    std::vector<uint64_t> want_first(n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) { want_first[r] = want.size(); want += want_row(k, reads[r]); }
    want_first[n] = want.size();
    // k_tsv_lengths
    std::vector<uint64_t> row_first(n + 1, 0);
    std::vector<uint32_t> nlen(n, 0), keep(n, 0);
    uint64_t title_bytes = 0;
    for (uint32_t r = 0; r < n; ++r) {
        const Read& x = reads[r];
        title_bytes += x.title.size();
        if (x.dropped) continue;
        const bool blank = x.title.find(' ') != std::string::npos;
        const uint32_t nl = name_len(text.data() + title_off[r], (uint32_t)x.title.size(), blank);
        Row row;
        if (!row_of(B.T, title_off[r], (uint32_t)x.title.size(), nl, x.keep, x.bc, x.bc2, x.adapter, x.adapter_end, x.raw, x.den, &row)) return 1;
        row_first[r] = row_len(row); nlen[r] = nl; keep[r] = x.keep;
    }
    // the scan
    uint64_t run = 0;
    for (uint32_t r = 0; r <= n; ++r) { const uint64_t l = row_first[r]; row_first[r] = run; run += l; }
    const uint64_t total = row_first[n];
    if (row_first != want_first) return 1;
    const uint64_t bound = output_bound(title_bytes, n, B.T);
    if (total > bound) return 1;
    // k_tsv_tiles
    const uint64_t max_tiles = tiles_of(bound);
    std::vector<uint32_t> tile_first(max_tiles + 1, 0xFFFFFFFFu);
    const auto off = [&](uint32_t j) { return row_first[j]; };
    for (uint64_t c = 0; c < max_tiles; ++c)
        if (c * TSV_TILE < total) tile_first[c] = qpart::find_segment(off, 0u, n, c * TSV_TILE);
    // k_tsv_write
    std::vector<uint8_t> out(total, 0xA5);
    uint64_t stray = 0;
    for (uint64_t c = 0; c < max_tiles; ++c) {
        const uint64_t c0 = c * TSV_TILE;
        if (c0 >= total) continue;
        const uint64_t cend = std::min<uint64_t>(c0 + TSV_TILE, total);
        std::vector<uint8_t> tile(TSV_TILE, 0xA5), times(TSV_TILE, 0);
        uint32_t jf, jl;
        tile_rows(off, [&](uint64_t t) { if (t >= tile_first.size() || tile_first[t] == 0xFFFFFFFFu) { ++stray; return 0u; } return tile_first[t]; },
                  n, c, total, &jf, &jl);
        for (uint32_t tid = 0; tid < TSV_THREADS; ++tid) {
            const uint32_t group = tid / TSV_GROUP, gl = tid % TSV_GROUP;
            for (uint64_t r = (uint64_t)jf + group; r <= jl; r += TSV_GROUPS) {
                const uint64_t b = row_first[r], e = row_first[r + 1];
                if (e == b) continue;
                const Read& x = reads[r];
                Row row;
                (void)row_of(B.T, title_off[r], (uint32_t)x.title.size(), nlen[r], keep[r], x.bc, x.bc2, x.adapter, x.adapter_end, x.raw, x.den, &row);
                tile_put_row(row, b, e, c0, cend, gl, text.data(), B.T.blob,
                             [&](uint32_t o, uint32_t w) {
                                 if ((o & 3u) || o + 4 > TSV_TILE) { ++stray; return; }
                                 for (uint32_t i = 0; i < 4; ++i) { tile[o + i] = (uint8_t)(w >> (8 * i)); times[o + i]++; }
                             },
                             [&](uint32_t o, uint8_t v) { if (o >= TSV_TILE) { ++stray; return; } tile[o] = v; times[o]++; });
            }
        }
        for (uint64_t i = 0; i < TSV_TILE; ++i) if (times[i] != (c0 + i < cend ? 1 : 0)) ++stray;
        for (uint32_t it = 0; it < TSV_VECS_PER_LANE; ++it)
            for (uint32_t tid = 0; tid < TSV_THREADS; ++tid) {
                const uint32_t v = it * TSV_THREADS + tid;
                const uint64_t d0 = c0 + (uint64_t)v * TSV_VEC;
                if (d0 >= cend) continue;
                if (vector_whole(d0, total)) { if (d0 + TSV_VEC > out.size()) { ++stray; continue; } memcpy(out.data() + d0, tile.data() + (d0 - c0), TSV_VEC); }
                else for (uint64_t d = d0; d < total; ++d) out[d] = tile[d - c0];
            }
    }
    if (stray) return 1;
    return (out.size() == want.size() && (want.empty() || memcmp(out.data(), want.data(), want.size()) == 0)) ? 0 : 1;
}

// ---- kits and reads ----------------------------------------------------------------------------------------------------------------
static Kit make_kit(int mode /* 0 epi2me, 1 dual, 2 simple */) {
    Kit k;
    k.simple = mode == 2; k.dual = mode == 1;
    k.nt = k.simple ? 1 : 3;
    const char* names[3] = {"NBD103/NBD104", "RBK004", "PBC096"};
    for (uint32_t t = 0; t < k.nt; ++t) {
        std::vector<int32_t> a, b;
        const uint32_t na = 5 + 40 * t;
        for (uint32_t i = 0; i < na; ++i) a.push_back(t == 2 && i == 3 ? -7 : (int32_t)(i + 1 + 100 * t * (i & 1)));
        for (uint32_t i = 0; i < 7 + t; ++i) b.push_back((int32_t)(i * 13 + 1));
        k.ids.push_back(a); k.ids2.push_back(b);
        k.kit_name.push_back(k.simple ? "" : names[t]);
    }
    k.dens = {40, 46, 39};
    k.max_raw = {40, 46, 39};
    return k;
}
static std::string word(uint64_t len) {
    std::string s;
    for (uint64_t i = 0; i < len; ++i) s.push_back((char)('a' + rnd_below(26)));
    return s;
}
// the six title forms: name only, comment, several blanks, two blanks in a row, leading blank, empty
static std::string title_form(uint32_t form, uint64_t name, uint64_t comment) {
    switch (form % 6) {
        case 0: return word(name ? name : 1);
        case 1: return word(name ? name : 1) + " " + word(comment ? comment : 1);
        case 2: return word(name ? name : 1) + " " + word(3) + " " + word(comment ? comment : 1) + " x=" + word(2);
        case 3: return word(name ? name : 1) + "  " + word(comment ? comment : 1);
        case 4: return " " + word(comment ? comment : 1);
        default: return std::string();
    }
}
static Read random_read(const Kit& k, uint32_t form) {
    Read r;
    r.title = title_form(form, 1 + rnd_below(40), 1 + rnd_below(30));
    static const uint64_t below[6] = {1, 10, 100, 1000, 100000, 0x80000000ull};
    r.keep = (uint32_t)rnd_below(below[rnd_below(6)]);
    const uint32_t kind = (uint32_t)rnd_below(8);
    const uint32_t t = (uint32_t)rnd_below(k.nt);
    r.adapter = k.simple ? -1 : (int32_t)t;
    r.bc = (int32_t)rnd_below(k.ids[t].size());
    r.bc2 = k.dual ? (int32_t)rnd_below(k.ids2[t].size()) : -1;
    r.den = k.dens[rnd_below(k.dens.size())];
    r.raw = (int32_t)rnd_below((uint64_t)r.den + 1);
    r.adapter_end = (int32_t)rnd_below(200) - (rnd_below(10) == 0 ? 150 : 0);
    if (kind == 0) { r.bc = -1; r.bc2 = -1; r.adapter = -1; r.raw = 0; r.den = 1; }        // no call
    if (kind == 1) r.bc = -1;                                                             // an adapter without a barcode
    if (kind == 2) r.bc = (int32_t)k.ids[t].size() + (int32_t)rnd_below(3);               // outside the table: not called
    if (kind == 3 && k.dual) r.bc2 = rnd_below(2) ? -1 : (int32_t)k.ids2[t].size();
    if (kind == 3 && !k.simple && !k.dual) r.adapter = (int32_t)k.nt;                     // outside the templates
    if (kind == 3 && k.simple) r.adapter = 0;                                             // simple mode: a call has no adapter
    return r;
}

static void test_titles() {
    Section s{"titles"};
    for (int mode = 0; mode < 3; ++mode) {
        const Kit k = make_kit(mode);
        for (uint32_t form = 0; form < 6; ++form)
            for (int call = 0; call < 2; ++call) {
                Read r = random_read(k, form);
                if (!call) { r.bc = -1; r.adapter = -1; }
                // the split itself, then the row through the passes
                const size_t sp = r.title.find(' ');
                const uint32_t nl = name_len((const uint8_t*)r.title.data(), (uint32_t)r.title.size(), sp != std::string::npos);
                s.cases++; if (nl != (sp == std::string::npos ? r.title.size() : sp)) s.bad++;
                s.cases++; s.bad += run_batch(k, std::vector<Read>(1, r));
            }
    }
    report(s);
}

static void test_rows_and_tiles() {
    Section s{"rows and tiles"};
    for (int mode = 0; mode < 3; ++mode) {
        const Kit k = make_kit(mode);
        // a row that ends one byte before, at, and one byte behind a tile edge (the first and the second edge), by its name and by
        // its comment; rows of ordinary size around it
        for (int edge = 1; edge <= 2; ++edge)
            for (int by_comment = 0; by_comment < 2; ++by_comment)
                for (int d = -1; d <= 1; ++d) {
                    std::vector<Read> reads;
                    for (uint32_t i = 0; i < 3; ++i) reads.push_back(random_read(k, i));
                    uint64_t front = 0;
                    for (const Read& r : reads) front += want_row(k, r).size();
                    Read x = random_read(k, 1);
                    x.title = "n c";
                    const uint64_t base = want_row(k, x).size(), target = (uint64_t)edge * TSV_TILE + (uint64_t)(int64_t)d - front;
                    x.title = by_comment ? "n " + word(target - base + 1) : word(target - base + 1) + " c";
                    reads.push_back(x);
                    for (uint32_t i = 0; i < 5; ++i) reads.push_back(random_read(k, i + 3));
                    uint64_t upto = 0;
                    for (uint32_t i = 0; i < 4; ++i) upto += want_row(k, reads[i]).size();
                    s.cases++; if (upto != (uint64_t)edge * TSV_TILE + (uint64_t)(int64_t)d) s.bad++;
                    s.cases++; s.bad += run_batch(k, reads);
                }
        // a row longer than two tiles, by its name and by its comment, between ordinary rows and alone
        for (int by_comment = 0; by_comment < 2; ++by_comment)
            for (int alone = 0; alone < 2; ++alone) {
                std::vector<Read> reads;
                if (!alone) for (uint32_t i = 0; i < 70; ++i) reads.push_back(random_read(k, i));
                Read x = random_read(k, 1);
                const std::string big = word(2 * TSV_TILE + 1 + rnd_below(TSV_TILE));
                x.title = by_comment ? "name " + big : big + " comment";
                reads.insert(reads.begin() + (alone ? 0 : 33), x);
                s.cases++; s.bad += run_batch(k, reads);
            }
        // sizes; dropped reads at the first, a middle and the last position; all reads dropped
        const uint32_t sizes[6] = {1, 2, 63, 64, 65, 257};
        for (uint32_t n : sizes)
            for (int drop = 0; drop < 5; ++drop) {
                std::vector<Read> reads;
                for (uint32_t i = 0; i < n; ++i) reads.push_back(random_read(k, (uint32_t)rnd_below(6)));
                if (drop == 1) reads[0].dropped = true;
                if (drop == 2) reads[n / 2].dropped = true;
                if (drop == 3) reads[n - 1].dropped = true;
                if (drop == 4) for (Read& r : reads) r.dropped = true;
                s.cases++; s.bad += run_batch(k, reads);
            }
        // many rows: several tiles of ordinary rows, one read in five dropped
        std::vector<Read> reads;
        for (uint32_t i = 0; i < 900; ++i) { reads.push_back(random_read(k, (uint32_t)rnd_below(6))); reads.back().dropped = rnd_below(5) == 0; }
        s.cases++; s.bad += run_batch(k, reads);
        s.cases++; s.bad += run_batch(k, std::vector<Read>());
    }
    // a record outside the score table is reported, not formatted
    {
        const Kit k = make_kit(0);
        Read r = random_read(k, 1);
        r.adapter = 0; r.bc = 0; r.den = 41; r.raw = 3;
        Built B;
        Row row;
        s.cases++; if (!build_tables(k, &B) || row_of(B.T, 0, 3, 1, 5, r.bc, r.bc2, r.adapter, 0, r.raw, r.den, &row)) s.bad++;
        r.den = 40; r.raw = 41;
        s.cases++; if (row_of(B.T, 0, 3, 1, 5, r.bc, r.bc2, r.adapter, 0, r.raw, r.den, &row)) s.bad++;
        r.raw = -1;
        s.cases++; if (row_of(B.T, 0, 3, 1, 5, r.bc, r.bc2, r.adapter, 0, r.raw, r.den, &row)) s.bad++;
        r.raw = 40;
        s.cases++; if (!row_of(B.T, 0, 3, 1, 5, r.bc, r.bc2, r.adapter, 0, r.raw, r.den, &row)) s.bad++;
    }
    report(s);
}

static int print_scores() {
    std::vector<int32_t> dens, max_raw;
    for (int32_t d = 1; d <= 200; ++d) { dens.push_back(d); max_raw.push_back(d); }
    ScoreTable t;
    const std::string err = score_table_build(dens, max_raw, repr_double, &t);
    if (!err.empty()) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    for (int32_t d = 1; d <= 200; ++d)
        for (int32_t raw = 0; raw <= t.den_last[d]; ++raw) {
            const uint8_t* slot = t.slots.data() + (size_t)(t.den_first[d] + raw) * TSV_SCORE_SLOT;
            printf("%d %d %.*s\n", d, raw, (int)slot[0], (const char*)slot + 1);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "--scores") == 0) return print_scores();
    g_rng = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    test_decimal();
    test_titles();
    test_rows_and_tiles();
    return 0;
}

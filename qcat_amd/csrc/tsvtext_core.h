// tsvtext_core.h -- the arithmetic of the driver's TSV rows in device memory (kernels_tsvtext.inc, tsvtext_host.inc), as pure
// functions that compile for host and device: decimal digits of a 32-bit value, the name of a stored title, the `called`
// predicate of the host writer (fastq_host.inc, FqWriter::called), the field list of one row, its length and its bytes, the
// tiles the output is cut into and what a group of lanes writes of one row into a tile, and the output's upper bound.  The
// host part below them builds the tables a row looks its strings up in.  tests/tsvtext_check.cpp runs the writer's tile, group
// and lane schedule through these on the host.
//
// Vocabulary.  A ROW is what FqWriter::write_range prints for one kept read:
//   name \t kept length \t id \t score \t kit \t adapter_end \t comment \n          a called read (dual mode: id "/" id2)
//   name \t kept length \t none \t -1 \t none \t -1 \t comment \n                   any other read
// name = the stored title up to its first blank, comment = the bytes behind that blank ("None" when there is none); a read the
// minimum-length filter drops has a row of 0 bytes.  A row is TSV_FIELDS FIELDS, each a length, a source and the separator byte
// behind it (0: none).  The sources: bytes of the text plane; bytes of the TABLES blob -- constants, one slot of TSV_ID_SLOT
// bytes per (template, set, barcode) with str(Barcode.id), one of TSV_KIT_SLOT bytes per template with the kit's name, one of
// TSV_SCORE_SLOT bytes per (denominator, raw score) with repr(raw * 100.0 / (1.0 * den)); every slot a length byte and the
// text --; the digits of an unsigned or a signed 32-bit value.  The OUTPUT is the rows of the kept reads in read order,
// row_first[r] the first byte of row r (row_first[n] = total), cut into TILES of TSV_TILE bytes, one workgroup each: tiles own
// bytes, not rows.
#pragma once
#include <stdint.h>

#include "../../include/qcat_hip.h"
#include "partition_core.h"

namespace qtsv {

constexpr uint32_t TSV_THREADS = 256;                          // lanes of a writer workgroup
constexpr uint32_t TSV_GROUP = 8;                              // lanes that write one row together, a dword of the tile each and round
constexpr uint32_t TSV_GROUPS = TSV_THREADS / TSV_GROUP;       // rows a workgroup has in hand at a time
constexpr uint32_t TSV_VEC = 16;                               // bytes of a stored vector
constexpr uint32_t TSV_TILE = 16384;                           // bytes of the output per workgroup, assembled in the LDS
constexpr uint32_t TSV_VECS_PER_LANE = TSV_TILE / TSV_VEC / TSV_THREADS;
constexpr uint32_t TSV_FIELDS = 8;
constexpr uint32_t TSV_ID_SLOT = 12;                           // length byte + str(int32): at most 11 characters
constexpr uint32_t TSV_KIT_SLOT = 64;                          // length byte + a kit name of at most 63 bytes
constexpr uint32_t TSV_SCORE_SLOT = 24;                        // length byte + repr(float) of at most 23 characters
constexpr uint32_t TSV_MAX_DEN = 255;                          // denominators the index covers (a kit writes QCAT_MAX_TARGET_LEN at most)
static_assert(TSV_MAX_DEN >= QCAT_MAX_TARGET_LEN, "every score_den a kit can write has an index entry");
constexpr uint32_t TSV_SCORE_TABLE_MAX = 1u << 20;             // bytes of score slots a kit may need (43 690 (den, raw) pairs)
constexpr uint32_t TSV_NO_SLOT = 0xFFFFFFFFu;
// the constants in front of the blob: the four middle columns of a read without a call, and "None"
constexpr uint32_t TSV_C_NOCALL = 0, TSV_C_NOCALL_LEN = 15, TSV_C_NONE = 16, TSV_C_NONE_LEN = 4, TSV_CONST_BYTES = 32;
QP_HD void tsv_constants(uint8_t* c /* TSV_CONST_BYTES */) {
    const char s[21] = "none\t-1\tnone\t-1\0None";
    for (uint32_t i = 0; i < TSV_CONST_BYTES; ++i) c[i] = i < 20 ? (uint8_t)s[i] : 0;
}

// what a row looks up: the blob and where its parts lie, the denominators' index, the sizes of the caller's id tables (the
// `called` predicate's bounds) and the longest entries (the output's bound).  The pointers are the host's on the host and the
// device's on the device.
struct Tables {
    const uint8_t* blob;
    const int32_t* den_first;                  // TSV_MAX_DEN + 1 entries: the score slot of raw 0 with denominator d; -1: the kit never writes d
    const int32_t* den_last;                   // ... the largest raw score that has a slot
    uint32_t ids_off, kits_off, scores_off;    // bytes into the blob
    uint32_t simple, dual, nt;
    uint32_t id_first[QCAT_MAX_TEMPLATES][2];  // the id slot of barcode 0 of (template, set)
    uint32_t id_n[QCAT_MAX_TEMPLATES][2];      // barcodes of (template, set)
    uint32_t max_id[2], max_kit, max_score;    // the longest text of every kind
};

// ---- decimal digits ------------------------------------------------------------------------------------------------------------
QP_HD uint32_t dec_len_u32(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10u) { v /= 10u; ++n; }
    return n;
}
QP_HD uint32_t dec_len_i32(int32_t v) { return v < 0 ? 1u + dec_len_u32(0u - (uint32_t)v) : dec_len_u32((uint32_t)v); }
// character k (0: the first) of the len characters of v
QP_HD uint8_t dec_char_u32(uint32_t v, uint32_t len, uint32_t k) {
    for (uint32_t i = len - 1u - k; i; --i) v /= 10u;
    return (uint8_t)('0' + v % 10u);
}
QP_HD uint8_t dec_char_i32(int32_t v, uint32_t len, uint32_t k) {
    if (v >= 0) return dec_char_u32((uint32_t)v, len, k);
    return k == 0 ? (uint8_t)'-' : dec_char_u32(0u - (uint32_t)v, len - 1u, k - 1u);
}

// ---- name and comment: the title is split at its first blank (a tab counts: cli.py:200-214; the text plane holds them as
// blanks already).  name_len == title_len: no blank, the comment prints "None" -------------------------------------------------------
QP_HD uint32_t name_len(const uint8_t* title, uint32_t title_len, bool has_blank) {
    if (!has_blank) return title_len;
    uint32_t i = 0;
    while (i < title_len && title[i] != ' ' && title[i] != '\t') ++i;
    return i;
}

// ---- FqWriter::called: the simple-mode rule, and an index outside a table counts as "not called" -------------------------------------
QP_HD bool called(const Tables& T, int32_t bc, int32_t bc2, int32_t adapter) {
    if (T.simple ? !(bc >= 0 && adapter == -1) : !(bc >= 0 && adapter >= 0 && adapter < (int32_t)T.nt)) return false;
    const uint32_t t = T.simple ? 0u : (uint32_t)adapter;
    return (uint32_t)bc < T.id_n[t][0] && (!T.dual || (bc2 >= 0 && (uint32_t)bc2 < T.id_n[t][1]));
}

// the slot (bytes into the blob) of the text of raw * 100.0 / (1.0 * den), TSV_NO_SLOT outside the table
QP_HD uint32_t score_slot(const Tables& T, int32_t raw, int32_t den) {
    if (den < 0 || den > (int32_t)TSV_MAX_DEN || raw < 0) return TSV_NO_SLOT;
    const int32_t first = T.den_first[den];
    if (first < 0 || raw > T.den_last[den]) return TSV_NO_SLOT;
    return T.scores_off + (uint32_t)(first + raw) * TSV_SCORE_SLOT;
}

// ---- the fields of one row -----------------------------------------------------------------------------------------------------
enum : uint32_t { SRC_TEXT = 0, SRC_BLOB = 1, SRC_U32 = 2, SRC_I32 = 3 };
struct Field {
    uint32_t len, kind;
    uint64_t src;                              // SRC_TEXT / SRC_BLOB: the first byte's offset; SRC_U32 / SRC_I32: the value
    uint32_t sep;                              // the byte behind the field, 0: none
};
struct Row { Field f[TSV_FIELDS]; };

QP_HD Field field_of(uint32_t len, uint32_t kind, uint64_t src, uint32_t sep) { Field f; f.len = len; f.kind = kind; f.src = src; f.sep = sep; return f; }
QP_HD Field slot_field(const Tables& T, uint32_t slot, uint32_t sep) { return field_of(T.blob[slot], SRC_BLOB, (uint64_t)slot + 1u, sep); }

// One read of the record table and its record: title_off / title_len of the stored title, nl its name's length, keep the kept
// length.  False: the read is called and its (raw, den) lies outside the score table -- the score field is empty then.
QP_HD bool row_of(const Tables& T, uint64_t title_off, uint32_t title_len, uint32_t nl, uint32_t keep, int32_t bc, int32_t bc2,
                  int32_t adapter, int32_t adapter_end, int32_t raw, int32_t den, Row* row) {
    bool ok = true;
    Field* f = row->f;
    f[0] = field_of(nl, SRC_TEXT, title_off, '\t');
    f[1] = field_of(dec_len_u32(keep), SRC_U32, keep, '\t');
    if (called(T, bc, bc2, adapter)) {
        const uint32_t t = T.simple ? 0u : (uint32_t)adapter;
        f[2] = slot_field(T, T.ids_off + (T.id_first[t][0] + (uint32_t)bc) * TSV_ID_SLOT, T.dual ? '/' : '\t');
        f[3] = T.dual ? slot_field(T, T.ids_off + (T.id_first[t][1] + (uint32_t)bc2) * TSV_ID_SLOT, '\t') : field_of(0, SRC_BLOB, 0, 0);
        const uint32_t ss = score_slot(T, raw, den);
        ok = ss != TSV_NO_SLOT;
        f[4] = ok ? slot_field(T, ss, '\t') : field_of(0, SRC_BLOB, 0, '\t');
        f[5] = T.simple ? field_of(TSV_C_NONE_LEN, SRC_BLOB, TSV_C_NONE, '\t') : slot_field(T, T.kits_off + t * TSV_KIT_SLOT, '\t');
        f[6] = field_of(dec_len_i32(adapter_end), SRC_I32, (uint64_t)(uint32_t)adapter_end, '\t');
    } else {
        f[2] = field_of(TSV_C_NOCALL_LEN, SRC_BLOB, TSV_C_NOCALL, '\t');
        for (uint32_t i = 3; i < 7; ++i) f[i] = field_of(0, SRC_BLOB, 0, 0);
    }
    f[7] = nl < title_len ? field_of(title_len - nl - 1u, SRC_TEXT, title_off + nl + 1u, '\n')
                          : field_of(TSV_C_NONE_LEN, SRC_BLOB, TSV_C_NONE, '\n');
    return ok;
}

QP_HD uint64_t row_len(const Row& row) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < TSV_FIELDS; ++i) n += (uint64_t)row.f[i].len + (row.f[i].sep ? 1u : 0u);
    return n;
}

// byte i (i < row_len) of a row
QP_HD uint8_t row_byte(const Row& row, uint64_t i, const uint8_t* text, const uint8_t* blob) {
    for (uint32_t k = 0; k < TSV_FIELDS; ++k) {
        const Field& f = row.f[k];
        if (i < f.len) {
            if (f.kind == SRC_TEXT) return text[f.src + i];
            if (f.kind == SRC_BLOB) return blob[f.src + i];
            if (f.kind == SRC_U32) return dec_char_u32((uint32_t)f.src, f.len, (uint32_t)i);
            return dec_char_i32((int32_t)(uint32_t)f.src, f.len, (uint32_t)i);
        }
        i -= f.len;
        if (f.sep) { if (i == 0) return (uint8_t)f.sep; --i; }
    }
    return 0;                                  // (i >= row_len: not asked for)
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------------
QP_HD uint64_t tiles_of(uint64_t total) { return (total + TSV_TILE - 1) / TSV_TILE; }

// the rows of tile c (c * TSV_TILE < total): [*first, *last], the rows that hold its first and its last byte.  first_of(c): the
// row of the first byte of tile c (qpart::find_segment over the whole table, one lane per tile: k_tsv_tiles); the last row lies
// at or in front of the next tile's first.
template <class Off, class First>
QP_HD void tile_rows(const Off& row_first, const First& first_of, uint32_t n, uint64_t c, uint64_t total, uint32_t* first, uint32_t* last) {
    const uint64_t c0 = c * TSV_TILE;
    const uint64_t cend = c0 + TSV_TILE < total ? c0 + TSV_TILE : total;
    *first = first_of(c);
    uint32_t hi = cend < total ? first_of(c + 1) + 1u : n;
    if (hi > n) hi = n;
    *last = qpart::find_segment(row_first, *first, hi, cend - 1);
}

// What lane gl (0 .. TSV_GROUP - 1) of a row's group writes into the tile that owns output bytes [c0, cend): the row lies at
// [b, e) of the output, tile[0] is byte c0.  The row's part inside the tile is taken a dword of the TILE at a time -- lane gl
// the dwords gl, gl + TSV_GROUP, ... behind the part's first -- and stored as one dword where the row owns all four bytes,
// byte by byte at the two edges, whose dwords it may share with its neighbours' groups.  put32(o, w) / put8(o, v): store at
// byte o of the tile.
template <class Put32, class Put8>
QP_HD void tile_put_row(const Row& row, uint64_t b, uint64_t e, uint64_t c0, uint64_t cend, uint32_t gl, const uint8_t* text,
                        const uint8_t* blob, const Put32& put32, const Put8& put8) {
    const uint64_t a = b > c0 ? b : c0, z = e < cend ? e : cend;
    for (uint64_t d = (a & ~3ull) + 4ull * gl; d < z; d += 4ull * TSV_GROUP) {
        if (d >= a && d + 4 <= z) {
            uint32_t w = 0;
            for (uint32_t k = 0; k < 4; ++k) w |= (uint32_t)row_byte(row, d + k - b, text, blob) << (8 * k);
            put32((uint32_t)(d - c0), w);
        } else {
            for (uint32_t k = 0; k < 4; ++k) if (d + k >= a && d + k < z) put8((uint32_t)(d + k - c0), row_byte(row, d + k - b, text, blob));
        }
    }
}

// the vector at byte d0 (a multiple of TSV_VEC, d0 < total) is stored whole; the output's last, partial one byte by byte
QP_HD bool vector_whole(uint64_t d0, uint64_t total) { return d0 + TSV_VEC <= total; }

// ---- the output's upper bound: title bytes plus a per-read constant ------------------------------------------------------------
// the stored titles of n plain records in text_bytes bytes with n_bases bases: a record has at least
// '@' title '\n' seq '\n' '+' '\n' qual '\n' = title + 2 seq + 6 bytes, the last one may lack its newline
QP_HD uint64_t title_bound(uint64_t text_bytes, uint64_t n_bases, uint64_t n) {
    const uint64_t rest = 2 * n_bases + 6 * n;
    return text_bytes + 1 > rest ? text_bytes + 1 - rest : 0;
}
// the same for FASTA text: a record has at least '>' title '\n' seq '\n' = title + seq + 3 bytes
QP_HD uint64_t fa_title_bound(uint64_t text_bytes, uint64_t n_bases, uint64_t n) {
    const uint64_t rest = n_bases + 3 * n;
    return text_bytes + 1 > rest ? text_bytes + 1 - rest : 0;
}
// name + comment <= title + 4 ("None"), three separators around them, a kept length of at most 10 digits, and the longer of the
// two middles with its separators: "none\t-1\tnone\t-1" or id "/" id2, score, kit, an adapter_end of at most 11 characters
QP_HD uint64_t row_const(const Tables& T) {
    const uint64_t kit = T.max_kit > TSV_C_NONE_LEN ? T.max_kit : TSV_C_NONE_LEN;
    const uint64_t mid = (uint64_t)T.max_id[0] + 1 + T.max_id[1] + T.max_score + kit + 11 + 4;
    return 4 + 3 + 10 + (mid > TSV_C_NOCALL_LEN + 1 ? mid : TSV_C_NOCALL_LEN + 1);
}
QP_HD uint64_t output_bound(uint64_t title_bytes, uint64_t n, const Tables& T) { return title_bytes + n * row_const(T); }

}  // namespace qtsv

// ---- host only: the tables -------------------------------------------------------------------------------------------------------
#ifndef QCAT_RTC
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace qtsv {

// the score slots of one kit: for every denominator d it can write, the texts of raw 0 .. max_raw(d)
struct ScoreTable {
    int32_t den_first[TSV_MAX_DEN + 1], den_last[TSV_MAX_DEN + 1];
    std::vector<uint8_t> slots;
    uint32_t max_len = 0;
};

// dens[i] with the largest raw score max_raw[i] (a denominator may come twice: the larger bound holds); repr(v, out) writes
// Python's repr of the double v into out[40] and returns its length.  An error text, or empty.
template <class Repr>
static inline std::string score_table_build(const std::vector<int32_t>& dens, const std::vector<int32_t>& max_raw, const Repr& repr, ScoreTable* out) {
    int32_t last[TSV_MAX_DEN + 1];
    for (uint32_t d = 0; d <= TSV_MAX_DEN; ++d) { out->den_first[d] = -1; out->den_last[d] = -1; last[d] = -1; }
    for (size_t i = 0; i < dens.size(); ++i) {
        if (dens[i] < 1 || dens[i] > (int32_t)TSV_MAX_DEN) return "a score denominator outside 1 .. " + std::to_string(TSV_MAX_DEN);
        if (max_raw[i] > last[dens[i]]) last[dens[i]] = max_raw[i] < 0 ? 0 : max_raw[i];
    }
    uint64_t entries = 0;
    for (uint32_t d = 0; d <= TSV_MAX_DEN; ++d) if (last[d] >= 0) entries += (uint64_t)last[d] + 1;
    if (entries * TSV_SCORE_SLOT > TSV_SCORE_TABLE_MAX)
        return "the score table of this kit would hold " + std::to_string(entries) + " entries (at most " +
               std::to_string(TSV_SCORE_TABLE_MAX / TSV_SCORE_SLOT) + ")";
    out->slots.assign((size_t)entries * TSV_SCORE_SLOT, 0);
    out->max_len = 0;
    uint32_t at = 0;
    for (uint32_t d = 0; d <= TSV_MAX_DEN; ++d) {
        if (last[d] < 0) continue;
        out->den_first[d] = (int32_t)at; out->den_last[d] = last[d];
        for (int32_t raw = 0; raw <= last[d]; ++raw, ++at) {
            char text[48];
            const size_t len = repr((double)raw * 100.0 / (1.0 * (double)(int)d), text);
            if (len >= TSV_SCORE_SLOT) return "a score text of " + std::to_string(len) + " characters does not fit its slot";
            uint8_t* slot = out->slots.data() + (size_t)at * TSV_SCORE_SLOT;
            slot[0] = (uint8_t)len;
            memcpy(slot + 1, text, len);
            if (len > out->max_len) out->max_len = (uint32_t)len;
        }
    }
    return std::string();
}

// The blob of one call and its description: constants, the denominators' index, the id slots of (template, set) in that order,
// the kit slots, the score slots.  n_ids[2 t + s] / ids[2 t + s]: the caller's Barcode.id tables (s = 1: dual mode only);
// kit_name[t] null: "None".  T->blob / den_first / den_last are set to the HOST blob; den_off: where the index lies in it.
static inline std::string tables_build(bool simple, bool dual, uint32_t nt, const uint32_t* n_ids, const int32_t* const* ids,
                                       const char* const* kit_name, const ScoreTable& scores, std::vector<uint8_t>* blob, Tables* T,
                                       uint32_t* den_off) {
    memset(T, 0, sizeof *T);
    T->simple = simple; T->dual = dual; T->nt = nt;
    uint32_t n_slots = 0;
    for (uint32_t t = 0; t < nt; ++t)
        for (uint32_t s = 0; s < 2; ++s) {
            T->id_first[t][s] = n_slots;
            T->id_n[t][s] = (s == 0 || dual) ? n_ids[2 * t + s] : 0;
            n_slots += T->id_n[t][s];
        }
    *den_off = TSV_CONST_BYTES;
    T->ids_off = (*den_off + 2 * 4 * (TSV_MAX_DEN + 1) + 15u) & ~15u;
    T->kits_off = T->ids_off + ((n_slots * TSV_ID_SLOT + 15u) & ~15u);
    T->scores_off = T->kits_off + nt * TSV_KIT_SLOT;
    blob->assign((size_t)T->scores_off + scores.slots.size() + TSV_VEC, 0);
    uint8_t* p = blob->data();
    tsv_constants(p);
    memcpy(p + *den_off, scores.den_first, 4 * (TSV_MAX_DEN + 1));
    memcpy(p + *den_off + 4 * (TSV_MAX_DEN + 1), scores.den_last, 4 * (TSV_MAX_DEN + 1));
    for (uint32_t t = 0; t < nt; ++t) {
        for (uint32_t s = 0; s < 2; ++s)
            for (uint32_t b = 0; b < T->id_n[t][s]; ++b) {
                uint8_t* slot = p + T->ids_off + (size_t)(T->id_first[t][s] + b) * TSV_ID_SLOT;
                char num[16];
                const int len = snprintf(num, sizeof num, "%d", (int)ids[2 * t + s][b]);
                slot[0] = (uint8_t)len;
                memcpy(slot + 1, num, (size_t)len);
                if ((uint32_t)len > T->max_id[s]) T->max_id[s] = (uint32_t)len;
            }
        const char* name = kit_name[t] ? kit_name[t] : "None";
        const size_t len = strlen(name);
        if (len >= TSV_KIT_SLOT) return "a kit name of " + std::to_string(len) + " bytes does not fit its slot (at most " + std::to_string(TSV_KIT_SLOT - 1) + ")";
        uint8_t* slot = p + T->kits_off + (size_t)t * TSV_KIT_SLOT;
        slot[0] = (uint8_t)len;
        memcpy(slot + 1, name, len);
        if (len > T->max_kit) T->max_kit = (uint32_t)len;
    }
    if (!scores.slots.empty()) memcpy(p + T->scores_off, scores.slots.data(), scores.slots.size());
    T->max_score = scores.max_len;
    T->blob = p;
    T->den_first = reinterpret_cast<const int32_t*>(p + *den_off);
    T->den_last = T->den_first + (TSV_MAX_DEN + 1);
    return std::string();
}

}  // namespace qtsv
#endif

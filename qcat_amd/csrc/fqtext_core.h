// fqtext_core.h -- the lane arithmetic of FASTQ text in device memory (kernels_fqtext.inc), as pure functions that compile for
// host and device: the blocks a text is cut into, the newline and byte-class masks of a 16-byte vector, the rank of a newline
// inside its wave, the checks of one four-line record against the line table, and the segment table of one output record.
// tests/fqtext_check.cpp runs the passes' block and lane schedule through these on the host.  The two-line FASTA form of the
// record checks and segments stands at the end of the file (tests/textstream_check.cpp).
//
// Vocabulary.  The TEXT is n_bytes bytes of a FASTQ file.  LINE k begins at line_start[k] and ends in front of its '\n' (the
// last line may have none); a text has n_lines = newlines + (1 when its last byte is no newline) lines, and
// line_start[n_lines] = (the byte behind the last line's end) + 1, so that every line's length is
// line_start[k + 1] - line_start[k] - 1.  The KIND of a line is k mod 4: title, sequence, '+', quality.  RECORD r is lines
// 4 r .. 4 r + 3.  A text is PLAIN when fq_parse (fastq_host.inc) accepts every record of it; the first record that is not
// plain is the smallest r with a failed check in one of its lines, since every record in front of it has exactly four lines.
// The text plane of a batch holds the text, then FQ_CONST_BYTES of constants (fq_constants) that the writers' records are
// completed from, with the batches' slack on both sides.
#pragma once
#include <stdint.h>

#include "partition_core.h"

namespace qfq {

constexpr uint32_t FQ_THREADS = 256;                           // lanes of a text workgroup
constexpr uint32_t FQ_VEC = 16;                                // bytes a lane loads at once (aligned)
constexpr uint32_t FQ_ROUND = FQ_THREADS * FQ_VEC;             // consecutive bytes of one round of a workgroup: 4 KiB
constexpr uint32_t FQ_ROUNDS = 4;
constexpr uint32_t FQ_BLOCK = FQ_ROUND * FQ_ROUNDS;            // the fixed block of text a workgroup owns: 16 KiB
constexpr uint32_t FQ_SEGS = 6;                                // segments of one output record
constexpr uint32_t FQ_CONST_BYTES = 16;
// the constants block behind the text: " \n" at 0, "\n" at 1, "\n+\n" at 2, "\n" at 5
constexpr uint32_t FQ_C_BLANK_NL = 0, FQ_C_NL = 1, FQ_C_PLUS = 2, FQ_C_LAST_NL = 5;
QP_HD void fq_constants(uint8_t* c /* FQ_CONST_BYTES */) {
    const char s[7] = " \n\n+\n\n";
    for (uint32_t i = 0; i < FQ_CONST_BYTES; ++i) c[i] = i < 6 ? (uint8_t)s[i] : 0;
}

constexpr uint64_t FQ_NO_LINE = ~0ull;                         // "no bad line"

// one read of the record table (the meanings of qk::FqRec): the title without '@' and right-stripped of blanks and tabs
struct Rec {
    uint64_t title_off, seq_off, qual_off;
    uint32_t title_len, seq_len;
    uint32_t title_blank;                                      // the stored title holds a blank (or a tab, printed as one)
    uint32_t pad;
};

QP_HD uint64_t blocks_of(uint64_t n_bytes) { return (n_bytes + FQ_BLOCK - 1) / FQ_BLOCK; }

// ---- masks of a vector: bit b = byte b -----------------------------------------------------------------------------------------
// the high bits 0x80 of four bytes as bits 0..3
QP_HD uint32_t pack_high(uint32_t m) { return (((m >> 7) & 0x01010101u) * 0x00204081u >> 21) & 15u; }
// bytes of w that are zero, as high bits
QP_HD uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }

QP_HD uint32_t nl_mask16(const qpart::Vec16& v) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < 4; ++i) m |= pack_high(zero_bytes(v.w[i] ^ 0x0A0A0A0Au)) << (4 * i);
    return m;
}
// bytes a sequence or quality line must not hold: <= 0x20 or >= 0x80
QP_HD uint32_t odd_seq16(const qpart::Vec16& v) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t w = v.w[i];
        const uint32_t ge21 = ((w & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) & 0x80808080u;         // low seven bits >= 0x21
        m |= pack_high((~ge21 & 0x80808080u) | (w & 0x80808080u)) << (4 * i);
    }
    return m;
}
// bytes a title or '+' line must not hold: a control character but tab, or >= 0x80
QP_HD uint32_t odd_title16(const qpart::Vec16& v) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t w = v.w[i];
        const uint32_t ge20 = ((w & 0x7F7F7F7Fu) + 0x60606060u) & 0x80808080u;
        const uint32_t tab = zero_bytes(w ^ 0x09090909u);
        m |= pack_high((~ge20 & ~tab & 0x80808080u) | (w & 0x80808080u)) << (4 * i);
    }
    return m;
}
// the bytes in front of bit b
QP_HD uint32_t below(uint32_t b) { return (1u << b) - 1u; }

// The bad bytes of a vector whose first byte lies in a line of kind `kind`: the bytes between its newlines against the class
// of their line's kind (the newlines themselves belong to no class).  All masks hold the vector's valid bytes only.
QP_HD uint32_t lines_bad(uint32_t nl, uint32_t odd_title, uint32_t odd_seq, uint32_t kind) {
    uint32_t bad = 0, done = 0, rest = nl;
    for (;;) {
        const uint32_t next = rest & (0u - rest);                              // the next newline (0: none)
        const uint32_t upto = next ? next - 1u : 0xFFFFu;
        bad |= upto & ~done & ((kind & 1u) ? odd_seq : odd_title);
        if (!next) break;
        done = upto | next;
        rest &= rest - 1u;
        kind = (kind + 1u) & 3u;
    }
    return bad;
}

// ---- the rank of a lane's first newline inside its wave: bal[b] = the wave's ballot of "byte b of my vector is a newline"; the
// bytes of lane l lie in front of those of lane l + 1 ------------------------------------------------------------------------------
QP_HD uint32_t popc64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}
QP_HD uint32_t popc32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}
QP_HD uint32_t wave_rank(const uint64_t (&bal)[FQ_VEC], uint32_t lane) {
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t r = 0;
    for (uint32_t b = 0; b < FQ_VEC; ++b) r += popc64(bal[b] & lt);
    return r;
}
QP_HD uint32_t wave_total(const uint64_t (&bal)[FQ_VEC]) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < FQ_VEC; ++b) r += popc64(bal[b]);
    return r;
}

// ---- one record against the line table ----------------------------------------------------------------------------------------
QP_HD bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// ls[0..4]: the starts of the record's four lines and of the line behind them; at(i): byte i of the text.  The checks of
// fq_parse that the byte classes of the lines pass does not make: '@' and '+', a non-empty sequence of at most 2^31 - 1 bases,
// as many quality bytes, a title of at most 2^32 - 1 bytes, and a '+' line that is alone, followed by blanks, or by the title.
template <class Byte>
QP_HD bool record_of(const Byte& at, const uint64_t* ls, Rec* r) {
    const uint64_t l0 = ls[0], l1 = ls[1], l2 = ls[2], l3 = ls[3], l4 = ls[4];
    if (at(l0) != '@' || at(l2) != '+') return false;                          // (an empty line: its first byte is its '\n')
    const uint64_t sl = l2 - l1 - 1, ql = l4 - l3 - 1;
    if (sl == 0 || sl > 0x7FFFFFFFull || ql != sl) return false;
    uint64_t tl = l1 - l0 - 2;                                                 // the title line without '@'
    while (tl && is_blank(at(l0 + tl))) --tl;                                  // (l0 + tl: the title's last byte)
    if (tl > 0xFFFFFFFFull) return false;
    uint64_t pll = l3 - l2 - 2;
    if (pll) {                                                                 // the rare long path
        while (pll && is_blank(at(l2 + pll))) --pll;
        if (pll && pll != tl) return false;
        for (uint64_t i = 0; i < pll; ++i) if (at(l2 + 1 + i) != at(l0 + 1 + i)) return false;
    }
    uint32_t blank = 0;
    for (uint64_t i = 0; i < tl; ++i) blank |= is_blank(at(l0 + 1 + i)) ? 1u : 0u;
    r->title_off = l0 + 1; r->title_len = (uint32_t)tl;
    r->seq_off = l1; r->seq_len = (uint32_t)sl;
    r->qual_off = l3;
    r->title_blank = blank; r->pad = 0;
    return true;
}

// lines of a text with `newlines` newlines, and its records (a last record of fewer than four lines counts: it is the bad one)
QP_HD uint64_t lines_of(uint64_t newlines, bool ends_with_newline) { return newlines + (ends_with_newline ? 0 : 1); }
QP_HD uint64_t records_of(uint64_t n_lines) { return (n_lines + 3) / 4; }

// ---- one output record: '@' title' '\n' seq[s : s + keep] "\n+\n" qual[s : s + keep] '\n', title' = the title plus one blank
// when it holds none (the writers print name + " " + comment).  Six (length, source position) pairs; a skipped read: zeros.
// const_off: where the constants block lies in the text plane (= n_bytes of the text). ---------------------------------------------
QP_HD void record_segments(const Rec& r, uint64_t s, uint64_t keep, bool skipped, uint64_t const_off, uint64_t* len, uint64_t* src) {
    if (skipped) { for (uint32_t i = 0; i < FQ_SEGS; ++i) { len[i] = 0; src[i] = 0; } return; }
    len[0] = 1 + (uint64_t)r.title_len; src[0] = r.title_off - 1;
    len[1] = r.title_blank ? 1 : 2;     src[1] = const_off + (r.title_blank ? FQ_C_NL : FQ_C_BLANK_NL);
    len[2] = keep;                      src[2] = r.seq_off + s;
    len[3] = 3;                         src[3] = const_off + FQ_C_PLUS;
    len[4] = keep;                      src[4] = r.qual_off + s;
    len[5] = 1;                         src[5] = const_off + FQ_C_LAST_NL;
}
// an upper bound of the output text of n reads parsed from n_bytes of text: a record of the text has at least
// 1 + title + 1 + seq + 3 + seq bytes, a record of the output at most 1 + title + 2 + seq + 3 + seq + 1
QP_HD uint64_t output_bound(uint64_t n_bytes, uint64_t n) { return n_bytes + 2 * n + 1; }

// ---- FASTA text: '>' title line and ONE sequence line per record (fa_parse, fastq_host.inc) -------------------------------------
// The line table is the same -- the kind of line k is k mod 2, and lines_bad picks the byte class by the kind's parity, which is
// that of k mod 4 --, RECORD r is lines 2 r and 2 r + 1.  fa_parse fails record r when the line BEHIND its sequence does not begin
// with '>' (a wrapped sequence, a blank line, a FASTQ record in the middle), so the lane of a record looks at two things and
// blames two records: its own first line without '>' lowers the bad line to FA_FRONT -- the sequence line of the record in front
// of it --, a missing or empty or overlong sequence line and an overlong title to FA_SELF, its own title line.  The first record
// fa_parse refuses is (the smallest lowered line) / 2: every record in front of it has exactly two lines, so the lines 2 r are
// their titles; no lane r' <= r finds its first line without '>' (record r' - 1 passed the check of the line behind it, and
// the text's first byte is '>'), the byte classes flag nothing below line 2 r, and each of fa_parse's reasons for r lowers line
// 2 r or 2 r + 1: a title line without newline or nothing behind it (r has one line), an empty or overlong sequence, a title
// too long (FA_SELF); a byte outside a line's class (k_fq_lines, line 2 r or 2 r + 1); a line behind the sequence that does
// not begin with '>' (lane r + 1, which exists because that line does: FA_FRONT of r + 1 = 2 r + 1).
enum : uint32_t { FA_OK = 0, FA_SELF = 1, FA_FRONT = 2 };
QP_HD uint64_t fa_records_of(uint64_t n_lines) { return (n_lines + 1) / 2; }
// the line a lane with verdict v (not FA_OK) lowers the status to
QP_HD uint64_t fa_blamed_line(uint64_t r, uint32_t v) { return v == FA_FRONT && r ? 2 * r - 1 : 2 * r; }
// the 1-based record the host names for a lowered line
QP_HD uint64_t fa_record_of_line(uint64_t bad_line) { return bad_line / 2 + 1; }

// ls[0..2]: the starts of the record's two lines and of the line behind them (ls[2] is not read when the record has one line);
// lines: 1 or 2, the lines the text holds of this record
template <class Byte>
QP_HD uint32_t fa_record_of(const Byte& at, const uint64_t* ls, uint32_t lines, Rec* r) {
    const uint64_t l0 = ls[0], l1 = ls[1];
    if (at(l0) != '>') return FA_FRONT;                                        // (an empty line: its first byte is its '\n')
    if (lines < 2) return FA_SELF;
    const uint64_t l2 = ls[2];
    const uint64_t sl = l2 - l1 - 1;
    if (sl == 0 || sl > 0x7FFFFFFFull) return FA_SELF;
    uint64_t tl = l1 - l0 - 2;                                                 // the title line without '>'
    while (tl && is_blank(at(l0 + tl))) --tl;
    if (tl > 0xFFFFFFFFull) return FA_SELF;
    uint32_t blank = 0;
    for (uint64_t i = 0; i < tl; ++i) blank |= is_blank(at(l0 + 1 + i)) ? 1u : 0u;
    r->title_off = l0 + 1; r->title_len = (uint32_t)tl;
    r->seq_off = l1; r->seq_len = (uint32_t)sl;
    r->qual_off = 0;
    r->title_blank = blank; r->pad = 0;
    return FA_OK;
}

// one output record of a FASTA batch: '>' title' '\n' seq[s : s + keep] '\n' -- the sigil is the byte in front of the stored
// title --, in the six segments of record_segments with the two of the quality part empty
QP_HD void fa_record_segments(const Rec& r, uint64_t s, uint64_t keep, bool skipped, uint64_t const_off, uint64_t* len, uint64_t* src) {
    for (uint32_t i = 0; i < FQ_SEGS; ++i) { len[i] = 0; src[i] = 0; }
    if (skipped) return;
    len[0] = 1 + (uint64_t)r.title_len; src[0] = r.title_off - 1;
    len[1] = r.title_blank ? 1 : 2;     src[1] = const_off + (r.title_blank ? FQ_C_NL : FQ_C_BLANK_NL);
    len[2] = keep;                      src[2] = r.seq_off + s;
    len[5] = 1;                         src[5] = const_off + FQ_C_LAST_NL;
}

}  // namespace qfq

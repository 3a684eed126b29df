// eval_core.h -- the arithmetic of the evaluation of a scanned text batch in device memory (kernels_eval.inc, eval_host.inc), as
// pure functions that compile for host and device: the masks of a 16-byte vector of a title, the tokens they resolve to, the
// truth a title states, the call's text from the id slots, the eval class and the ROC kind of one read, the score bucket, and
// the ROC table of a histogram.  tests/eval_check.cpp runs the classify pass's vector and lane schedule through these on the host.
//
// The contract (qcat/eval.py and qcat/eval_roc.py of the reference, over the rows of --tsv).  The reads evaluated are the reads
// that have a TSV row: every read the minimum-length filter keeps.  Per evaluated read:
//   call text bc   what the TSV's barcode column prints: str(id) from the id slots, id "/" id2 in dual mode, "none" for a read
//                  that is not qtsv::called
//   comment        the bytes behind the stored title's first blank
//   truth          the comment split at every single blank; a token COUNTS when it holds exactly one '=': key = the bytes in
//                  front, value = the bytes behind (may be empty); the LAST counting token whose key is exactly "truebc" gives
//                  the value V, and truebc = V.split(",")
//   eval class     CORRECT when bc equals an element of the list ("none" against "none" included); otherwise FN when bc is
//                  "none"; otherwise FP when V == "none"; otherwise INCORRECT
//   ROC kind       truth none (V == "none"), whole (bc equals the WHOLE of V: the reference compares with [str(truebc)], a list of
//                  one, so a comma list never matches) or other
//   bucket         0 for a read without a call, else min(1001, raw_score * 1000 / score_den + 1): at threshold q in 0 .. 1000 the
//                  call stands exactly when q < bucket, which is score >= q / 10.0 for score = raw * 100.0 / den in doubles
//   ROC row q      reads with bucket > q: false_positive (truth none), correct (whole), incorrect (other); reads with bucket <= q:
//                  true_negative (truth none), false_negative (whole or other)
// A read the reference cannot read is BAD: no "truebc" token, an empty name, a name that begins with "name" (taken for the header
// line); a called record with score_den < 1 or raw_score < 0 has no score.  Comment mode (qcat-eval reads.fastq): bc is the value
// of the last counting "barcode" token ("none" when empty), the bucket is 0, every read is evaluated, and a read without "truebc"
// or without "barcode" is BAD.
#pragma once
#include <stdint.h>

#include "fqtext_core.h"
#include "tsvtext_core.h"

namespace qev {

constexpr uint32_t EVAL_THREADS = 256;                         // lanes of a classify workgroup, one read each and round
constexpr uint32_t EVAL_MAX_BLOCKS = 1024;                     // workgroups of the classify pass: each flushes one histogram
constexpr uint32_t EVAL_VEC = 16;                              // bytes of a loaded vector
constexpr uint32_t EVAL_GROUP = 8;                             // lanes of the group shape: they load eight vectors of a title, one 128-byte line, at once
constexpr uint32_t EVAL_GROUPS = EVAL_THREADS / EVAL_GROUP;    // reads a workgroup of the group shape has in hand at a time
constexpr uint32_t EVAL_Q = 1001;                              // thresholds 0.0, 0.1 ... 100.0
constexpr uint32_t EVAL_BUCKETS = EVAL_Q + 1;
constexpr uint32_t EVAL_KINDS = 3;
constexpr uint32_t EVAL_ROC_COLS = 6;                          // total, correct, incorrect, true_negative, false_negative, false_positive
constexpr uint32_t EVAL_HIST = EVAL_KINDS * EVAL_BUCKETS + 4;  // the (kind, bucket) counts, the four class counts behind them
constexpr uint32_t EVAL_ROC_THREADS = 1024;
static_assert(EVAL_ROC_THREADS >= EVAL_Q, "one lane per threshold");
constexpr uint32_t EVAL_NO_BAD = 0xFFFFFFFFu;                  // "no bad read": the minimum's start

enum : uint8_t { CLS_DROPPED = 0, CLS_CORRECT = 1, CLS_INCORRECT = 2, CLS_FN = 3, CLS_FP = 4, CLS_BAD = 0x80 };
enum : uint8_t { BAD_NO_TRUEBC = 1, BAD_EMPTY_NAME = 2, BAD_NAME_HEADER = 3, BAD_NO_BARCODE = 4, BAD_SCORE = 5 };
enum : uint8_t { KIND_TRUTH_NONE = 0, KIND_WHOLE = 1, KIND_OTHER = 2 };

QP_HD uint32_t ctz32(uint32_t m) { return (uint32_t)__builtin_ctz(m); }
QP_HD uint32_t pop32(uint32_t m) { return (uint32_t)__builtin_popcount(m); }

// ---- masks of a vector: bit b = byte b is the byte c --------------------------------------------------------------------------------
QP_HD uint32_t byte_mask16(const qpart::Vec16& v, uint32_t c) {
    const uint32_t p = c * 0x01010101u;
    uint32_t m = 0;
    for (uint32_t i = 0; i < 4; ++i) m |= qfq::pack_high(qfq::zero_bytes(v.w[i] ^ p)) << (4 * i);
    return m;
}
QP_HD uint32_t blank_mask16(const qpart::Vec16& v) { return byte_mask16(v, ' ') | byte_mask16(v, '\t'); }
// bits [lo, hi) of a vector's mask, 0 <= lo <= hi <= 16
QP_HD uint32_t bits_between(uint32_t lo, uint32_t hi) { return ((1u << hi) - 1u) & ~((1u << lo) - 1u); }

// ---- the tokens of a title ----------------------------------------------------------------------------------------------------------
struct Span { uint64_t b, e; };                                // bytes [b, e) of the text plane
// the scan's state between two vectors: the token in hand -- its first byte, the '=' seen in it (2: two or more), the first of
// them -- and what the finished tokens gave
struct Scan {
    uint64_t tok, eq;
    uint32_t n_eq, in_name;                                    // in_name: the token in hand is the name (it states nothing)
    uint32_t has_truebc, has_barcode, name_len;
    Span truebc, barcode;
};

QP_HD bool key_is(const uint8_t* text, uint64_t at, const char* key, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) if (text[at + i] != (uint8_t)key[i]) return false;
    return true;
}
// the token [S.tok, end) ends: a counting token with the key "truebc" or "barcode" replaces the value held so far
QP_HD void token_end(Scan& S, const uint8_t* text, uint64_t end) {
    if (S.in_name) { S.name_len = (uint32_t)(end - S.tok); return; }
    if (S.n_eq != 1) return;
    const uint64_t klen = S.eq - S.tok;
    if (klen == 6 && key_is(text, S.tok, "truebc", 6)) { S.has_truebc = 1; S.truebc.b = S.eq + 1; S.truebc.e = end; }
    else if (klen == 7 && key_is(text, S.tok, "barcode", 7)) { S.has_barcode = 1; S.barcode.b = S.eq + 1; S.barcode.e = end; }
}
// the '=' of `seg` (bits of the vector at v0) belong to the token in hand
QP_HD void token_eqs(Scan& S, uint32_t seg, uint64_t v0) {
    if (!seg) return;
    if (S.n_eq == 0) S.eq = v0 + ctz32(seg);
    const uint32_t k = S.n_eq + pop32(seg);
    S.n_eq = k > 2 ? 2 : k;
}
// one vector: its blanks and its '=' as masks, v0 its first byte (a multiple of EVAL_VEC), the title at [t0, t1)
QP_HD void scan_vector(Scan& S, const uint8_t* text, uint32_t blank, uint32_t eq, uint64_t v0, uint64_t t0, uint64_t t1) {
    const uint32_t lo = t0 > v0 ? (uint32_t)(t0 - v0) : 0u;
    const uint32_t hi = t1 < v0 + EVAL_VEC ? (uint32_t)(t1 - v0) : EVAL_VEC;
    const uint32_t valid = bits_between(lo, hi);
    blank &= valid; eq &= valid;
    uint32_t pos = lo;
    while (blank) {
        const uint32_t p = ctz32(blank);
        blank &= blank - 1u;
        token_eqs(S, eq & bits_between(pos, p), v0);
        token_end(S, text, v0 + p);
        S.tok = v0 + p + 1u; S.n_eq = 0; S.in_name = 0;
        pos = p + 1u;
    }
    token_eqs(S, eq & bits_between(pos, EVAL_VEC), v0);
}
// the whole title [t0, t0 + len): load16(a) is the aligned vector at byte a of the text plane (a may lie up to 15 bytes in front
// of the title, and the vector may end up to 15 bytes behind it: the plane's slack)
template <class Load>
QP_HD void scan_title(Scan& S, const uint8_t* text, const Load& load16, uint64_t t0, uint32_t len) {
    S.tok = t0; S.eq = 0; S.n_eq = 0; S.in_name = 1;
    S.has_truebc = S.has_barcode = 0; S.name_len = 0;
    S.truebc.b = S.truebc.e = S.barcode.b = S.barcode.e = 0;
    const uint64_t t1 = t0 + len;
    for (uint64_t v0 = t0 & ~(uint64_t)(EVAL_VEC - 1); v0 < t1; v0 += EVAL_VEC) {
        const qpart::Vec16 v = load16(v0);
        scan_vector(S, text, blank_mask16(v), byte_mask16(v, '='), v0, t0, t1);
    }
    token_end(S, text, t1);
}

// The same scan by a group of EVAL_GROUP lanes, all of which end with the same state: in every round lane gl loads vector gl of
// the round's EVAL_GROUP vectors and takes its two masks (vector_masks: blanks in the low half, '=' in the high half), the
// lanes exchange them -- xchg(m, k, v0): the word m of lane k, which holds the masks of the vector at v0 --, and every lane
// resolves the round's vectors in order from the masks.  No load waits for another.
template <class Load>
QP_HD uint32_t vector_masks(const Load& load16, uint64_t v0, uint64_t t1) {
    if (v0 >= t1) return 0u;
    const qpart::Vec16 v = load16(v0);
    return blank_mask16(v) | (byte_mask16(v, '=') << 16);
}
template <class Load, class Xchg>
QP_HD void scan_title_group(Scan& S, const uint8_t* text, const Load& load16, const Xchg& xchg, uint32_t gl, uint64_t t0, uint32_t len) {
    S.tok = t0; S.eq = 0; S.n_eq = 0; S.in_name = 1;
    S.has_truebc = S.has_barcode = 0; S.name_len = 0;
    S.truebc.b = S.truebc.e = S.barcode.b = S.barcode.e = 0;
    const uint64_t t1 = t0 + len;
    for (uint64_t base = t0 & ~(uint64_t)(EVAL_VEC - 1); base < t1; base += (uint64_t)EVAL_VEC * EVAL_GROUP) {
        const uint32_t mine = vector_masks(load16, base + (uint64_t)EVAL_VEC * gl, t1);
        for (uint32_t k = 0; k < EVAL_GROUP; ++k) {
            const uint64_t v0 = base + (uint64_t)EVAL_VEC * k;
            const uint32_t m = xchg(mine, k, v0);          // (every lane of the group takes part, whatever v0)
            if (v0 < t1) scan_vector(S, text, m & 0xFFFFu, m >> 16, v0, t0, t1);
        }
    }
    token_end(S, text, t1);
}

// ---- the call's text ------------------------------------------------------------------------------------------------------------------
// a "/" b (b null: a alone), or "none"
struct Call { const uint8_t* a; const uint8_t* b; uint32_t la, lb, none; };
QP_HD uint32_t call_len(const Call& c) { return c.none ? 4u : c.la + (c.b ? 1u + c.lb : 0u); }
QP_HD uint8_t none_byte(uint32_t i) { return (uint8_t)(0x656E6F6Eu >> (8u * i)); }       // "none"
QP_HD uint8_t call_byte(const Call& c, uint32_t i) {
    if (c.none) return none_byte(i);
    if (i < c.la) return c.a[i];
    return i == c.la ? (uint8_t)'/' : c.b[i - c.la - 1u];
}
QP_HD bool call_is_none(const Call& c) {
    if (c.none) return true;
    if (call_len(c) != 4u) return false;
    for (uint32_t i = 0; i < 4; ++i) if (call_byte(c, i) != none_byte(i)) return false;
    return true;
}
QP_HD Call call_none() { Call c; c.a = c.b = nullptr; c.la = c.lb = 0; c.none = 1; return c; }
// the call of a record as the TSV's barcode column prints it, from the id slots of the tables' blob
QP_HD Call call_of(const qtsv::Tables& T, int32_t bc, int32_t bc2, int32_t adapter) {
    if (!qtsv::called(T, bc, bc2, adapter)) return call_none();
    const uint32_t t = T.simple ? 0u : (uint32_t)adapter;
    Call c;
    const uint32_t s0 = T.ids_off + (T.id_first[t][0] + (uint32_t)bc) * qtsv::TSV_ID_SLOT;
    c.a = T.blob + s0 + 1; c.la = T.blob[s0]; c.b = nullptr; c.lb = 0; c.none = 0;
    if (T.dual) {
        const uint32_t s1 = T.ids_off + (T.id_first[t][1] + (uint32_t)bc2) * qtsv::TSV_ID_SLOT;
        c.b = T.blob + s1 + 1; c.lb = T.blob[s1];
    }
    return c;
}
// comment mode: the value of the "barcode" token, "none" when it is empty
QP_HD Call call_from(const uint8_t* text, Span v) {
    if (v.e == v.b) return call_none();
    Call c; c.a = text + v.b; c.la = (uint32_t)(v.e - v.b); c.b = nullptr; c.lb = 0; c.none = 0;
    return c;
}

// ---- the verdict ------------------------------------------------------------------------------------------------------------------------
QP_HD bool span_is_call(const uint8_t* text, Span v, const Call& c) {
    const uint32_t n = call_len(c);
    if (v.e - v.b != n) return false;
    for (uint32_t i = 0; i < n; ++i) if (text[v.b + i] != call_byte(c, i)) return false;
    return true;
}
// bc in V.split(","): every element against the call, byte by byte
QP_HD bool list_holds_call(const uint8_t* text, Span v, const Call& c) {
    const uint32_t n = call_len(c);
    bool same = true;
    uint32_t k = 0;
    for (uint64_t i = v.b; i <= v.e; ++i) {
        if (i == v.e || text[i] == ',') {
            if (same && k == n) return true;
            same = true; k = 0;
        } else {
            same = same && k < n && text[i] == call_byte(c, k);
            ++k;
        }
    }
    return false;
}
// a read with a call survives exactly the thresholds q with q * den <= raw * 1000 (den >= 1, raw >= 0)
QP_HD uint32_t bucket_of(int32_t raw, int32_t den) {
    const uint64_t b = (uint64_t)raw * 1000u / (uint64_t)den + 1u;
    return b > EVAL_Q ? EVAL_Q : (uint32_t)b;
}

struct Verdict { uint8_t cls, kind; uint16_t bucket; };
QP_HD Verdict verdict_bad(uint8_t why) { Verdict v; v.cls = CLS_BAD | why; v.kind = 0; v.bucket = 0; return v; }
QP_HD Verdict verdict_of(const uint8_t* text, Span V, const Call& bc, uint32_t bucket) {
    Verdict v;
    const bool no_call = call_is_none(bc);
    const bool truth_none = span_is_call(text, V, call_none());
    v.cls = list_holds_call(text, V, bc) ? CLS_CORRECT : no_call ? CLS_FN : truth_none ? CLS_FP : CLS_INCORRECT;
    v.kind = truth_none ? KIND_TRUTH_NONE : span_is_call(text, V, bc) ? KIND_WHOLE : KIND_OTHER;
    v.bucket = (uint16_t)(no_call ? 0u : bucket);
    return v;
}
// one evaluated read from the scan of its stored title at t0 and, without from_comment, its record
QP_HD Verdict verdict_from_scan(const Scan& S, const qtsv::Tables& T, const uint8_t* text, uint64_t t0, bool from_comment,
                                int32_t bc, int32_t bc2, int32_t adapter, int32_t raw, int32_t den) {
    if (from_comment) {
        if (!S.has_truebc) return verdict_bad(BAD_NO_TRUEBC);
        if (!S.has_barcode) return verdict_bad(BAD_NO_BARCODE);
        return verdict_of(text, S.truebc, call_from(text, S.barcode), 0u);
    }
    if (S.name_len == 0) return verdict_bad(BAD_EMPTY_NAME);
    if (S.name_len >= 4 && key_is(text, t0, "name", 4)) return verdict_bad(BAD_NAME_HEADER);
    if (!S.has_truebc) return verdict_bad(BAD_NO_TRUEBC);
    const Call c = call_of(T, bc, bc2, adapter);
    if (c.none) return verdict_of(text, S.truebc, c, 0u);
    if (den < 1 || raw < 0) return verdict_bad(BAD_SCORE);
    return verdict_of(text, S.truebc, c, bucket_of(raw, den));
}
// ... by one lane: its stored title [t0, t0 + len)
template <class Load>
QP_HD Verdict read_verdict(const qtsv::Tables& T, const uint8_t* text, const Load& load16, uint64_t t0, uint32_t len, bool from_comment,
                           int32_t bc, int32_t bc2, int32_t adapter, int32_t raw, int32_t den) {
    Scan S;
    scan_title(S, text, load16, t0, len);
    return verdict_from_scan(S, T, text, t0, from_comment, bc, bc2, adapter, raw, den);
}
// ... by lane gl of a group (every lane of the group gets the same verdict)
template <class Load, class Xchg>
QP_HD Verdict read_verdict_group(const qtsv::Tables& T, const uint8_t* text, const Load& load16, const Xchg& xchg, uint32_t gl, uint64_t t0,
                                 uint32_t len, bool from_comment, int32_t bc, int32_t bc2, int32_t adapter, int32_t raw, int32_t den) {
    Scan S;
    scan_title_group(S, text, load16, xchg, gl, t0, len);
    return verdict_from_scan(S, T, text, t0, from_comment, bc, bc2, adapter, raw, den);
}
QP_HD const char* bad_text(uint8_t why) {
    return why == BAD_NO_TRUEBC ? "its comment holds no truebc=<ids> token"
         : why == BAD_EMPTY_NAME ? "its name is empty (the reference's reader shifts the row's columns)"
         : why == BAD_NAME_HEADER ? "its name begins with \"name\" (the reference's reader takes the row for the header line)"
         : why == BAD_NO_BARCODE ? "its comment holds no barcode=<id> token"
         : "its record is called with score_den < 1 or raw_score < 0";
}

// ---- counting -------------------------------------------------------------------------------------------------------------------------
QP_HD uint32_t hist_slot(uint32_t kind, uint32_t bucket) { return kind * EVAL_BUCKETS + bucket; }
QP_HD uint32_t class_slot(uint32_t cls) { return EVAL_KINDS * EVAL_BUCKETS + cls - 1u; }
// suffix sums of one kind's buckets: put(b, sum of hist(kind, b') over b' >= b) for b = EVAL_BUCKETS .. 0 (EVAL_BUCKETS + 1 entries,
// the last one 0) -- one pass, one lane per kind
template <class Hist, class Put>
QP_HD void suffix_sums(const Hist& hist, uint32_t kind, const Put& put) {
    uint32_t sum = 0;
    put(EVAL_BUCKETS, 0u);
    for (uint32_t b = EVAL_BUCKETS; b-- > 0;) { sum += hist(hist_slot(kind, b)); put(b, sum); }
}
// row q of the ROC table from the suffix sums suf(kind, b): the reads behind q stand, the reads up to q are "none"
template <class Suf>
QP_HD void roc_row(const Suf& suf, uint32_t q, int64_t* row /* EVAL_ROC_COLS */) {
    int64_t above[EVAL_KINDS], upto[EVAL_KINDS];
    for (uint32_t k = 0; k < EVAL_KINDS; ++k) { above[k] = (int64_t)suf(k, q + 1u); upto[k] = (int64_t)suf(k, 0u) - above[k]; }
    row[1] = above[KIND_WHOLE]; row[2] = above[KIND_OTHER]; row[3] = upto[KIND_TRUTH_NONE];
    row[4] = upto[KIND_WHOLE] + upto[KIND_OTHER]; row[5] = above[KIND_TRUTH_NONE];
    row[0] = row[1] + row[2] + row[3] + row[4] + row[5];
}
// the workgroups of the classify pass over n reads
QP_HD uint32_t classify_blocks(uint32_t n) {
    const uint32_t want = n / EVAL_THREADS + 1u;
    return want < EVAL_MAX_BLOCKS ? want : EVAL_MAX_BLOCKS;
}
// ... of its group shape
QP_HD uint32_t classify_group_blocks(uint32_t n) {
    const uint32_t want = n / EVAL_GROUPS + 1u;
    return want < EVAL_MAX_BLOCKS ? want : EVAL_MAX_BLOCKS;
}

}  // namespace qev

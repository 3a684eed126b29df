// kernels_common.inc -- kernels shared by the generic and the packed path:
//   k_pack_windows   reads (ASCII, any length)  ->  one 160-byte code window per read end
//   k_finalize       per-end records            ->  qcat_result per read + count histogram
// Included by qcat_hip.hip.

namespace qk {

struct KitPtrs {
    const DevKit* kit;
    const uint8_t* codes;
    const int32_t* ids;
    const uint32_t* tables;
};

__device__ __forceinline__ uint32_t dev_code_of(uint32_t c) {
    uint32_t u = c & 0xDFu;
    uint32_t r = QCAT_CODE_OTHER;
    r = (u == 'A') ? (uint32_t)QCAT_CODE_A : r;
    r = (u == 'T') ? (uint32_t)QCAT_CODE_T : r;
    r = (u == 'G') ? (uint32_t)QCAT_CODE_G : r;
    r = (u == 'C') ? (uint32_t)QCAT_CODE_C : r;
    r = (u == 'N') ? (uint32_t)QCAT_CODE_N : r;
    r = (u == 'X') ? (uint32_t)QCAT_CODE_X : r;
    return r;
}

// ---------------------------------------------------------------------------------------------
// k_pack_windows: replaces extract_align_sequence + utils.revcomp (qcat/scanner_base.py:223-244,
// qcat/utils.py:20-21).  Window e = 2*r + side (side 0: read[:n]; side 1: revcomp(read[-n:]));
// with QCAT_ENDS_5P only side 0 exists.  Codes beyond the window length are PAD.  In code space
// the complement is `code ^ 1` for A,T,G,C and the identity for everything else (IUPAC letters
// map to "other" before and after complementing).
// One thread produces 32 consecutive codes; a window is 5 threads.  The 32 source bytes are fetched
// as nine aligned dwords and funnel-shifted into place (the batch buffer has slack on both
// sides), and converted four at a time:  idx = (c & 0xDF) >> 1 & 7 separates
// A, C, G, T, N, X; one v_perm_b32 maps idx to the code, a second one to the letter idx stands
// for, and a byte that is not that letter becomes "other".
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t dev_codes_of4(uint32_t w) {
    const uint32_t u = w & 0xDFDFDFDFu;
    const uint32_t idx = (u >> 1) & 0x07070707u;
    uint32_t code = __builtin_amdgcn_perm(0x04060605u, 0x02010300u, idx);        // A0 C3 T1 G2 | X5 -6 -6 N4
    const uint32_t expect = __builtin_amdgcn_perm(0x4EFFFF58u, 0x47544341u, idx); // 'A' 'C' 'T' 'G' | 'X' - - 'N'
    const uint32_t diff = u ^ expect;
    const uint32_t nz = (((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) & 0x80808080u;   // bit 7 of every non-zero byte
    const uint32_t m = nz - (nz >> 7);                   // 0x7F in every flagged byte, all a code's bits (0x80 - 0x01 borrows nothing; a 32-bit multiply is quarter rate)
    return __builtin_amdgcn_bitop3_b32(code, 0x06060606u, m, 0xD8u);       // m ? 6 : code
}

// 16 bytes starting at the (unaligned) address p, as four dwords in address order
__device__ __forceinline__ void dev_load16_unaligned(const uint8_t* p, uint32_t (&w)[4]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
    w[0] = __builtin_amdgcn_alignbyte(r1, r0, sh);
    w[1] = __builtin_amdgcn_alignbyte(r2, r1, sh);
    w[2] = __builtin_amdgcn_alignbyte(r3, r2, sh);
    w[3] = __builtin_amdgcn_alignbyte(r4, r3, sh);
}

// keep the first n (0..4) bytes of w, PAD the rest
__device__ __forceinline__ uint32_t dev_pad_tail(uint32_t w, int n) {
    const uint32_t mask = n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : ((1u << (8 * n)) - 1u));
    return (w & mask) | (0x07070707u & ~mask);
}

// sixteen 2-bit codes (code i in bits 2 i, 2 i + 1) -> sixteen byte codes
__device__ __forceinline__ void dev_expand16(uint32_t w, uint32_t (&out)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (w >> (8 * q)) & 0xFFu;
        out[q] = (x & 3u) | ((x & 0xCu) << 6) | ((x & 0x30u) << 12) | ((x & 0xC0u) << 18);
    }
}
// 16 codes of read end e's window from code position pos on, as bytes.  Round 4: k_pack_windows writes the byte window of an
// end only when it has to (k_expand_special: a letter outside A, C, G, T -- `wspec`), every other window exists at two bits
// per code only (`win2`) and is expanded here.  Codes beyond the window's length are whatever the neighbour holds: the caller
// pads by the window / region length.  win2 == nullptr: every end has its byte window.
__device__ __forceinline__ void dev_window16(const uint8_t* __restrict__ win, const uint32_t* __restrict__ win2, const uint8_t* __restrict__ wspec,
                                             uint32_t e, int pos, uint32_t (&out)[4]) {
    if (win2 == nullptr || wspec[e]) { dev_load16_unaligned(win + (size_t)e * WIN_STRIDE + pos, out); return; }
    const uint32_t* __restrict__ r = win2 + (size_t)e * WIN2_WORDS + (pos >> 4);
    dev_expand16(__builtin_amdgcn_alignbit(r[1], r[0], (uint32_t)(pos & 15) * 2u), out);
}
// ... one code at a time (the general DP of k_barcode_redo over a plain window)
struct Win2Seq {
    const uint32_t* row; int start;
    __device__ __forceinline__ int operator()(int i) const { const int p = start + i; return (int)((row[p >> 4] >> (2 * (p & 15))) & 3u); }
};

// 16 codes of a virtual window at positions i0 .. i0+15 (PAD from position L on).  side 0: position
// p is the byte p0[p]; side 1: the reverse complement, position p is the byte pend[-1-p],
// complemented in code space (code ^ 1 for A,T,G,C).
__device__ __forceinline__ void dev_window_codes16(const uint8_t* p0, const uint8_t* pend, int side, int i0, int L,
                                                   uint32_t (&out)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = 0x07070707u;
    if (i0 >= L) return;
    uint32_t w[4];
    if (side == 0) {
        dev_load16_unaligned(p0 + i0, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = dev_pad_tail(dev_codes_of4(w[q]), L - i0 - 4 * q);
    } else {
        dev_load16_unaligned(pend - i0 - 16, w);             // the 16 bytes below pend - i0, to be reversed
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t c = dev_codes_of4(__builtin_amdgcn_perm(0u, w[3 - q], 0x00010203u));
            c ^= ~(c >> 2) & 0x01010101u;
            out[q] = dev_pad_tail(c, L - i0 - 4 * q);
        }
    }
}

// 32 bytes starting at the (unaligned) address p, as eight dwords in address order
__device__ __forceinline__ void dev_load32_unaligned(const uint8_t* p, uint32_t (&w)[8]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t r[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = q[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbyte(r[i + 1], r[i], sh);
}

// 32 codes per thread: 36 bytes in flight per lane, and the index and length arithmetic once per 32 codes.  A workgroup is
// PACK_WINDOWS windows, so window and part come from the thread index by one multiply, and ENDS is a template argument (the
// first form, one thread per 16 codes, divided a 64-bit global index by 10 and by `ends`).  The two sides share one
// instruction stream: the side picks the address, the byte order (v_perm selector) and the complement mask, where a branch
// made every wave -- windows of both sides in each -- walk both bodies.  That form was bound by the VALU, not by its bytes
// (DESIGN.md 3.1: 308 VALU instructions per wave, 1.57 of its 1.59 ms per 10 M reads; now 1.04 ms).
constexpr uint32_t PACK_CODES = 32;                                      // codes per thread
constexpr uint32_t PACK_PARTS = WIN_STRIDE / PACK_CODES;                 // 5
constexpr uint32_t PACK_WINDOWS = 64;
constexpr uint32_t PACK_THREADS = PACK_WINDOWS * PACK_PARTS;

// One thread's share of a window: the 32 codes from position part * 32 on of read end e, stored exactly as k_pack_windows
// stores them (the body of that kernel; k_pack_planes, kernels_abs.inc, is the second caller).  p: the codes at two bits
// each, whether or not win2 is given; the return value: this part holds a letter outside A, C, G, T, or the window is shorter
// than max_align -- the end stays off the bit-sliced adapter path.
template <int ENDS>
__device__ __forceinline__ bool dev_pack_part(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets, int max_align,
                                              uint64_t e, uint32_t part,
                                              uint8_t* __restrict__ win, int32_t* __restrict__ wlen, uint8_t* __restrict__ wspec,
                                              uint32_t* __restrict__ win2, int lazy_bytes, uint32_t (&p)[PACK_CODES / 16]) {
    const uint64_t r = ENDS == 2 ? e >> 1 : e;
    const uint32_t side = ENDS == 2 ? (uint32_t)e & 1u : 0u;
    uint64_t beg = offsets[r], end = offsets[r + 1];
    uint64_t len = end - beg;
    int L = len < (uint64_t)max_align ? (int)len : max_align;
    if (part == 0) wlen[e] = L;
    const int i0 = (int)(part * PACK_CODES);
    constexpr int NW = PACK_CODES / 4;
    uint32_t out[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) out[q] = 0x07070707u;
    if (i0 < L) {
        // dev_window_codes16 with the side as data: side 1 reads the 32 bytes below end - i0, reverses them and complements the codes
        uint32_t w[NW];
        dev_load32_unaligned(bases + (side ? end - (uint64_t)i0 - PACK_CODES : beg + (uint64_t)i0), w);
        const uint32_t rev = 0u - side;                                  // all ones on side 1
        const uint32_t order = side ? 0x00010203u : 0x03020100u, comp = rev & 0x01010101u;
        const int n8 = 8 * (L - i0);                                     // bits of these codes inside the window
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const uint32_t x = __builtin_amdgcn_bitop3_b32(w[q], w[NW - 1 - q], rev, 0xD8u);   // rev ? w[NW - 1 - q] : w[q]
            uint32_t c = dev_codes_of4(__builtin_amdgcn_perm(0u, x, order));
            c ^= ~(c >> 2) & comp;
            // dev_pad_tail(c, L - i0 - 4 q): the bytes from the window's end on are PAD (a 64-bit shift, so that 32 clears the word)
            const int keep = min(max(n8 - 32 * q, 0), 32);
            const uint32_t pad = (uint32_t)(0xFFFFFFFFull << keep);
            out[q] = __builtin_amdgcn_bitop3_b32(c, 0x07070707u, pad, 0xD8u);
        }
    }
    if (!lazy_bytes) {
        uint4* __restrict__ to = reinterpret_cast<uint4*>(win + e * WIN_STRIDE + part * PACK_CODES);
#pragma unroll
        for (int h = 0; h < NW / 4; ++h) to[h] = make_uint4(out[4 * h], out[4 * h + 1], out[4 * h + 2], out[4 * h + 3]);
    }
    // code i of a 16-code chunk in bits 2 i, 2 i + 1 of its dword
#pragma unroll
    for (int h = 0; h < NW / 4; ++h) {
        p[h] = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t t = out[4 * h + q] & 0x03030303u;
            t = (t | (t >> 6)) & 0x000F000Fu;
            t = (t | (t >> 12)) & 0xFFu;
            p[h] |= t << (8 * q);
        }
    }
    if (win2) *reinterpret_cast<uint2*>(win2 + e * WIN2_WORDS + part * (PACK_CODES / 16)) = make_uint2(p[0], p[1]);
    uint32_t spec = 0;
    if (wspec) {                 // a letter outside A, C, G, T (codes 4, 5, 6; 7 is padding): the window stays off the bit-sliced path
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const uint32_t t = out[q] & 0x07070707u;
            spec |= (t >> 2) & ~(t & (t >> 1) & (t >> 2)) & 0x01010101u;
        }
        if (spec) wspec[e] = 1;
    }
    return spec != 0 || L != max_align;
}

template <int ENDS>
__global__ void __launch_bounds__(PACK_THREADS)
k_pack_windows(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets,
               uint32_t n_reads, int max_align,
               uint8_t* __restrict__ win, int32_t* __restrict__ wlen, uint8_t* __restrict__ wspec,
               uint32_t* __restrict__ win2 /* two bits per code beside the bytes (WIN2_WORDS dwords per window; meaningful for
                                              windows of plain A, C, G, T): what the bit-sliced kernels read; or null */,
               int lazy_bytes = 0 /* 1: no byte windows here -- k_expand_special writes those of the flagged ends, every reader
                                     expands the others from win2 (dev_window16): 3.3 GB less to write per 10 M reads */) {
    static_assert(ENDS == 1 || ENDS == 2, "one or two windows per read");
    static_assert(PACK_PARTS == 5 && PACK_PARTS * PACK_CODES == WIN_STRIDE && PACK_THREADS < 1000, "threadIdx.x / 5 below is (x * 205) >> 10");
    const uint32_t wl = (threadIdx.x * 205u) >> 10;
    const uint32_t part = threadIdx.x - wl * PACK_PARTS;
    const uint64_t e = (uint64_t)blockIdx.x * PACK_WINDOWS + wl;
    if (e >= (uint64_t)n_reads * ENDS) return;
    uint32_t p[PACK_CODES / 16];
    (void)dev_pack_part<ENDS>(bases, offsets, max_align, e, part, win, wlen, wspec, win2, lazy_bytes, p);
}

// the byte windows of the read ends k_pack_windows flagged (a letter outside A, C, G, T): the only ones a lazy scan has
__global__ void __launch_bounds__(256)
k_expand_special(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets, uint32_t n_reads, int ends, int max_align,
                 const uint8_t* __restrict__ wspec, uint8_t* __restrict__ win) {
    // one thread per read end; a flagged one (rare) writes its ten chunks.  (First form: one thread per chunk, 200 M threads per
    // 10 M reads that each read the flag and left -- 0.22 ms of config 3's step for a few thousand windows.)
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)n_reads * ends || !wspec[e]) return;
    const uint64_t r = e / ends;
    const uint64_t beg = offsets[r], end = offsets[r + 1], len = end - beg;
    const int L = len < (uint64_t)max_align ? (int)len : max_align;
    for (uint32_t chunk = 0; chunk < WIN_STRIDE / 16; ++chunk) {
        uint32_t out[4];
        dev_window_codes16(bases + beg, bases + end, (int)(e % ends), (int)chunk * 16, L, out);
        *reinterpret_cast<uint4*>(win + e * WIN_STRIDE + chunk * 16) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// ---------------------------------------------------------------------------------------------
// k_finalize: replaces the tail of scan() (build_return_dict, adapter_end clamp,
// scanner_epi2me.py:135-144; dual combination scanner_dual.py:130-146) and all of
// detect_barcode after the two scans (qcat/scanner_base.py:542-604, SURVEY.md R6).
// Integer only: thresholds were folded into the kit on the host (kit.h).
// ---------------------------------------------------------------------------------------------
struct EndScan {
    int has, bc0, bc1, raw, den, adapter, adapter_end, exit_status, pass, conflict_ok;
};

__device__ __forceinline__ EndScan dev_empty_scan() {
    EndScan s; s.has = 0; s.bc0 = -1; s.bc1 = -1; s.raw = 0; s.den = 1; s.adapter = -1;
    s.adapter_end = 0; s.exit_status = 1; s.pass = 0; s.conflict_ok = 0;
    return s;
}

__device__ __forceinline__ EndScan dev_make_scan(const KitPtrs& kp, const EndRec& a) {
    const DevKit* k = kp.kit;
    const DevTpl& p = k->tpl[a.used_tpl];
    EndScan s = dev_empty_scan();
    if (k->mode == QCAT_MODE_EPI2ME) {
        int ae = a.best_end + p.trim_offset;
        if (ae > a.window_len) ae = a.window_len;
        s.adapter = a.used_tpl; s.adapter_end = ae; s.exit_status = 0;
        if (a.bc_idx[0] >= 0) {
            s.has = 1; s.bc0 = a.bc_idx[0]; s.raw = a.bc_raw[0]; s.den = p.sets[0].tlen;
            s.pass = s.raw >= p.sets[0].min_raw_pass;
            s.conflict_ok = s.raw >= p.sets[0].min_raw_conflict;
        }
    } else if (k->mode == QCAT_MODE_SIMPLE) {
        // scanner_simple.py:70-91: the winner's score (returned in the `identity` slot, scanner_base.py:141) below
        // min_quality -> empty_return_dict(); otherwise adapter None and adapter_end = the winner's end_query
        // (barcodes of unequal length, a user FASTA: the winner's own length and thresholds -- kit_prepare.inc, len_off)
        int den = p.sets[0].tlen, thr_pass = p.sets[0].min_raw_pass, thr_conflict = p.sets[0].min_raw_conflict;
        if (p.sets[0].len_off >= 0 && a.bc_idx[0] >= 0) {
            const int32_t* e = kp.ids + p.sets[0].len_off + 3 * a.bc_idx[0];
            den = e[0]; thr_pass = e[1]; thr_conflict = e[2];
        }
        if (a.bc_idx[0] >= 0 && a.bc_raw[0] >= thr_pass) {
            s.has = 1; s.bc0 = a.bc_idx[0]; s.raw = a.bc_raw[0]; s.den = den;
            s.adapter = -1; s.adapter_end = a.best_end; s.exit_status = 0; s.pass = 1;
            s.conflict_ok = s.raw >= thr_conflict;
        }
    } else if (a.bc_idx[0] >= 0 && a.bc_idx[1] >= 0) {
        s.has = 1; s.bc0 = a.bc_idx[0]; s.bc1 = a.bc_idx[1];
        s.adapter = a.used_tpl; s.adapter_end = a.best_end; s.exit_status = 0;
        int r0 = a.bc_raw[0], d0 = p.sets[0].tlen, r1 = a.bc_raw[1], d1 = p.sets[1].tlen;
        if (r1 * d0 < r0 * d1) { s.raw = r1; s.den = d1; } else { s.raw = r0; s.den = d0; }   // min(s0, s1)
        s.pass = r0 >= p.sets[0].min_raw_pass && r1 >= p.sets[1].min_raw_pass;
        s.conflict_ok = r0 >= p.sets[0].min_raw_conflict && r1 >= p.sets[1].min_raw_conflict;
    }
    return s;
}

__device__ __forceinline__ bool dev_same_id(const KitPtrs& kp, const EndScan& a, const EndScan& b) {
    const DevTpl& pa = kp.kit->tpl[a.adapter < 0 ? 0 : a.adapter];      // (simple mode: adapter None, one barcode list)
    const DevTpl& pb = kp.kit->tpl[b.adapter < 0 ? 0 : b.adapter];
    if (kp.ids[pa.sets[0].ids_off + a.bc0] != kp.ids[pb.sets[0].ids_off + b.bc0]) return false;
    if (a.bc1 >= 0 || b.bc1 >= 0) {
        if (a.bc1 < 0 || b.bc1 < 0) return false;
        if (kp.ids[pa.sets[1].ids_off + a.bc1] != kp.ids[pb.sets[1].ids_off + b.bc1]) return false;
    }
    return true;
}

__device__ __forceinline__ void dev_store_result(qcat_result* o, const EndScan& s, int trim5, int64_t trim3) {
    qcat_result r;
    r.barcode_idx = (int16_t)s.bc0; r.barcode2_idx = (int16_t)s.bc1;
    r.adapter_idx = (int16_t)s.adapter; r.exit_status = (int16_t)s.exit_status;
    r.adapter_end = s.adapter_end; r.trim5p = trim5; r.trim3p = (int32_t)trim3;
    r.raw_score = (int16_t)s.raw; r.score_den = (int16_t)s.den;
    *o = r;
}

// ---------------------------------------------------------------------------------------------
// k_count: the count histogram from finished records (used when k_scan_middle may still change
// records after k_finalize; otherwise k_finalize counts on the fly).
// ---------------------------------------------------------------------------------------------
constexpr int FIN_LDS_BUCKETS = 16384;     // 64 KiB of LDS; the shipped dual kit needs 14 403
constexpr int FIN_DYN_BUCKETS = (65536 - 256 * (int)sizeof(qcat_result)) / 4;      // k_finalize: 64 KiB of dynamic LDS less its result lines
#ifndef QCAT_RTC
static inline size_t fin_lds_bytes(int nbuckets, bool counting) {
    return 256 * sizeof(qcat_result) + ((counting && nbuckets <= FIN_DYN_BUCKETS) ? (size_t)nbuckets * 4 : 0);
}
#endif

// the driver's min-length filter (qcat/cli.py:521-534): len(sequence[trim5p:trim3p]) (or len(sequence) without
// trimming) < min_read_length -> the read is only counted as skipped
__device__ __forceinline__ bool dev_skipped(const DevKit* k, int64_t len, int trim5, int64_t trim3) {
    if (k->min_read_length <= 0) return false;
    if (k->trim_reads && k->ends != QCAT_ENDS_5P) {
        const int64_t a = trim5 < len ? trim5 : len, b = trim3 < len ? trim3 : len;
        len = b > a ? b - a : 0;
    }
    return len < (int64_t)k->min_read_length;
}

// the barcode bucket of a call in the count vector (update_barcode_count, qcat/scanner_base.py:680-689): the slot of the
// barcode's id -- dual mode: slot1 * n_slots + slot2 -- for a call with an adapter (simple mode: any call), else `none`
// (= nbc).  One function for k_finalize, k_count and the bins of qcat_batch_partition (kernels_partition.inc).
__device__ __forceinline__ int dev_barcode_bucket(const KitPtrs& kp, int nb, int nbc, int bc0, int bc1, int adapter) {
    const DevKit* k = kp.kit;
    int slot = nbc;
    if (bc0 >= 0 && (adapter >= 0 || k->mode == QCAT_MODE_SIMPLE)) {
        const DevTpl& p = k->tpl[adapter < 0 ? 0 : adapter];
        slot = kp.ids[p.sets[0].ids_off + bc0];
        if (k->mode == QCAT_MODE_DUAL) slot = slot * nb + kp.ids[p.sets[1].ids_off + bc1];
    }
    return slot;
}

__global__ void __launch_bounds__(256)
k_count(KitPtrs kp, const qcat_result* __restrict__ results, const uint64_t* __restrict__ offsets,
        const uint32_t* __restrict__ true_len, uint32_t n_reads, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t hist[FIN_LDS_BUCKETS];
    const DevKit* k = kp.kit;
    const int nbuckets = k->n_buckets;
    const bool lds_hist = nbuckets <= FIN_LDS_BUCKETS;
    if (lds_hist) {
        for (int i = threadIdx.x; i < nbuckets; i += blockDim.x) hist[i] = 0;
        __syncthreads();
    }
    const int nb = k->n_barcode_slots;
    const int nbc = (k->mode == QCAT_MODE_DUAL) ? nb * nb : nb;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * blockDim.x) {
        const qcat_result res = results[r];
        int slot = dev_barcode_bucket(kp, nb, nbc, res.barcode_idx, res.barcode2_idx, res.adapter_idx);
        int kslot = nbc + 1 + (res.adapter_idx >= 0 ? k->tpl[res.adapter_idx].kit_slot : k->n_kit_slots);
        const int64_t len = true_len ? (int64_t)true_len[r] : (int64_t)(offsets[r + 1] - offsets[r]);
        if (dev_skipped(k, len, res.trim5p, res.trim3p)) { slot = nbuckets - 1; kslot = -1; }
        if (lds_hist) { atomicAdd(&hist[slot], 1u); if (kslot >= 0) atomicAdd(&hist[kslot], 1u); }
        else { atomicAdd(&counts[slot], 1ull); if (kslot >= 0) atomicAdd(&counts[kslot], 1ull); }
    }
    if (lds_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < nbuckets; i += blockDim.x)
            if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// k_vote: scan_ends + the vote of detect_kit (qcat/scanner_base.py:632-642, :662-678).  The
// normalised adapter scores of the two ends are compared by cross-multiplication; "no template
// beat -1.0" is the fraction -1/100 and indexes the LAST template (Python [-1]).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_vote(const DevKit* __restrict__ k, const EndRec* __restrict__ recs, uint32_t n_reads,
       unsigned long long* __restrict__ votes, unsigned long long* __restrict__ first_read, uint32_t batch_reads = 0) {
    // batch_reads > 0 (round 4, the kit-auto file loop): blockIdx.y is a batch of that many reads in file order with counters
    // of its own -- votes / first_read [batch][MAX_T], the first voting read counted from the batch's start
    __shared__ uint32_t cnt[MAX_T];
    __shared__ uint32_t first[MAX_T];
    if (threadIdx.x < MAX_T) { cnt[threadIdx.x] = 0; first[threadIdx.x] = 0xFFFFFFFFu; }
    __syncthreads();
    const uint32_t r0 = batch_reads ? blockIdx.y * batch_reads : 0u;
    const uint32_t r1 = batch_reads ? min(n_reads, r0 + batch_reads) : n_reads;
    for (uint32_t r = r0 + blockIdx.x * blockDim.x + threadIdx.x; r < r1; r += gridDim.x * blockDim.x) {
        const EndRec a = recs[2 * (size_t)r], b = recs[2 * (size_t)r + 1];
        const int ra = a.best_tpl < 0 ? -1 : a.best_raw, da = a.best_tpl < 0 ? 100 : k->tpl[a.best_tpl].den;
        const int rb = b.best_tpl < 0 ? -1 : b.best_raw, db = b.best_tpl < 0 ? 100 : k->tpl[b.best_tpl].den;
        const int pick = ((long long)ra * db > (long long)rb * da) ? a.used_tpl : b.used_tpl;   // score_5p > score_3p
        atomicAdd(&cnt[pick], 1u);
        atomicMin(&first[pick], r - r0);
    }
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * MAX_T;
    if (threadIdx.x < MAX_T && cnt[threadIdx.x]) {
        atomicAdd(&votes[base + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
        atomicMin(&first_read[base + threadIdx.x], (unsigned long long)first[threadIdx.x]);
    }
}

// detect_kit's choice (qcat/scanner_base.py:657-678) on the device: the votes of the templates folded onto their kit
// slots, most votes win, equal counts keep the order of first appearance (dict insertion order + stable sort); -1: nobody voted
__global__ void __launch_bounds__(64)
k_pick_kit(const DevKit* __restrict__ k, const unsigned long long* votes, const unsigned long long* first_read, int32_t* __restrict__ chosen) {
    // one thread per kit slot sums its templates' votes (shared memory: no dynamically indexed private arrays), thread 0 picks;
    // one block per batch of the vote (k_vote: counters [batch][MAX_T])
    __shared__ unsigned long long cnt[MAX_T], first[MAX_T], tv[MAX_T], tf[MAX_T];
    __shared__ int tslot[MAX_T];
    const int s = (int)threadIdx.x;
    votes += (size_t)blockIdx.x * MAX_T; first_read += (size_t)blockIdx.x * MAX_T;
    // (round 6: a template per thread fetches its slot and its counters -- one round trip to memory instead of one per template
    // in every thread's loop: 44 us of the reference driver's 4000-read call)
    const int nt = k->nt;
    if (s < MAX_T) {
        const bool live = s < nt;
        tslot[s] = live ? k->tpl[s].kit_slot : -1;
        tv[s] = live ? __atomic_load_n(&votes[s], __ATOMIC_RELAXED) : 0ull;
        tf[s] = live ? __atomic_load_n(&first_read[s], __ATOMIC_RELAXED) : ~0ull;
    }
    __syncthreads();
    if (s < MAX_T) {
        unsigned long long c = 0, f = ~0ull;
        for (int t = 0; t < nt; ++t) {
            if (tslot[t] != s) continue;
            const unsigned long long v = tv[t], fr = tf[t];
            c += v;
            if (v && fr < f) f = fr;
        }
        cnt[s] = c; first[s] = f;
    }
    __syncthreads();
    if (s != 0) return;
    int best = -1;
    unsigned long long bc = 0, bf = ~0ull;
    for (int q = 0; q < k->n_kit_slots && q < MAX_T; ++q) {
        const unsigned long long c = cnt[q], f = first[q];
        if (c && (best < 0 || c > bc || (c == bc && f < bf))) { best = q; bc = c; bf = f; }
    }
    chosen[blockIdx.x] = best;
}

__global__ void __launch_bounds__(256)
k_finalize(KitPtrs kp, const EndRec* __restrict__ recs, const uint64_t* __restrict__ offsets,
           const uint32_t* __restrict__ true_len,
           uint32_t n_reads, qcat_result* __restrict__ out, unsigned long long* __restrict__ counts,
           const int2* __restrict__ bcres /* packed (barcode index, raw score) per job, or null: the records hold them */,
           const uint32_t* __restrict__ fin /* window length | used template << 8 | adapter end << 16 per read end instead of
                                               the records (k_adapter_finish), or null */) {
    // dynamic LDS (fin_lds_bytes): the block's results, stored as whole lines, then the count histogram -- sized by the kit's
    // bucket count, so that a 100-bucket kit is not held to two blocks per CU by the 58 KiB a dual kit needs
    extern __shared__ uint32_t fin_lds[];
    static_assert(sizeof(qcat_result) % 4 == 0, "results leave as dwords");
    constexpr uint32_t RW = sizeof(qcat_result) / 4;
    uint32_t* const s_out = fin_lds;
    uint32_t* const hist = fin_lds + 256 * RW;
    const DevKit* k = kp.kit;
    const int nsets_all = k->mode == QCAT_MODE_DUAL ? 2 : 1;
    auto load = [&](uint64_t i) {
        EndRec a;
        if (fin) {                                       // all dev_make_scan reads besides the barcode results
            const uint32_t w = fin[i];
            a.window_len = (int32_t)(w & 0xFFu); a.used_tpl = (int32_t)((w >> 8) & 0xFFu); a.best_end = (int32_t)(int16_t)(w >> 16);
            a.best_tpl = a.used_tpl; a.best_raw = 0; a.region_path = 0;
            for (int s = 0; s < 2; ++s) { a.region_start[s] = 0; a.region_len[s] = 0; a.bc_idx[s] = -1; a.bc_raw[s] = 0; }
        } else a = recs[i];
        if (bcres) {                                     // (constant indices: a run-time loop bound puts the record into scratch memory)
            const int2 v0 = bcres[i * nsets_all];
            a.bc_idx[0] = v0.x; a.bc_raw[0] = v0.y;
            if (nsets_all > 1) { const int2 v1 = bcres[i * nsets_all + 1]; a.bc_idx[1] = v1.x; a.bc_raw[1] = v1.y; }
        }
        return a;
    };
    const int nbuckets = k->n_buckets;
    const bool lds_hist = counts != nullptr && nbuckets <= FIN_DYN_BUCKETS;
    if (lds_hist) {
        for (int i = threadIdx.x; i < nbuckets; i += blockDim.x) hist[i] = 0;
        __syncthreads();
    }
    const int nb = k->n_barcode_slots;
    const int nbc = (k->mode == QCAT_MODE_DUAL) ? nb * nb : nb;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n_reads; base += (uint64_t)gridDim.x * 256u) {
      const uint64_t r = base + threadIdx.x;
      if (r < n_reads) {
        EndScan res;
        int trim5 = 0; int64_t trim3 = 0;
        // (a batch uploaded as windows only carries the read's real length separately)
        const int64_t len = true_len ? (int64_t)true_len[r] : (int64_t)(offsets[r + 1] - offsets[r]);
        if (k->ends == QCAT_ENDS_5P) {
            res = dev_make_scan(kp, load(r));
        } else {
            EndScan s5 = dev_make_scan(kp, load(2 * r));
            EndScan s3 = dev_make_scan(kp, load(2 * r + 1));
            trim5 = s5.adapter_end > 0 ? s5.adapter_end : 0;
            trim3 = len;
            if (s3.adapter >= 0 && s3.adapter_end > 0) trim3 -= s3.adapter_end;
            if (!s5.pass) s5 = dev_empty_scan();
            if (!s3.pass) s3 = dev_empty_scan();
            int pick = -1;                            // best of the two, 5' wins ties, score > 0
            if (s5.raw > 0) pick = 0;
            if (s3.raw > 0 && (pick < 0 || (int64_t)s3.raw * s5.den > (int64_t)s5.raw * s3.den)) pick = 1;
            if (pick < 0) res = dev_empty_scan();
            else {
                res = pick == 0 ? s5 : s3;
                if (s5.has && s3.has && s5.conflict_ok && s3.conflict_ok && !dev_same_id(kp, s5, s3)) {
                    res = dev_empty_scan(); res.exit_status = 1002;
                }
            }
            if (trim3 < trim5) trim5 = 0;
        }
        dev_store_result(reinterpret_cast<qcat_result*>(s_out) + threadIdx.x, res, trim5, trim3);
        if (counts) {
            int slot = dev_barcode_bucket(kp, nb, nbc, res.bc0, res.bc1, res.adapter);
            int kslot = nbc + 1 + (res.adapter >= 0 ? k->tpl[res.adapter].kit_slot : k->n_kit_slots);
            if (dev_skipped(k, len, trim5, trim3)) { slot = nbuckets - 1; kslot = -1; }
            if (lds_hist) { atomicAdd(&hist[slot], 1u); if (kslot >= 0) atomicAdd(&hist[kslot], 1u); }
            else { atomicAdd(&counts[slot], 1ull); if (kslot >= 0) atomicAdd(&counts[kslot], 1ull); }
        }
      }
      // 24-byte records at a 24-byte lane stride are six partial writes per line (WRITE_SIZE 5x the payload): the block's
      // results leave the LDS as consecutive dwords instead
      __syncthreads();
      {
          const uint32_t cnt = (uint32_t)(n_reads - base < 256u ? n_reads - base : 256u) * RW;
          uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + base);
          for (uint32_t i = threadIdx.x; i < cnt; i += 256u) dst[i] = s_out[i];
      }
      __syncthreads();
    }
    if (lds_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < nbuckets; i += blockDim.x)
            if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
    }
}

}  // namespace qk

// kernels_generic.inc -- k_scan_generic: the fully general scan of one read end per thread
// (int32 cells, affine gaps, arbitrary 7x7 matrices, templates up to 128, targets up to 64).
// It is the device fall-back for qcat configurations the packed kernels do not cover
// (gap_open != gap_extend, N/X inside barcode targets, X inside templates, ...) and the
// in-library cross-check of the packed path.  Slow by design (one lane per read end, DP rows in
// LDS); never a CPU path.
// Included by qcat_hip.hip.

namespace qk {

constexpr int GEN_THREADS = 64;
constexpr int GEN_NEG = -(1 << 28);

struct DevAlign { int score, end_q, end_r; };

// Semi-global alignment, all end gaps free (SURVEY.md 8a R1).  q = window codes (global, one
// byte per position), t = target codes.  H/F: LDS rows with stride GEN_THREADS.
// query accessors: a packed code window (or a slice of it) / the interior of a read in ASCII
struct WinSeq {
    const uint8_t* p;
    __device__ __forceinline__ int operator()(int i) const { return p[i]; }
};
struct MidSeq {            // read[n:-n] (rev = 0) or its reverse complement (rev = 1), from offset `off`
    const uint8_t* read; int64_t len; int n; int rev; int off;
    __device__ __forceinline__ int operator()(int i) const {
        const int64_t idx = (int64_t)off + i;
        uint32_t c = rev ? dev_code_of(read[len - n - 1 - idx]) : dev_code_of(read[n + idx]);
        if (rev && c < 4) c ^= 1u;
        return (int)c;
    }
};

template <class Q>
__device__ inline DevAlign dev_sg_generic(const Q q, int L,
                                          const uint8_t* __restrict__ t, int M,
                                          int open, int ext, const int8_t* mat, int* H, int* F, bool r1_scalar = false) {
    // (r1_scalar: rule R1 in plain parasail.sg's order, include/qcat_hip.h QCAT_R1_SCALAR -- matters to adapter alignments
    // only: barcode alignments consume the score)
    for (int j = 0; j <= M; ++j) { H[j * GEN_THREADS] = 0; F[j * GEN_THREADS] = GEN_NEG; }
    int cmax = GEN_NEG, ci = 0;
    for (int i = 1; i <= L; ++i) {
        const int qc = q(i - 1);
        int diag = 0, hleft = 0, e = GEN_NEG;
        for (int j = 1; j <= M; ++j) {
            int up = H[j * GEN_THREADS];
            int f = max(F[j * GEN_THREADS] - ext, up - open);
            int ee = max(e - ext, hleft - open);
            int h = max(max(diag + mat[t[j - 1] * 7 + qc], ee), f);
            diag = up;
            H[j * GEN_THREADS] = h; F[j * GEN_THREADS] = f; e = ee; hleft = h;
        }
        if (hleft > cmax) { cmax = hleft; ci = i; }        // first row reaching the column max
    }
    DevAlign a; a.score = GEN_NEG; a.end_q = L - 1; a.end_r = 0;
    for (int j = 1; j <= M; ++j) {
        int v = H[j * GEN_THREADS];
        if (v > a.score) { a.score = v; a.end_r = j - 1; }
    }
    if (cmax > a.score || (cmax == a.score && (a.end_r == M - 1 || r1_scalar))) {
        a.score = cmax; a.end_r = M - 1; a.end_q = ci - 1;
    }
    return a;
}

// ---------------------------------------------------------------------------------------------
// k_sg_align: one semi-global alignment per thread, straight from ASCII -- parasail_sg / parasail_sg_stat as the
// reference's module-level helpers call them (qcat/scanner_base.py:111-117, :168-172, :214-218): score, end_query and
// end_ref under rule R1, and with `with_stats` the number of matches and of alignment columns along one optimal
// path under the rule `with_stats` names (include/qcat_hip.h QCAT_STATS_*: parasail's recalled order diagonal -> F (the
// gap that consumes a query letter) -> E with matches over mapped codes, or round 3's order; the same switch as
// the CPU restatement and the independent scalar DP of the test suite; parity with parasail unpinned for these
// two numbers -- no scanner path consumes them, scanner_base.py:141).  The per-column state lives in a scratch array interleaved by
// thread (coalesced); int32 cells, affine gaps, any 7x7 matrix.
// ---------------------------------------------------------------------------------------------
__device__ inline uint8_t dev_code_of_ascii(uint8_t c) {
    switch (c & 0xDF) {
        case 'A': return QCAT_CODE_A;
        case 'T': return QCAT_CODE_T;
        case 'G': return QCAT_CODE_G;
        case 'C': return QCAT_CODE_C;
        case 'N': return QCAT_CODE_N;
        case 'X': return QCAT_CODE_X;
        default: return QCAT_CODE_OTHER;
    }
}

struct SgMatrix { int8_t m[49]; };

__global__ void __launch_bounds__(GEN_THREADS)
k_sg_align(const uint8_t* __restrict__ q, const uint64_t* __restrict__ qoff, const uint8_t* __restrict__ t,
           const uint64_t* __restrict__ toff, uint32_t n, int open, int ext, SgMatrix mat, int with_stats_and_rule,
           int32_t* __restrict__ scratch /* 6 * (MAX_TLEN + 1) * n_threads */, qcat_alignment* __restrict__ out) {
    const int with_stats = with_stats_and_rule & 0xFF;                     // QCAT_STATS_*
    const bool r1_scalar = (with_stats_and_rule & QCAT_SG_R1_SCALAR) != 0; // rule R1 in plain parasail.sg's order
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (a >= n) return;
    const uint8_t* s1 = q + qoff[a];
    const uint8_t* s2 = t + toff[a];
    const int L = (int)(qoff[a + 1] - qoff[a]), M = (int)(toff[a + 1] - toff[a]);
    qcat_alignment r; r.score = 0; r.end_query = -1; r.end_ref = -1; r.matches = 0; r.length = 0;
    if (L <= 0 || M <= 0 || M > MAX_TLEN) { out[a] = r; return; }
    int32_t* H = scratch + a;
    int32_t* F = H + (size_t)(MAX_TLEN + 1) * stride;
    int32_t* HM = F + (size_t)(MAX_TLEN + 1) * stride;
    int32_t* HL = HM + (size_t)(MAX_TLEN + 1) * stride;
    int32_t* FM = HL + (size_t)(MAX_TLEN + 1) * stride;
    int32_t* FL = FM + (size_t)(MAX_TLEN + 1) * stride;
    for (int j = 0; j <= M; ++j) { H[j * stride] = 0; F[j * stride] = GEN_NEG; if (with_stats) { HM[j * stride] = 0; HL[j * stride] = 0; FM[j * stride] = 0; FL[j * stride] = 0; } }
    int cmax = GEN_NEG, cfirst = 0, cm = 0, cl = 0;
    for (int i = 1; i <= L; ++i) {
        const uint8_t c1 = s1[i - 1];
        const int qc = dev_code_of_ascii(c1);
        int diag = 0, dm = 0, dl = 0, hleft = 0, hlm = 0, hll = 0, e = GEN_NEG, em = 0, el = 0;
        for (int j = 1; j <= M; ++j) {
            const uint8_t c2 = s2[j - 1];
            const int tc = dev_code_of_ascii(c2);
            if (hleft - open > e - ext) { e = hleft - open; em = hlm; el = hll + 1; } else { e = e - ext; el = el + 1; }
            const int up = H[j * stride], fo = F[j * stride];
            int f, fm = 0, fl = 0;
            if (up - open > fo - ext) { f = up - open; if (with_stats) { fm = HM[j * stride]; fl = HL[j * stride] + 1; } }
            else { f = fo - ext; if (with_stats) { fm = FM[j * stride]; fl = FL[j * stride] + 1; } }
            int h = diag + mat.m[tc * 7 + qc];
            // a match: equal mapped codes (X maps to '*' under the five-letter alphabet), or round 3's "same letter"
            const int qm = (with_stats == QCAT_STATS_PARASAIL5 && qc == QCAT_CODE_X) ? QCAT_CODE_OTHER : qc;
            const int tm = (with_stats == QCAT_STATS_PARASAIL5 && tc == QCAT_CODE_X) ? QCAT_CODE_OTHER : tc;
            const bool same = with_stats == QCAT_STATS_ROUND3 ? (qc == tc && (c1 | 0x20) == (c2 | 0x20)) : qm == tm;
            int hm = dm + (same ? 1 : 0), hl = dl + 1;
            if (with_stats == QCAT_STATS_ROUND3) {                      // diagonal, E, F
                if (e > h) { h = e; hm = em; hl = el; }
                if (f > h) { h = f; hm = fm; hl = fl; }
            } else {                                                    // diagonal, F, E
                if (f > h) { h = f; hm = fm; hl = fl; }
                if (e > h) { h = e; hm = em; hl = el; }
            }
            diag = up;
            if (with_stats) { dm = HM[j * stride]; dl = HL[j * stride]; HM[j * stride] = hm; HL[j * stride] = hl; FM[j * stride] = fm; FL[j * stride] = fl; }
            H[j * stride] = h; F[j * stride] = f;
            hleft = h; hlm = hm; hll = hl;
        }
        if (hleft > cmax) { cmax = hleft; cfirst = i; cm = hlm; cl = hll; }
    }
    int score = GEN_NEG, end_q = L - 1, end_r = 0, mm = 0, ll = 0;
    for (int j = 1; j <= M; ++j) {
        const int v = H[j * stride];
        if (v > score) { score = v; end_r = j - 1; if (with_stats) { mm = HM[j * stride]; ll = HL[j * stride]; } }
    }
    if (cmax > score || (cmax == score && (end_r == M - 1 || r1_scalar))) { score = cmax; end_r = M - 1; end_q = cfirst - 1; mm = cm; ll = cl; }
    r.score = score; r.end_query = end_q; r.end_ref = end_r; r.matches = with_stats ? mm : 0; r.length = with_stats ? ll : 0;
    out[a] = r;
}

// extract_barcode_region with Python slice semantics (qcat/scanner_base.py:29-60, R4)
__device__ __host__ inline void dev_region(int tpl_len, int bc_end, int bc_len, int ext, int stop, int L,
                                           int* start_out, int* len_out) {
    int end_ref = stop - (tpl_len - bc_end) + 1;
    int start_ref = end_ref - bc_len;
    start_ref -= (ext < start_ref) ? ext : start_ref;
    end_ref += (ext < L - end_ref) ? ext : (L - end_ref);
    int a = start_ref, b = end_ref + 1;
    if (a < 0) { a += L; if (a < 0) a = 0; }
    if (b < 0) { b += L; if (b < 0) b = 0; }
    if (a > L) a = L;
    if (b > L) b = L;
    *start_out = a;
    *len_out = b > a ? b - a : 0;
}

__global__ void __launch_bounds__(GEN_THREADS)
k_scan_generic(KitPtrs kp, const uint8_t* __restrict__ win, const int32_t* __restrict__ wlen,
               uint32_t n_ends, EndRec* __restrict__ recs,
               int32_t* __restrict__ dbg_tpl /* [n_ends][2][MAX_T] or null */,
               int16_t* __restrict__ dbg_rows /* [n_ends][2][stride] or null */, uint32_t stride,
               int adapter_only) {
    __shared__ int H[(MAX_TLEN + 1) * GEN_THREADS];
    __shared__ int F[(MAX_TLEN + 1) * GEN_THREADS];
    __shared__ int8_t amat[49], bmat[49];
    const DevKit* k = kp.kit;
    if (threadIdx.x < 49) { amat[threadIdx.x] = k->amat[threadIdx.x]; bmat[threadIdx.x] = k->bmat[threadIdx.x]; }
    __syncthreads();
    uint32_t e = blockIdx.x * GEN_THREADS + threadIdx.x;
    if (e >= n_ends) return;
    int* h = H + threadIdx.x;
    int* f = F + threadIdx.x;
    const uint8_t* w = win + (size_t)e * WIN_STRIDE;
    const int L = wlen[e];

    // find_best_adapter_template (qcat/scanner_base.py:313-359): strict '<' on the normalised
    // score, starting from -1.0; norm_a < norm_b  <=>  raw_a*den_b < raw_b*den_a (den > 0).
    int best = -1, best_end = -1, best_raw = -1, best_den = 100;     // -1.0 == -1*100/100
    if (L > 0) {
        for (int t = 0; t < k->nt; ++t) {
            const DevTpl& p = k->tpl[t];
            DevAlign a = dev_sg_generic(WinSeq{w}, L, kp.codes + p.code_off, p.len, k->gap_open, k->gap_extend, amat, h, f, k->r1_scalar != 0);
            if (dbg_tpl) {
                dbg_tpl[((size_t)e * 2 + 0) * MAX_T + t] = a.score;
                dbg_tpl[((size_t)e * 2 + 1) * MAX_T + t] = a.end_q;
            }
            if ((int64_t)best_raw * p.den < (int64_t)a.score * best_den) {
                best = t; best_end = a.end_q; best_raw = a.score; best_den = p.den;
            }
        }
    }
    EndRec r;
    r.window_len = L; r.best_tpl = best; r.best_end = best_end; r.best_raw = best_raw;
    r.used_tpl = best < 0 ? k->nt - 1 : best;
    const DevTpl& p = k->tpl[r.used_tpl];
    const bool dual = k->mode == QCAT_MODE_DUAL;
    r.region_path = (dual || p.is_double || (best >= 0 && best_raw >= p.region_min_raw)) ? 1 : 0;
    for (int s = 0; s < 2; ++s) { r.region_start[s] = 0; r.region_len[s] = 0; r.bc_idx[s] = -1; r.bc_raw[s] = 0; }
    const int nsets = adapter_only ? 0 : (dual ? 2 : 1);
    for (int s = 0; s < nsets; ++s) {
        if (r.region_path) dev_region(p.len, p.bc_end[s], p.bc_len[s], k->ext, best_end, L, &r.region_start[s], &r.region_len[s]);
        else { r.region_start[s] = 0; r.region_len[s] = L < k->max_align ? L : k->max_align; }
        const DevSet& bs = p.sets[s];
        // find_highest_scoring_barcode (qcat/scanner_base.py:63-141) incl. the `not max_score`
        // replacement quirk (R2)
        int bi = -1, braw = 0;
        if (r.region_len[s] > 0) {
            for (int b = 0; b < bs.n; ++b) {
                DevAlign a = dev_sg_generic(WinSeq{w + r.region_start[s]}, r.region_len[s],
                                            kp.codes + bs.tgt_off + (size_t)b * bs.tlen, bs.tlen, 1, 1, bmat, h, f);
                if (dbg_rows) dbg_rows[((size_t)e * 2 + s) * stride + b] = (int16_t)a.score;
                if (bi < 0 || braw == 0 || braw < a.score) { bi = b; braw = a.score; }
            }
        }
        r.bc_idx[s] = bi; r.bc_raw[s] = braw;
    }
    recs[e] = r;
}

// ---------------------------------------------------------------------------------------------
// k_scan_middle: --detect-middle (qcat/scanner_base.py:479-519, :593-595).  For every read whose
// result names an adapter, scan() the read interior read[n:-n] and, if that stays below 50, its
// reverse complement, with the templates of the called kit; a hit voids the call (exit 997, trims
// kept).  General int32 DP, one thread per read (the interior can be tens of kilobases long); slow
// by design in round 1 -- the option is off by default in the reference.
// ---------------------------------------------------------------------------------------------
// scan() of ONE sequence of any length (qcat/scanner_epi2me.py:33-144, scanner_dual.py:35-146) with the
// templates of kit slot `kit_slot` (-1: every template of the kit): general int32 DP, one thread per
// sequence.  Q(off) is the query accessor shifted by `off` bases.
template <class MakeQ>
__device__ inline EndRec dev_scan_any(const KitPtrs& kp, MakeQ make_q, int m, int kit_slot,
                                      const int8_t* amat, const int8_t* bmat, int* h, int* f) {
    const DevKit* k = kp.kit;
    const int n = k->max_align;
    int best = -1, best_end = -1, best_raw = -1, best_den = 100, last = -1;
    for (int t = 0; t < k->nt; ++t) {
        const DevTpl& p = k->tpl[t];
        if (kit_slot >= 0 && p.kit_slot != kit_slot) continue;
        last = t;
        if (m <= 0) continue;
        DevAlign a = dev_sg_generic(make_q(0), m, kp.codes + p.code_off, p.len,
                                    k->gap_open, k->gap_extend, amat, h, f, k->r1_scalar != 0);
        if ((int64_t)best_raw * p.den < (int64_t)a.score * best_den) { best = t; best_end = a.end_q; best_raw = a.score; best_den = p.den; }
    }
    EndRec r;
    r.window_len = m; r.best_tpl = best; r.best_end = best_end; r.best_raw = best_raw;
    r.used_tpl = best < 0 ? last : best;                     // Python [-1]: the last template of the list
    const DevTpl& p = k->tpl[r.used_tpl];
    const bool dual = k->mode == QCAT_MODE_DUAL;
    r.region_path = (dual || p.is_double || (best >= 0 && best_raw >= p.region_min_raw)) ? 1 : 0;
    const int nsets = dual ? 2 : 1;
    for (int s = 0; s < 2; ++s) { r.region_start[s] = 0; r.region_len[s] = 0; r.bc_idx[s] = -1; r.bc_raw[s] = 0; }
    for (int s = 0; s < nsets; ++s) {
        int start = 0, rl = m < n ? m : n;
        if (r.region_path) dev_region(p.len, p.bc_end[s], p.bc_len[s], k->ext, best_end, m, &start, &rl);
        const DevSet& bs = p.sets[s];
        int bi = -1, braw = 0;
        if (rl > 0) {
            for (int b = 0; b < bs.n; ++b) {
                DevAlign a = dev_sg_generic(make_q(start), rl, kp.codes + bs.tgt_off + (size_t)b * bs.tlen,
                                            bs.tlen, 1, 1, bmat, h, f);
                if (bi < 0 || braw == 0 || braw < a.score) { bi = b; braw = a.score; }
            }
        }
        r.region_start[s] = start; r.region_len[s] = rl; r.bc_idx[s] = bi; r.bc_raw[s] = braw;
    }
    return r;
}

__device__ inline bool dev_middle_strand(const KitPtrs& kp, const uint8_t* read, int64_t len, int m, int rev,
                                         int kit_slot, const int8_t* amat, const int8_t* bmat, int* h, int* f) {
    const DevKit* k = kp.kit;
    const int n = k->max_align;
    const EndRec r = dev_scan_any(kp, [&](int off) { return MidSeq{read, len, n, rev, off}; }, m, kit_slot, amat, bmat, h, f);
    const DevTpl& p = k->tpl[r.used_tpl];
    const int nsets = k->mode == QCAT_MODE_DUAL ? 2 : 1;
    for (int s = 0; s < nsets; ++s)
        if ((r.bc_idx[s] < 0 ? 0 : r.bc_raw[s]) < p.sets[s].min_raw_middle) return false;   // barcode None (scores 0.0) / score < 50 (dual: min of both)
    return true;
}

__global__ void __launch_bounds__(GEN_THREADS)
k_scan_middle(KitPtrs kp, const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets,
              uint32_t n_reads, qcat_result* __restrict__ results, const uint8_t* __restrict__ only) {
    __shared__ int H[(MAX_TLEN + 1) * GEN_THREADS];
    __shared__ int F[(MAX_TLEN + 1) * GEN_THREADS];
    __shared__ int8_t amat[49], bmat[49];
    const DevKit* k = kp.kit;
    if (threadIdx.x < 49) { amat[threadIdx.x] = k->amat[threadIdx.x]; bmat[threadIdx.x] = k->bmat[threadIdx.x]; }
    __syncthreads();
    const uint32_t r = blockIdx.x * GEN_THREADS + threadIdx.x;
    if (r >= n_reads) return;
    if (only && !only[r]) return;                  // the packed interior scan took this read
    qcat_result res = results[r];
    if (res.adapter_idx < 0) return;
    const uint8_t* read = bases + offsets[r];
    const int64_t len = (int64_t)(offsets[r + 1] - offsets[r]);
    int64_t m64 = len - 2 * (int64_t)k->max_align;
    const int m = m64 < 0 ? 0 : (int)m64;
    const int kit_slot = k->tpl[res.adapter_idx].kit_slot;
    int* h = H + threadIdx.x;
    int* f = F + threadIdx.x;
    bool hit = dev_middle_strand(kp, read, len, m, 0, kit_slot, amat, bmat, h, f);
    if (!hit) hit = dev_middle_strand(kp, read, len, m, 1, kit_slot, amat, bmat, h, f);
    if (hit) {
        res.barcode_idx = -1; res.barcode2_idx = -1; res.adapter_idx = -1; res.exit_status = 997;
        res.adapter_end = 0; res.raw_score = 0; res.score_den = 1;
        results[r] = res;
    }
}

// ---------------------------------------------------------------------------------------------
// k_scan_sequences: BarcodeScanner.scan() of whole sequences of any length (the boundary's third
// method, qcat/scanner_base.py:466-477; called on read interiors by scan_middle, :479-519, and on
// arbitrary sequences by qcat/eval_full.py:199-203).  One record per sequence, as scan() returns it:
// no thresholds, no trims.  General int32 DP, one thread per sequence.
// ---------------------------------------------------------------------------------------------
struct AsciiSeq {
    const uint8_t* p;
    __device__ __forceinline__ int operator()(int i) const { return (int)dev_code_of(p[i]); }
};

__global__ void __launch_bounds__(GEN_THREADS)
k_scan_sequences(KitPtrs kp, const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets,
                 uint32_t n_seqs, qcat_result* __restrict__ results) {
    __shared__ int H[(MAX_TLEN + 1) * GEN_THREADS];
    __shared__ int F[(MAX_TLEN + 1) * GEN_THREADS];
    __shared__ int8_t amat[49], bmat[49];
    const DevKit* k = kp.kit;
    if (threadIdx.x < 49) { amat[threadIdx.x] = k->amat[threadIdx.x]; bmat[threadIdx.x] = k->bmat[threadIdx.x]; }
    __syncthreads();
    const uint32_t r = blockIdx.x * GEN_THREADS + threadIdx.x;
    if (r >= n_seqs) return;
    const uint8_t* seq = bases + offsets[r];
    const int m = (int)(offsets[r + 1] - offsets[r]);
    EndRec rec;
    if (k->mode == QCAT_MODE_SIMPLE) {                 // scanner_simple.py:41-91: the barcode list against the whole sequence
        const DevSet& bs = k->tpl[0].sets[0];
        rec.window_len = m; rec.best_tpl = -1; rec.used_tpl = 0; rec.best_end = -1; rec.best_raw = -1; rec.region_path = 0;
        for (int s = 0; s < 2; ++s) { rec.region_start[s] = 0; rec.region_len[s] = 0; rec.bc_idx[s] = -1; rec.bc_raw[s] = 0; }
        int bi = -1, braw = 0, bend = -1, blen = 1;
        for (int b = 0; m > 0 && b < bs.n; ++b) {
            // every barcode with its own length, the winners compared by their normalised scores -- as k_scan_simple does
            // (scanner_base.py:108-125; a user FASTA may hold barcodes of unequal length: the padded row ends in QCAT_CODE_PAD)
            const int tl = bs.len_off >= 0 ? kp.ids[bs.len_off + 3 * b] : bs.tlen;
            const DevAlign a = dev_sg_generic(AsciiSeq{seq}, m, kp.codes + bs.tgt_off + (size_t)b * bs.tlen, tl, 1, 1, bmat,
                                              H + threadIdx.x, F + threadIdx.x);
            if (bi < 0 || braw == 0 || braw * tl < a.score * blen) { bi = b; braw = a.score; bend = a.end_q; blen = tl; }
        }
        rec.bc_idx[0] = bi; rec.bc_raw[0] = braw; rec.best_end = bend;
    } else {
        rec = dev_scan_any(kp, [&](int off) { return AsciiSeq{seq + off}; }, m, -1, amat, bmat,
                           H + threadIdx.x, F + threadIdx.x);
    }
    dev_store_result(results + r, dev_make_scan(kp, rec), 0, 0);
}

// ---------------------------------------------------------------------------------------------
// k_scan_simple: BarcodeScannerSimple.scan (qcat/scanner_simple.py:41-91) of one read-end window per
// thread: find_highest_scoring_barcode over the kit's ONE barcode list, no contexts, the WHOLE window as
// the query (scanner_base.py:63-141, rule R2 incl.); the winner's end_query becomes adapter_end.
// General int32 DP: ragged lists, lengths without a width class and matrices outside binary16 (every other simple kit runs
// kernels_simple.inc), and the cross-check of those kernels (QCAT_HIP_NO_SIMPLE_PACKED=1).
// ---------------------------------------------------------------------------------------------
// one read-end window on that routine; the packed simple kernels (kernels_simple.inc) come back here for the read ends whose
// best raw score is exactly 0 (R2 depends on list order there)
__device__ inline EndRec dev_simple_end(KitPtrs kp, const uint8_t* __restrict__ w, int L, uint32_t e, const int8_t* bmat, int* H, int* F,
                                        int16_t* __restrict__ dbg_rows, uint32_t stride) {
    const DevSet& bs = kp.kit->tpl[0].sets[0];
    EndRec r;
    r.window_len = L; r.best_tpl = -1; r.used_tpl = 0; r.best_end = -1; r.best_raw = -1; r.region_path = 0;
    for (int s = 0; s < 2; ++s) { r.region_start[s] = 0; r.region_len[s] = 0; r.bc_idx[s] = -1; r.bc_raw[s] = 0; }
    r.region_len[0] = L;
    int bi = -1, braw = 0, bend = -1, blen = 1;
    if (L > 0) {
        for (int b = 0; b < bs.n; ++b) {
            // every barcode with its own length (scanner_base.py:108-119): a user FASTA may hold barcodes of unequal length
            const int tl = bs.len_off >= 0 ? kp.ids[bs.len_off + 3 * b] : bs.tlen;
            const DevAlign a = dev_sg_generic(WinSeq{w}, L, kp.codes + bs.tgt_off + (size_t)b * bs.tlen, tl, 1, 1, bmat, H, F);
            if (dbg_rows) dbg_rows[((size_t)e * 2) * stride + b] = (int16_t)a.score;
            // `not max_score or max_score < score` on raw * 100.0 / length (:119-125): the normalised scores compared by
            // cross-multiplication (exact: both are correctly rounded quotients of small integers)
            if (bi < 0 || braw == 0 || braw * tl < a.score * blen) { bi = b; braw = a.score; bend = a.end_q; blen = tl; }
        }
    }
    r.bc_idx[0] = bi; r.bc_raw[0] = braw; r.best_end = bend;
    return r;
}

__global__ void __launch_bounds__(GEN_THREADS)
k_scan_simple(KitPtrs kp, const uint8_t* __restrict__ win, const int32_t* __restrict__ wlen, uint32_t n_ends,
              EndRec* __restrict__ recs, int16_t* __restrict__ dbg_rows, uint32_t stride) {
    __shared__ int H[(MAX_TARGET + 1) * GEN_THREADS];
    __shared__ int F[(MAX_TARGET + 1) * GEN_THREADS];
    __shared__ int8_t bmat[49];
    const DevKit* k = kp.kit;
    if (threadIdx.x < 49) bmat[threadIdx.x] = k->bmat[threadIdx.x];
    __syncthreads();
    const uint32_t e = blockIdx.x * GEN_THREADS + threadIdx.x;
    if (e >= n_ends) return;
    recs[e] = dev_simple_end(kp, win + (size_t)e * WIN_STRIDE, wlen[e], e, bmat, H + threadIdx.x, F + threadIdx.x, dbg_rows, stride);
}

}  // namespace qk

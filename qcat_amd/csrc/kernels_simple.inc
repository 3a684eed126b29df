// kernels_simple.inc -- simple mode (BarcodeScannerSimple, qcat/scanner_simple.py:41-91) on packed binary16 lanes:
// every barcode of the kit's ONE list against the WHOLE window of a read end, and -- what the barcode kernels of the
// other modes do not need -- the END POSITION of every alignment under rule R1, because the winner's end_query becomes
// adapter_end.
//
// The DP is barcode_tile_h's (kernels_packed.inc): 128 alignments per wave, two per lane, a wave-uniform target
// right-aligned in W columns, linear gaps 1/1 in the biased form, one v_perm_b32 + v_pk_add_f16 + v_pk_maximum3_f16 per
// column.  On top of it, PER ROW (a row holds 3 W column instructions):
//   * the running maximum of the last column, with the FIRST row that reaches it.  All values are small integers in
//     binary16, so "did the maximum move" is min(new - old, 1), a packed 0/1, and the row index follows with one packed
//     multiply-add: ci += moved * (i - ci).  The maximum starts at -1 (H(i,M) + M >= 0), so row 1 always moves it.
//   * rows past a lane's own window length are PAD rows (kernels_packed.inc): they may not move that lane's index, so
//     their last-column value is replaced by -1 through a packed 0/1 "row is real" factor.
// and PER ALIGNMENT, after the rows:
//   * the last row's maximum over columns 1..M-1 and the value of column M, separately: the row maximum is the larger of
//     the two, and its FIRST column is column M exactly when column M's value is strictly larger than every earlier
//     one -- all rule R1 needs to know about the row side (PAD rows leave prefix maxima in h[], which keeps both facts).
// Rule R1 (the normative statements: dev_sg_generic, dev_sg_wave): the column result replaces the row result when it is
// strictly greater, or equal while the row maximum already sits in column M; end_query = L - 1 for a row result,
// first_row - 1 for a column result.  That is QCAT_R1_STRIPED's order whatever DevKit::r1_scalar says: the simple scan of
// k_scan_simple / dev_simple_end and of the CPU oracle place the end of a BARCODE alignment in that order
// under either rule -- QCAT_R1_SCALAR moves adapter alignments only -- and this path gives their records.
//
// Work unit = (tile of 128 consecutive read ends, chunk of the barcode list): a small batch still spreads over the chip.
// Results: one partial best per (unit, alignment) -- barcode_key extended by the end position (summary mode,
// kernels_packed.inc) -- merged by k_simple_select; device memory per read end does not grow with the list.  An alignment
// whose best raw score is exactly 0 is order dependent (R2) and goes to k_simple_redo, which runs the general routine of
// k_scan_simple in list order.  Debug scans with rows keep (raw, end) of every barcode and take the sequential R2 loop
// (k_simple_select_rows), as k_barcode_select does.
// Kits: one list length with a width class (16..64 letters), max_align <= 150, a binary16 barcode matrix
// (kit_prepare.inc); ragged lists and everything else stay on k_scan_simple.
// Included by qcat_hip.hip.

namespace qk {

// (raw, end_query) of barcode b in a debug scan's per-barcode array
__device__ __forceinline__ u32 simple_pack(int raw, int endq) { return ((u32)raw & 0xFFFFu) | ((u32)(endq + 1) << 16); }

template <int W>
__global__ void __launch_bounds__(64, W <= 40 ? 4 : (W <= 56 ? 3 : 2))
k_simple_packed(KitPtrs kp, const uint8_t* __restrict__ win, const int32_t* __restrict__ wlen, uint32_t n_ends,
                uint32_t n_tiles, int nch, uint2* __restrict__ part /* [tile][chunk][half][lane]: (key, end_query) */,
                u32* __restrict__ full /* debug scans: [tile][barcode][half][lane] simple_pack, or null */) {
    __shared__ uint8_t qbuf[PK_ROWS * 64];
    __shared__ __attribute__((aligned(16))) u32 ltbl[2 * 64];
    const DevKit* __restrict__ k = kp.kit;
    const int lane = threadIdx.x & 63;
    const uint32_t unit = blockIdx.x;
    if (unit >= n_tiles * (uint32_t)nch) return;
    const int chunk = (int)(unit / n_tiles);             // the slow index: neighbouring waves run the same barcodes
    const uint32_t tile = unit % n_tiles;
    const DevSet& bs = k->tpl[0].sets[0];
    const int M = uni(bs.tlen), B = uni(bs.n);
    const int per = (B + nch - 1) / nch;
    const int b0 = chunk * per, b1 = min(B, b0 + per);
    if (b0 >= b1) return;
    const uint32_t e2[2] = {tile * PK_TILE + lane, tile * PK_TILE + 64 + lane};
    const bool valid[2] = {e2[0] < n_ends, e2[1] < n_ends};
    const int L2[2] = {valid[0] ? wlen[e2[0]] : 0, valid[1] ? wlen[e2[1]] : 0};
    const int Lmax = wave_max(max(L2[0], L2[1]));
    if (Lmax == 0) return;                               // nothing but empty windows: k_simple_select needs no partial of theirs
    // the two windows of this lane into the LDS: row i, byte = lo | hi << 4 (codes past a window's length are PAD already)
    const uint4 padv = make_uint4(0x07070707u, 0x07070707u, 0x07070707u, 0x07070707u);
    for (int c = 0; c * 16 <= Lmax && c < WIN_STRIDE / 16; ++c) {
        const uint4 a = valid[0] ? *reinterpret_cast<const uint4*>(win + (size_t)e2[0] * WIN_STRIDE + c * 16) : padv;
        const uint4 b = valid[1] ? *reinterpret_cast<const uint4*>(win + (size_t)e2[1] * WIN_STRIDE + c * 16) : padv;
        const u32 aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const u32 lo = (aw[q >> 2] >> (8 * (q & 3))) & 0xFu;
            const u32 hi = (bw[q >> 2] >> (8 * (q & 3))) & 0xFu;
            if (c * 16 + q < PK_ROWS) qbuf[(c * 16 + q) * 64 + lane] = (uint8_t)(lo | (hi << 4));
        }
    }
    const u32 special = to_vgpr(k->special_barcode);
    const u32* __restrict__ tbase = kp.tables + uni(bs.tbl_off);
    const int start = W - M;
    u32 spv[PADMAX];
#pragma unroll
    for (int j = 0; j < PADMAX; ++j) spv[j] = (j + 1 > start) ? special : 0u;
    const h2 gL2 = h2{(_Float16)(float)L2[0], (_Float16)(float)L2[1]};
    const h2 one = hsplat(1.0f), zero = hsplat(0.0f), mone = hsplat(-1.0f);
    u32 best_key[2] = {0u, 0u};
    int best_end[2] = {-1, -1};
    if (lane < W) ltbl[(b0 & 1) * 64 + lane] = tbase[b0 * W + lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int b = b0; b < b1; ++b) {
        u32 nxt = 0;
        if (b + 1 < b1 && lane < W) nxt = tbase[(b + 1) * W + lane];
        const uint4* __restrict__ lrow = reinterpret_cast<const uint4*>(ltbl + (b & 1) * 64);
        u32 tbl[W];
#pragma unroll
        for (int j = 0; j < (W + 3) / 4; ++j) {
            const uint4 v = lrow[j];
            tbl[4 * j] = v.x;
            if (4 * j + 1 < W) tbl[4 * j + 1] = v.y;
            if (4 * j + 2 < W) tbl[4 * j + 2] = v.z;
            if (4 * j + 3 < W) tbl[4 * j + 3] = v.w;
        }
        int st = start;
        asm volatile("" : "+s"(st));        // per-barcode opaque copy: keeps row 0 / row-scan constants out of LICM
        h2 h[W + 1];
        {
            h2 r = hsplat((float)(-st));                         // row 0: H'(0,j) = max(j - start, 0)
            h[0] = zero;
#pragma unroll
            for (int j = 1; j <= W; ++j) { r = r + one; h[j] = hmax(r, zero); }
        }
        h2 colmax = mone, ci = zero, h0old = zero, fi = zero, rem = gL2;
        u32 qb = qbuf[lane];
        for (int i = 1; i <= Lmax; ++i) {
            const u32 qb_next = qbuf[(i < PK_ROWS ? i : PK_ROWS - 1) * 64 + lane];
            const u32 sel = make_sel_h(qb);
            fi = fi + one;
            const h2 h0new = hmin(fi, gL2);
            h2 left = h0new, carry = h0old;
#define QK_W(J) as_h2(__builtin_amdgcn_perm(QK_POOL(J), tbl[(J) - 1], sel))
#define QK_FENCE()
#define QK_T h2
#define QK_ADD(a, b) ((a) + (b))
#define QK_MAX3(d, u, l) hmax3(d, u, l)
            QK_ROW_COLS_DISPATCH(W)
#undef QK_MAX3
#undef QK_ADD
#undef QK_T
#undef QK_FENCE
#undef QK_W
            // last column of this row, H(i,M) + M, or -1 in a PAD row of the lane (rem = L - i + 1: real while >= 1)
            const h2 real = hmin(hmax(rem, zero), one);
            const h2 c = (left - h0new) * real + (real - one);
            const h2 nm = hmax(colmax, c);
            const h2 moved = hmin(nm - colmax, one);             // 0 / 1: strictly greater than every row before
            ci = ci + moved * (fi - ci);                         // ... then this is the first row that reaches it
            colmax = nm;
            rem = rem - one;
            h0old = h0new;
            qb = qb_next;
        }
        // last row: max over the real columns before M of H(L,j) + L + 1 (padding -> below zero), and column M's own value
        h2 rowpre = zero;
        h2 r = hsplat((float)(-st - 1));
#pragma unroll
        for (int j = 1; j < W; ++j) {
            r = r + one;
            // padding columns (r < 0) get a subtrahend >= 4096, which sinks them below zero
            const h2 rr = (j <= PADMAX) ? hmax(r, r * hsplat(-4096.0f)) : r;
            rowpre = hmax(rowpre, h[j] - rr);
        }
        const h2 rowlast = h[W] - (r + one);
        const float rp[2] = {(float)rowpre.x, (float)rowpre.y}, rl[2] = {(float)rowlast.x, (float)rowlast.y};
        const float cm[2] = {(float)colmax.x, (float)colmax.y}, cf[2] = {(float)ci.x, (float)ci.y};
        u32 out[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int L = L2[hf];
            const int vpre = (int)rp[hf], vlast = (int)rl[hf];
            const int s_row = max(vpre, vlast) - 1 - L, s_col = (int)cm[hf] - M;
            const bool row_at_m = vlast > vpre;                  // the row maximum's first column is column M
            const bool col = s_col > s_row || (s_col == s_row && row_at_m);     // rule R1 in sg_striped_32's order (see the file comment)
            const int score = col ? s_col : s_row;
            const int endq = col ? (int)cf[hf] - 1 : L - 1;
            out[hf] = simple_pack(score, endq);
            const u32 key = barcode_key(score, b);
            if (L > 0 && key > best_key[hf]) { best_key[hf] = key; best_end[hf] = endq; }    // (equal raw: the smaller index keeps it)
        }
        if (full) {
            full[(((size_t)tile * B + b) * 2 + 0) * 64 + lane] = out[0];
            full[(((size_t)tile * B + b) * 2 + 1) * 64 + lane] = out[1];
        }
        if (lane < W) ltbl[((b + 1) & 1) * 64 + lane] = nxt;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (!full) {
        uint2* __restrict__ dst = part + ((size_t)tile * nch + chunk) * 128 + lane;
        dst[0] = make_uint2(best_key[0], (u32)best_end[0]);
        dst[64] = make_uint2(best_key[1], (u32)best_end[1]);
    }
}

// the record of a simple scan's read end as k_scan_simple leaves it
__device__ __forceinline__ EndRec simple_rec(int L, int bi, int braw, int bend) {
    EndRec r;
    r.window_len = L; r.best_tpl = -1; r.used_tpl = 0; r.best_end = bend; r.best_raw = -1; r.region_path = 0;
    for (int s = 0; s < 2; ++s) { r.region_start[s] = 0; r.region_len[s] = 0; r.bc_idx[s] = -1; r.bc_raw[s] = 0; }
    r.region_len[0] = L; r.bc_idx[0] = bi; r.bc_raw[0] = braw;
    return r;
}

// k_simple_select: per read end the maximum key over its tile's units.  The running arg-max of the reference (R2) is
// the plain maximum with the first index among equals unless the largest raw score is exactly 0 (kernels_packed.inc,
// "Summary mode"); those read ends are queued for k_simple_redo.  A list of one length: raw scores order as the
// normalised ones do.
__global__ void __launch_bounds__(256)
k_simple_select(const int32_t* __restrict__ wlen, uint32_t n_ends, int nch, const uint2* __restrict__ part,
                EndRec* __restrict__ recs, u32* __restrict__ redo /* [0]: count, [1..]: read ends */) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ends) return;
    const int L = wlen[e];
    if (L <= 0) { recs[e] = simple_rec(L, -1, 0, -1); return; }
    const uint2* __restrict__ src = part + (size_t)(e / PK_TILE) * nch * 128 + (e % PK_TILE);
    uint2 best = make_uint2(0u, 0u);
    for (int c = 0; c < nch; ++c) {
        const uint2 v = src[(size_t)c * 128];
        if (v.x > best.x) best = v;
    }
    const int raw = (int)(best.x >> 16) - 32768;
    if (raw == 0) { redo[1 + atomicAdd(redo, 1u)] = e; return; }
    recs[e] = simple_rec(L, 1023 - (int)(best.x & 0x3FFu), raw, (int)best.y);
}

// k_simple_select_rows: a debug scan's sequential arg-max over every barcode's (raw, end) in list order, R2 included
__global__ void __launch_bounds__(256)
k_simple_select_rows(const DevKit* __restrict__ k, const int32_t* __restrict__ wlen, uint32_t n_ends, const u32* __restrict__ full,
                     EndRec* __restrict__ recs, int16_t* __restrict__ dbg_rows, uint32_t stride) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ends) return;
    const int L = wlen[e], B = k->tpl[0].sets[0].n;
    int bi = -1, braw = 0, bend = -1;
    if (L > 0) {
        const u32* __restrict__ src = full + (size_t)(e / PK_TILE) * B * 128 + (e % PK_TILE);
        for (int b = 0; b < B; ++b) {
            const u32 v = src[(size_t)b * 128];
            const int raw = (int)(int16_t)(v & 0xFFFFu);
            dbg_rows[((size_t)e * 2) * stride + b] = (int16_t)raw;
            if (bi < 0 || braw == 0 || braw < raw) { bi = b; braw = raw; bend = (int)(v >> 16) - 1; }
        }
    }
    recs[e] = simple_rec(L, bi, braw, bend);
}

// k_simple_redo: the queued read ends (best raw score exactly 0) on the general routine, one thread each, in list order
__global__ void __launch_bounds__(GEN_THREADS)
k_simple_redo(KitPtrs kp, const uint8_t* __restrict__ win, const int32_t* __restrict__ wlen, EndRec* __restrict__ recs,
              const u32* __restrict__ redo) {
    __shared__ int H[(MAX_TARGET + 1) * GEN_THREADS];
    __shared__ int F[(MAX_TARGET + 1) * GEN_THREADS];
    __shared__ int8_t bmat[49];
    if (threadIdx.x < 49) bmat[threadIdx.x] = kp.kit->bmat[threadIdx.x];
    __syncthreads();
    const u32 n = redo[0];
    for (u32 i = blockIdx.x * GEN_THREADS + threadIdx.x; i < n; i += gridDim.x * GEN_THREADS) {
        const u32 e = redo[1 + i];
        recs[e] = dev_simple_end(kp, win + (size_t)e * WIN_STRIDE, wlen[e], e, bmat, H + threadIdx.x, F + threadIdx.x, nullptr, 0);
    }
}

}  // namespace qk

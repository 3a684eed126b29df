// kernels_middle.inc -- packed --detect-middle (qcat/scanner_base.py:479-519, :593-595).
//
// For every read whose result names an adapter the reference scan()s the read INTERIOR
// read[n:-n] (n = max_align_length) and, if that stays below 50, its reverse complement, with the
// templates of the called kit; a hit voids the call (exit 997, trims kept).  The interior can be
// tens of kilobases long, so this is the one read-length-dependent alignment of the path.
//
// Packed form ("M-end" = one strand of one read's interior):
//   k_mid_count / k_mid_offsets / k_mid_scatter   counting sort of the M-ends by (kit slot, length
//                        class of 64 rows); every class is padded to whole tiles of 128, so a tile
//                        has ONE kit (wave-uniform templates) and lengths within 64 rows;
//   k_adapter_middle<M, Cols>   the static-letter adapter chain over an arbitrarily long query:
//                        the rows are staged from the read 152 at a time straight into LDS (nibble
//                        codes, strand-aware), the biased DP row is RE-BASED by g*152 at every block
//                        boundary so the binary16 values stay exact small integers, and the
//                        block-local end-position keys are merged into an absolute (value, row);
//   k_adapter_finish     (shared) path choice + barcode regions of the interior;
//   k_mid_gather         tile images of the barcode regions, read from the interior;
//   barcode kernels + k_barcode_select   (shared, kernels_packed.inc / kernels_static.inc);
//   k_mid_finalize       hit on either strand -> exit 997.
// Both strands are always computed: the reference evaluates the reverse strand only when the
// forward one fails, which gives the same "hit on either" answer.
// Reads whose interior is longer than 16 384 nt, and kits with a template that has no generated
// static-letter kernel, keep the general int32 kernel k_scan_middle.
// Included by qcat_hip.hip after kernels_static.inc; the host side -- scratch and launch sequence -- is middle_host.inc.

namespace qk {

constexpr int MID_CLASS_ROWS = 64;
constexpr int MID_CLASSES = 256;                    // interiors up to 16 384 nt on the packed path
constexpr int MID_MAX_KITS = 16;
constexpr int MID_BINS = MID_MAX_KITS * MID_CLASSES;

struct MidTables {
    uint32_t hist[MID_BINS];                        // M-ends per (kit slot, length class)
    uint32_t cursor[MID_BINS];
    uint32_t bin_slot_start[MID_BINS + 1];          // first slot of each bin (multiples of 128)
};

__device__ __forceinline__ bool dev_mid_eligible(const DevKit* k, const uint64_t* offsets, const qcat_result* results,
                                                 uint32_t r, int* m_out, int* bin_out, bool* generic) {
    *generic = false;
    const qcat_result res = results[r];
    if (res.adapter_idx < 0) return false;
    const int64_t len = (int64_t)(offsets[r + 1] - offsets[r]);
    const int64_t m = len - 2 * (int64_t)k->max_align;
    if (m <= 0) return false;
    const int64_t cls = (m - 1) / MID_CLASS_ROWS;
    const int kit = k->tpl[res.adapter_idx].kit_slot;
    if (cls >= MID_CLASSES || kit >= MID_MAX_KITS) { *generic = true; return false; }
    *m_out = (int)m; *bin_out = kit * MID_CLASSES + (int)cls;
    return true;
}

__global__ void __launch_bounds__(256)
k_mid_count(const DevKit* __restrict__ k, const uint64_t* __restrict__ offsets, uint32_t n_reads,
            const qcat_result* __restrict__ results, MidTables* __restrict__ mt, uint8_t* __restrict__ generic_flag) {
    __shared__ uint32_t h[MID_BINS];
    for (int i = threadIdx.x; i < MID_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) {
        int m, bin; bool gen;
        const bool ok = dev_mid_eligible(k, offsets, results, r, &m, &bin, &gen);
        generic_flag[r] = gen ? 1 : 0;
        if (ok) atomicAdd(&h[bin], 2u);                  // two strands
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MID_BINS; i += blockDim.x) if (h[i]) atomicAdd(&mt->hist[i], h[i]);
}

// one block of 1024 threads, four bins each: bin starts with every bin padded to whole tiles
__global__ void __launch_bounds__(1024)
k_mid_offsets(MidTables* __restrict__ mt) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { c[q] = (mt->hist[4 * t + q] + PK_TILE - 1) / PK_TILE * PK_TILE; sum += c[q]; }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t base = part[t] - sum;
#pragma unroll
    for (int q = 0; q < 4; ++q) { mt->bin_slot_start[4 * t + q] = base; mt->cursor[4 * t + q] = base; base += c[q]; }
    if (t == 1023) mt->bin_slot_start[MID_BINS] = base;
}

constexpr int MID_SCAT = 4;
__global__ void __launch_bounds__(256)
k_mid_scatter(const DevKit* __restrict__ k, const uint64_t* __restrict__ offsets, uint32_t n_reads,
              const qcat_result* __restrict__ results, MidTables* __restrict__ mt,
              uint32_t* __restrict__ msorted, int32_t* __restrict__ mlen, int32_t* __restrict__ mfallback,
              uint32_t* __restrict__ mslot) {
    __shared__ uint32_t cnt[MID_BINS], basep[MID_BINS];
    for (int i = threadIdx.x; i < MID_BINS; i += blockDim.x) cnt[i] = 0;
    __syncthreads();
    const uint32_t blk0 = blockIdx.x * 256u * MID_SCAT;
    int key[MID_SCAT], mm[MID_SCAT]; uint32_t rank[MID_SCAT];
#pragma unroll
    for (int it = 0; it < MID_SCAT; ++it) {
        const uint32_t r = blk0 + it * 256u + threadIdx.x;
        key[it] = -1; rank[it] = 0; mm[it] = 0;
        if (r < n_reads) {
            int m, bin; bool gen;
            if (dev_mid_eligible(k, offsets, results, r, &m, &bin, &gen)) { key[it] = bin; mm[it] = m; rank[it] = atomicAdd(&cnt[bin], 2u); }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MID_BINS; i += blockDim.x) if (cnt[i]) basep[i] = atomicAdd(&mt->cursor[i], cnt[i]);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MID_SCAT; ++it) {
        if (key[it] < 0) continue;
        const uint32_t r = blk0 + it * 256u + threadIdx.x;
        const uint32_t slot = basep[key[it]] + rank[it];
        const int kit = key[it] / MID_CLASSES;
        int last = 0;                                   // Python's [-1] of the kit's template list (best index -1)
        for (int t = 0; t < k->nt; ++t) if (k->tpl[t].kit_slot == kit) last = t;
        msorted[slot] = 2u * r; msorted[slot + 1] = 2u * r + 1u;
        mlen[slot] = mm[it]; mlen[slot + 1] = mm[it];
        mfallback[slot] = last; mfallback[slot + 1] = last;
        mslot[r] = slot;
    }
}

struct MiddleAdapterArgs {
    KitPtrs kp;
    const uint8_t* bases;
    const uint64_t* offsets;
    const uint32_t* msorted;
    const int32_t* mlen;
    const MidTables* mt;
    AdapterBest* bests;          // this template's slice, indexed by slot
    int tpl;
    const uint8_t* need128;      // per tile of 128 slots: 1 = this kernel's (an interior with a letter outside A, C, G, T, a tile the bit-sliced
                                 // interior scan did not take: kernels_abs_mid.inc); null: every tile
};

// parameter block of the bit-sliced interior adapter scan (kernels_abs_mid.inc; launched through abs_mid_kernels.hip).
// A "big tile" = 2048 consecutive slots of the sorted M-ends = sixteen tiles of 128.
constexpr int ABSM_C2_SLACK = 1040;                // dwords addressable before / after the packed batch (c2): a row block of an alignment that
                                                   // has not started points up to 16 384 + 31 bases outside its interior
struct AbsMidArgs {
    const uint8_t* bases;
    const uint64_t* offsets;
    const uint32_t* msorted;
    const int32_t* mlen;
    const MidTables* mt;
    int32_t max_align;
    uint32_t n_tiles;            // big tiles
    uint32_t slot_cap;           // slots of a template's slice of `bests` (a multiple of 128)
    int32_t nt;                  // templates of the kit bundle: slices of `bests`
    uint32_t kit_mask;           // kit slots whose templates all have a two-stage plan
    int32_t* t_rows;             // per big tile: rows = its longest interior (0: not on this path)
    int32_t* t_pz;               // ... rows of its padding zone = longest - shortest interior
    int32_t* t_kit;              // ... kit slot (-1: mixed or no plan, -2: no room in `planes`)
    uint32_t* t_off;             // ... its first row in `planes` / `ns`
    uint32_t* nonempty;          // [big tile][64]: slots that hold an M-end
    uint32_t* invalid;           // [big tile][64]: ... whose interior has a letter outside A, C, G, T
    uint8_t* need128;            // [slot_cap / 128]
    uint32_t* c2;                // the whole batch at two bits per base (dword j = bases 16 j .. 16 j + 15 of `bases`; ABSM_C2_SLACK dwords
                                 // are addressable on either side); k_absmid_codes
    uint8_t* rspec;              // [read]: a letter outside A, C, G, T inside the read's interior
    uint4* sinfo;                // [slot]: x, y = (base index of the M-end's position 0) << 1 | strand -- position p of strand 0 is base
                                 // index + p, of strand 1 base index - p, complemented; z = the interior's length (0: no M-end here);
                                 // w = 1: a letter outside A, C, G, T inside it.  One 16-byte load per reader (the plane kernel is
                                 // bound by the NUMBER of its load instructions: 72 cycles of a CU each)
    uint64_t n_bases;
    uint32_t n_reads;
    uint2* planes;               // [row][64]: letter planes (c1, c0), front-padded to the tile's rows
    uint32_t* ns;                // [row][64]: alignments that have not started at this row (rows of the padding zone only)
    uint32_t row_cap;            // rows `planes` / `ns` hold
    AdapterBest* bests;          // k_absmid_tiles: all slices; k_adapter_mid: the template's slice
    int32_t tpl, den, kit_slot;  // k_adapter_mid: kit template index, its denominator, its kit slot
    uint32_t* cursor;            // next big tile (zeroed before the launch)
    int32_t prio;
    int32_t r1_scalar;           // DevKit::r1_scalar: rule R1 in plain parasail.sg's order (abs_decide)
};

template <int M, class Cols>
__device__ __forceinline__ void adapter_middle_body(const MiddleAdapterArgs& a) {
    __shared__ uint8_t qbuf[PK_ROWS * 64];
    __shared__ uint16_t slow_tbl[5 * 16];
    const DevKit* __restrict__ k = a.kp.kit;
    const int lane = threadIdx.x & 63;
    const uint32_t n_slots = a.mt->bin_slot_start[MID_BINS];
    const uint32_t base = blockIdx.x * PK_TILE;
    const uint32_t s2[2] = {base + lane, base + 64 + lane};
    if (a.need128 && !uni((int)a.need128[blockIdx.x])) return;      // the bit-sliced interior scan has written this tile's results
    if (base >= n_slots) {                              // capacity beyond the last class: no M-end here
        AdapterBest none; none.raw = -1; none.den = 100; none.end = -1; none.tpl = -1;
        a.bests[s2[0]] = none; a.bests[s2[1]] = none;
        return;
    }
    int blo = 0, bhi = MID_BINS;                       // the bin this tile belongs to (last start <= base)
    while (bhi - blo > 1) { const int mid = (blo + bhi) >> 1; if (a.mt->bin_slot_start[mid] <= base) blo = mid; else bhi = mid; }
    const int kit_slot = uni(blo) / MID_CLASSES;
    const int t = a.tpl;
    if (uni(k->tpl[t].kit_slot) != kit_slot) {          // another kit's tile: this template did not compete
        AdapterBest none; none.raw = -1; none.den = 100; none.end = -1; none.tpl = -1;
        a.bests[s2[0]] = none; a.bests[s2[1]] = none;
        return;
    }
    const int n = uni(k->max_align);
    int L2[2]; int strand[2]; const uint8_t* p0[2]; const uint8_t* pend[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const uint32_t me = a.msorted[s2[hf]];
        L2[hf] = a.mlen[s2[hf]];
        strand[hf] = 0; p0[hf] = a.bases; pend[hf] = a.bases;
        if (L2[hf] > 0) {
            const uint32_t r = me >> 1;
            strand[hf] = (int)(me & 1u);
            p0[hf] = a.bases + a.offsets[r] + n;
            pend[hf] = a.bases + a.offsets[r + 1] - n;
        }
    }
    if (lane < 5 * 16 / 2) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = lane * 2 + q, x = idx >> 4, nb = idx & 15;
            const int code = nb < 4 ? nb : (nb == 8 ? QCAT_CODE_N : (nb == 9 ? QCAT_CODE_X : (nb == 10 ? QCAT_CODE_OTHER : QCAT_CODE_PAD)));
            slow_tbl[idx] = k->adapter_w16[x * 8 + code];
        }
    }
    const int Lmax = wave_max(max(L2[0], L2[1]));
    const int g = uni(k->gap_open);
    const int den = uni(k->tpl[t].den);
    u32 plo[5], phi[5];
#pragma unroll
    for (int x = 0; x < 5; ++x) { plo[x] = to_vgpr(k->adapter_pool_lo[x]); phi[x] = to_vgpr(k->adapter_pool_hi[x]); }
    const u32 sel_klo = to_vgpr(QS_SEL_KEY_LO), sel_khi = to_vgpr(QS_SEL_KEY_HI);
    const h2 zero = hsplat(0.0f);
    const h2 g2 = as_h2(opaque_v(as_u32(hsplat((float)g))));
    const h2 rebase = hsplat((float)(g * PK_ROWS));

    h2 h[M + 1];
    {
        h2 r = as_h2(opaque_v(0u));                              // row 0: H'(0,j) = g*j
        h[0] = r;
#pragma unroll
        for (int j = 1; j <= M; ++j) { r = r + g2; h[j] = r; }
    }
    int cval[2] = {-1, -1}, cidx[2] = {0, 0};                    // last-column maximum so far: value, absolute row
    const int nblk = (Lmax + PK_ROWS - 1) / PK_ROWS;
    for (int blk = 0; blk < nblk; ++blk) {
        const int row0 = blk * PK_ROWS;
        const int rows = min(PK_ROWS, Lmax - row0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the previous block's LDS reads are done
        u32 specacc = 0;
        for (int c = 0; c * 16 < rows; ++c) {
            u32 ca[4], cb[4];
            dev_window_codes16(p0[0], pend[0], strand[0], row0 + c * 16, L2[0], ca);
            dev_window_codes16(p0[1], pend[1], strand[1], row0 + c * 16, L2[1], cb);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const u32 na = __builtin_amdgcn_perm(0x0C0A0908u, 0x03020100u, ca[d]);
                const u32 nb = __builtin_amdgcn_perm(0x0C0A0908u, 0x03020100u, cb[d]);
                const u32 both = na | (nb << 4);
                specacc |= (both & 0x88888888u) & ~((both & 0x44444444u) << 1);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (c * 16 + d * 4 + q < PK_ROWS) qbuf[(c * 16 + d * 4 + q) * 64 + lane] = (uint8_t)((both >> (8 * q)) & 0xFFu);
            }
        }
        const bool tile_special = __builtin_amdgcn_ballot_w64(specacc != 0) != 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // block-local coordinates: every biased value is taken relative to g*row0
        const h2 gL2 = h2{(_Float16)(float)(g * (L2[0] - row0)), (_Float16)(float)(g * (L2[1] - row0))};
        if (blk > 0) {
#pragma unroll
            for (int j = 1; j <= M; ++j) h[j] = h[j] - rebase;
        }
        h2 h0old = hmin(zero, gL2), gi = zero;
        u32 ck[2] = {0, 0};
        u32 qb = qbuf[lane];
        for (int i = 1; i <= rows; ++i) {
            const u32 qb_next = qbuf[(i < PK_ROWS ? i : PK_ROWS - 1) * 64 + lane];
            const u32 sel = make_sel2(qb);
            h2 E[5];
#pragma unroll
            for (int x = 0; x < 5; ++x) E[x] = as_h2(__builtin_amdgcn_perm(phi[x], plo[x], sel));
            if (tile_special && __builtin_amdgcn_ballot_w64(((qb & 0x88u) & ~((qb & 0x44u) << 1)) != 0) != 0) {
                const u32 n0 = qb & 15u, n1 = (qb >> 4) & 15u;
#pragma unroll
                for (int x = 0; x < 5; ++x) E[x] = as_h2((u32)slow_tbl[x * 16 + n0] | ((u32)slow_tbl[x * 16 + n1] << 16));
            }
            gi = gi + g2;
            const u32 ci = (u32)(255 - i);
            const h2 h0new = hmin(gi, gL2);
            h2 left = h0new, carry = h0old;
            Cols::run(h, carry, left, E);
            const u32 dcol = as_u32(left - h0new);              // H(i,M) + g*M  (>= 0, independent of the re-basing)
            ck[0] = max(ck[0], __builtin_amdgcn_perm(dcol, ci, sel_klo));
            ck[1] = max(ck[1], __builtin_amdgcn_perm(dcol, ci, sel_khi));
            h0old = h0new;
            qb = qb_next;
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {                         // strict '>' keeps the earliest row over the blocks too
            const int v = (int)(float)__builtin_bit_cast(_Float16, (uint16_t)(ck[hf] >> 8));
            const int il = 255 - (int)(ck[hf] & 255u);
            if (v > cval[hf]) { cval[hf] = v; cidx[hf] = row0 + il; }
        }
    }
    // last-row scan in the last block's coordinates.  A lane that ended up to 63 rows before the
    // tile's longest read carries values down to about -g*(M + 62); OFF keeps the keys positive.
    const int rebased = g * PK_ROWS * (nblk > 0 ? nblk - 1 : 0);
    const int OFF = g * (MAX_TLEN + MID_CLASS_ROWS);
    u32 rk[2] = {0, 0};
    {
        h2 r = hsplat((float)(-1 - OFF));
        r = as_h2(opaque_v(as_u32(r)));
        u32 cj = to_vgpr(255u);
#pragma unroll
        for (int j = 1; j <= M; ++j) {
            r = r + g2;
            cj -= 1u;
            const u32 v = as_u32(h[j] - r);                     // H(L,j) + g*L - rebased + 1 + OFF  (> 0)
            rk[0] = max(rk[0], __builtin_amdgcn_perm(v, cj, sel_klo));
            rk[1] = max(rk[1], __builtin_amdgcn_perm(v, cj, sel_khi));
        }
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        AdapterBest best; best.raw = -1; best.den = 100; best.end = -1; best.tpl = -1;
        const int L = L2[hf];
        if (L > 0) {
            const int vr = (int)(float)__builtin_bit_cast(_Float16, (uint16_t)(rk[hf] >> 8)) - 1 - OFF + rebased;
            const int jr = 255 - (int)(rk[hf] & 255u);
            const int s_row = vr - g * L, s_col = cval[hf] - g * M;
            const bool col = s_col > s_row || (s_col == s_row && (jr == M || uni(k->r1_scalar) != 0));   // rule R1 (QCAT_R1_*)
            const int score = col ? s_col : s_row;
            const int endq = col ? cidx[hf] - 1 : L - 1;
            if (best.raw * den < score * best.den) { best.raw = score; best.den = den; best.end = endq; best.tpl = t; }
        }
        a.bests[s2[hf]] = best;
    }
}

template <int M, class Cols>
__global__ void __launch_bounds__(PK_WAVES * 64, QS_ADAPTER_WAVES(M))
k_adapter_middle(MiddleAdapterArgs a) { adapter_middle_body<M, Cols>(a); }

// ---------------------------------------------------------------------------------------------
// k_mid_gather: tile images of the interior's barcode regions (same output as k_job_gather, source =
// the read itself, strand-aware).  One thread per (tile, lane, 16-byte chunk).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_mid_gather(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets, int n,
             const uint32_t* __restrict__ msorted, const EndRec* __restrict__ recs, const int32_t* __restrict__ sorted,
             const JobTables* __restrict__ jt, int nsets, uint8_t* __restrict__ tilebuf, TileMeta* __restrict__ tmeta,
             const BsPlan* __restrict__ taken = nullptr /* the tiles inside its super-tiles have no reader (round 4) */) {
    const uint32_t chunks = WIN_STRIDE / 16;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t chunk = (uint32_t)(gid % chunks);
    const uint64_t tl = gid / chunks;
    const uint32_t lane = (uint32_t)(tl & 63);
    const uint32_t tile = (uint32_t)(tl >> 6);
    if (tile >= jt->group_tile_start[JOB_GROUPS]) return;
    int gidx = 0;
    for (int q = 1; q < JOB_GROUPS; ++q) if (jt->group_tile_start[q] <= tile) gidx = q;
    if (bs_covers(taken, gidx, tile)) return;
    const int set = gidx & 1;
    const int32_t id2[2] = {sorted[(size_t)tile * PK_TILE + lane], sorted[(size_t)tile * PK_TILE + 64 + lane]};
    uint32_t e2[2] = {0, 0};
    int L2[2] = {0, 0};
    const int i0 = (int)chunk * 16;
    uint32_t a[2][4];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a[hf][q] = 0x07070707u;
        if (id2[hf] >= 0) {
            e2[hf] = (uint32_t)id2[hf] / (uint32_t)nsets;
            L2[hf] = recs[e2[hf]].region_len[set];
            const int start = recs[e2[hf]].region_start[set];
            const uint32_t me = msorted[e2[hf]];
            const uint32_t r = me >> 1;
            // positions start + i of the interior: a window of L2 codes beginning `start` into the strand
            const uint8_t* p0 = bases + offsets[r] + n + start;
            const uint8_t* pend = bases + offsets[r + 1] - n - start;
            dev_window_codes16(p0, pend, (int)(me & 1u), i0, L2[hf], a[hf]);
        }
    }
    uint32_t out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = (a[0][q] & 0x0F0F0F0Fu) | ((a[1][q] & 0x0F0F0F0Fu) << 4);
    *reinterpret_cast<uint4*>(tilebuf + ((size_t)tile * 64 + lane) * WIN_STRIDE + chunk * 16) = make_uint4(out[0], out[1], out[2], out[3]);
    if (chunk == 0) {
        TileMeta m; m.e_lo = e2[0]; m.e_hi = e2[1]; m.len2 = (uint32_t)L2[0] | ((uint32_t)L2[1] << 16); m.pad = 0;
        tmeta[(size_t)tile * 64 + lane] = m;
    }
}

// k_mid_windows (round 4): the first max_align codes of every M-end at two bits per code + its flag -- what the bit-sliced
// BARCODE kernels read (kernels_bitslice.inc).  Almost every interior carries no adapter, so its barcode scan takes the
// whole-window path (scanner_epi2me.py:74-82: the first max_align bases of the interior against every barcode): 2 M such jobs
// per 1 M called reads, 3 ms on the binary16 kernels.  flag 2 = plain letters (hot for a job that starts at code 0),
// 1 = a letter outside A, C, G, T, a padding slot or an interior shorter than a window (never hot).
__global__ void __launch_bounds__(256)
k_mid_windows(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets, int n, const uint32_t* __restrict__ msorted,
              uint32_t n_slots, uint32_t* __restrict__ win2, uint8_t* __restrict__ wspec) {
    // sixteen lanes per slot (WIN2_WORDS <= 16 of them carry a chunk of sixteen codes): the chunks' verdicts meet in a
    // four-step exchange among the slot's lanes and one lane stores the flag byte.  (First form: one thread per chunk and an
    // atomicOr of every chunk into the zeroed flag word -- 20 M atomics for a million reads, 1.09 ms of a 7.2 ms step.)
    static_assert(WIN2_WORDS <= 16, "one lane per chunk in a group of sixteen");
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t slot = gid >> 4;
    const uint32_t chunk = (uint32_t)(gid & 15u);
    uint32_t verdict = 0;                                        // 1: not plain, 2: plain, 0: nothing to say
    if (slot < n_slots && chunk < (uint32_t)WIN2_WORDS) {
        const uint32_t me = msorted[slot];
        if (me == 0xFFFFFFFFu) {
            win2[slot * WIN2_WORDS + chunk] = 0;
            verdict = 1;
        } else {
            const uint32_t r = me >> 1;
            const uint64_t beg = offsets[r] + (uint64_t)n, end = offsets[r + 1] - (uint64_t)n;
            const int64_t m = (int64_t)end - (int64_t)beg;
            const int L = m < (int64_t)n ? (int)(m < 0 ? 0 : m) : n;
            uint32_t out[4];
            dev_window_codes16(bases + beg, bases + end, (int)(me & 1u), (int)chunk * 16, L, out);
            uint32_t p = 0, spec = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t t = out[q] & 0x03030303u;
                t = (t | (t >> 6)) & 0x000F000Fu;
                t = (t | (t >> 12)) & 0xFFu;
                p |= t << (8 * q);
                const uint32_t c = out[q] & 0x07070707u;
                spec |= (c >> 2) & ~(c & (c >> 1) & (c >> 2)) & 0x01010101u;       // codes 4, 5, 6: N, X, other (7 is the padding past the window)
            }
            win2[slot * WIN2_WORDS + chunk] = p;
            // a mixture of verdicts reads as "not plain"; an interior shorter than a window is never hot
            if ((int)chunk * 16 < n) verdict = (spec || m < (int64_t)n) ? 1u : 2u;
        }
    }
    verdict |= (uint32_t)__shfl_xor((int)verdict, 1, 16);
    verdict |= (uint32_t)__shfl_xor((int)verdict, 2, 16);
    verdict |= (uint32_t)__shfl_xor((int)verdict, 4, 16);
    verdict |= (uint32_t)__shfl_xor((int)verdict, 8, 16);
    if (chunk == 0 && slot < n_slots) wspec[slot] = (uint8_t)verdict;
}

// k_mid_finalize: a read is voided (997) when the interior scan of either strand found a barcode
// with score >= 50 in every set (scanner_base.py:489-519: barcode None or score < 50 -> no hit).
__global__ void __launch_bounds__(256)
k_mid_finalize(const DevKit* __restrict__ k, const EndRec* __restrict__ mrecs, const uint32_t* __restrict__ mslot,
               uint32_t n_reads, qcat_result* __restrict__ results, uint8_t* __restrict__ generic_flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t slot = mslot[r];
    const int nsets = k->mode == QCAT_MODE_DUAL ? 2 : 1;
    if (slot == 0xFFFFFFFFu) {
        // no slot and not left to the general kernel: no called adapter, or no interior (read[n:-n] is empty).  The scan of an
        // empty interior finds no barcode, which the reference scores 0.0: a hit only under a threshold of 0 or less
        if (!k->middle_hits_empty || generic_flag[r]) return;
        qcat_result res = results[r];
        if (res.adapter_idx < 0) return;
        res.barcode_idx = -1; res.barcode2_idx = -1; res.adapter_idx = -1; res.exit_status = 997;
        res.adapter_end = 0; res.raw_score = 0; res.score_den = 1;
        results[r] = res;
        return;
    }
    // a barcode region longer than an end window (Python's slice wrap when the adapter ends within the interior's first
    // few bases, qcat/scanner_base.py:29-60, gives interior[0 : L - x]) is beyond the rows the barcode kernels hold:
    // the general kernel, which runs after this one over the flagged reads, decides for that read
    for (int st = 0; st < 2; ++st)
        for (int s = 0; s < nsets; ++s)
            if (mrecs[slot + st].region_len[s] > k->max_align) { generic_flag[r] = 1; return; }
    bool hit = false;
    for (int st = 0; st < 2 && !hit; ++st) {
        const EndRec rec = mrecs[slot + st];
        const DevTpl& p = k->tpl[rec.used_tpl];
        bool ok = true;
        // (barcode None scores 0.0 in the reference: below every positive threshold, not below one of 0 or less)
        for (int s = 0; s < nsets; ++s) ok = ok && (rec.bc_idx[s] >= 0 ? rec.bc_raw[s] : 0) >= p.sets[s].min_raw_middle;
        hit = ok;
    }
    if (hit) {
        qcat_result res = results[r];
        res.barcode_idx = -1; res.barcode2_idx = -1; res.adapter_idx = -1; res.exit_status = 997;
        res.adapter_end = 0; res.raw_score = 0; res.score_den = 1;
        results[r] = res;
    }
}

}  // namespace qk

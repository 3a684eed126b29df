// kernels_abs_mid.inc -- the interior ADAPTER scan of --detect-middle in bit-sliced difference form (round 4).
//
// detect_barcode scans read[n:-n] of every called read and, if that finds nothing, its reverse complement with the templates
// of the called kit (qcat/scanner_base.py:479-519, :593-595); kernels_middle.inc sorts both strands of every such interior
// ("M-ends") by (kit slot, length class of 64 rows) into slots and k_adapter_middle walks them on packed binary16 lanes --
// 3.0 ms of the 6.1 ms step at 1 M reads.  Here the same alignments run on the arithmetic of abs_core.h (24 full-rate
// v_bitop3_b32 per 2048 cells) and on the two-stage plans of abs_generated.inc, over queries of any length:
//
//  * a BIG TILE is 2048 consecutive slots; its row count L is its longest interior, and every other interior is padded at
//    the FRONT by pad = L - len rows.  Semi-global alignment starts from H(0, j) = 0 whatever came before, so an alignment
//    that "has not started" simply keeps the boundary state of row 0: after such a row its difference planes are put back
//    to 2 (abs_hold2, four instructions per letter column and two per N column, only in the rows of the tile's padding zone = L - shortest interior:
//    the slots are sorted by length class, so that zone is a few dozen rows of several hundred), its first real row is the
//    one where the border walk is forced to a new maximum (`first` of abs_border_step, here a per-alignment mask), and its
//    end position is the tile row minus pad.  Every alignment ends in the tile's last row, so the walk along the last row
//    and the decision (abs_decide) are those of the window kernels.
//  * the deficit counters keep their ten planes (H along a border stays within [-2M, 5M] however long the query is); the
//    row index needs 14 planes (interiors up to 16 384 rows, the limit of the length classes): this translation unit is
//    compiled with -DQCAT_ABS_NI=14.
//  * k_absmid_codes packs the whole batch at two bits per base (one streaming pass; a letter outside A, C, G, T inside an
//    interior flags its read); k_absmid_tiles / k_absmid_scan / k_absmid_planes make the tiles' row counts, their places in
//    the plane buffer and the letter planes (a lane = 32 alignments x 16 rows: two dwords of the packed batch per alignment,
//    funnel-shifted to the row block -- the reverse strand read backwards: bit reversal, pair swap, complement = code ^ 1 --
//    and transposed as a 32 x 32 bit matrix in registers; the first form converted the read's bytes in every lane: 0.93 ms
//    at 1 M reads).  An interior with a letter outside A, C, G, T, a tile of two kits or of a kit without plans, and whatever
//    does not fit the plane buffer are flagged per tile of 128 slots for k_adapter_middle, which then skips every other tile.
//
// Included by abs_mid_kernels.hip (a translation unit of its own, namespaces qk_absmid / qabs_mid).

// (after kernels_abs.inc: abs_core.h, abs_generated.inc, abs_setprio)

namespace qk {

constexpr int ABSM_TILE = 2048;
#ifndef QCAT_ABS_R
#define QCAT_ABS_R 6
#endif
constexpr int ABSM_R = QCAT_ABS_R;
constexpr int ABSM_GY = 8;                         // workgroups of k_absmid_planes per big tile
// (ABSM_C2_SLACK, the dwords addressable on either side of the packed batch: kernels_middle.inc, beside AbsMidArgs)

// 16 codes (one per byte) -> two bits per code
__device__ __forceinline__ uint32_t absm_pack2(const uint32_t (&c)[4]) {
    uint32_t p = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t t = c[q] & 0x03030303u;
        t = (t | (t >> 6)) & 0x000F000Fu;
        t = (t | (t >> 12)) & 0xFFu;
        p |= t << (8 * q);
    }
    return p;
}
__device__ __forceinline__ uint32_t absm_special(const uint32_t (&c)[4], int q) {        // byte q of the chunk: a letter outside A, C, G, T (codes 4..7)
    return (c[q >> 2] >> (8 * (q & 3))) & 4u;
}

// two adjacent dwords at a dword-aligned address: one global_load_dwordx2 (global accesses need dword alignment only)
struct __attribute__((packed, aligned(4))) AbsmPair { uint32_t lo, hi; };
__device__ __forceinline__ u32 absm_codes_at(const uint32_t* __restrict__ c2, long long s0) {
    const AbsmPair p = *reinterpret_cast<const AbsmPair*>(c2 + (s0 >> 4));       // (arithmetic shift: floor; the slack covers what lies outside the batch)
    return __builtin_amdgcn_alignbit(p.hi, p.lo, (u32)(s0 & 15) * 2u);
}
// sixteen codes read backwards and complemented: bit reversal (code order reversed, the two bits of a code swapped), the pairs
// swapped back, complement = code ^ 1
__device__ __forceinline__ u32 absm_revcomp16(u32 f) {
    const u32 x = __builtin_bitreverse32(f);
    return (((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1)) ^ 0x55555555u;
}

// ---------------------------------------------------------------------------------------------
// k_absmid_codes: the batch at two bits per base, one thread per 16 bases; rspec[r] = 1 for a read with a letter outside
// A, C, G, T in its interior [n, len - n) (rspec zeroed before the launch).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_absmid_codes(AbsMidArgs a) {
    const uint64_t chunks = (a.n_bases + 15) / 16 + 1;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < chunks; j += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t w[4], c[4];
        if ((reinterpret_cast<uintptr_t>(a.bases) & 15u) == 0) {     // (a batch's bases start 64 bytes into a hipMalloc'ed block: one 16-byte load)
            const uint4 v = *reinterpret_cast<const uint4*>(a.bases + j * 16);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else dev_load16_unaligned(a.bases + j * 16, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = dev_codes_of4(w[q]);
        a.c2[j] = absm_pack2(c);
        if ((c[0] | c[1] | c[2] | c[3]) & 0x04040404u) {
            for (int q = 0; q < 16; ++q) {
                const uint64_t p = j * 16 + (uint64_t)q;
                if (p >= a.n_bases || !absm_special(c, q)) continue;
                uint32_t lo = 0, hi = a.n_reads;                      // the read of base p: offsets[lo] <= p < offsets[lo + 1]
                while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (a.offsets[mid] <= p) lo = mid; else hi = mid; }
                const uint64_t beg = a.offsets[lo], end = a.offsets[lo + 1];
                if (p >= beg + (uint64_t)a.max_align && p + (uint64_t)a.max_align < end) a.rspec[lo] = 1;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_absmid_tiles: one workgroup per big tile -- longest / shortest interior, the slots that hold an M-end, the tile's kit;
// every template's result of every slot starts as "none" (what k_adapter_middle writes for a slot without an M-end and for
// a template of another kit).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_absmid_tiles(AbsMidArgs a) {
    __shared__ int s_max, s_min;
    const uint32_t tile = blockIdx.x, base = tile * ABSM_TILE;
    const uint32_t n_slots = a.mt->bin_slot_start[MID_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { s_max = 0; s_min = 0x7FFFFFFF; }
    __syncthreads();
    int mx = 0, mn = 0x7FFFFFFF;
    AdapterBest none; none.raw = -1; none.den = 100; none.end = -1; none.tpl = -1;
    if (threadIdx.x < ABSM_TILE / PK_TILE) {
        const uint32_t t128 = base / PK_TILE + threadIdx.x;
        if (t128 < a.slot_cap / PK_TILE) a.need128[t128] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ABSM_TILE / 256; ++q) {
        const uint32_t slot = base + (uint32_t)q * 256u + threadIdx.x;
        const int len = slot < n_slots ? a.mlen[slot] : 0;
        bool bad = false;
        uint64_t si = 0;
        if (len > 0) {
            mx = max(mx, len); mn = min(mn, len);
            const uint32_t me = a.msorted[slot];
            const uint32_t r = me >> 1;
            const uint64_t p0 = (me & 1u) ? a.offsets[r + 1] - (uint64_t)a.max_align - 1u : a.offsets[r] + (uint64_t)a.max_align;
            si = (p0 << 1) | (uint64_t)(me & 1u);
            bad = a.rspec[r] != 0;
        }
        if (slot < a.slot_cap) a.sinfo[slot] = make_uint4((uint32_t)si, (uint32_t)(si >> 32), (uint32_t)len, bad ? 1u : 0u);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(len > 0);
        const unsigned long long mb = __builtin_amdgcn_ballot_w64(bad);
        const int pl = (q * 256 + wave * 64) / 32;
        if (lane < 2) {
            a.nonempty[(size_t)tile * 64 + pl + lane] = (uint32_t)(lane ? m >> 32 : m);
            a.invalid[(size_t)tile * 64 + pl + lane] = (uint32_t)(lane ? mb >> 32 : mb);
        }
        if (mb != 0 && lane == 0 && slot < a.slot_cap) a.need128[slot / PK_TILE] = 1;
        if (slot < a.slot_cap)
            for (int t = 0; t < a.nt; ++t) a.bests[(size_t)t * a.slot_cap + slot] = none;
    }
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    if (lane == 0) { atomicMax(&s_max, mx); atomicMin(&s_min, mn); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int kit = -1;
        if (s_max > 0) {
            int k2[2];
            const uint32_t probe[2] = {base, min(base + ABSM_TILE - 1, n_slots - 1)};
            for (int e = 0; e < 2; ++e) {
                int blo = 0, bhi = MID_BINS;                 // the bin of a slot: the last start <= slot
                while (bhi - blo > 1) { const int mid = (blo + bhi) >> 1; if (a.mt->bin_slot_start[mid] <= probe[e]) blo = mid; else bhi = mid; }
                k2[e] = blo / MID_CLASSES;
            }
            if (k2[0] == k2[1] && ((a.kit_mask >> k2[0]) & 1u)) kit = k2[0];
        }
        a.t_rows[tile] = s_max;
        a.t_pz[tile] = s_max > 0 ? s_max - s_min : 0;
        a.t_kit[tile] = kit;
    }
}

// ---------------------------------------------------------------------------------------------
// k_absmid_windows: k_mid_windows (kernels_middle.inc: the first max_align codes of every M-end at two bits per code + its flag,
// what the bit-sliced BARCODE kernels read) from the packed batch: sixteen lanes per slot, two dwords in, one out (the
// original converts the read's bytes: 0.28 ms at 1 M reads).  The flag is conservative here: "plain" (2) needs an interior
// without any letter outside A, C, G, T (rspec), not only a first window without one; such an M-end's barcode jobs then take
// the binary16 kernels, whose tile images k_mid_gather reads from the read itself.  After k_absmid_tiles (sinfo).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_absmid_windows(AbsMidArgs a, uint32_t n_slots_cap, uint32_t* __restrict__ win2, uint8_t* __restrict__ wspec) {
    static_assert(WIN2_WORDS <= 16, "one lane per chunk in a group of sixteen");
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t slot = gid >> 4;
    const uint32_t chunk = (uint32_t)(gid & 15u);
    if (slot >= n_slots_cap) return;
    const uint4 rec = a.sinfo[slot];
    const int m = (int)rec.z, n = a.max_align;
    if (m == 0) {                                                    // no M-end in this slot
        if (chunk < (uint32_t)WIN2_WORDS) win2[slot * WIN2_WORDS + chunk] = 0;
        if (chunk == 0) wspec[slot] = 1;
        return;
    }
    if (chunk < (uint32_t)WIN2_WORDS) {
        const uint64_t si = (uint64_t)rec.x | ((uint64_t)rec.y << 32);
        const bool rev = (si & 1ull) != 0;
        const int pos0 = (int)chunk * 16;
        const long long s0 = rev ? (long long)(si >> 1) - pos0 - 15 : (long long)(si >> 1) + pos0;
        const u32 f = absm_codes_at(a.c2, s0);
        u32 w = rev ? absm_revcomp16(f) : f;
        const int L = m < n ? m : n, keep = L - pos0;              // codes of this chunk inside the window; the rest reads as padding & 3
        if (keep < 16) w |= keep <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (2 * keep);
        win2[slot * WIN2_WORDS + chunk] = w;
    }
    if (chunk == 0) wspec[slot] = (uint8_t)((rec.w || m < n) ? 1 : 2);
}

// k_absmid_scan: one workgroup -- the tiles' first rows in the plane buffer; a tile that does not fit leaves the path
__global__ void __launch_bounds__(1024)
k_absmid_scan(AbsMidArgs a) {
    __shared__ unsigned long long part[1024];
    const int t = threadIdx.x;
    const uint32_t per = (a.n_tiles + 1023u) / 1024u;
    const uint32_t lo = min(a.n_tiles, (uint32_t)t * per), hi = min(a.n_tiles, lo + per);
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) if (a.t_kit[i] >= 0) sum += (unsigned long long)a.t_rows[i];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned long long v = t >= off ? part[t - off] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long at = part[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        const int rows = a.t_rows[i];
        if (a.t_kit[i] >= 0 && at + (unsigned long long)rows <= (unsigned long long)a.row_cap) { a.t_off[i] = (uint32_t)at; at += (unsigned long long)rows; }
        else {
            if (a.t_kit[i] >= 0) { at += (unsigned long long)rows; a.t_kit[i] = -2; }
            a.t_off[i] = 0u;
            if (rows > 0) a.t_rows[i] = -rows;             // (negative: M-ends here, but not on this path)
        }
    }
}

__device__ __forceinline__ void absm_transpose32(u32 (&a)[32]) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int j = 16 >> s;
        const u32 m = s == 0 ? 0x0000FFFFu : (s == 1 ? 0x00FF00FFu : (s == 2 ? 0x0F0F0F0Fu : (s == 3 ? 0x33333333u : 0x55555555u)));
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (k & j) continue;
            const u32 lo = a[k], hi = a[k + j];
            a[k] = (lo & m) | ((hi & m) << j);
            a[k + j] = ((lo >> j) & m) | (hi & ~m);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_absmid_planes: grid (big tiles, ABSM_GY).  A wave takes items of 4 plane lanes x 16 blocks of 16 rows: hardware lane =
// (plane lane, row block); the sixteen lanes of a plane lane read neighbouring 16-byte pieces of the same 32 reads.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_absmid_planes(AbsMidArgs a) {
    const uint32_t tile = blockIdx.x, base = tile * ABSM_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Ls = a.t_rows[tile];
    if (Ls <= 0) {
        // not on the path: every tile of 128 slots that holds an M-end is k_adapter_middle's
        if (Ls < 0 && blockIdx.y == 0 && threadIdx.x < ABSM_TILE / PK_TILE) {
            const uint32_t t128 = base / PK_TILE + threadIdx.x;
            const uint32_t* ne = a.nonempty + (size_t)tile * 64 + threadIdx.x * 4;
            if (t128 < a.slot_cap / PK_TILE && (ne[0] | ne[1] | ne[2] | ne[3]) != 0u) a.need128[t128] = 1;
        }
        return;
    }
    const int L = Ls, pz = a.t_pz[tile];
    const uint32_t off = a.t_off[tile];
    const int nblk = (L + 15) / 16, ngg = (nblk + 15) / 16;
    __shared__ uint4 s_rec[4][128];                                // per wave: the records of the item's four plane lanes = 128 consecutive slots
    for (int item = (int)blockIdx.y * 4 + wave; item < 16 * ngg; item += ABSM_GY * 4) {
        // two coalesced loads per lane instead of one scattered record load per alignment (32 per lane): the kernel is bound by
        // the number of its load instructions.  (The LDS serves a wave's accesses in order: no barrier between the waves needed.)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t slot = base + (uint32_t)(item & 15) * 128u + (uint32_t)(k * 64 + lane);
            s_rec[wave][k * 64 + lane] = slot < a.slot_cap ? a.sinfo[slot] : make_uint4(0u, 0u, 0u, 0u);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const int pl = (item & 15) * 4 + (lane >> 4), g = (item >> 4) * 16 + (lane & 15);
        const int row0 = g * 16;
        if (row0 >= L) continue;
        u32 v[32], nsv[32];
        const bool in_pz = row0 < pz;
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const uint4 rec = s_rec[wave][(lane >> 4) * 32 + b];
            const int len = (int)rec.z;
            u32 w = 0;
            int pad = L;
            if (len > 0) {
                const uint64_t si = (uint64_t)rec.x | ((uint64_t)rec.y << 32);
                const bool rev = (si & 1ull) != 0;
                pad = L - len;
                const int pos0 = row0 - pad;                       // (negative: rows before the alignment's first -- whatever letters)
                // the 16 bases of the forward strand that hold positions pos0 .. pos0 + 15
                const long long s0 = rev ? (long long)(si >> 1) - pos0 - 15 : (long long)(si >> 1) + pos0;
                const u32 f = absm_codes_at(a.c2, s0);
                w = rev ? absm_revcomp16(f) : f;
            }
            v[b] = w;
            const int cnt = min(max(pad - row0, 0), 16);           // rows of this block before the alignment's first
            nsv[b] = (1u << cnt) - 1u;
        }
        absm_transpose32(v);
        uint2* __restrict__ dst = a.planes + ((size_t)off + row0) * 64 + pl;
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (row0 + q < L) dst[(size_t)q * 64] = make_uint2(v[2 * q + 1], v[2 * q]);
        if (in_pz) {
            absm_transpose32(nsv);
            uint32_t* __restrict__ nd = a.ns + ((size_t)off + row0) * 64 + pl;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (row0 + q < pz) nd[(size_t)q * 64] = nsv[q];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_adapter_mid<P>: the two-wave pipeline of a single-template plan P (abs_generated.inc: QAB_T<n>) over the big tiles of the
// template's kit -- kernels_abs.inc's abs_body with a row count per tile, the hold of the padding zone and one more ring
// plane (the not-started mask of the row, which stage 1 needs as well).
// ---------------------------------------------------------------------------------------------
template <class P>
__device__ __forceinline__ void abs_mid_body(const AbsMidArgs& A) {
    using namespace qabs;
    static_assert(P::NT == 1 && P::NH == 1, "single-template plans");
    constexpr int PL = 3 + 4;                                      // planes of a ring row: letters, not-started mask, the hand-over set
    constexpr int LR_WORDS = 2 * ABS_NF + 1;
    static_assert(LR_WORDS <= ABSM_R * PL, "the last-row hand-over must fit a ring buffer");
    __shared__ u32 ring[2][ABSM_R * PL * 64];
    __shared__ int s_item[2][2];                                   // [step parity]: tile (-1: the end), block
    const int lane = threadIdx.x & 63, wave = uni((int)(threadIdx.x >> 6));

    if (wave == 0) {
        // ---- stage 0 ---------------------------------------------------------------------------------------
        u32 h[P::NC0][4];
        int tile = -1, blk = 0, L = 0, NB = 0, pz = 0;
        constexpr int ABS_PF = 3;
        uint2 pf[ABS_PF];
        u32 pn[ABS_PF];
        const uint2* __restrict__ src = A.planes + lane;
        const uint32_t* __restrict__ nsrc = A.ns + lane;
        for (int step = 0;; ++step) {
            const int buf = step & 1;
            if (tile < 0 || blk > NB) {                            // next tile of this template's kit
                for (;;) {
                    u32 t = 0;
                    if (lane == 0) t = atomicAdd(A.cursor, 1u);
                    t = (u32)uni((int)t);
                    if (t >= A.n_tiles) { tile = -1; break; }
                    if (uni(A.t_rows[t]) > 0 && uni(A.t_kit[t]) == A.kit_slot) { tile = (int)t; break; }
                }
                blk = 0;
                if (tile >= 0) {
                    L = uni(A.t_rows[tile]); pz = uni(A.t_pz[tile]);
                    NB = (L + ABSM_R - 1) / ABSM_R;
                    abs_set2_cols<P, 0>(h);
                    const size_t off = (size_t)(uint32_t)uni((int)A.t_off[tile]);
                    src = A.planes + off * 64 + lane;
                    nsrc = A.ns + off * 64 + lane;
#pragma unroll
                    for (int r = 0; r < ABS_PF; ++r) {
                        pf[r] = src[(size_t)min(r, L - 1) * 64];
                        pn[r] = r < pz ? nsrc[(size_t)r * 64] : 0u;
                    }
                }
            }
            if (lane == 0) { s_item[buf][0] = tile; s_item[buf][1] = blk; }
            if (tile < 0) { __syncthreads(); __syncthreads(); break; }   // stage 1 reads the end mark in the next step
            u32* __restrict__ rb = ring[buf];
            if (blk < NB) {
#pragma unroll 1
                for (int r = 0; r < ABSM_R; ++r) {
                    const int i = blk * ABSM_R + r;
                    if (i < L) {
                        abs_setprio(A.prio, i, (int)blockIdx.x);
                        const uint2 c = pf[0];
                        const u32 nsm = pn[0];
#pragma unroll
                        for (int q = 0; q + 1 < ABS_PF; ++q) { pf[q] = pf[q + 1]; pn[q] = pn[q + 1]; }
                        pf[ABS_PF - 1] = src[(size_t)min(i + ABS_PF, L - 1) * 64];
                        pn[ABS_PF - 1] = i + ABS_PF < pz ? nsrc[(size_t)(i + ABS_PF) * 64] : 0u;
                        u32 nq[4], ho[1][4];
                        abs_neq_masks(c.x, c.y, nq);
                        P::row0(nq, h, ho);
                        if (i < pz) {                              // (wave-uniform: the rows in which some alignment of the tile has not started)
                            abs_hold2_cols<P, 0>(h, nsm);
                            abs_hold2(ho[0], nsm);
                        }
                        u32* __restrict__ row = rb + r * PL * 64 + lane;
                        row[0] = c.x; row[64] = c.y; row[2 * 64] = nsm;
#pragma unroll
                        for (int p = 0; p < 4; ++p) row[(3 + p) * 64] = ho[0][p];
                    }
                }
            } else {
                AbsLastRow lo[1];
                P::last0(h, lo);
                u32* __restrict__ w = rb + lane;
#pragma unroll
                for (int q = 0; q < ABS_NF; ++q) { w[q * 64] = lo[0].Fr[q]; w[(ABS_NF + q) * 64] = lo[0].sum[q]; }
                w[2 * ABS_NF * 64] = lo[0].newmax;
            }
            ++blk;
            __syncthreads();
        }
    } else {
        // ---- stage 1 ---------------------------------------------------------------------------------------
        u32 h[P::NC1][4];
        AbsBorder bd[1];
        u32 prev_ns = 0xFFFFFFFFu;
        int L = 0, NB = 0, pz = 0;
        __syncthreads();                                           // step 0: nothing to consume yet
        for (int step = 1;; ++step) {
            const int buf = (step - 1) & 1;
            const int tile = uni(s_item[buf][0]), blk = uni(s_item[buf][1]);
            if (tile < 0) { __syncthreads(); break; }
            const u32* __restrict__ rb = ring[buf];
            if (blk == 0) {
                L = uni(A.t_rows[tile]); pz = uni(A.t_pz[tile]);
                NB = (L + ABSM_R - 1) / ABSM_R;
                abs_set2_cols<P, 1>(h);
#pragma unroll
                for (int q = 0; q < ABS_NF; ++q) bd[0].Fc[q] = 0u;
#pragma unroll
                for (int q = 0; q < ABS_NI; ++q) bd[0].ic[q] = 0u;
                prev_ns = 0xFFFFFFFFu;
            }
            if (blk < NB) {
#pragma unroll 1
                for (int r = 0; r < ABSM_R; ++r) {
                    const int i = blk * ABSM_R + r;
                    if (i < L) {
                        abs_setprio(A.prio, i + 1, (int)blockIdx.x);
                        const u32* __restrict__ row = rb + r * PL * 64 + lane;
                        u32 nq[4], hi[1][4];
                        abs_neq_masks(row[0], row[64], nq);
                        const u32 nsm = row[2 * 64];
#pragma unroll
                        for (int p = 0; p < 4; ++p) hi[0][p] = row[(3 + p) * 64];
                        const u32 first = prev_ns & ~nsm;          // the alignments whose first row this is
                        prev_ns = nsm;
                        P::row1(nq, h, hi, bd, first, (unsigned)i);
                        if (i < pz) {
                            abs_hold2_cols<P, 1>(h, nsm);
                        }
                    }
                }
            } else {
                AbsLastRow li[1], lr[1];
                const u32* __restrict__ w = rb + lane;
#pragma unroll
                for (int q = 0; q < ABS_NF; ++q) { li[0].Fr[q] = w[q * 64]; li[0].sum[q] = w[(ABS_NF + q) * 64]; }
                li[0].newmax = w[2 * ABS_NF * 64];
                P::last1(h, li, lr);
                const u32 keep = A.nonempty[(size_t)tile * 64 + lane] & ~A.invalid[(size_t)tile * 64 + lane];
                u32 val[ABS_NF + 1], endq[ABS_NI];
                abs_decide(bd[0], lr[0], (unsigned)(L - 1), val, endq, A.r1_scalar != 0);
                const uint32_t slot0 = (uint32_t)tile * ABSM_TILE + (uint32_t)lane * 32u;
                for (int bit = 0; bit < 32; ++bit) {
                    if (!((keep >> bit) & 1u)) continue;
                    int v = 0, e = 0;
#pragma unroll
                    for (int q = 0; q <= ABS_NF; ++q) v |= (int)((val[q] >> bit) & 1u) << q;
#pragma unroll
                    for (int q = 0; q < ABS_NI; ++q) e |= (int)((endq[q] >> bit) & 1u) << q;
                    const int score = v - 2 * P::M0 - 1;
                    e -= L - A.mlen[slot0 + bit];                  // tile row -> row of the interior
                    // the record adapter_middle_body writes: a template that does not beat -1.0 leaves "none"
                    AdapterBest best; best.raw = -1; best.den = 100; best.end = -1; best.tpl = -1;
                    if (best.raw * A.den < score * best.den) { best.raw = score; best.den = A.den; best.end = e; best.tpl = A.tpl; }
                    A.bests[slot0 + bit] = best;
                }
            }
            __syncthreads();
        }
    }
}

template <class P>
__global__ void __launch_bounds__(128, 2)
k_adapter_mid(AbsMidArgs a) { abs_mid_body<P>(a); }

// ---------------------------------------------------------------------------------------------
// k_adapter_mid1<P>: the same walk on ONE wave per big tile for the templates whose row state fits a wave's registers
// (four planes per column: up to ABSM_ONE_WAVE_COLS columns beside the border state and the cell's temporaries) -- no ring,
// no barrier per six rows, no stage that waits for the other.  The two-wave pipeline exists because a fused plan of 81
// columns needs 324 registers; a single template of NBD103 / NBD104 / NBD114 (45 and 39 columns) does not, and with about
// one big tile per workgroup slot (1 M reads: ~1000 tiles) the pipeline's waves were active half of the time
// (5.3 cycles per instruction at two waves per SIMD against the 2.64 they sustain).
// ---------------------------------------------------------------------------------------------
constexpr int ABSM_ONE_WAVE_COLS = 46;

template <class P>
__device__ __forceinline__ void abs_mid1_body(const AbsMidArgs& A) {
    using namespace qabs;
    static_assert(P::NT == 1 && P::NH == 1, "single-template plans");
    const int lane = threadIdx.x & 63;
    u32 h0[P::NC0][4], h1[P::NC1][4];
    AbsBorder bd[1];
    constexpr int ABS_PF = 3;
    for (;;) {
        int tile = -1;
        for (;;) {                                                 // next big tile of this template's kit
            u32 t = 0;
            if (lane == 0) t = atomicAdd(A.cursor, 1u);
            t = (u32)uni((int)t);
            if (t >= A.n_tiles) break;
            if (uni(A.t_rows[t]) > 0 && uni(A.t_kit[t]) == A.kit_slot) { tile = (int)t; break; }
        }
        if (tile < 0) break;
        const int L = uni(A.t_rows[tile]), pz = uni(A.t_pz[tile]);
        const size_t off = (size_t)(uint32_t)uni((int)A.t_off[tile]);
        const uint2* __restrict__ src = A.planes + off * 64 + lane;
        const uint32_t* __restrict__ nsrc = A.ns + off * 64 + lane;
        abs_set2_cols<P, 0>(h0);
        abs_set2_cols<P, 1>(h1);
#pragma unroll
        for (int q = 0; q < ABS_NF; ++q) bd[0].Fc[q] = 0u;
#pragma unroll
        for (int q = 0; q < ABS_NI; ++q) bd[0].ic[q] = 0u;
        uint2 pf[ABS_PF];
        u32 pn[ABS_PF];
#pragma unroll
        for (int r = 0; r < ABS_PF; ++r) {
            pf[r] = src[(size_t)min(r, L - 1) * 64];
            pn[r] = r < pz ? nsrc[(size_t)r * 64] : 0u;
        }
        u32 prev_ns = 0xFFFFFFFFu;
#pragma unroll 1
        for (int i = 0; i < L; ++i) {
            abs_setprio(A.prio, i, (int)blockIdx.x);
            const uint2 c = pf[0];
            const u32 nsm = pn[0];
#pragma unroll
            for (int q = 0; q + 1 < ABS_PF; ++q) { pf[q] = pf[q + 1]; pn[q] = pn[q + 1]; }
            pf[ABS_PF - 1] = src[(size_t)min(i + ABS_PF, L - 1) * 64];
            pn[ABS_PF - 1] = i + ABS_PF < pz ? nsrc[(size_t)(i + ABS_PF) * 64] : 0u;
            u32 nq[4], ho[1][4];
            abs_neq_masks(c.x, c.y, nq);
            P::row0(nq, h0, ho);
            const u32 first = prev_ns & ~nsm;                      // the alignments whose first row this is
            prev_ns = nsm;
            if (i < pz) {                                          // (wave-uniform: the rows in which some alignment of the tile has not started)
                abs_hold2_cols<P, 0>(h0, nsm);
                abs_hold2(ho[0], nsm);
            }
            P::row1(nq, h1, ho, bd, first, (unsigned)i);
            if (i < pz) {
                abs_hold2_cols<P, 1>(h1, nsm);
            }
        }
        AbsLastRow lo[1], lr[1];
        P::last0(h0, lo);
        P::last1(h1, lo, lr);
        const u32 keep = A.nonempty[(size_t)tile * 64 + lane] & ~A.invalid[(size_t)tile * 64 + lane];
        u32 val[ABS_NF + 1], endq[ABS_NI];
        abs_decide(bd[0], lr[0], (unsigned)(L - 1), val, endq, A.r1_scalar != 0);
        const uint32_t slot0 = (uint32_t)tile * ABSM_TILE + (uint32_t)lane * 32u;
        for (int bit = 0; bit < 32; ++bit) {
            if (!((keep >> bit) & 1u)) continue;
            int v = 0, e = 0;
#pragma unroll
            for (int q = 0; q <= ABS_NF; ++q) v |= (int)((val[q] >> bit) & 1u) << q;
#pragma unroll
            for (int q = 0; q < ABS_NI; ++q) e |= (int)((endq[q] >> bit) & 1u) << q;
            const int score = v - 2 * P::M0 - 1;
            e -= L - A.mlen[slot0 + bit];
            AdapterBest best; best.raw = -1; best.den = 100; best.end = -1; best.tpl = -1;
            if (best.raw * A.den < score * best.den) { best.raw = score; best.den = A.den; best.end = e; best.tpl = A.tpl; }
            A.bests[slot0 + bit] = best;
        }
    }
}

template <class P>
__global__ void __launch_bounds__(64, 2)
k_adapter_mid1(AbsMidArgs a) {
    if constexpr (P::NC0 + P::NC1 <= ABSM_ONE_WAVE_COLS) abs_mid1_body<P>(a);
}

}  // namespace qk

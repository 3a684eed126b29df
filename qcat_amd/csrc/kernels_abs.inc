// kernels_abs.inc -- the ADAPTER scan in bit-sliced difference form (round 3): device kernels around abs_core.h.
//
// find_best_adapter_template (qcat/scanner_base.py:313-359) aligns every template of the kit to every read window.
// The packed-binary16 kernels (kernels_static.inc) spend two half-rate packed instructions per 128 cells; abs_core.h
// computes a cell of 2048 alignments in 27 (letter column) / 25 (N column) full-rate v_bitop3_b32.  What it takes:
//
//  * letter planes.  k_abs_planes transposes the packed windows (`win`, one code per byte) into bit planes: a tile =
//    2048 consecutive read ends, per row one uint2 per lane (plane c1, plane c0; alignment of (lane, bit) = tile * 2048 +
//    lane * 32 + bit).  Only FULL-LENGTH windows of plain A/C/G/T take the path (every base-called read of at least
//    max_align_length bases): the kernel computes all 2048 slots of a tile and `valid` says which results to keep; the
//    ordinary 128-end tiles that hold any other window are flagged in `need128` and scanned again by the binary16 kernel
//    of the same kit (which then skips every tile that is not flagged).
//  * registers.  The row state is four planes per letter column and two per N column (abs_core.h; four everywhere until the narrow N cell): 240 VGPRs for a 60-column template, 324 for the
//    two templates of PBC096 with their 38 shared columns.  A plan (abs_generated.inc) is therefore cut into TWO stages
//    that run on the two waves of a workgroup as a software pipeline over blocks of ABS_R rows: wave 0 computes its
//    columns of block k and hands the difference planes at the cut (and the letters) to wave 1 through a double-buffered
//    LDS ring while wave 1 computes its columns of block k - 1; one workgroup barrier per block.  Both waves hold <= 256
//    VGPRs, two waves per SIMD -- v_bitop3_b32 issues every 2.64 cycles per SIMD at that occupancy against 2.52 at four
//    (tools/valu_bank.hip, profiles/r02_valu_operand_rates.txt).
//  * borders.  Wave 1 owns the last columns: per row the deficit step and the index latch (abs_border_step,
//    abs_latch_index); after the last block one more pipeline item walks the last row through both waves' columns
//    (P::last0 / P::last1), wave 1 decides (abs_decide), un-transposes the score and end planes and writes the same
//    `AdapterBest` records the binary16 kernels write.
//
// Workgroups are persistent (four per CU) and draw tiles from an atomic cursor.  Included by abs_kernels.hip, which is a
// translation unit of its own (namespace qk_abs, like bs_static.hip) so that it compiles beside qcat_hip.hip.

#include "abs_core.h"
#ifndef QCAT_ABS_NO_BUILTIN                    // (run-time generated plans, qcat_amd/jit.py: the kernel bodies without the built-in kits' plans)
#include "abs_generated.inc"
#endif

namespace qk {

#ifndef QCAT_ABS_TILE_DEFINED                 // (packed_host.inc states the same constant for the host side; a hipcc-built
#define QCAT_ABS_TILE_DEFINED                 // generated unit sees both files)
constexpr int ABS_TILE = 2048;                // read ends per tile (64 lanes x 32 bits)
#endif
#ifndef QCAT_ABS_R
#define QCAT_ABS_R 6
#endif
constexpr int ABS_R = QCAT_ABS_R;             // rows per pipeline block (A/B builds: -DQCAT_ABS_R=<n>)
constexpr int ABS_MAX_ROWS = 150;
#ifndef QCAT_ABS_PLANE_WAVES
#define QCAT_ABS_PLANE_WAVES 8
#endif
constexpr int ABS_PLANE_WAVES = QCAT_ABS_PLANE_WAVES;     // waves of a k_abs_planes workgroup (4 or 8)

// ---------------------------------------------------------------------------------------------
// k_abs_planes<ROWS>: windows at two bits per code (win2) -> letter planes + eligibility.  One 256-thread workgroup per tile; a wave takes
// eight slices of 64 consecutive read ends: a lane gets its window's 40 bytes through the LDS, every row costs two ballots, and lane 0
// stores the slice's 16 bytes of that row -- the plane words (c1, c0) of plane lanes 2 sl and 2 sl + 1.  The eight
// slices of a wave fill two whole 64-byte lines per row.  ROWS > 0: max_align_length known at compile time (150, the
// default: no per-row bound checks); ROWS = 0: any length up to a window.
// ---------------------------------------------------------------------------------------------
// acc[LANE] = value (wave-uniform): v_writelane_b32 (this clang has no builtin for it).  The lane select is an inline
// constant: a second SGPR would break gfx9's one-SGPR constant-bus limit.
template <int LANE>
__device__ __forceinline__ void abs_writelane(u32 value, u32& acc) {
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(acc) : "s"(value), "n"(LANE));
}
template <int V> struct AbsIC { static constexpr int value = V; };
template <int I, int N, class F>
__device__ __forceinline__ void abs_static_for(F&& f) {
    if constexpr (I < N) { f(AbsIC<I>{}); abs_static_for<I + 1, N>(f); }
}

template <int ROWS>
__device__ __forceinline__ void abs_planes_body(const uint32_t* __restrict__ win2, const int32_t* __restrict__ wlen, const uint8_t* __restrict__ wspec,
                                                uint32_t n_ends, int rows_rt, uint2* __restrict__ planes, uint32_t* __restrict__ valid,
                                                uint8_t* __restrict__ need128, uint32_t* __restrict__ tile_any) {
    const int rows = ROWS > 0 ? ROWS : rows_rt;
    constexpr int NG = ROWS > 0 ? (ROWS + 63) / 64 : (WIN_STRIDE + 63) / 64;         // groups of 64 rows
    const uint32_t tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = uni((int)(threadIdx.x >> 6));
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(planes + (size_t)tile * rows * 64);      // [row][slice]: 16 bytes
    __shared__ uint4 s_win[ABS_PLANE_WAVES * 64 * 3];                                // per wave: the 64 windows of the slice in hand
    bool any = false;
    // four slices at a time: row r's words of slice k go to lane r & 63 of acc[r >> 6][k] (v_writelane), and after the
    // fourth slice every lane stores the 64 bytes of its rows -- whole lines (16-byte pieces were written back one by
    // one: WRITE_SIZE 2x the plane bytes)
    // (round 4: eight waves per tile, four slices each -- a 1 M-end batch is 488 tiles, and four waves walking eight slices
    //  one after the other made the kernel 54 us of latency in a 1 ms step; a big batch is bound by HBM either way)
    constexpr int HALVES = 32 / (4 * ABS_PLANE_WAVES);
    for (int half = 0; half < HALVES; ++half) {
        const int sl0 = wave * 4 * HALVES + half * 4;
        u32 acc[NG][4][4];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[g][k][q] = 0u;
        bool any4 = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sl = sl0 + k;
            const uint32_t e = tile * ABS_TILE + (uint32_t)sl * 64u + (uint32_t)lane;
            const bool in = e < n_ends;
            const uint32_t ec = in ? e : n_ends - 1;
            uint4* __restrict__ mine = s_win + (size_t)wave * 64 * 3;
            const bool ok = in && wlen[ec] == rows && !wspec[ec];
            const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
            const unsigned long long badm = __builtin_amdgcn_ballot_w64(in && !ok);
            if (lane < 2) valid[(size_t)tile * 64 + 2 * sl + lane] = (uint32_t)(lane ? okm >> 32 : okm);
            if (badm != 0 && lane == 0) need128[(tile * ABS_TILE + (uint32_t)sl * 64u) / PK_TILE] = 1;
            if (okm == 0) continue;                                 // nothing of this slice is kept: its planes stay zero
            any4 = true;
            u32 img2[WIN2_WORDS];                                   // the lane's window at two bits per code (k_pack_windows: win2)
            {
                // the slice's 64 windows are 2 560 contiguous bytes at two bits per code: every lane loads ten dwords of that
                // block (a coalesced 256 bytes per instruction) into the wave's LDS area and reads its own window back from
                // there.  (The byte windows, 10 240 bytes per slice, were 3.3 GB of this kernel's 4.1 GB per 10 M reads; a lane
                // fetching its own row touches 64 different cache lines per instruction)
                const uint32_t e0 = tile * ABS_TILE + (uint32_t)sl * 64u;
                const uint32_t* __restrict__ src = win2 + (size_t)e0 * WIN2_WORDS;
                const size_t lim = ((size_t)n_ends - e0) * WIN2_WORDS;                  // dwords of this slice that exist
                u32* __restrict__ mine2 = reinterpret_cast<u32*>(mine);
                u32 t[WIN2_WORDS];
#pragma unroll
                for (int c = 0; c < WIN2_WORDS; ++c) t[c] = (size_t)(c * 64 + lane) < lim ? src[c * 64 + lane] : 0u;
#pragma unroll
                for (int c = 0; c < WIN2_WORDS; ++c) mine2[c * 64 + lane] = t[c];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int c = 0; c < WIN2_WORDS; ++c) img2[c] = mine2[lane * WIN2_WORDS + c];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            abs_static_for<0, NG * 64 < WIN_STRIDE ? NG * 64 : WIN_STRIDE>([&](auto R_) {
                constexpr int r = decltype(R_)::value, c = r >> 4, q = r & 15;
                if (ROWS > 0 ? r < ROWS : r < rows) {
                    const unsigned long long m1 = __builtin_amdgcn_ballot_w64((img2[c] & (2u << (2 * q))) != 0);
                    const unsigned long long m0 = __builtin_amdgcn_ballot_w64((img2[c] & (1u << (2 * q))) != 0);
                    abs_writelane<(r & 63)>((u32)m1, acc[r >> 6][k][0]);
                    abs_writelane<(r & 63)>((u32)m0, acc[r >> 6][k][1]);
                    abs_writelane<(r & 63)>((u32)(m1 >> 32), acc[r >> 6][k][2]);
                    abs_writelane<(r & 63)>((u32)(m0 >> 32), acc[r >> 6][k][3]);
                }
            });
        }
        any = any || any4;
        if (!any4) continue;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int row = g * 64 + lane;
            if (row < rows) {
                uint4* __restrict__ out = dst + (size_t)row * 32 + sl0;
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = make_uint4(acc[g][k][0], acc[g][k][1], acc[g][k][2], acc[g][k][3]);
            }
        }
    }
    if (any && lane == 0) tile_any[tile] = 1;
}

template <int ROWS>
__global__ void __launch_bounds__(ABS_PLANE_WAVES * 64)
k_abs_planes(const uint32_t* __restrict__ win2, const int32_t* __restrict__ wlen, const uint8_t* __restrict__ wspec,
             uint32_t n_ends, int rows_rt, uint2* __restrict__ planes, uint32_t* __restrict__ valid,
             uint8_t* __restrict__ need128, uint32_t* __restrict__ tile_any) {
    abs_planes_body<ROWS>(win2, wlen, wspec, n_ends, rows_rt, planes, valid, need128, tile_any);
}

// ---------------------------------------------------------------------------------------------
// k_pack_planes<ENDS>: k_pack_windows and k_abs_planes in one pass over the reads (big batches of kits with a bit-sliced
// adapter plan).  A workgroup takes PP_ENDS consecutive read ends, a quarter of a plane tile.
//   pack       every thread is a thread of k_pack_windows (dev_pack_part, kernels_common.inc: 32 codes, nine dwords in
//              flight; win2 / wlen / wspec and the byte windows leave exactly as from that kernel), PP_ITER items each; the
//              window's ten dwords also go to the LDS, and an end that stays off the path sets its bit in s_bad.
//   transpose  after the barrier one thread takes 32 read ends x one window dword from the LDS, transposes the 32 x 32 bit
//              matrix in registers (bs_transpose32, bs_core.h) and stores the plane words of its sixteen rows; consecutive
//              lanes hold consecutive groups of 32 ends, so a row's stores are 128 contiguous bytes.  LDS layout: ten
//              dwords per end, four dwords of padding per group of 32 ends -- lane (group g, dword d) reads bank
//              4 g + d + 10 i for end i of its group, the 64 lanes of a wave (16 g x 4 d) 64 different banks.
//   flags      valid, need128 and tile_any from s_bad and the read-end count: the values k_abs_planes derives from wlen and
//              wspec.  Unlike that kernel, the planes of a slice without any valid end are written too (nobody reads them:
//              their keep masks are zero).
// The grid covers whole tiles: a workgroup past the last read end only clears its keep masks.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t PP_ENDS = 512;                                        // read ends per workgroup
constexpr uint32_t PP_THREADS = 640;
constexpr uint32_t PP_ITER = PP_ENDS * PACK_PARTS / PP_THREADS;          // pack items per thread
constexpr uint32_t PP_GROUPS = PP_ENDS / 32;                             // plane lanes per workgroup
constexpr uint32_t PP_GSTRIDE = 32 * WIN2_WORDS + 4;                     // dwords of a group of 32 ends in the LDS
static_assert(PP_ITER * PP_THREADS == PP_ENDS * PACK_PARTS && PP_THREADS % PACK_PARTS == 0 && ABS_TILE % PP_ENDS == 0 && PP_ENDS % PK_TILE == 0 &&
              PP_GROUPS * WIN2_WORDS + PP_GROUPS <= PP_THREADS && PACK_CODES == 32, "k_pack_planes: the item arithmetic below");

template <int ENDS>
__global__ void __launch_bounds__(PP_THREADS)
k_pack_planes(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offsets, uint32_t n_reads, int max_align,
              uint8_t* __restrict__ win, int32_t* __restrict__ wlen, uint8_t* __restrict__ wspec, uint32_t* __restrict__ win2, int lazy_bytes,
              uint2* __restrict__ planes, uint32_t* __restrict__ valid, uint8_t* __restrict__ need128, uint32_t* __restrict__ tile_any) {
    __shared__ __attribute__((aligned(8))) u32 s_win[PP_GROUPS * PP_GSTRIDE];
    __shared__ u32 s_bad[PP_GROUPS];
    const uint64_t n_ends = (uint64_t)n_reads * ENDS;
    const uint64_t e0 = (uint64_t)blockIdx.x * PP_ENDS;
    const uint32_t tile = (uint32_t)(e0 / ABS_TILE), lane0 = (uint32_t)(e0 % ABS_TILE) / 32u;
    if (e0 >= n_ends) {
        if (threadIdx.x < PP_GROUPS) valid[(size_t)tile * 64 + lane0 + threadIdx.x] = 0u;
        return;
    }
    if (threadIdx.x < PP_GROUPS) s_bad[threadIdx.x] = 0u;
    __syncthreads();
    {
        const uint32_t wl = threadIdx.x / PACK_PARTS, part = threadIdx.x - wl * PACK_PARTS;
#pragma unroll
        for (uint32_t it = 0; it < PP_ITER; ++it) {
            const uint32_t el = it * (PP_THREADS / PACK_PARTS) + wl;
            const uint64_t e = e0 + el;
            uint32_t p[PACK_CODES / 16] = {0u, 0u};                      // (past the last read end: zero planes, as k_abs_planes reads them)
            if (e < n_ends && dev_pack_part<ENDS>(bases, offsets, max_align, e, part, win, wlen, wspec, win2, lazy_bytes, p))
                atomicOr(&s_bad[el >> 5], 1u << (el & 31u));
            *reinterpret_cast<uint2*>(&s_win[(el >> 5) * PP_GSTRIDE + (el & 31u) * WIN2_WORDS + part * (PACK_CODES / 16)]) = make_uint2(p[0], p[1]);
        }
    }
    __syncthreads();
    const int rows = max_align;
    if (threadIdx.x < PP_GROUPS * WIN2_WORDS) {
        const uint32_t g = threadIdx.x % PP_GROUPS, d = threadIdx.x / PP_GROUPS;
        u32 v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = s_win[g * PP_GSTRIDE + (uint32_t)i * WIN2_WORDS + d];
        bs_transpose32(v);                                               // v[2 q + 1], v[2 q]: planes c1, c0 of code 16 d + q, bit i = end i of the group
        uint2* __restrict__ dst = planes + ((size_t)tile * rows + d * 16u) * 64 + lane0 + g;
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if ((int)(d * 16u) + q < rows) dst[(size_t)q * 64] = make_uint2(v[2 * q + 1], v[2 * q]);
    } else if (threadIdx.x < PP_GROUPS * WIN2_WORDS + PP_GROUPS) {
        const uint32_t g = threadIdx.x - PP_GROUPS * WIN2_WORDS;
        const uint64_t eg = e0 + g * 32u;
        const u32 in = eg >= n_ends ? 0u : (n_ends - eg >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)(n_ends - eg)) - 1u);
        const u32 ok = in & ~s_bad[g];
        valid[(size_t)tile * 64 + lane0 + g] = ok;
        if (in & ~ok) need128[eg / PK_TILE] = 1;
        if (ok) tile_any[tile] = 1;
    }
}

// ---------------------------------------------------------------------------------------------
// k_adapter_bs<P>: the two-wave pipeline of plan P over the tiles.
// ---------------------------------------------------------------------------------------------
// The VALU serves the highest priority first, then the oldest wave: two waves of different workgroups share a SIMD, and
// left alone the older one runs ahead until its partner's barrier stops it.  mode 1: the priority alternates by row and
// workgroup; mode 2: by pairs of rows; mode m: every 2^(m-1) rows; mode 0: no rotation (A/B: QCAT_HIP_ABS_PRIO).
__device__ __forceinline__ void abs_setprio(int mode, int row, int wg) {
    if (mode == 0) return;
    const int bit = ((row >> (mode - 1)) ^ wg ^ (wg >> 3)) & 1;   // (mode m: the priority changes every 2^(m-1) rows)
    if (bit) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
}

// The row state of a stage's columns.  An N column keeps TWO planes (abs_core.h: b stays in 0..3 there; the plan's table
// N0 / N1, or N of a stage of a four-stage plan, says which columns those are): h[j][2], h[j][3] of such a column are never
// written nor read, so they take no registers.  S: 0 / 1 = stage of a two-stage plan P, 2 = P is a stage of a four-stage plan.
template <class P, int S>
constexpr bool abs_is_n(int j) {
    if constexpr (S == 0) return P::N0[j] != 0;
    else if constexpr (S == 1) return P::N1[j] != 0;
    else return P::N[j] != 0;
}
template <class P, int S, int J = 0, int NC>
__device__ __forceinline__ void abs_set2_cols(u32 (&h)[NC][4]) {
    if constexpr (J < NC) {
        if constexpr (abs_is_n<P, S>(J)) qabs::abs_set2_n(h[J]); else qabs::abs_set2(h[J]);
        abs_set2_cols<P, S, J + 1>(h);
    }
}
template <class P, int S, int J = 0, int NC>
__device__ __forceinline__ void abs_hold2_cols(u32 (&h)[NC][4], u32 hold) {
    if constexpr (J < NC) {
        if constexpr (abs_is_n<P, S>(J)) qabs::abs_hold2_n(h[J], hold); else qabs::abs_hold2(h[J], hold);
        abs_hold2_cols<P, S, J + 1>(h, hold);
    }
}

template <class P>
__device__ __forceinline__ void abs_body(const AbsArgs& A) {
    using namespace qabs;
    constexpr int NH = P::NH, NT = P::NT;
    constexpr int PL = 2 + 4 * NH;                                // planes of a ring row: the letters, then the hand-over sets
    constexpr int LR_WORDS = 2 * ABS_NF + 1;                      // an AbsLastRow in the ring
    static_assert(NH * LR_WORDS <= ABS_R * PL, "the last-row hand-over must fit a ring buffer");
    __shared__ u32 ring[2][ABS_R * PL * 64];
    __shared__ int s_item[2][2];                                   // [step parity]: tile (-1: the end), block
    const int lane = threadIdx.x & 63, wave = uni((int)(threadIdx.x >> 6));
    const int L = A.rows;
    const int NB = (L + ABS_R - 1) / ABS_R;                        // row blocks of a tile; item NB = the walk along the last row

    if (wave == 0) {
        // ---- stage 0 ---------------------------------------------------------------------------------------
        u32 h[P::NC0][4];
        int tile = -1, blk = 0;
        // letters: a rolling prefetch ABS_PF rows ahead (a row's uint2 per lane is one coalesced 512-byte load; a row of
        // this stage's columns takes ~3000 cycles, so three rows cover the memory latency with six registers)
        // The row loop is NOT unrolled: a row body of this stage is ~9 KB of code, six of them per stage would be
        // 110 KB for the two stages against a 64 KB instruction cache; the prefetch registers rotate by moves instead.
        constexpr int ABS_PF = 3;
        uint2 pf[ABS_PF];
        const uint2* __restrict__ src = A.planes + lane;
        for (int step = 0;; ++step) {
            const int buf = step & 1;
            if (tile < 0 || blk > NB) {                            // next tile
                for (;;) {
                    u32 t = 0;
                    if (lane == 0) t = atomicAdd(A.cursor, 1u);
                    t = (u32)uni((int)t);
                    if (t >= A.n_tiles) { tile = -1; break; }
                    if (A.tile_any[t]) { tile = (int)t; break; }
                }
                blk = 0;
                if (tile >= 0) {
                    abs_set2_cols<P, 0>(h);
                    src = A.planes + ((size_t)tile * L) * 64 + lane;
#pragma unroll
                    for (int r = 0; r < ABS_PF; ++r) pf[r] = src[(size_t)min(r, L - 1) * 64];
                }
            }
            if (lane == 0) { s_item[buf][0] = tile; s_item[buf][1] = blk; }
            if (tile < 0) { __syncthreads(); __syncthreads(); break; }   // stage 1 reads the end mark in the next step
            u32* __restrict__ rb = ring[buf];
            if (blk < NB) {
#pragma unroll 1
                for (int r = 0; r < ABS_R; ++r) {
                    const int i = blk * ABS_R + r;
                    if (i < L) {
                        abs_setprio(A.prio, i, (int)blockIdx.x);
                        const uint2 c = pf[0];
#pragma unroll
                        for (int q = 0; q + 1 < ABS_PF; ++q) pf[q] = pf[q + 1];
                        pf[ABS_PF - 1] = src[(size_t)min(i + ABS_PF, L - 1) * 64];
                        u32 nq[4], ho[NH][4];
                        abs_neq_masks(c.x, c.y, nq);
                        P::row0(nq, h, ho);
                        u32* __restrict__ row = rb + r * PL * 64 + lane;
                        row[0] = c.x; row[64] = c.y;
#pragma unroll
                        for (int k = 0; k < NH; ++k)
#pragma unroll
                            for (int p = 0; p < 4; ++p) row[(2 + 4 * k + p) * 64] = ho[k][p];
                    }
                }
            } else {
                AbsLastRow lo[NH];
                P::last0(h, lo);
#pragma unroll
                for (int k = 0; k < NH; ++k) {
                    u32* __restrict__ w = rb + k * LR_WORDS * 64 + lane;
#pragma unroll
                    for (int q = 0; q < ABS_NF; ++q) { w[q * 64] = lo[k].Fr[q]; w[(ABS_NF + q) * 64] = lo[k].sum[q]; }
                    w[2 * ABS_NF * 64] = lo[k].newmax;
                }
            }
            ++blk;
            __syncthreads();
        }
    } else {
        // ---- stage 1 ---------------------------------------------------------------------------------------
        u32 h[P::NC1][4];
        AbsBorder bd[NT];
        __syncthreads();                                           // step 0: nothing to consume yet
        for (int step = 1;; ++step) {
            const int buf = (step - 1) & 1;
            const int tile = uni(s_item[buf][0]), blk = uni(s_item[buf][1]);
            if (tile < 0) { __syncthreads(); break; }
            const u32* __restrict__ rb = ring[buf];
            if (blk == 0) {
                abs_set2_cols<P, 1>(h);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int q = 0; q < ABS_NF; ++q) bd[t].Fc[q] = 0u;
#pragma unroll
                    for (int q = 0; q < ABS_NI; ++q) bd[t].ic[q] = 0u;
                }
            }
            if (blk < NB) {
#pragma unroll 1
                for (int r = 0; r < ABS_R; ++r) {
                    const int i = blk * ABS_R + r;
                    if (i < L) {
                        abs_setprio(A.prio, i + 1, (int)blockIdx.x);
                        const u32* __restrict__ row = rb + r * PL * 64 + lane;
                        u32 nq[4], hi[NH][4];
                        abs_neq_masks(row[0], row[64], nq);
#pragma unroll
                        for (int k = 0; k < NH; ++k)
#pragma unroll
                            for (int p = 0; p < 4; ++p) hi[k][p] = row[(2 + 4 * k + p) * 64];
                        P::row1(nq, h, hi, bd, i == 0 ? 0xFFFFFFFFu : 0u, (unsigned)i);
                    }
                }
            } else {
                AbsLastRow li[NH], lr[NT];
#pragma unroll
                for (int k = 0; k < NH; ++k) {
                    const u32* __restrict__ w = rb + k * LR_WORDS * 64 + lane;
#pragma unroll
                    for (int q = 0; q < ABS_NF; ++q) { li[k].Fr[q] = w[q * 64]; li[k].sum[q] = w[(ABS_NF + q) * 64]; }
                    li[k].newmax = w[2 * ABS_NF * 64];
                }
                P::last1(h, li, lr);
                const u32 keep = A.valid[(size_t)tile * 64 + lane];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    u32 val[ABS_NF + 1], endq[ABS_NI];
                    abs_decide(bd[t], lr[t], (unsigned)(L - 1), val, endq, A.r1_scalar != 0);
                    const int M = t == 0 ? P::M0 : P::M1;
                    const int den = A.den[t], tpl = A.tpl[t];
                    AdapterBest* __restrict__ out = A.bests[t] + (size_t)tile * ABS_TILE + (size_t)lane * 32;
                    for (int bit = 0; bit < 32; ++bit) {
                        if (!((keep >> bit) & 1u)) continue;
                        int v = 0, e = 0;
#pragma unroll
                        for (int q = 0; q <= ABS_NF; ++q) v |= (int)((val[q] >> bit) & 1u) << q;
#pragma unroll
                        for (int q = 0; q < ABS_NI; ++q) e |= (int)((endq[q] >> bit) & 1u) << q;
                        const int score = v - 2 * M - 1;
                        if (A.dbg_tpl) {
                            const size_t eidx = (size_t)tile * ABS_TILE + (size_t)lane * 32 + (size_t)bit;
                            A.dbg_tpl[(eidx * 2 + 0) * MAX_T + tpl] = score;
                            A.dbg_tpl[(eidx * 2 + 1) * MAX_T + tpl] = e;
                        }
                        // the same record adapter_fused2_body writes: a template that does not beat -1.0 leaves "none"
                        AdapterBest best; best.raw = -1; best.den = 100; best.end = -1; best.tpl = -1;
                        if (best.raw * den < score * best.den) { best.raw = score; best.den = den; best.end = e; best.tpl = tpl; }
                        out[bit] = best;
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <class P>
__global__ void __launch_bounds__(128, 2)
k_adapter_bs(AbsArgs a) { abs_body<P>(a); }

// ---------------------------------------------------------------------------------------------
// k_adapter_ms<P>: the same pipeline with one wave per stage of a plan of P::NS stages (QAM_*, tools/gen_abs_kernels.py).
// Twice the waves per tile of the two-stage plans -- a 1 M-read batch of a one-end kit is 488 tiles, one two-stage
// workgroup per tile leaves every SIMD with one wave (an instruction every 5 cycles instead of every 2.6) -- and at most 13
// columns per wave: 128 VGPRs, four waves per SIMD, so that the kernels of a kit's two templates run side by side.  Every stage reads the letter planes of its rows itself
// (a coalesced 512-byte load per row, three rows ahead); a cut hands over four planes per live difference through a ring
// of its own (two buffers of ABS_R rows); a stage that holds a template's border keeps that template's end-position
// state and writes its result.  Step k: stage s works on item k - s (a block of ABS_R rows of a tile, or the walk along
// its last row); one barrier per step; every wave executes the same number of barriers.
// ---------------------------------------------------------------------------------------------
template <class P, class SS, int SI>
__device__ __forceinline__ void abs_stage(const AbsArgs& A, u32* __restrict__ rings, int (*s_item)[2]) {
    using namespace qabs;
    constexpr int NS = P::NS;
    constexpr int LR_WORDS = 2 * ABS_NF + 1;
    static_assert(LR_WORDS <= ABS_R * 4, "a last-row hand-over must fit the ring rows of its difference");
    const int lane = threadIdx.x & 63;
    const int L = A.rows;
    const int NB = (L + ABS_R - 1) / ABS_R;
    // ring of cut c: rings + (RING_* planes offset) * ABS_R * 64, two buffers of ABS_R rows x 4 NH planes
    constexpr int PLI = 4 * SS::HI, PLO = 4 * SS::HO;
    u32* const ring_in = SS::NHI ? rings + (size_t)SS::RING_IN * ABS_R * 64 : rings;
    u32* const ring_out = SS::NHO ? rings + (size_t)SS::RING_OUT * ABS_R * 64 : rings;
    u32 h[SS::NC][4];
    AbsBorder bd[SS::BD];
    constexpr int ABS_PF = 3;
    uint2 pf[ABS_PF];
    const uint2* __restrict__ src = A.planes + lane;
    int tile = -1, blk = 0;
    for (int step = 0;; ++step) {
        if (step < SI) { __syncthreads(); continue; }               // nothing has reached this stage yet
        if (SI == 0) {
            if (tile < 0 || blk > NB) {                              // next tile
                for (;;) {
                    u32 t = 0;
                    if (lane == 0) t = atomicAdd(A.cursor, 1u);
                    t = (u32)uni((int)t);
                    if (t >= A.n_tiles) { tile = -1; break; }
                    if (A.tile_any[t]) { tile = (int)t; break; }
                }
                blk = 0;
            }
            if (lane == 0) { s_item[step & 7][0] = tile; s_item[step & 7][1] = blk; }
        } else {
            tile = uni(s_item[(step - SI) & 7][0]); blk = uni(s_item[(step - SI) & 7][1]);
        }
        if (tile < 0) {                                              // the end mark: the later stages still have NS - 1 - SI steps to go
            for (int q = 0; q < NS - 1 - SI; ++q) __syncthreads();
            break;
        }
        if (blk == 0) {
            abs_set2_cols<SS, 2>(h);
#pragma unroll
            for (int t = 0; t < SS::BD; ++t) {
#pragma unroll
                for (int q = 0; q < ABS_NF; ++q) bd[t].Fc[q] = 0u;
#pragma unroll
                for (int q = 0; q < ABS_NI; ++q) bd[t].ic[q] = 0u;
            }
            src = A.planes + ((size_t)tile * L) * 64 + lane;
#pragma unroll
            for (int r = 0; r < ABS_PF; ++r) pf[r] = src[(size_t)min(r, L - 1) * 64];
        }
        const u32* __restrict__ rin = ring_in + (size_t)((step - 1) & 1) * ABS_R * PLI * 64;
        u32* __restrict__ rout = ring_out + (size_t)(step & 1) * ABS_R * PLO * 64;
        if (blk < NB) {
#pragma unroll 1
            for (int r = 0; r < ABS_R; ++r) {
                const int i = blk * ABS_R + r;
                if (i < L) {
                    const uint2 c = pf[0];
#pragma unroll
                    for (int q = 0; q + 1 < ABS_PF; ++q) pf[q] = pf[q + 1];
                    pf[ABS_PF - 1] = src[(size_t)min(i + ABS_PF, L - 1) * 64];
                    u32 nq[4], hi[SS::HI][4], ho[SS::HO][4];
                    if (SS::NHI) {
#pragma unroll
                        for (int k = 0; k < SS::HI; ++k)
#pragma unroll
                            for (int p = 0; p < 4; ++p) hi[k][p] = rin[(r * PLI + 4 * k + p) * 64 + lane];
                    }
                    abs_neq_masks(c.x, c.y, nq);
                    SS::row(nq, h, hi, ho, bd, i == 0 ? 0xFFFFFFFFu : 0u, (unsigned)i);
                    if (SS::NHO) {
#pragma unroll
                        for (int k = 0; k < SS::HO; ++k)
#pragma unroll
                            for (int p = 0; p < 4; ++p) rout[(r * PLO + 4 * k + p) * 64 + lane] = ho[k][p];
                    }
                }
            }
        } else {
            AbsLastRow li[SS::HI], lo[SS::HO], lr[SS::BD];
            if (SS::NHI) {
#pragma unroll
                for (int k = 0; k < SS::HI; ++k) {
                    const u32* __restrict__ w = rin + (size_t)k * ABS_R * 4 * 64 + lane;
#pragma unroll
                    for (int q = 0; q < ABS_NF; ++q) { li[k].Fr[q] = w[q * 64]; li[k].sum[q] = w[(ABS_NF + q) * 64]; }
                    li[k].newmax = w[2 * ABS_NF * 64];
                }
            }
            SS::last(h, li, lo, lr);
            if (SS::NHO) {
#pragma unroll
                for (int k = 0; k < SS::HO; ++k) {
                    u32* __restrict__ w = rout + (size_t)k * ABS_R * 4 * 64 + lane;
#pragma unroll
                    for (int q = 0; q < ABS_NF; ++q) { w[q * 64] = lo[k].Fr[q]; w[(ABS_NF + q) * 64] = lo[k].sum[q]; }
                    w[2 * ABS_NF * 64] = lo[k].newmax;
                }
            }
            if (SS::NBD) {
                const u32 keep = A.valid[(size_t)tile * 64 + lane];
#pragma unroll
                for (int b = 0; b < SS::NBD; ++b) {
                    const int t = b == 0 ? SS::BT0 : SS::BT1;
                    u32 val[ABS_NF + 1], endq[ABS_NI];
                    abs_decide(bd[b], lr[b], (unsigned)(L - 1), val, endq, A.r1_scalar != 0);
                    const int M = t == 0 ? P::M0 : P::M1;
                    const int den = A.den[t], tpl = A.tpl[t];
                    AdapterBest* __restrict__ out = A.bests[t] + (size_t)tile * ABS_TILE + (size_t)lane * 32;
                    for (int bit = 0; bit < 32; ++bit) {
                        if (!((keep >> bit) & 1u)) continue;
                        int v = 0, e = 0;
#pragma unroll
                        for (int q = 0; q <= ABS_NF; ++q) v |= (int)((val[q] >> bit) & 1u) << q;
#pragma unroll
                        for (int q = 0; q < ABS_NI; ++q) e |= (int)((endq[q] >> bit) & 1u) << q;
                        const int score = v - 2 * M - 1;
                        if (A.dbg_tpl) {
                            const size_t eidx = (size_t)tile * ABS_TILE + (size_t)lane * 32 + (size_t)bit;
                            A.dbg_tpl[(eidx * 2 + 0) * MAX_T + tpl] = score;
                            A.dbg_tpl[(eidx * 2 + 1) * MAX_T + tpl] = e;
                        }
                        AdapterBest best; best.raw = -1; best.den = 100; best.end = -1; best.tpl = -1;
                        if (best.raw * den < score * best.den) { best.raw = score; best.den = den; best.end = e; best.tpl = tpl; }
                        out[bit] = best;
                    }
                }
            }
        }
        if (SI == 0) ++blk;
        __syncthreads();
    }
}

template <class P>
__device__ __forceinline__ void abs_ms_body(const AbsArgs& a) {
    static_assert(P::NS == 4, "one case per stage below");
    __shared__ u32 rings[P::RING_PLANES * ABS_R * 64];
    __shared__ int s_item[8][2];
    switch (uni((int)(threadIdx.x >> 6))) {
    case 0: abs_stage<P, typename P::S0, 0>(a, rings, s_item); break;
    case 1: abs_stage<P, typename P::S1, 1>(a, rings, s_item); break;
    case 2: abs_stage<P, typename P::S2, 2>(a, rings, s_item); break;
    default: abs_stage<P, typename P::S3, 3>(a, rings, s_item); break;
    }
}

template <class P>
__global__ void __launch_bounds__(64 * P::NS, 4)
k_adapter_ms(AbsArgs a) { abs_ms_body<P>(a); }

// k_adapter_mw<P>: the same four-stage pipeline for templates too long for two stages of 52 columns (VMK001: 102 columns,
// /root/reference/qcat/resources/kits/VMK001.yml) -- up to 26 columns per stage, so a wave may hold up to 256 VGPRs: two
// workgroups per CU, two waves per SIMD like the two-stage plans (QAW_T<n>, tools/gen_abs_kernels.py); big batches.
template <class P>
__global__ void __launch_bounds__(64 * P::NS, 2)
k_adapter_mw(AbsArgs a) { abs_ms_body<P>(a); }

}  // namespace qk

// kernels_bitslice.inc -- the barcode DP in BIT-SLICED difference form (round 2).
//
// find_highest_scoring_barcode (qcat/scanner_base.py:63-141) aligns every barcode target to the barcode region with
// match +1 / mismatch -1 / gap 1 (config.py:26, scanner_base.py:115-116).  With those scores the differences between
// neighbouring DP cells take four values,
//       dv(i,j) = H(i,j) - H(i-1,j),   dh(i,j) = H(i,j) - H(i,j-1)      in {-1, 0, 1, 2},
// and one cell is a boolean function of five bits: with a = dv(i,j-1) + 1, b = dh(i-1,j) + 1 (two bits each) and
// eq = [query letter == target letter],
//       m = eq ? 3 : max(a, b, 1)          ( = H(i,j) - H(i-1,j-1) + 2 )
//       dv(i,j) + 1 = m - b,   dh(i,j) + 1 = m - a.
// Bit-slicing ACROSS ALIGNMENTS puts bit k of a quantity of 32 different alignments into one 32-bit VGPR, so a wave
// advances 64 x 32 = 2048 alignments per cell with NINE full-rate three-input boolean instructions (v_bitop3_b32: seven
// for the cell -- a network found by search, tools/lut3_search.cpp -- and two to match the wave-uniform run-time target
// letter against the alignments' letter planes), where the packed-binary16 form (kernels_static.inc) spends two
// half-rate packed instructions per 128 (tools/bitslice_rate.hip, profiles/r02_bitslice_rate.txt).
//
// Static letters.  For the built-in kits (static_generated.inc) and for kits with run-time generated code (jit.py) the
// row loop of every barcode is its own piece of code with the target letters as template constants: the four possible
// mismatch masks of a row are formed once per row and a column just names one, so a cell is the seven instructions of
// its network (k_bs_barcode<QBS_n>, bs_rows_static); other kits run k_bs_barcode<BsDyn<C>> with letters from memory.
//
// Shared columns.  Every target of a set is  upstream context + barcode + downstream context  (layout.py:191-238), and
// column j of the DP depends on columns < j only: the columns of the leading context are the same for every barcode.
// The score of a semi-global alignment does not change when both sequences are reversed, so the LONGER of the two
// contexts is made the leading one (DevSet::bs_rev: rows and target letters run backwards), its P columns are computed
// once per super-tile, and dv at column P of every row waits in the LDS for the barcodes: 11 of PBC096's 42 columns.
//
// The price is paid at the borders: the scores themselves (last row, last column) are sums of differences.  The last
// row is summed in bit-sliced 7-bit counters per column once per barcode; the last column keeps, per row, only the
// DEFICIT  max_k<=i H(k,M) - H(i,M)  (an 8-bit counter, F = deficit + 1 = max(F + 1 - a, 1)), and the column maximum is
// H(L,M) + deficit at the end.  The whole 2048-alignment "super-tile" must share the target, the row count and plain
// letters -- so only the two lengths almost every barcode region has (the nominal region length 2 * extension + barcode
// + 1 and the full window) take this path, in full super-tiles; everything else (other lengths, windows holding letters
// outside A, C, G, T, the last < 2048 jobs of a class, debug scans, small batches) runs the packed-binary16 kernels,
// tile by tile, and both feed the same (max, first index) keys (kernels_packed.inc).
//
// Data: k_job_scatter sorts the "hot" jobs of a (template, set) group into two classes of their own; k_bs_plan cuts
// each class into super-tiles of 2048 consecutive sorted jobs (128-aligned: sixteen ordinary tiles, which the
// binary16 kernels then skip).  k_bs_barcode<C> (C = columns after the shared ones) runs ONE 16-wave workgroup per CU:
// the workgroup transposes the super-tile's regions -- out of the sixteen ordinary tile images k_job_gather made --
// into letter bit planes in the LDS (ballots; codes A,T,G,C = 0..3 in planes c1 c0; 16 bytes per row and lane: c1, c0
// and, after the shared columns, dv at column P; the alignment of (lane, bit) is sorted job first + lane * 32 + bit),
// the waves take the unit's barcodes round robin with the dh planes of their C columns in registers, and the
// per-alignment best keys of the waves meet in the LDS before they leave; k_bs_select merges the units, writes
// the record fields and queues best-raw-0 alignments for k_barcode_redo.
// Included by qcat_hip.hip after kernels_packed.inc.

// build-time variants (A/B runs of two builds, tools/ab_run.sh)
#ifndef QCAT_BS_WAVES
#define QCAT_BS_WAVES 16
#endif
#ifndef QCAT_BS_PAIRS
#define QCAT_BS_PAIRS 1                       // static-letter rows two per pass
#endif
#ifndef QCAT_BS_ROTATE_BY_WAVES
#define QCAT_BS_ROTATE_BY_WAVES 0             // priority rotation with the period of the SIMD's barcode waves (measured: slower)
#endif
#ifndef QCAT_BS_STATIC_SHARED
#define QCAT_BS_STATIC_SHARED 1               // generated kernels: the shared columns with compile-time letters as well
#endif

#include "bs_core.h"                       // the cell, the counters, the deficit updates: shared with tests/bs_host_check.cpp

namespace qk {

constexpr int BS_JOBS = 2048;                 // alignments per super-tile (64 lanes x 32 bits)
constexpr int BS_TILES = BS_JOBS / PK_TILE;   // ordinary tiles it covers
constexpr int BS_MAX_CHUNKS = 4;              // units per super-tile (barcode chunks)
constexpr int BS_WAVES = QCAT_BS_WAVES;                 // waves of a k_bs_barcode workgroup: one workgroup per CU, four waves per SIMD (all the
                                              // registers allow).  Sustained v_bitop3_b32 issue per SIMD: one wave 5.15 cycles, two
                                              // 2.64, three 2.77, four 2.52, eight 2.28 (tools/valu_bank.hip)
constexpr int BS_PRE_WAVES = 4;                // waves that walk the leading context of a unit -- as many walk the trailing one (one each per SIMD)
constexpr bool BS_STATIC_PAIRS = QCAT_BS_PAIRS != 0;        // static-letter rows two per pass as well (one per pass: 2 KiB loop bodies instead of 4, measured 3 % slower)
constexpr int BS_MAX_ROWS = 150;              // LDS rows, 1 KiB each (the packed path's max_align_length limit, kit_prepare.inc)

struct BsPlan {                               // device-resident, written by k_bs_plan
    uint32_t first[JOB_BINS];                 // sorted position of the first super-tile of a hot bin
    uint32_t count[JOB_BINS];                 // super-tiles of the bin
    uint32_t cov[JOB_BINS];                   // sorted jobs of the bin inside its super-tiles, from `first` (a multiple of 128; count * 2048 unless
                                              // the last super-tile is a PADDED one -- small batches, k_bs_plan: pad_min)
    uint32_t tile_prefix[JOB_BINS + 1];       // super-tiles before the bin
    uint32_t len[JOB_BINS];                   // rows of the bin's units (the "short of nominal" class: the nominal length -- its alignments
                                              // start up to BS_PAD_ROWS rows late)
    uint32_t split[JOB_BINS];                 // the LAST `split` super-tiles of the bin are cut into twice the barcode chunks (k_bs_plan: the
                                              // units of a last, less than half full round of long units -- config 2: 266 units for 256 CUs)
    uint32_t n_seg;                           // hot bins with work, longest rows first (the long units start first)
    uint32_t seg_bin[JOB_BINS];
    uint32_t seg_prefix[JOB_BINS + 1];        // units (super-tile x chunk) before the segment
    uint32_t cursor[8][32];                   // [slot][0]: next unit of one k_bs_barcode<C> launch; a cache line each
};

struct BsNch { int v[JOB_GROUPS]; };          // barcode chunks per super-tile of every group (0: group not bit-sliced)

// is ordinary tile `tile` (128 sorted jobs) of group gidx inside a super-tile?
__device__ __forceinline__ bool bs_covers(const BsPlan* __restrict__ bp, int gidx, uint32_t tile) {
    if (!bp) return false;
    const uint32_t pos = tile * (uint32_t)PK_TILE;
#pragma unroll
    for (int c = JOB_CLASSES - JOB_HOT; c < JOB_CLASSES; ++c) {
        const int b = gidx * JOB_CLASSES + c;
        const uint32_t f = bp->first[b];
        if (pos >= f && pos < f + bp->cov[b]) return true;
    }
    return false;
}

__device__ __forceinline__ void bs_uncovered_runs(const BsPlan* __restrict__ bp, uint32_t t0, uint32_t t1, int gidx, uint32_t (&start)[4], uint32_t (&len)[4]) {
    // (the covered ranges of the three hot classes lie in sorted order inside [t0, t1): the same walk as barcode_static_body)
    static_assert(JOB_HOT == 3, "four runs of tiles around three covered ranges");
    uint32_t prev = t0;
#pragma unroll
    for (int h = 0; h < JOB_HOT; ++h) {
        uint32_t cs = prev, ce = prev;
        const int b = gidx * JOB_CLASSES + JOB_CLASSES - JOB_HOT + h;
        if (bp->count[b]) { cs = bp->first[b] / PK_TILE; ce = cs + bp->cov[b] / (uint32_t)PK_TILE; }
        start[h] = prev; len[h] = cs > prev ? cs - prev : 0u;
        prev = ce;
    }
    start[3] = prev; len[3] = t1 > prev ? t1 - prev : 0u;
}

// barcode chunks of super-tile st_local of a bin (n_lo: the group's chunks per super-tile, BsNch)
__device__ __forceinline__ int bs_chunks_hi(int n_lo) { return min(BS_MAX_CHUNKS, 2 * n_lo); }
__device__ __forceinline__ int bs_chunks_of(const BsPlan* __restrict__ bp, int bin, int n_lo, uint32_t st_local) {
    return st_local + bp->split[bin] >= bp->count[bin] ? bs_chunks_hi(n_lo) : n_lo;
}

// after k_job_scatter: cursor[bin] is the END of the bin.  One thread per bin, thread 0 strings the bins together
// (round 3's single thread walked the bins through global memory: 20 us of a 1 ms step).
// Tail split (round 4): a workgroup holds a CU for a whole unit, so when the long units (full windows) fill the CUs a
// little more than k times, the kernel lasts k + 1 long units while most CUs idle -- config 2 at 1 M reads has 266 long
// units for 256 CUs.  When that last round is less than half full its units are cut into twice the barcode chunks (two
// chunks of six barcodes run on separate CUs in 0.6 of a whole unit's time); cus <= 0: never.
__global__ void __launch_bounds__(256)
k_bs_plan(const DevKit* __restrict__ k, const JobTables* __restrict__ jt, BsNch nch, BsPlan* __restrict__ bp, int cus, uint32_t pad_min = 0, int allow_short = 1) {
    // pad_min > 0 (round 4, small batches -- the reference driver's 4000-read call): what is left of a hot bin after its whole
    // super-tiles becomes one more, PADDED super-tile when it holds pad_min jobs or more (whole 128-job tiles only): the unit
    // computes all 2048 slots, the slots past the covered jobs repeat the super-tile's first job and nobody reads their keys
    static_assert(JOB_BINS <= 256, "one thread per bin");
    __shared__ uint32_t s_count[JOB_BINS];
    const int b = (int)threadIdx.x;
    if (b < JOB_BINS) {
        const int gidx = b / JOB_CLASSES, c = b % JOB_CLASSES;
        uint32_t first = 0, n = 0, len = 0, cov = 0;
        // (allow_short = 0: the units read tile images, which know no front padding -- the class stays on the binary16 kernels)
        if (c >= JOB_CLASSES - JOB_HOT && nch.v[gidx] > 0 && (allow_short || c != JOB_CLASSES - JOB_HOT)) {
            const uint32_t end = jt->cursor[b], start = end - jt->hist[b];
            first = (start + PK_TILE - 1) / PK_TILE * PK_TILE;
            n = end > first ? (end - first) / BS_JOBS : 0;
            cov = n * (uint32_t)BS_JOBS;
            if (pad_min && end > first) {
                const uint32_t whole = (end - first) / PK_TILE * PK_TILE;      // whole ordinary tiles of the bin
                if (whole - cov >= pad_min) { n += 1; cov = whole; }
            }
            const DevSet& bs = k->tpl[gidx >> 1].sets[gidx & 1];
            len = (uint32_t)(c == JOB_CLASSES - 1 ? k->max_align : bs.hot_len);
        }
        bp->cov[b] = cov;
        bp->first[b] = first; bp->count[b] = n; bp->len[b] = len; bp->split[b] = 0;
        s_count[b] = n;
    }
    __syncthreads();
    if (b != 0) return;
    uint32_t tiles = 0;
    for (int q = 0; q < JOB_BINS; ++q) { bp->tile_prefix[q] = tiles; tiles += s_count[q]; }
    bp->tile_prefix[JOB_BINS] = tiles;
    uint32_t split_of[JOB_GROUPS];
    for (int g = 0; g < JOB_GROUPS; ++g) split_of[g] = 0;
    if (cus > 0) {
        uint32_t total = 0, best_n = 0;
        int best_g = -1;
        for (int g = 0; g < JOB_GROUPS; ++g) {
            const uint32_t n = s_count[g * JOB_CLASSES + JOB_CLASSES - 1];
            if (!n) continue;
            total += n * (uint32_t)nch.v[g];
            const DevSet& bs = k->tpl[g >> 1].sets[g & 1];
            const int hi = bs_chunks_hi(nch.v[g]);
            if (hi > nch.v[g] && bs.n / hi >= 3 && n > best_n) { best_n = n; best_g = g; }   // (a chunk keeps three barcodes or more)
        }
        const uint32_t r = total % (uint32_t)cus;
        if (best_g >= 0 && r > 0 && r * 2 <= (uint32_t)cus) {
            const uint32_t st = (r + (uint32_t)nch.v[best_g] - 1) / (uint32_t)nch.v[best_g];
            split_of[best_g] = st < best_n ? st : best_n;
            bp->split[best_g * JOB_CLASSES + JOB_CLASSES - 1] = split_of[best_g];
        }
    }
    uint32_t units = 0, ns = 0;
    for (int c = JOB_CLASSES - 1; c >= JOB_CLASSES - JOB_HOT; --c)    // the full windows, then the nominal regions, then the ones short of nominal
        for (int g = 0; g < JOB_GROUPS; ++g) {
            const int q = g * JOB_CLASSES + c;
            if (s_count[q] == 0) continue;
            bp->seg_bin[ns] = (uint32_t)q; bp->seg_prefix[ns] = units;
            const uint32_t sp = c == JOB_CLASSES - 1 ? split_of[g] : 0;
            units += (s_count[q] - sp) * (uint32_t)nch.v[g] + sp * (uint32_t)bs_chunks_hi(nch.v[g]);
            ++ns;
        }
    bp->n_seg = ns; bp->seg_prefix[ns] = units;
    for (int q = 0; q < 8; ++q) bp->cursor[q][0] = 0;
}

// shared columns of a super-tile: dv at column PP of every row into the LDS rows, and what the last row of a barcode with
// `cown` own columns starts from after PP columns -- H(L,PP) + 64 - cown and the row maximum's deficit E (bs_core.h:
// bs_last_row_start) -- into the tail.  The rows depend on each other.  Two forms:
//  * SOLO = false (every wave of the workgroup has barcodes to do): the workgroup waits for the phase, so the waves that
//    take part each compute all rows and store their share.  Round 5: ONE wave per SIMD walks the leading context and one
//    the trailing context (bs_trailing_columns) -- two waves per SIMD run at the full issue rate, so the second context's
//    columns cost the phase nothing (before: two waves per SIMD on the leading context alone);
//  * SOLO = true (round 4: a unit with fewer barcodes than waves, e.g. every 12-barcode kit): ONE otherwise idle wave is the
//    producer.  It stores every row and publishes its progress in `ready` (rows done; L + 1 once the tail is written) with
//    release semantics, and the barcode waves start their row loops at once and check `ready` before they read a row's dv
//    (bs_wait_rows) -- the producer needs ~80 instructions per row against ~200 per row and barcode, so after the first rows
//    nobody waits: the phase (65 k of a 485 k-cycle unit of config 2) disappears behind the row loops.
// `hold` / npad (round 5, units of the "short of nominal" class): hold[i * 64 + lane] = the alignments that have not started in
// row i < npad -- their dh planes go back to the boundary state after the row (bs_core.h: bs_hold)
template <int PP, bool SOLO, class NEQ>
__device__ __forceinline__ void bs_shared_columns(uint4* __restrict__ s_rows, u32* __restrict__ s_tail, int L, int lane, int wave, NEQ neq, u32* ready,
                                                  const u32* __restrict__ hold, int npad, int cown) {
    u32 h1[PP > 0 ? PP : 1], h0[PP > 0 ? PP : 1];
#pragma unroll
    for (int j = 0; j < PP; ++j) { h1[j] = 0u; h0[j] = 0xFFFFFFFFu; }
    for (int i = 0; i < L; ++i) {
        const uint2 c = *reinterpret_cast<const uint2*>(&s_rows[i * 64 + lane]);
        u32 a1 = 0u, a0 = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < PP; ++j) bs_cell(neq(j, c.x, c.y), a1, a0, h1[j], h0[j]);
        if (i < npad) {
            const u32 hm = hold[i * 64 + lane];
#pragma unroll
            for (int j = 0; j < PP; ++j) bs_hold(h1[j], h0[j], hm);
        }
        if (SOLO) {
            *(reinterpret_cast<uint2*>(&s_rows[i * 64 + lane]) + 1) = make_uint2(a1, a0);
            __hip_atomic_store(ready, (u32)(i + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (i % BS_PRE_WAVES == wave) {
            *(reinterpret_cast<uint2*>(&s_rows[i * 64 + lane]) + 1) = make_uint2(a1, a0);
        }
    }
    if (SOLO || wave == 0) {
        u32 base[BS_NB], e[BS_NE];
        bs_last_row_start(base, e, h1, h0, PP, cown);
#pragma unroll
        for (int q = 0; q < BS_NB; ++q) s_tail[q * 64 + lane] = base[q];
#pragma unroll
        for (int q = 0; q < BS_NE; ++q) s_tail[(BS_NB + q) * 64 + lane] = e[q];
        if (SOLO) __hip_atomic_store(ready, (u32)(L + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// trailing columns of a super-tile (round 5, bs_core.h): the DP R of the REVERSED region against the REVERSED trailing
// context -- the rows are walked L - 1 .. 0, column j holds the target's last letter but j -- whose last column, one
// difference per row, is all a barcode needs of the QQ columns behind its own ones: dv + 1 of R's last column at row i goes
// to `rp` (global memory, [row][lane]: the LDS rows of the full-window class fill the CU; 8 bytes per row and lane, read
// back by the barcode waves a row pair ahead, from L2) and max_j R(L, j) -- the paths that lie behind the line altogether
// -- to the tail.  `part`: this wave's share of the row stores when several waves walk the columns side by side (SOLO: all).
// QQ = 0 (a set without a trailing context): G(0) = H(0, M) is not a cell, so the first row's step is forced to drop it
// (r = 0: D + 0 - a <= 0), every other row has dvR = 0, and no path lies behind the line.
// Units of the "short of nominal" class (hold / npad): the reversed DP meets the rows in front of an alignment LAST -- there its
// state stays what it was after the alignment's own last row and r = 0 is handed out (bs_keep; QQ > 0 only: job_class_hot).
template <int QQ, bool SOLO, class NEQ>
__device__ __forceinline__ void bs_trailing_columns(const uint4* __restrict__ s_rows, uint2* __restrict__ rp, u32* __restrict__ s_tail, int L, int lane,
                                                    int part, NEQ neq, u32* ready, const u32* __restrict__ hold, int npad) {
    u32 h1[QQ > 0 ? QQ : 1], h0[QQ > 0 ? QQ : 1];
#pragma unroll
    for (int j = 0; j < QQ; ++j) { h1[j] = 0u; h0[j] = 0xFFFFFFFFu; }
    for (int i = L - 1; i >= 0; --i) {
        u32 a1 = 0u, a0 = 0xFFFFFFFFu;
        if (QQ > 0) {
            const uint2 c = *reinterpret_cast<const uint2*>(&s_rows[i * 64 + lane]);
            if (i < npad) {
                u32 o1[QQ > 0 ? QQ : 1], o0[QQ > 0 ? QQ : 1];
#pragma unroll
                for (int j = 0; j < QQ; ++j) { o1[j] = h1[j]; o0[j] = h0[j]; }
#pragma unroll
                for (int j = 0; j < QQ; ++j) bs_cell(neq(j, c.x, c.y), a1, a0, h1[j], h0[j]);
                const u32 hm = hold[i * 64 + lane];
#pragma unroll
                for (int j = 0; j < QQ; ++j) { bs_keep(h1[j], o1[j], hm); bs_keep(h0[j], o0[j], hm); }
                a1 &= ~hm; a0 &= ~hm;
            } else {
#pragma unroll
                for (int j = 0; j < QQ; ++j) bs_cell(neq(j, c.x, c.y), a1, a0, h1[j], h0[j]);
            }
        } else if (i == 0) a0 = 0u;
        if (SOLO || (i & (BS_PRE_WAVES - 1)) == part) rp[i * 64 + lane] = make_uint2(a1, a0);
    }
    if (SOLO || part == 0) {
        u32 r[BS_NB], cmax[BS_NB];
#pragma unroll
        for (int q = 0; q < BS_NB; ++q) { r[q] = (BS_OFF >> q) & 1 ? 0xFFFFFFFFu : 0u; cmax[q] = 0u; }
#pragma unroll
        for (int j = 0; j < QQ; ++j) { bs_step(r, h1[j], h0[j]); bs_max(cmax, r); }
#pragma unroll
        for (int q = 0; q < BS_NB; ++q) s_tail[(2 * BS_NB + q) * 64 + lane] = cmax[q];
    }
    if (SOLO) __hip_atomic_store(ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);      // (all of it: row 0 is the last one computed)
}

// a barcode wave of a SOLO unit: rows [0, need) must have their dv planes (need = L + 1: the tail as well); null: no producer
__device__ __forceinline__ void bs_wait_rows(const u32* ready, int need) {
#ifdef QCAT_BS_NO_WAIT
    return;
#endif
    if (ready == nullptr) return;
    while (uni((int)__hip_atomic_load(ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) < need) __builtin_amdgcn_s_sleep(2);
}

// ... letters from memory: bit j of (l1, l0) = letter of column j (two more instructions per cell, both with a scalar source)
template <int PP, bool SOLO>
__device__ __forceinline__ void bs_shared_columns_dynamic(uint4* __restrict__ s_rows, u32* __restrict__ s_tail, int L, int lane, int wave,
                                                          u32 l1, u32 l0, u32* ready, const u32* hold, int npad, int cown) {
    bs_shared_columns<PP, SOLO>(s_rows, s_tail, L, lane, wave, [&](int j, u32 c1, u32 c0) {
        const u32 L1 = (u32)-(int)((l1 >> j) & 1u), L0 = (u32)-(int)((l0 >> j) & 1u);
        return bs_neq(c1, c0, L1, L0);
    }, ready, hold, npad, cown);
}
template <int QQ, bool SOLO>
__device__ __forceinline__ void bs_trailing_columns_dynamic(const uint4* __restrict__ s_rows, uint2* __restrict__ rp, u32* __restrict__ s_tail, int L, int lane,
                                                            int part, u32 l1, u32 l0, u32* ready, const u32* hold, int npad) {
    bs_trailing_columns<QQ, SOLO>(s_rows, rp, s_tail, L, lane, part, [&](int j, u32 c1, u32 c0) {
        const u32 L1 = (u32)-(int)((l1 >> j) & 1u), L0 = (u32)-(int)((l0 >> j) & 1u);
        return bs_neq(c1, c0, L1, L0);
    }, ready, hold, npad);
}

// ... letters as template constants (generated code: the two contexts of a target family)
template <int PP, unsigned S1, unsigned S0, bool SOLO>
__device__ __forceinline__ void bs_shared_columns_static(uint4* __restrict__ s_rows, u32* __restrict__ s_tail, int L, int lane, int wave, u32* ready,
                                                         const u32* hold, int npad, int cown) {
    bs_shared_columns<PP, SOLO>(s_rows, s_tail, L, lane, wave, [&](int j, u32 c1, u32 c0) {
        return bs_neq_letter((int)((S1 >> j) & 1u) * 2 + (int)((S0 >> j) & 1u), c1, c0);
    }, ready, hold, npad, cown);
}
template <int QQ, unsigned T1, unsigned T0, bool SOLO>
__device__ __forceinline__ void bs_trailing_columns_static(const uint4* __restrict__ s_rows, uint2* __restrict__ rp, u32* __restrict__ s_tail, int L, int lane,
                                                           int part, u32* ready, const u32* hold, int npad) {
    bs_trailing_columns<QQ, SOLO>(s_rows, rp, s_tail, L, lane, part, [&](int j, u32 c1, u32 c0) {
        return bs_neq_letter((int)((T1 >> j) & 1u) * 2 + (int)((T0 >> j) & 1u), c1, c0);
    }, ready, hold, npad);
}

__device__ __forceinline__ void bs_setprio(int p) {                    // (the priority is an immediate)
    switch (p) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// the rows of one barcode.  Two rows per pass, the lower one a column behind the upper one: cell (i, j) and cell
// (i + 1, j - 1) do not depend on each other, so the in-order VALU always has a second dependency chain to issue from.
// NEQ(j, c1, c0): mismatch mask of own column j against a row's letter planes.  The last own cell of a row feeds the
// deficit of G(i) = H(i, c) + R(L - i, Q) together with the row's plane pair of the trailing columns (bs_deficit_split).
// what a barcode's row loop is given (one struct: the generated kernels pass it through).  SHARED (a template parameter of
// the row loops: the generated kernels know it, the letters-from-memory kernels switch on it once per barcode): the set has
// shared columns -- dv + 1 left of the first own column comes from the rows
struct BsRowArgs {
    const uint4* rows;                          // LDS rows of the unit
    int L, lane;
    const u32* ready;                           // a SOLO unit's progress word (bs_shared_columns); null: the planes are complete
    int nact;                                   // waves of this wave's SIMD that walk barcodes in this unit (1..4): the priority rotation's period
    const uint2* rp;                            // global: per row and lane dv + 1 of the trailing columns' last column (bs_trailing_columns)
    const u32* ready_r;                         // a SOLO unit's flag "rp and the trailing tail are complete"; null: they are
    int npad;                                   // units of the "short of nominal" class: rows in which some alignments have not started yet,
    const u32* hold;                            // and who (LDS, [row][lane]); 0: none
};

template <int C, bool PAIRS, bool SHARED, class NEQ>
__device__ __forceinline__ void bs_rows(const BsRowArgs& ra, NEQ neq, u32 (&h1)[C], u32 (&h0)[C], u32 (&f)[BS_ND]) {
    const uint4* __restrict__ s_rows = ra.rows;
    const uint2* __restrict__ rp = ra.rp + ra.lane;
    const int L = ra.L, lane = ra.lane;
    constexpr bool shared = SHARED;
    const u32* ready = ra.ready;
    int i = 0;
    bs_wait_rows(ra.ready_r, 1);
    // units of the "short of nominal" class: their first ra.npad rows one by one -- after a row the alignments that have not
    // started go back to the boundary state (bs_core.h: bs_hold; their r is 0 there, so their deficit stays 0)
    for (; i < ra.npad; ++i) {
        bs_wait_rows(ready, i + 1);
        const uint4 v = s_rows[i * 64 + lane];
        const uint2 rv = rp[i * 64];
        const u32 hm = ra.hold[i * 64 + lane];
        u32 a1 = shared ? v.z : 0u, a0 = shared ? v.w : 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < C; ++j) bs_cell(neq(j, v.x, v.y), a1, a0, h1[j], h0[j]);
#pragma unroll
        for (int j = 0; j < C; ++j) bs_hold(h1[j], h0[j], hm);
        bs_deficit_split(f, a1, a0, rv.x, rv.y);
    }
    if (!PAIRS) {                                                       // one row per pass: half the code
        bs_wait_rows(ready, i + 1);
        uint4 v = s_rows[i * 64 + lane];
        uint2 rv = rp[i * 64];
        for (; i < L; ++i) {
            bs_wait_rows(ready, min(i + 2, L));
            const uint4 nv = s_rows[min(i + 1, L - 1) * 64 + lane];
            const uint2 nrv = rp[min(i + 1, L - 1) * 64];
            u32 a1 = shared ? v.z : 0u, a0 = shared ? v.w : 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < C; ++j) bs_cell(neq(j, v.x, v.y), a1, a0, h1[j], h0[j]);
            bs_deficit_split(f, a1, a0, rv.x, rv.y);
            v = nv; rv = nrv;
        }
        return;
    }
    if ((L - i) & 1) {                                                  // an odd row count: the first row alone
        bs_wait_rows(ready, i + 1);
        const uint4 v = s_rows[i * 64 + lane];
        const uint2 rv = rp[i * 64];
        u32 a1 = shared ? v.z : 0u, a0 = shared ? v.w : 0xFFFFFFFFu;   // dv + 1 left of the first own column (column 0: H(i, 0) = 0)
#pragma unroll
        for (int j = 0; j < C; ++j) bs_cell(neq(j, v.x, v.y), a1, a0, h1[j], h0[j]);
        bs_deficit_split(f, a1, a0, rv.x, rv.y);                        // G(i) = G(i - 1) + dv(i, c) - dvR
        ++i;
    }
    if (i >= L) return;
    bs_wait_rows(ready, min(i + 2, L));
    uint4 v = s_rows[i * 64 + lane], w = s_rows[(i + 1) * 64 + lane];
    uint2 rv = rp[i * 64], rw = rp[(i + 1) * 64];
    const int rank = uni((int)(threadIdx.x >> 8));                      // the wave's place among the waves of its SIMD (round robin); scalar:
                                                                        // the rotation below is a scalar switch, not a walk through exec masks
    const int nact = QCAT_BS_ROTATE_BY_WAVES ? ra.nact : 4;
    int pr = rank < nact ? rank : 0;
    for (; i < L; i += 2) {
        // the VALU serves the highest priority first, then the oldest wave: without this rotation the old waves of a
        // SIMD run ahead, wait at the unit's barrier, and the young ones finish two to a SIMD (85 % of the issue rate).
        // (Round 4, measured and not kept -- QCAT_BS_ROTATE_BY_WAVES: a period equal to the barcode waves of the SIMD, three for a
        // 12-barcode unit.  With the period of four one wave is on top twice as often as the others and the three finish
        // 250-370 k cycles into a unit; with a period of three they finished 235-408 k: the oldest wave wins more, not less.)
#ifndef QCAT_BS_NO_ROTATE
        bs_setprio(pr);
#endif
        pr = pr + 1 == nact ? 0 : pr + 1;
        const int nx = min(i + 2, L - 2);                               // the next pair is on its way while this one is computed
        bs_wait_rows(ready, nx + 2);
        const uint4 nv = s_rows[nx * 64 + lane], nw = s_rows[(nx + 1) * 64 + lane];
        const uint2 nrv = rp[nx * 64], nrw = rp[(nx + 1) * 64];
        u32 a1 = shared ? v.z : 0u, a0 = shared ? v.w : 0xFFFFFFFFu;
        u32 b1 = shared ? w.z : 0u, b0 = shared ? w.w : 0xFFFFFFFFu;
        bs_cell(neq(0, v.x, v.y), a1, a0, h1[0], h0[0]);
#pragma unroll
        for (int j = 1; j < C; ++j) {
            bs_cell(neq(j, v.x, v.y), a1, a0, h1[j], h0[j]);
            bs_cell(neq(j - 1, w.x, w.y), b1, b0, h1[j - 1], h0[j - 1]);
        }
        bs_cell(neq(C - 1, w.x, w.y), b1, b0, h1[C - 1], h0[C - 1]);
        bs_deficit_split(f, a1, a0, rv.x, rv.y);
        bs_deficit_split(f, b1, b0, rw.x, rw.y);
        v = nv; w = nw; rv = nrv; rw = nrw;
    }
}

// ... letters from memory: bit j of (l1w, l0w) = letter of own column j
template <int C, bool SHARED>
__device__ __forceinline__ void bs_rows_dynamic(const BsRowArgs& ra, unsigned long long l1w, unsigned long long l0w,
                                                u32 (&h1)[C], u32 (&h0)[C], u32 (&f)[BS_ND]) {
    bs_rows<C, true, SHARED>(ra, [&](int j, u32 c1, u32 c0) {
        const u32 L1 = (u32)-(int)((l1w >> j) & 1ull), L0 = (u32)-(int)((l0w >> j) & 1ull);       // scalar 0 / ~0
        return bs_neq(c1, c0, L1, L0);
    }, h1, h0, f);
}

// ... letters as template constants (generated code: static_generated.inc, jit.py): a column names one of the four
// mismatch masks a row has (c1 c0 != l1 l0 for the letters 0..3); the optimiser forms each mask once per row
template <int C, bool SHARED, unsigned long long W1, unsigned long long W0>
__device__ __forceinline__ void bs_rows_static(const BsRowArgs& ra, u32 (&h1)[C], u32 (&h0)[C], u32 (&f)[BS_ND]) {
    bs_rows<C, BS_STATIC_PAIRS, SHARED>(ra, [&](int j, u32 c1, u32 c0) {
        return bs_neq_letter((int)((W1 >> j) & 1ull) * 2 + (int)((W0 >> j) & 1ull), c1, c0);
    }, h1, h0, f);
}

struct BsArgs {                                // one struct: run-time generated kernels are launched with a single parameter
    KitPtrs kp;
    const uint8_t* tilebuf;
    BsPlan* bp;
    BsNch nch;
    u32* keys;
    uint32_t key_stride;
    int slot;
    int use_static;                            // 0: every group on the letters-from-memory kernels (A/B tests)
    unsigned long long* trace;                 // diagnostics (QCAT_HIP_BS_TRACE): s_memtime of workgroup 0's waves at the phase
                                               // boundaries of its first units, [unit < 8][wave][event < 8]; null: off
    const uint32_t* win;                       // the read ends' windows at two bits per code (k_pack_windows: win2): the regions are read in place
    const uint32_t* jobinfo;                   // through the sorted job list (k_job_gather leaves the super-tiles' images out); null: from tile images
    const int32_t* sorted;
    int nsets;
    int use_solo;                              // units with an idle wave let it produce the shared columns beside the row loops (0: A/B runs)
    uint2* rplanes;                            // [launch slot][workgroup][BS_MAX_ROWS][64]: the trailing columns' plane pairs of the unit a workgroup
                                               // is working on (bs_trailing_columns)
    int trace_wg, trace_seq;                   // diagnostics: the workgroup whose stamps are taken, from its trace_seq-th unit on
    int draw;                                  // 1: the waves of a workgroup DRAW the unit's barcodes from a counter in the LDS instead of taking them
                                               // round robin (round 6: the VALU's arbiter favours the old waves of a SIMD whatever the priorities say --
                                               // with six barcodes each the four waves of a SIMD finished at 0.70 / 0.74 / 0.84 / 0.98 of the row phase,
                                               // drawn they finish at 0.90 .. 0.98 and a unit takes 10 % fewer cycles; the launch time hardly moves --
                                               // the kernel runs at a constant instruction rate, profiles/r06_ab_draw_pipe.txt)
};
constexpr int BS_TRACE_STAMPS = 8 * 8 * BS_WAVES * 8;        // [launch slot][unit][wave][event] stamps, then the unit log: count, entries of 4
constexpr int BS_TRACE_LOG = 4096;
#define BS_STAMP(EV) do { if (args.trace && (int)blockIdx.x == args.trace_wg && seq >= args.trace_seq && seq < args.trace_seq + 8 && lane == 0) \
        args.trace[(((size_t)args.slot * 8 + (seq - args.trace_seq)) * BS_WAVES + wave) * 8 + (EV)] = __builtin_amdgcn_s_memtime(); } while (0)

template <int CC> struct BsDyn { static constexpr int C = CC; static constexpr int KERNEL = -1; };

// the trailing context's columns of a unit on this wave; `part`: its share of the row stores (SOLO: all of them)
template <class G, bool SOLO>
__device__ __forceinline__ void bs_trailing_of(const uint4* __restrict__ s_rows, uint2* __restrict__ rp, u32* __restrict__ s_tail, int L, int lane,
                                               int part, int Q, u32 tl1, u32 tl0, u32* rdy, const u32* hold, int npad) {
    if constexpr (G::KERNEL >= 0) {
        bs_trailing_columns_static<G::POST, G::T1, G::T0, SOLO>(s_rows, rp, s_tail, L, lane, part, rdy, hold, npad);
    } else {
        switch (Q) {                                 // (kit_prepare.inc: bs_post is one of these)
        case 4: bs_trailing_columns_dynamic<4, SOLO>(s_rows, rp, s_tail, L, lane, part, tl1, tl0, rdy, hold, npad); break;
        case 6: bs_trailing_columns_dynamic<6, SOLO>(s_rows, rp, s_tail, L, lane, part, tl1, tl0, rdy, hold, npad); break;
        case 7: bs_trailing_columns_dynamic<7, SOLO>(s_rows, rp, s_tail, L, lane, part, tl1, tl0, rdy, hold, npad); break;
        case 8: bs_trailing_columns_dynamic<8, SOLO>(s_rows, rp, s_tail, L, lane, part, tl1, tl0, rdy, hold, npad); break;
        case 11: bs_trailing_columns_dynamic<11, SOLO>(s_rows, rp, s_tail, L, lane, part, tl1, tl0, rdy, hold, npad); break;
        default: bs_trailing_columns_dynamic<0, SOLO>(s_rows, rp, s_tail, L, lane, part, tl1, tl0, rdy, hold, npad); break;
        }
    }
}

struct BsUnitMeta {                               // a decoded unit (bs_decode_unit)
    int state;
    int bin, chunk, n_ch, L, npad, b0, b1;
    uint32_t pos0, u;
};

// which (super-tile, chunk) is unit u, and is it one of kernel G's?  (k_bs_plan's segments)
template <class G>
__device__ __forceinline__ bool bs_decode_unit(const BsArgs& args, uint32_t u, BsUnitMeta& m) {
    const BsPlan* __restrict__ bp = args.bp;
    const DevKit* __restrict__ k = args.kp.kit;
    const uint32_t n_seg = bp->n_seg;
    uint32_t seg = 0;
    for (uint32_t q = 1; q < n_seg; ++q) if (bp->seg_prefix[q] <= u) seg = q;
    const int bin = uni((int)bp->seg_bin[seg]);
    const int gidx = bin / JOB_CLASSES;
    const DevSet& bs = k->tpl[gidx >> 1].sets[gidx & 1];
    const int P = uni(bs.bs_pre), Q = uni(bs.bs_post);
    const int sk = args.use_static ? uni(bs.bs_kernel) : -1;
    if (G::KERNEL >= 0 ? sk != G::KERNEL : (sk >= 0 || uni(bs.tlen) - P - Q != G::C)) return false;
    const uint32_t local = u - bp->seg_prefix[seg];
    uint32_t st_local;
    {   // the bin's first super-tiles carry the group's chunk count, its last `split` ones twice that (k_bs_plan)
        const int n_lo = args.nch.v[gidx], n_hi = bs_chunks_hi(n_lo);
        const uint32_t whole_st = bp->count[bin] - bp->split[bin], whole_units = whole_st * (uint32_t)n_lo;
        if (local < whole_units) { st_local = local / (uint32_t)n_lo; m.chunk = (int)(local % (uint32_t)n_lo); m.n_ch = n_lo; }
        else { const uint32_t l2 = local - whole_units; st_local = whole_st + l2 / (uint32_t)n_hi; m.chunk = (int)(l2 % (uint32_t)n_hi); m.n_ch = n_hi; }
    }
    m.state = 1; m.bin = bin; m.u = u;
    m.L = (int)bp->len[bin];
    m.npad = bin % JOB_CLASSES == JOB_CLASSES - JOB_HOT ? BS_PAD_ROWS : 0;      // the "short of nominal" class: alignments start up to npad rows late
    const int B = uni(bs.n);
    const int per = (B + m.n_ch - 1) / m.n_ch;
    m.b0 = m.chunk * per; m.b1 = min(B, m.b0 + per);
    m.pos0 = bp->first[bin] + st_local * BS_JOBS;
    return true;
}

// ---------------------------------------------------------------------------------------------
// k_bs_barcode<G>: persistent 16-wave workgroups (one per CU: the LDS rows fill the CU) pull (super-tile, barcode chunk)
// units.  Per unit: planes into the LDS, the shared columns, then per barcode of a wave: L rows of C columns, the
// last-column deficit on the way, the last row at the end, raw = max of both (scanner_base.py:63-141 with R1's score);
// per alignment the best (raw, smallest index) over the chunk leaves as one key (kernels_packed.inc, barcode_key).
// G = BsDyn<C> (letters from memory, every group with C own columns) or a generated QBS_n (one target family).
// ---------------------------------------------------------------------------------------------
template <class G>
__device__ __forceinline__ void bs_barcode_body(const BsArgs& args) {
    constexpr int C = G::C;
    __shared__ uint4 s_rows[BS_MAX_ROWS * 64];                  // per row and lane: c1, c0, dv + 1 at the last shared column
    __shared__ u32 s_tail[3 * BS_NB * 64];                      // last row after the shared columns: H(L,P) + 64 - C, the row maximum's deficit (BS_NE planes); maximum of the trailing columns' last row
    __shared__ u32 s_unit;
    __shared__ u32 s_draw;                                      // next barcode of the unit (BsArgs::draw)
    __shared__ u32 s_ready;                                     // a SOLO unit's shared-column progress (bs_shared_columns)
    __shared__ u32 s_ready_r;                                   // ... and "the trailing columns are done" (bs_trailing_columns)
    static_assert(BS_PAD_ROWS * 64 <= BS_WAVES * 64, "one thread clears one word of s_hold");
    __shared__ u32 s_hold[BS_PAD_ROWS * 64];                    // units of the "short of nominal" class: per row < BS_PAD_ROWS the alignments that have not started
    const KitPtrs& kp = args.kp;
    const uint8_t* __restrict__ tilebuf = args.tilebuf;
    BsPlan* __restrict__ bp = args.bp;
    u32* __restrict__ keys = args.keys;
    const uint32_t key_stride = args.key_stride;
    const DevKit* __restrict__ k = kp.kit;
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    uint2* __restrict__ rp = args.rplanes + ((size_t)args.slot * gridDim.x + blockIdx.x) * (size_t)(BS_MAX_ROWS * 64);
    const uint32_t n_seg = bp->n_seg, n_units = bp->seg_prefix[n_seg];
    int seq = 0;                                                 // (diagnostics: own units taken so far)
    for (;;) {
        __syncthreads();                                         // the previous unit's keys have left the LDS
        BS_STAMP(0);
        if (tid == 0) { s_unit = atomicAdd(&bp->cursor[args.slot][0], 1u); s_ready = 0u; s_ready_r = 0u; s_draw = 0u; }
        if (tid < BS_PAD_ROWS * 64) s_hold[tid] = 0u;
        __syncthreads();
        const uint32_t u = (uint32_t)uni((int)s_unit);
        if (u >= n_units) break;
        BsUnitMeta m;
        if (!bs_decode_unit<G>(args, u, m)) continue;                // whose unit is it?
        const int bin = m.bin, chunk = m.chunk, n_ch = m.n_ch, L = m.L, npad = m.npad, b0 = m.b0, b1 = m.b1;
        const uint32_t pos0 = m.pos0;
        const unsigned long long t_unit0 = args.trace ? __builtin_amdgcn_s_memtime() : 0ull;
        const int gidx = bin / JOB_CLASSES;
        const DevSet& bs = k->tpl[gidx >> 1].sets[gidx & 1];
        const int P = uni(bs.bs_pre), Q = uni(bs.bs_post);
        const int32_t* __restrict__ bits = kp.ids + uni(bs.bs_off);    // per barcode: letter bit 1 (lo, hi), letter bit 0 (lo, hi)
        const int32_t* __restrict__ kases = kp.ids + uni(bs.bs_case_off);
        BS_STAMP(1);
        {   // letter planes into the LDS, in the order the rows are walked: a slice of 64 alignments is one nibble half of
            // an ordinary tile image (lane = alignment, 16 rows per 16-byte load, two ballots per row)
            const bool rev = uni(bs.bs_rev) != 0;
            u32* __restrict__ dst = reinterpret_cast<u32*>(s_rows);
#ifndef QCAT_BS_NO_NEWT
            if (args.win) {
                // from the windows at two bits per code, through the sorted job list (round 4: a bit-matrix transposition in
                // registers instead of two ballots per row and slice -- 58-75 k of a 485 k-cycle unit of config 2 before).
                // Pass 1: where every alignment's region starts (read end, first code), parked in the dv half of LDS rows
                // 0..31 (free until the shared columns): slot k * 64 + l = alignment pos0 + 32 l + k.
                // Pass 2: a wave owns BS_TL plane lanes; its hardware lane h works for plane lane l = BS_TL wave + h / BS_TG
                // on row block g = h % BS_TG (16 rows): it fetches the two dwords that hold those rows of each of l's 32
                // alignments -- the BS_TG lanes of one l read neighbouring dwords of the same windows, so an instruction
                // touches BS_TL windows, not 64 -- funnel-shifts the region into place, transposes the 32 x 32 bit matrix
                // (16 codes x 2 bits of 32 alignments -> plane words c0, c1 of 16 rows) and stores l's words of its rows.
                static_assert(64 % BS_WAVES == 0, "plane lanes are split evenly over the waves");
                constexpr int BS_TL = 64 / BS_WAVES, BS_TG = 64 / BS_TL;              // plane lanes per wave, row blocks per wave pass
                static_assert(BS_TG * 16 >= BS_MAX_ROWS, "one pass covers every row");
                const uint32_t covered = uni((int)(bp->first[bin] + bp->cov[bin] - pos0));   // jobs of this super-tile (2048 unless padded)
                for (int q = tid; q < BS_JOBS; q += BS_WAVES * 64) {
                    const int32_t job = args.sorted[pos0 + ((uint32_t)q < covered ? (uint32_t)q : 0u)];
                    const u32 ji = args.jobinfo[job];
                    u32 start = ji >> 16;
                    if (npad) {
                        // a region `pad` rows short of the unit starts `pad` rows late: forward sets fetch from `pad` bases in front of
                        // it (whatever is there: held rows are never looked at; the start may become negative), reversed sets walk
                        // their rows backwards, so the bases behind the region land in front of the walk by themselves
                        const int pad = L - (int)(ji & 0xFFu);
                        if (!rev) start = (u32)((int)start - pad) & 0xFFFFu;
                        for (int i = 0; i < pad; ++i) atomicOr(&s_hold[i * 64 + (q >> 5)], 1u << (q & 31));
                    }
                    *(reinterpret_cast<uint2*>(&s_rows[(q & 31) * 64 + (q >> 5)]) + 1) = make_uint2((u32)job / (u32)args.nsets, start);
                }
                __syncthreads();
                {
                    const int pl = wave * BS_TL + lane / BS_TG, g = lane % BS_TG;
                    if (g * 16 < L) {
                        u32 v[32];
                        // (sixteen alignments' loads in flight at a time: all 32 -- 64 data and 64 address registers -- spill)
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            u32 lo[16], hi[16];
#pragma unroll
                            for (int kk = 0; kk < 16; ++kk) {
                                const uint2 es = *(reinterpret_cast<const uint2*>(&s_rows[(half * 16 + kk) * 64 + pl]) + 1);
                                const int fs = (int)(int16_t)(uint16_t)es.y;               // first base of the unit's row 0 in the window (padded classes: may be < 0)
                                const uint32_t* __restrict__ src2 = args.win + ((long long)es.x * WIN2_WORDS + (fs >> 4) + g);   // (fs < 0: the dword in front -- the buffer has front slack)
                                lo[kk] = src2[0]; hi[kk] = src2[1];
                                v[half * 16 + kk] = ((u32)fs & 15u) * 2u;
                            }
#pragma unroll
                            for (int kk = 0; kk < 16; ++kk) v[half * 16 + kk] = __builtin_amdgcn_alignbit(hi[kk], lo[kk], v[half * 16 + kk]);
                            asm volatile("" ::: "memory");
                        }
                        bs_transpose32(v);
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int i = g * 16 + q;
                            if (i < L) {
                                const int row = rev ? L - 1 - i : i;
                                *reinterpret_cast<uint2*>(dst + (row * 64 + pl) * 4) = make_uint2(v[2 * q + 1], v[2 * q]);
                            }
                        }
                    }
                }
            } else
#endif
            for (int sl = wave; sl < BS_JOBS / 64; sl += BS_WAVES) {
#ifdef QCAT_BS_NO_NEWT
                if (args.win) {
                    // (round 3's form, kept for A/B builds: lane = alignment, two ballots per row and slice)
                    const int32_t job = args.sorted[pos0 + (uint32_t)sl * 64u + (uint32_t)lane];
                    const u32 start = args.jobinfo[job] >> 16;
                    const uint32_t* __restrict__ src4 = args.win + (size_t)((uint32_t)job / (uint32_t)args.nsets) * WIN2_WORDS + (start >> 4);
                    const u32 shb = (start & 15u) * 2u;
                    for (int h0 = 0; h0 < L; h0 += 80) {
                        u32 raw[6];
#pragma unroll
                        for (int c = 0; c < 6; ++c) raw[c] = src4[h0 / 16 + c];
#pragma unroll
                        for (int c = 0; c < 5; ++c) {
                            const u32 v = __builtin_amdgcn_alignbit(raw[c + 1], raw[c], shb);
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const int i = h0 + c * 16 + q;
                                if (i < L) {
                                    const u32 c2 = v >> (2 * q);
                                    const unsigned long long m1 = __builtin_amdgcn_ballot_w64((c2 & 2u) != 0);
                                    const unsigned long long m0 = __builtin_amdgcn_ballot_w64((c2 & 1u) != 0);
                                    if (lane < 2) {
                                        const int row = rev ? L - 1 - i : i;
                                        *reinterpret_cast<uint2*>(dst + (row * 64 + 2 * sl + lane) * 4) =
                                            make_uint2((u32)(lane ? m1 >> 32 : m1), (u32)(lane ? m0 >> 32 : m0));
                                    }
                                }
                            }
                        }
                    }
                    continue;
                }
#endif
                const uint8_t* __restrict__ src = tilebuf + ((size_t)(pos0 / PK_TILE + (uint32_t)(sl >> 1)) * 64 + lane) * WIN_STRIDE;
                const int sh = (sl & 1) * 4;
                for (int h0 = 0; h0 < L; h0 += 80) {                   // five loads in flight: a memory round trip per 80 rows
                    uint4 img[5];
#pragma unroll
                    for (int c = 0; c < 5; ++c) img[c] = reinterpret_cast<const uint4*>(src + h0)[c];
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        const int i0 = h0 + c * 16;
                        const u32 v[4] = {img[c].x, img[c].y, img[c].z, img[c].w};
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            if (i0 + q < L) {
                                const u32 c2 = v[q >> 2] >> (8 * (q & 3) + sh);
                                const unsigned long long m1 = __builtin_amdgcn_ballot_w64((c2 & 2u) != 0);
                                const unsigned long long m0 = __builtin_amdgcn_ballot_w64((c2 & 1u) != 0);
                                if (lane < 2) {                         // the ballots' words belong to plane lanes 2 sl, 2 sl + 1
                                    const int row = rev ? L - 1 - (i0 + q) : i0 + q;
                                    *reinterpret_cast<uint2*>(dst + (row * 64 + 2 * sl + lane) * 4) =
                                        make_uint2((u32)(lane ? m1 >> 32 : m1), (u32)(lane ? m0 >> 32 : m0));
                                }
                            }
                        }
                    }
                }
            }
        }
        BS_STAMP(2);
        __syncthreads();
        BS_STAMP(3);
        // a unit with two waves to spare: they are the producers of the two contexts' columns, nobody waits for the leading one (SOLO)
        const bool solo = P != 0 && (b1 - b0) <= BS_WAVES - 2 && args.use_solo != 0;
        u32 tl1 = 0u, tl0 = 0u;                                         // letters from memory: the trailing columns, last column first
        if constexpr (G::KERNEL < 0) {
            const int M = uni(bs.tlen);
            const unsigned long long w1 = (unsigned long long)(u32)uni(bits[4 * b0]) | ((unsigned long long)(u32)uni(bits[4 * b0 + 1]) << 32);
            const unsigned long long w0 = (unsigned long long)(u32)uni(bits[4 * b0 + 2]) | ((unsigned long long)(u32)uni(bits[4 * b0 + 3]) << 32);
            for (int j = 0; j < Q; ++j) { tl1 |= (u32)((w1 >> (M - 1 - j)) & 1ull) << j; tl0 |= (u32)((w0 >> (M - 1 - j)) & 1ull) << j; }
        }
        if (solo) {
            if (wave == BS_WAVES - 1) {
                __builtin_amdgcn_s_setprio(3);                            // (the barcode waves rotate through 0..3: the producer must not starve)
                if constexpr (G::KERNEL >= 0 && QCAT_BS_STATIC_SHARED) {
                    if constexpr (G::PRE > 0) bs_shared_columns_static<G::PRE, G::S1, G::S0, true>(s_rows, s_tail, L, lane, wave, &s_ready, s_hold, npad, C);
                } else {
                    const u32 l1 = (u32)uni(bits[4 * b0]), l0 = (u32)uni(bits[4 * b0 + 2]);
                    switch (P) {
                    case 4: bs_shared_columns_dynamic<4, true>(s_rows, s_tail, L, lane, wave, l1, l0, &s_ready, s_hold, npad, C); break;
                    case 8: bs_shared_columns_dynamic<8, true>(s_rows, s_tail, L, lane, wave, l1, l0, &s_ready, s_hold, npad, C); break;
                    default: bs_shared_columns_dynamic<11, true>(s_rows, s_tail, L, lane, wave, l1, l0, &s_ready, s_hold, npad, C); break;
                    }
                }
                __builtin_amdgcn_s_setprio(0);
            } else if (wave == BS_WAVES - 2) {
                // the trailing columns come out last row first, so the barcode waves need all of them before their first row:
                // ~50 instructions per row at the top priority against ~200 per row and barcode afterwards
                __builtin_amdgcn_s_setprio(3);
                bs_trailing_of<G, true>(s_rows, rp, s_tail, L, lane, 0, Q, tl1, tl0, &s_ready_r, s_hold, npad);
                __builtin_amdgcn_s_setprio(0);
            }
            BS_STAMP(4);
            BS_STAMP(5);
        } else {
            if (wave < BS_PRE_WAVES) {
                bool done = false;
                if constexpr (G::KERNEL >= 0 && QCAT_BS_STATIC_SHARED) {     // the family's leading context is a compile-time constant
                    if constexpr (G::PRE > 0) { bs_shared_columns_static<G::PRE, G::S1, G::S0, false>(s_rows, s_tail, L, lane, wave, nullptr, s_hold, npad, C); done = true; }
                } else {
                    const u32 l1 = (u32)uni(bits[4 * b0]), l0 = (u32)uni(bits[4 * b0 + 2]);     // the shared columns: any barcode's
                    switch (P) {
                    case 4: bs_shared_columns_dynamic<4, false>(s_rows, s_tail, L, lane, wave, l1, l0, nullptr, s_hold, npad, C); done = true; break;
                    case 8: bs_shared_columns_dynamic<8, false>(s_rows, s_tail, L, lane, wave, l1, l0, nullptr, s_hold, npad, C); done = true; break;
                    case 11: bs_shared_columns_dynamic<11, false>(s_rows, s_tail, L, lane, wave, l1, l0, nullptr, s_hold, npad, C); done = true; break;
                    default: break;
                    }
                }
                if (!done && wave == 0) {                                  // no shared columns: bs_last_row_start with P = 0
#pragma unroll
                    for (int q = 0; q < BS_NB; ++q) { s_tail[q * 64 + lane] = ((BS_OFF - C) >> q) & 1 ? 0xFFFFFFFFu : 0u; s_tail[(BS_NB + q) * 64 + lane] = 0u; }
                }
            } else if (wave < 2 * BS_PRE_WAVES) {
                bs_trailing_of<G, false>(s_rows, rp, s_tail, L, lane, wave - BS_PRE_WAVES, Q, tl1, tl0, nullptr, s_hold, npad);    // (wave w and wave w + 4 share a SIMD: one context each)
            }
            BS_STAMP(4);
            __syncthreads();
            BS_STAMP(5);
        }
        const int nb_waves = min(BS_WAVES, b1 - b0);                       // waves that walk barcodes: wave w sits on SIMD w % 4
        const BsRowArgs ra{s_rows, L, lane, solo ? &s_ready : nullptr, max(1, (nb_waves - (wave & 3) + 3) / 4), rp, solo ? &s_ready_r : nullptr, npad, s_hold};

        u32 bestv[BS_NB], besti[BS_NB];
#pragma unroll
        for (int q = 0; q < BS_NB; ++q) { bestv[q] = 0u; besti[q] = 0u; }   // value 0 = H of -64: below every score
        // a wave's barcodes come in increasing index order either way (the counter only grows)
        const bool draw = args.draw != 0 && (b1 - b0) >= 2 * BS_WAVES;      // (a small set's unit has a barcode per wave or less: nothing to even out)
        auto bs_next = [&](int prev) -> int {
            if (!draw) return prev < 0 ? b0 + wave : prev + BS_WAVES;
            u32 t = 0u;
            if (lane == 0) t = atomicAdd(&s_draw, 1u);
            return b0 + uni((int)t);
        };
        bool had = false;                                              // this wave walked a barcode of the unit
        for (int b = bs_next(-1); b < b1; b = bs_next(b)) {
            had = true;
            u32 h1[C], h0[C];                                          // dh + 1 per column: row 0 is all zeros -> code 1
#pragma unroll
            for (int j = 0; j < C; ++j) { h1[j] = 0u; h0[j] = 0xFFFFFFFFu; }
            u32 f[BS_ND];                                              // the deficit of G(i) = H(i, c) + R(L - i, Q): G(0) is the first candidate
#pragma unroll
            for (int q = 0; q < BS_ND; ++q) f[q] = 0u;
            if constexpr (G::KERNEL >= 0) {
                G::rows(uni(kases[b]), ra, h1, h0, f);
            } else {
                const unsigned long long l1w = ((unsigned long long)(u32)uni(bits[4 * b]) | ((unsigned long long)(u32)uni(bits[4 * b + 1]) << 32)) >> P;
                const unsigned long long l0w = ((unsigned long long)(u32)uni(bits[4 * b + 2]) | ((unsigned long long)(u32)uni(bits[4 * b + 3]) << 32)) >> P;
                if (P != 0) bs_rows_dynamic<C, true>(ra, l1w, l0w, h1, h0, f);
                else bs_rows_dynamic<C, false>(ra, l1w, l0w, h1, h0, f);
            }
            // last row: raw = max(H(L, c) + deficit, the last row's maximum, the trailing columns' own maximum) (bs_core.h)
            // (round 7: the row maximum as a deficit and H(L, c) as one carry-save sum of the codes instead of a counter step and a
            // maximum per column -- bs_core.h: bs_last_row)
            u32 rowbest[BS_NB];
            bs_wait_rows(ra.ready, L + 1);                               // (SOLO: the producer's tail)
            const auto tail = [&](int q) { return s_tail[q * 64 + lane]; };
            if constexpr (G::KERNEL >= 0) {
                bs_last_row<C, G::PRE != 0>(rowbest, h1, h0, tail, f);
            } else {
                if (P != 0) bs_last_row<C, true>(rowbest, h1, h0, tail, f);
                else bs_last_row<C, false>(rowbest, h1, h0, tail, f);
            }
            // keep (raw, smallest index): a wave's barcodes come in increasing index order, so strictly greater replaces
            const u32 gt = bs_gt(rowbest, bestv);
#pragma unroll
            for (int q = 0; q < BS_NB; ++q) {
                bestv[q] = bs_bfi(gt, rowbest[q], bestv[q]);
                besti[q] = bs_bfi(gt, (b >> q) & 1 ? 0xFFFFFFFFu : 0u, besti[q]);
            }
        }
        // un-transpose: one key per alignment, the maximum over the waves through the LDS
        BS_STAMP(6);
        __syncthreads();
        BS_STAMP(7);
        ++seq;
        if (args.trace && tid == 0) {                               // (diagnostics: one line per unit -- who ran what, when)
            unsigned long long* lg = args.trace + BS_TRACE_STAMPS;
            const unsigned long long slot_ = atomicAdd(lg, 1ull);
            if (slot_ < BS_TRACE_LOG) {
                unsigned long long* e = lg + 1 + slot_ * 4;
                e[0] = ((unsigned long long)args.slot << 56) | ((unsigned long long)bin << 40) | ((unsigned long long)n_ch << 32) | ((unsigned long long)chunk << 24) | blockIdx.x;
                e[1] = t_unit0; e[2] = __builtin_amdgcn_s_memtime(); e[3] = (unsigned long long)L;
            }
        }
        u32* __restrict__ s_keys = reinterpret_cast<u32*>(s_rows);      // [bit][lane]
        for (int q = tid; q < BS_JOBS; q += BS_WAVES * 64) s_keys[q] = 0u;
        __syncthreads();
        if (had) {
            // (round 7: the keys are a bit-matrix transposition of the planes -- bs_core.h: bs_keys32 -- not 14 bits picked per alignment)
            static_assert(BS_OFF == 64 && BS_NB == 7, "bs_keys32 spells barcode_key(raw, b) out in planes");
            u32 key[32];
            bs_keys32(key, bestv, besti);
#pragma unroll
            for (int bit = 0; bit < 32; ++bit) atomicMax(&s_keys[bit * 64 + lane], key[bit]);
        }
        __syncthreads();
        {
            u32* __restrict__ dst = keys + (size_t)chunk * key_stride + pos0;
            const int covered = (int)min((uint32_t)BS_JOBS, uni((int)(bp->first[bin] + bp->cov[bin] - pos0)));    // (a padded super-tile: its jobs only)
            static_assert(BS_JOBS % (BS_WAVES * 64) == 0, "whole passes of the workgroup");
            // (a fixed trip count and an index the optimiser cannot see through: neither the loop's set-up nor the addresses it forms
            // from the thread index are hoisted out of the unit loop, where they would hold registers through every barcode's rows)
            int t = tid;
            asm volatile("" : "+v"(t));
#pragma unroll
            for (int pass = 0; pass < BS_JOBS / (BS_WAVES * 64); ++pass) {
                const int q = t + pass * (BS_WAVES * 64);
                if (q < covered) dst[q] = s_keys[(q & 31) * 64 + (q >> 5)];
            }
        }
    }
}

template <class G>
__global__ void __launch_bounds__(BS_WAVES * 64)
k_bs_barcode(BsArgs args) { bs_barcode_body<G>(args); }

// ---------------------------------------------------------------------------------------------
// k_bs_select: per alignment of a super-tile, the maximum key over its units -> record fields; a best raw score of
// exactly 0 goes to the redo list (kernels_packed.inc: the one case in which R2 depends on the list order).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_bs_select(const DevKit* __restrict__ k, EndRec* __restrict__ recs, const int32_t* __restrict__ sorted, const BsPlan* __restrict__ bp,
            BsNch nch, int nsets, const u32* __restrict__ keys, uint32_t key_stride, u32* __restrict__ redo_list, u32* __restrict__ redo_count) {
    const uint32_t n_super = bp->tile_prefix[JOB_BINS];
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < (uint64_t)n_super * BS_JOBS; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t st = (uint32_t)(t / BS_JOBS), a = (uint32_t)(t % BS_JOBS);
        int bin = 0;
        for (int b = 1; b < JOB_BINS; ++b) if (bp->tile_prefix[b] <= st) bin = b;
        const int gidx = bin / JOB_CLASSES, set = gidx & 1;
        const uint32_t pos = bp->first[bin] + (st - bp->tile_prefix[bin]) * BS_JOBS + a;
        if (pos >= bp->first[bin] + bp->cov[bin]) continue;             // (a padded super-tile's empty slots)
        u32 best = 0;
        const int n_ch = bs_chunks_of(bp, bin, nch.v[gidx], st - bp->tile_prefix[bin]);
        for (int c = 0; c < n_ch; ++c) best = max(best, keys[(size_t)c * key_stride + pos]);
        const uint32_t e = (uint32_t)sorted[pos] / (uint32_t)nsets;
        const int raw = (int)(best >> 16) - 32768;
        recs[e].bc_idx[set] = 1023 - (int)(best & 0x3FFu);
        recs[e].bc_raw[set] = raw;
        if (raw == 0) {                                                // (tile, lane, half) of the ordinary tile image
            const uint32_t tile = pos / PK_TILE, within = pos % PK_TILE;
            redo_list[atomicAdd(redo_count, 1u)] = (u32)((((size_t)tile * 64 + (within & 63u)) << 1) | (within >> 6));
        }
    }
}

// the same in READ order (round 3): thread = job (read end x set), its sorted position comes from `posof` (k_job_scatter),
// its keys are gathered, and the result goes to the packed array `bcres` that k_finalize reads -- 8 bytes per job, coalesced,
// instead of 8 bytes scattered into 52-byte records (WRITE_SIZE 0.78 GB for 160 MB of payload per 10 M reads)
__global__ void __launch_bounds__(256)
k_bs_select_ordered(const uint32_t* __restrict__ jobinfo, const uint32_t* __restrict__ posof, uint32_t n_cand, const BsPlan* __restrict__ bp,
                    BsNch nch, const u32* __restrict__ keys, uint32_t key_stride, int2* __restrict__ bcres,
                    u32* __restrict__ redo_list, u32* __restrict__ redo_count) {
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < n_cand; id += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t ji = jobinfo[id];
        if (!ji) continue;
        const int bin = (int)((ji >> 8) & 0xFFu);
        if (bin % JOB_CLASSES < JOB_CLASSES - JOB_HOT) continue;       // not a hot class
        const uint32_t pos = posof[id], f = bp->first[bin];
        if (pos < f || pos >= f + bp->cov[bin]) continue;               // outside the super-tiles: the binary16 kernels' job
        const int gidx = bin / JOB_CLASSES;
        u32 best = 0;
        const int n_ch = bs_chunks_of(bp, bin, nch.v[gidx], (pos - f) / (uint32_t)BS_JOBS);
        for (int c = 0; c < n_ch; ++c) best = max(best, keys[(size_t)c * key_stride + pos]);
        const int raw = (int)(best >> 16) - 32768;
        bcres[id] = make_int2(1023 - (int)(best & 0x3FFu), raw);
        if (raw == 0) {
            const uint32_t tile = pos / PK_TILE, within = pos % PK_TILE;
            redo_list[atomicAdd(redo_count, 1u)] = (u32)((((size_t)tile * 64 + (within & 63u)) << 1) | (within >> 6));
        }
    }
}

#ifndef QCAT_RTC
static inline void launch_bs_static(int kernel, dim3 grid, hipStream_t stream, const BsArgs& a);    // static_generated.inc
// one instantiation per number of own columns (every launch walks all units and takes those of its width)
static inline void launch_bs_barcode(int c, dim3 grid, hipStream_t stream, const BsArgs& a) {
    switch (c) {
#define QB_CASE(CC) case CC: hipLaunchKernelGGL(k_bs_barcode<BsDyn<CC>>, grid, dim3(BS_WAVES * 64), 0, stream, a); break;
        QB_CASE(20) QB_CASE(21) QB_CASE(22) QB_CASE(23) QB_CASE(24) QB_CASE(25) QB_CASE(26) QB_CASE(27) QB_CASE(28) QB_CASE(29)
        QB_CASE(30) QB_CASE(31) QB_CASE(32) QB_CASE(33) QB_CASE(34) QB_CASE(35) QB_CASE(36) QB_CASE(37) QB_CASE(38) QB_CASE(39)
        QB_CASE(40) QB_CASE(41) QB_CASE(42) QB_CASE(43) QB_CASE(44) QB_CASE(45) QB_CASE(46) QB_CASE(47) QB_CASE(48)
#undef QB_CASE
    default: break;
    }
}
#endif

}  // namespace qk

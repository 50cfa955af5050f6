// tfft_stats.hip -- the statistics stage: per-plane medians of |F| (sampled bracket + verified radix select, with the plain
// three-level select behind it) and the capacity settled from the bracket pass.  Each launcher sits beside its kernels.
//
// Reference lines (steganosaurus/src/steganosaur.cpp) replaced by each kernel are cited as S:<line>.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "tfft_fft.h"
#include "tfft_device.h"
#include "tfft_kernels.h"

namespace tfft {

// ---------------------------------------------------------------------------
// median_abs S:404-409: the exact order statistic (sorted index P/2) of |F| over
// the full plane.  Stored bins of columns 1..M-1 count twice (bin + Hermitian
// mirror); the packed column 0 yields F[.][0] and F[.][M] once each.
//
// FAST path (one full read of the spectrum):
//   1. k_hist_spec over every 16th row: 4096-bucket histogram (top 13 bits of the float) of a SAMPLE
//   2. k_select_guess: bucket b of the sample median -> bracket [b-1, b+1]
//   3. k_collect_bracket over everything: exact weight below the bracket + compaction of the members
//      of the bracket (value relative to the bracket start, 21 bits) + their 1024-bucket histogram
//   4. k_select_fast<2>: rank - weight_below must fall inside the bracket (this VERIFIES the guess:
//      the result is exact or the path declares failure), pick the level-2 bucket
//   5. k_hist_cand / k_select_fast<3>: 2048-bucket level over the candidates -> the exact median
// FALLBACK (only if step 4 fails; every kernel returns at once when st->done): the plain 3-level radix
// select (4096 / 1024 / 512 buckets) with a full histogram pass and a compaction pass.
// Grids are a few blocks per CU with row loops and LDS-staged results: thousands of blocks adding to
// the same few global counters serialise at ~11 ns per atomic.
//   grid (NB, 3, n_images)   block 256   st[img*3+plane]
// ---------------------------------------------------------------------------
__device__ __forceinline__ SelectState* sel_of(SelectState* st) { return st + (size_t)blockIdx.z * 3 + blockIdx.y; }

// mags.size()/2 (S:407)
static unsigned long long median_rank(int PH, int PW) { return ((unsigned long long)PH * PW) / 2; }
// the image flags of the batch capacity: n_images words behind the partial counts
static unsigned* stat_flags(unsigned* partial, int n_images) { return partial + (size_t)n_images * 3 * TFFT_STAT_MAX_BLOCKS; }
// blocks per plane that give the whole launch about 4 blocks per CU (256 CUs)
static int stat_fill(int n_images) { return (1024 + 3 * n_images - 1) / (3 * n_images); }
static unsigned stat_blocks(int rows, int n_images) {      // ... never more blocks than rows
    int nb = stat_fill(n_images);
    if (nb < 1) nb = 1;
    if (nb > rows) nb = rows;
    if (nb > TFFT_STAT_MAX_BLOCKS) nb = TFFT_STAT_MAX_BLOCKS;
    return (unsigned)nb;
}

// The selection works on |F|^2 (mag2_of).
// col0 != nullptr: `pl` is a plane of |F|^2 (float, the batched delta embeds store nothing else: ColParams::em_m2) and the packed
// column 0, which cannot be unpacked from magnitudes, lives in col0[PH]
template <class F>
__device__ __forceinline__ void for_each_mag(const float2* __restrict__ pl, int PH, int M, int y, int x, F&& f, bool col0_packed = true,
                                             const float2* __restrict__ col0 = nullptr) {
    if (x == 0 && col0_packed) {
        float2 f0, fm;
        if (col0) unpack_col0(col0, y, PH, 1, f0, fm);
        else unpack_col0(pl, y, PH, M, f0, fm);
        f(__float_as_uint(mag2_of(f0)), 1u); f(__float_as_uint(mag2_of(fm)), 1u);
    } else if (col0) {
        f(__float_as_uint(reinterpret_cast<const float*>(pl)[(size_t)y * M + x]), 2u);
    } else {
        f(__float_as_uint(mag2_of(pl[(size_t)y * M + x])), 2u);
    }
}
// plane `plane` of image `img`: complex planes are img_stride float2 apart; the |F|^2 planes sit at the same BYTE offsets per image
__device__ __forceinline__ const float2* stat_plane(const float2* spec, size_t img_stride, int img, int plane, int PH, int M, bool m2) {
    return m2 ? reinterpret_cast<const float2*>(reinterpret_cast<const float*>(spec + (size_t)img * img_stride) + (size_t)plane * PH * M)
              : spec + (size_t)img * img_stride + (size_t)plane * PH * M;
}

// histogram of rows y0, y0+row_step, ... ; guarded != 0: fallback role, skip when the fast path succeeded
__global__ void k_hist_spec(const float2* __restrict__ spec, int PH, int M, size_t img_stride,
                            SelectState* __restrict__ st, int row_step, int guarded, int col0_packed = 1, const float2* __restrict__ col0 = nullptr) {
    SelectState* s = sel_of(st);
    if (guarded && s->done) return;
    unsigned* hist = reinterpret_cast<unsigned*>(tfft_smem);      // 4096 counters
    for (int i = threadIdx.x; i < 4096; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const float2* pl = stat_plane(spec, img_stride, blockIdx.z, blockIdx.y, PH, M, col0 != nullptr);
    const float2* c0 = col0 ? col0 + ((size_t)blockIdx.z * 3 + blockIdx.y) * PH : nullptr;
    for (int y = blockIdx.x * row_step; y < PH; y += gridDim.x * row_step)
        for (int x = threadIdx.x; x < M; x += blockDim.x)
            for_each_mag(pl, PH, M, y, x, [&](unsigned b, unsigned w) { atomicAdd(&hist[b >> 19], w); }, col0_packed != 0, c0);
    __syncthreads();
    for (int i = threadIdx.x; i < 4096; i += blockDim.x)
        if (hist[i]) atomicAdd(&s->hist[i], hist[i]);
}
constexpr unsigned HIST_SPEC_LDS = 4096 * sizeof(unsigned);
// The sample pass: rows 0, step, 2*step, .. with step = want_step within [1, 64].  It is LDS-atomic bound (a block histograms its rows
// one element per atomic), so it gets more and shorter blocks than the full passes: 4 sampled rows per block, at most max_blocks
// blocks per plane (their ~150 non-zero buckets each go to global atomics)
static void launch_hist_sample(const float2* spec, int PH, int M, size_t img_stride, int n_images, SelectState* st, long long want_step,
                               unsigned max_blocks, int col0_packed, const float2* col0, hipStream_t s) {
    const int step = (int)(want_step < 1 ? 1 : want_step > 64 ? 64 : want_step);
    unsigned nbs = (unsigned)(((PH + step - 1) / step + 3) / 4);
    if (nbs < 1) nbs = 1;
    if (nbs > max_blocks) nbs = max_blocks;
    hipLaunchKernelGGL(k_hist_spec, dim3(nbs, 3, n_images), dim3(256), HIST_SPEC_LDS, s, spec, PH, M, img_stride, st, step, 0, col0_packed, col0);
}

// ---- the select core: what the select kernels share --------------------------------------------------------------------------------
// LDS of a select kernel (one block per plane, 256 threads or more): a level's counters, zero padded to 4096, their sums 16 by 16 and
// 256 by 256, and the block's scalars
struct SelLds {
    unsigned h[4096], p1[256], p2[16];
    unsigned long long res[2];      // find_bucket_all: the bucket and the weight before it
    unsigned long long total;       // sum_hist
    int ok;
};
// Bucket holding `rank` among nb <= 4096 counters in L.h: three-level sums so that no thread walks more than 16 LDS words.  Every
// thread calls, behind a barrier after the last write to L.h; the result (bucket, weight before it) is valid in thread 0.
__device__ __forceinline__ void find_bucket(SelLds& L, unsigned long long rank, int nb, int& bucket, unsigned long long& before) {
    const int t = threadIdx.x;
    if (t < 256) { unsigned a = 0; for (int i = 0; i < 16; i++) a += L.h[t * 16 + i]; L.p1[t] = a; }
    __syncthreads();
    if (t < 16) { unsigned a = 0; for (int i = 0; i < 16; i++) a += L.p1[t * 16 + i]; L.p2[t] = a; }
    __syncthreads();
    bucket = nb - 1; before = 0;
    if (t == 0) {
        unsigned long long cum = 0;
        int g2 = 15; for (int i = 0; i < 16; i++) { if (cum + L.p2[i] > rank) { g2 = i; break; } cum += L.p2[i]; }
        int g1 = g2 * 16 + 15; for (int i = 0; i < 16; i++) { if (cum + L.p1[g2 * 16 + i] > rank) { g1 = g2 * 16 + i; break; } cum += L.p1[g2 * 16 + i]; }
        int b = g1 * 16 + 15; for (int i = 0; i < 16; i++) { if (cum + L.h[g1 * 16 + i] > rank) { b = g1 * 16 + i; break; } cum += L.h[g1 * 16 + i]; }
        if (b >= nb) b = nb - 1;
        bucket = b; before = cum;
    }
}
// ... with the result in every thread, for the kernels that go on working with it as a block (1024 threads): a barrier in front (they
// fill L.h with atomics right before) and two to hand the result round
__device__ __forceinline__ void find_bucket_all(SelLds& L, unsigned long long rank, int nb, int& bucket, unsigned long long& before) {
    __syncthreads();
    find_bucket(L, rank, nb, bucket, before);
    if (threadIdx.x == 0) { L.res[0] = (unsigned long long)bucket; L.res[1] = before; }
    __syncthreads();
    bucket = (int)L.res[0]; before = L.res[1];
}
// The loops over the 4096 counters take the block's size as an argument: the kernels of SEL_THREADS threads pass the constant, so that
// their sixteen loads are unrolled and in flight together
constexpr int SEL_THREADS = 256;
// the plane's global counters -> L.h (and L.total cleared for sum_hist)
__device__ __forceinline__ void stage_hist(const SelectState* s, SelLds& L, int nb, int threads) {
    for (int i = threadIdx.x; i < 4096; i += threads) L.h[i] = (i < nb) ? s->hist[i] : 0u;
    if (threadIdx.x == 0) L.total = 0;
    __syncthreads();
}
// L.total = the sum of the staged counters
__device__ __forceinline__ void sum_hist(SelLds& L, int threads) {
    { unsigned long long a = 0; for (int i = threadIdx.x; i < 4096; i += threads) a += L.h[i]; if (a) atomicAdd(&L.total, a); }
    __syncthreads();
}
// Every select kernel leaves the global counters zero behind it (the context zeroes the state once at creation), so that no launch
// has to clear them in front.
__device__ __forceinline__ void clear_hist(SelectState* s, int threads) {
    for (int i = threadIdx.x; i < 4096; i += threads) s->hist[i] = 0;
}
// the per-call fields, as a call's first select kernel sets them (one thread)
__device__ __forceinline__ void sel_reset(SelectState* s, unsigned long long rank) {
    s->rank = rank; s->prefix = 0; s->n_cand = 0; s->cand_fixed = 0; s->done = 0; s->below = 0; s->lo = 0; s->hi = 0; s->fast = 0; s->n_amb = 0;
    s->t2_lo = 0.f; s->t2_hi = 0.f;
}
// the bracket did not hold the median: open the plane for the fallback select, which starts from the untouched s->rank (one thread)
__device__ __forceinline__ void sel_reopen(SelectState* s) { s->n_cand = 0; s->cand_fixed = 0; s->prefix = 0; s->done = 0; }
// the verification of the fast path: does the bracket, `total` weights above `below`, hold the rank?  Then the result is exact.
__device__ __forceinline__ bool bracket_holds(unsigned long long rank, unsigned long long below, unsigned long long total) {
    return !(rank < below || rank - below >= total);
}

__global__ void k_select_init(SelectState* __restrict__ st, unsigned long long rank) {
    SelectState* s = st + blockIdx.x;
    clear_hist(s, blockDim.x);
    if (threadIdx.x == 0) sel_reset(s, rank);
}

// ---- fast path ----------------------------------------------------------------------------------
// Also resets the per-call fields, so the compact pipeline needs no k_select_init launch.
__global__ void k_select_guess(SelectState* __restrict__ st, double magmin, unsigned long long rank) {
    SelLds& L = *reinterpret_cast<SelLds*>(tfft_smem);
    SelectState* s = st + blockIdx.x;
    stage_hist(s, L, 4096, SEL_THREADS);
    sum_hist(L, SEL_THREADS);        // the sample's weight: its median has rank total/2
    int b; unsigned long long before;
    find_bucket(L, L.total / 2, 4096, b, before);
    if (threadIdx.x == 0) {
        const unsigned lo = (unsigned)(b > 0 ? b - 1 : 0), hi = (unsigned)(b < 4095 ? b + 1 : 4095);
        sel_reset(s, rank);
        s->lo = lo; s->hi = hi;
        if (magmin >= 0.0) {
            // the median's |F|^2 lies in [bits(lo<<19), bits((hi+1)<<19)); sqrtf and mag2_threshold are monotone, so the capacity
            // threshold T2 = mag2_threshold(magmin * sqrtf(.)) lies in [t2_lo, t2_hi]
            const float m_lo = sqrtf(__uint_as_float(lo << 19)), m_hi = sqrtf(__uint_as_float(hi >= 4079u ? 0x7F7FFFFFu : ((hi + 1u) << 19)));
            s->t2_lo = mag2_threshold(magmin * (double)m_lo);
            s->t2_hi = mag2_threshold(magmin * (double)m_hi);
        }
    }
    __syncthreads();
    clear_hist(s, SEL_THREADS);
}
// test hook (TFFT_STATS_SKEW): move every bracket by `skew` level-1 buckets, so that the fast path fails and the fallbacks run
__global__ void k_skew_bracket(SelectState* __restrict__ st, int skew) {
    SelectState* s = st + blockIdx.x;
    if (threadIdx.x == 0) { s->lo = (unsigned)imax(0, imin(4093, (int)s->lo + skew)); s->hi = s->lo + 2; }
}
// the bracket of every plane out of its sample histogram
static int guess_launches(const StatOpts& o) { return o.skew ? 2 : 1; }
static void launch_guess(int PH, int PW, int n_images, SelectState* st, const StatOpts& o, hipStream_t s) {
    hipLaunchKernelGGL(k_select_guess, dim3(3 * n_images), dim3(SEL_THREADS), sizeof(SelLds), s, st, o.cap ? o.cap->magmin : -1.0, median_rank(PH, PW));
    if (o.skew) hipLaunchKernelGGL(k_skew_bracket, dim3(3 * n_images), dim3(64), 0, s, st, o.skew);
}

// One pass over the whole spectrum: weight of everything below the bracket (registers -> one atomic per
// block) and compaction of the bracket's members.  Each WAVE stages its candidates in a private LDS
// buffer and flushes it with one global atomic when it is half full: no workgroup barrier in the loop.
// A wave walks whole rows in segments of 1024 columns (8 x 16-byte loads per lane) and issues the loads
// of the NEXT segment before it classifies the current one, so ~16 KB per wave are in flight: with one
// segment of 256 columns per dependent step the pass ran at 3 TB/s, bound by load latency.
struct BracketSeg {
    float4 v[8];                        // columns x0 + 2*(q*64 + lane) and the one after it
    float2 partner;                     // lane 0 of segment 0: row PH-y of the packed column 0
};
// |F|^2 planes (M2IN): the two values of a lane and q land in .x and .z, the packed column 0 is not in the plane (k_col0_stats)
__device__ __forceinline__ void bracket_load_m2(BracketSeg& r, const float* __restrict__ pl, int M, int y, int x0, int lane) {
    const float* row = pl + (size_t)y * M;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int x = x0 + 2 * (q * 64 + lane);
        if (x + 1 < M) { const float2 a = *reinterpret_cast<const float2*>(row + x); r.v[q] = make_float4(a.x, 0.f, a.y, 0.f); }
        else if (x < M) r.v[q] = make_float4(row[x], 0.f, 0.f, 0.f);
        else r.v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    r.partner = make_float2(0.f, 0.f);
}
__device__ __forceinline__ void bracket_load(BracketSeg& r, const float2* __restrict__ pl, int PH, int M, int y, int x0, int lane) {
    const float2* row = pl + (size_t)y * M;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int x = x0 + 2 * (q * 64 + lane);
        if (x + 1 < M) r.v[q] = *reinterpret_cast<const float4*>(row + x);
        else if (x < M) { const float2 a = row[x]; r.v[q] = make_float4(a.x, a.y, 0.f, 0.f); }   // M == 1
        else r.v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    r.partner = make_float2(0.f, 0.f);
    if (x0 == 0 && lane == 0) r.partner = pl[(size_t)((PH - y) & (PH - 1)) * M];
}
// columns x of row y (full-grid indices) with s_lo <= y*y + x*x <= s_hi: [a, b], empty when a > b
__device__ __forceinline__ void annulus_row(unsigned long long yy, unsigned long long s_lo, unsigned long long s_hi, int& a, int& b) {
    if (yy > s_hi) { a = 1; b = 0; return; }
    unsigned long long hb = (unsigned long long)sqrt((double)(s_hi - yy));
    while ((hb + 1) * (hb + 1) + yy <= s_hi) hb++;
    while (hb * hb + yy > s_hi) hb--;
    unsigned long long la = 0;
    if (s_lo > yy) {
        la = (unsigned long long)sqrt((double)(s_lo - yy));
        while (la * la + yy < s_lo) la++;
        while (la > 0 && (la - 1) * (la - 1) + yy >= s_lo) la--;
    }
    a = (int)(la > 0x3FFFFFFFull ? 0x3FFFFFFFull : la); b = (int)(hb > 0x3FFFFFFFull ? 0x3FFFFFFFull : hb);
}
// CAP: capacity (S:998-1008) counted in the same pass.  A stored bin (y, x), 0 < x < M, stands for the full-grid bins (y, x)
// and its mirror ((PH-y)%PH, PW-x) of equal magnitude; each counts when it is off the axes and inside the annulus.  Per row
// that is two column intervals (wave uniform), per element two range tests and a compare against the bracket of the
// threshold (SelectState::t2_lo/t2_hi); the few values inside that bracket are parked for k_capacity_settle.
template <bool CAP, bool M2IN = false>
__global__ void __launch_bounds__(256) k_collect_bracket(const float2* __restrict__ spec, int PH, int M, size_t img_stride,
                                  SelectState* __restrict__ st, unsigned* __restrict__ cand, size_t cand_stride,
                                  unsigned long long s_lo, unsigned long long s_hi, int PWfull, unsigned* __restrict__ partial,
                                  float* __restrict__ amb) {
    unsigned* hist = reinterpret_cast<unsigned*>(tfft_smem);      // 1024 level-2 counters
    unsigned* wbuf = hist + 1024;                                 // 4 waves x 512 staged candidates
    unsigned* wcnt = wbuf + 4 * 512;                              // per wave: [0] staged count, [1] global base
    SelectState* s = sel_of(st);
    const unsigned lo = s->lo, hi = s->hi, base_bits = lo << 19;
    unsigned* out = cand + ((size_t)blockIdx.z * 3 + blockIdx.y) * cand_stride;
    const float2* pl = stat_plane(spec, img_stride, blockIdx.z, blockIdx.y, PH, M, M2IN);
    const float* plm = reinterpret_cast<const float*>(pl);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned* buf = wbuf + wave * 512; unsigned* cnt = wcnt + wave * 2;
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) hist[i] = 0;
    if (lane == 0) cnt[0] = 0;
    __syncthreads();
    // Per element: one compare-and-add for the weight below the bracket and one ballot for membership.
    // The staged count lives in a wave-uniform register (ballot + popcount), slots come from mbcnt: no
    // returning LDS atomic and no divergent branch on the common path -- the first version spent ~150
    // instructions per element on exec-masked branches and ran at 3 TB/s, instruction bound.
    unsigned below32 = 0;               // per lane < 2^32: a lane sees at most PH*PW/64 weights
    unsigned nstaged = 0;               // wave uniform
    const unsigned span = hi - lo;
    // capacity: intervals of the current row (wave uniform), definite count, parked values
    int ca1 = 1, cb1 = 0, ca2 = 1, cb2 = 0;
    unsigned capcount = 0;
    const float t2_lo = CAP ? s->t2_lo : 0.f, t2_hi = CAP ? s->t2_hi : 0.f;
    float* amb_out = CAP ? amb + ((size_t)blockIdx.z * 3 + blockIdx.y) * TFFT_AMB_CAP : nullptr;
    auto cap_row = [&](int y) {
        ca1 = ca2 = 1; cb1 = cb2 = 0;
        if (y == 0 || 2 * y == PH) return;                   // excluded rows (S:698-700); the mirror row is excluded with it
        annulus_row((unsigned long long)y * (unsigned long long)y, s_lo, s_hi, ca1, cb1);
        if (ca1 < 1) ca1 = 1;
        if (cb1 > M - 1) cb1 = M - 1;
        int ma, mb;                                          // mirror row PH-y, mirror columns xm in [ma, mb] -> stored x = PW - xm
        const unsigned long long ym = (unsigned long long)(PH - y);
        annulus_row(ym * ym, s_lo, s_hi, ma, mb);
        ca2 = PWfull - mb; cb2 = PWfull - ma;
        if (ma > mb) { ca2 = 1; cb2 = 0; }
        if (ca2 < 1) ca2 = 1;
        if (cb2 > M - 1) cb2 = M - 1;
    };
    auto cap_elem = [&](int x, float m2) {
        const unsigned w = ((x >= ca1 && x <= cb1) ? 1u : 0u) + ((x >= ca2 && x <= cb2) ? 1u : 0u);
        if (!(m2 < t2_hi)) capcount += w;
        else if (w && !(m2 < t2_lo)) {                       // rare (a few bins per plane): settle once the median is known
            for (unsigned k = 0; k < w; k++) {
                const unsigned slot = atomicAdd(&s->n_amb, 1u);
                if (slot < TFFT_AMB_CAP) amb_out[slot] = m2;
            }
        }
    };
    auto classify = [&](bool valid, unsigned b, unsigned w) {
        const unsigned bk = b >> 19;
        below32 += (valid && bk < lo) ? w : 0u;
        const bool c = valid && (bk - lo) <= span;
        const unsigned long long m = __ballot(c);
        if (m) {                        // wave uniform
            if (c) {
                const unsigned rel = b - base_bits;              // < 3 * 2^19
                buf[nstaged + wave_rank(m)] = rel | (w == 2u ? 0x80000000u : 0u);
                atomicAdd(&hist[rel >> 11], w);
            }
            nstaged += (unsigned)__popcll(m);
        }
    };
    // the trip counts are wave uniform: (y, x0) advance identically in every lane
    const int ystep = gridDim.x * 4;
    int y = blockIdx.x * 4 + wave, x0 = 0;
    bool have = y < PH;
    BracketSeg cur;
    if (have) { if (M2IN) bracket_load_m2(cur, plm, M, y, x0, lane); else bracket_load(cur, pl, PH, M, y, x0, lane); }
    while (have) {
        int ny = y, nx0 = x0 + 1024;
        if (nx0 >= M) { nx0 = 0; ny = y + ystep; }
        const bool nhave = ny < PH;
        BracketSeg nxt;
        if (nhave) { if (M2IN) bracket_load_m2(nxt, plm, M, ny, nx0, lane); else bracket_load(nxt, pl, PH, M, ny, nx0, lane); }
        if (CAP && x0 == 0) cap_row(y);
        const bool cap_live = CAP && (ca1 <= cb1 || ca2 <= cb2);      // wave uniform
        if (!M2IN && x0 == 0) {         // packed column 0 (lane 0): F[y][0] and F[y][M], once each (unpack_col0); M2IN: k_col0_stats
            const float2 a = make_float2(cur.v[0].x, cur.v[0].y), b2 = cur.partner;
            const float2 f0 = make_float2(0.5f * (a.x + b2.x), 0.5f * (a.y - b2.y));
            const float2 fm = make_float2(0.5f * (a.y + b2.y), -0.5f * (a.x - b2.x));
            classify(lane == 0, __float_as_uint(mag2_of(f0)), 1u);
            classify(lane == 0, __float_as_uint(mag2_of(fm)), 1u);
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int x = x0 + 2 * (q * 64 + lane);
            const float ma2 = M2IN ? cur.v[q].x : mag2_of(make_float2(cur.v[q].x, cur.v[q].y)), mb2 = M2IN ? cur.v[q].z : mag2_of(make_float2(cur.v[q].z, cur.v[q].w));
            classify(x != 0 && x < M, __float_as_uint(ma2), 2u);
            classify(x + 1 < M, __float_as_uint(mb2), 2u);
            if (cap_live) { cap_elem(x, ma2); cap_elem(x + 1, mb2); }          // x = 0 and x >= M fall outside [1, M-1] by themselves
            if ((q & 1) && nstaged > 250) {     // at most 4 * 64 + 2 more before the next check: 508 <= 512
                WaveSync::sync();
                if (lane == 0) cnt[1] = atomicAdd(&s->n_cand, nstaged);
                WaveSync::sync();
                const unsigned gbase = cnt[1];
                for (unsigned i = lane; i < nstaged; i += 64) out[gbase + i] = buf[i];
                WaveSync::sync();
                nstaged = 0;
            }
        }
        cur = nxt; y = ny; x0 = nx0; have = nhave;
    }
    if (nstaged) {   // final flush of this wave
        WaveSync::sync();
        if (lane == 0) cnt[1] = atomicAdd(&s->n_cand, nstaged);
        WaveSync::sync();
        const unsigned gbase = cnt[1];
        for (unsigned i = lane; i < nstaged; i += 64) out[gbase + i] = buf[i];
    }
    unsigned long long below = below32;
    if (below) atomicAdd(&s->below, below);
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += blockDim.x)
        if (hist[i]) atomicAdd(&s->hist[i], hist[i]);
    if (CAP) {                          // one partial count per block (plain store, no global atomics)
        __syncthreads();
        if (threadIdx.x == 0) wcnt[0] = 0;
        __syncthreads();
        if (capcount) atomicAdd(&wcnt[0], capcount);
        __syncthreads();
        if (threadIdx.x == 0) partial[((size_t)blockIdx.z * 3 + blockIdx.y) * gridDim.x + blockIdx.x] = wcnt[0];
    }
}
// its LDS (hist, wbuf, wcnt) and its instantiations
constexpr unsigned COLLECT_BRACKET_LDS = (1024 + 4 * 512 + 8) * sizeof(unsigned);
typedef void (*collect_bracket_fn)(const float2*, int, int, size_t, SelectState*, unsigned*, size_t, unsigned long long, unsigned long long, int,
                                   unsigned*, float*);
static collect_bracket_fn collect_bracket_kernel(bool cap, bool m2in) {
    if (m2in) return cap ? k_collect_bracket<true, true> : k_collect_bracket<false, true>;
    return cap ? k_collect_bracket<true, false> : k_collect_bracket<false, false>;
}
// workgroups of k_collect_bracket that one CU holds at a time (queried once per context)
int collect_bracket_resident_blocks() {
    int r = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, collect_bracket_kernel(true, false), 256, COLLECT_BRACKET_LDS) != hipSuccess) r = 0;
    return r;
}
// The bracket pass over the spectrum (o.m2: over the |F|^2 planes); returns its blocks per plane, as many partial capacity counts.
// The whole grid is resident at once, so its run time is that of the fullest CU: 1056 workgroups on 256 CUs meant 4 on most and 5
// on some, i.e. 5/1056 of the work on the critical CU.  Fill every CU to the same depth instead: the largest grid that fits the
// residency limit.
static unsigned launch_collect_bracket(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, const StatOpts& o,
                                       hipStream_t s) {
    const int cus = o.fill_cus > 0 ? o.fill_cus : 256, resident = o.fill_resident > 0 ? o.fill_resident : 4;
    unsigned nbc = (unsigned)(((long long)cus * resident) / (3LL * n_images));
    // at least 4 rows per wave: every block ends with up to ~770 global atomics (its level-2 histogram), and a single image
    // spread over 426 one-row-per-wave blocks spent more time on those than on its rows (49 us for 50 MB)
    if (nbc > (unsigned)((PH + 15) / 16)) nbc = (unsigned)((PH + 15) / 16);
    if (nbc > TFFT_STAT_MAX_BLOCKS) nbc = TFFT_STAT_MAX_BLOCKS;
    if (nbc < 1) nbc = 1;
    const CapParams* cap = o.cap;
    hipLaunchKernelGGL(collect_bracket_kernel(cap != nullptr, o.m2), dim3(nbc, 3, n_images), dim3(256), COLLECT_BRACKET_LDS, s, spec, PH, PW >> 1,
                       img_stride, b.st, b.cand, b.cand_stride, cap ? cap->s_lo : 0ull, cap ? cap->s_hi : 0ull, cap ? cap->PW : 0,
                       cap ? b.partial : nullptr, cap ? b.amb : nullptr);
    return nbc;
}

// usable[img] = sum_p floor(c_p / 2) from the bracket pass: c_p = the blocks' definite counts + the parked values that reach
// T2 = mag2_threshold(magmin * median_p).  One block of three waves per image.  When a plane's median came from the fallback
// select (its bracket was wrong) or it parked more than TFFT_AMB_CAP values the image cannot be settled: flag[img] = 1 and
//   recount = 0: k_capacity recounts it (guarded launches behind this one);
//   recount = 1: this block recounts it itself over the annulus box (rare and slow: one block per image).
__global__ void k_capacity_settle(const SelectState* __restrict__ st, const float* __restrict__ med, double magmin, const unsigned* __restrict__ partial,
                                  int nb, const float* __restrict__ amb, unsigned long long* __restrict__ usable, unsigned* __restrict__ flag,
                                  const float2* __restrict__ spec, CapParams P, int recount, int m2in = 0) {
    unsigned long long* c = reinterpret_cast<unsigned long long*>(tfft_smem);   // [3] + bad
    unsigned* bad = reinterpret_cast<unsigned*>(c + 3);
    const int img = blockIdx.x, p = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < 3) c[threadIdx.x] = 0;
    if (threadIdx.x == 0) bad[0] = 0;
    __syncthreads();
    const SelectState* s = st + (size_t)img * 3 + p;
    const unsigned n_amb = s->n_amb;
    if (lane == 0 && (!s->fast || n_amb > TFFT_AMB_CAP)) atomicOr(&bad[0], 1u);
    const float t2 = mag2_threshold(magmin * (double)med[img * 3 + p]);
    unsigned long long a = 0;
    for (int i = lane; i < nb; i += 64) a += partial[((size_t)img * 3 + p) * nb + i];
    const float* av = amb + ((size_t)img * 3 + p) * TFFT_AMB_CAP;
    for (unsigned i = lane; i < n_amb && i < TFFT_AMB_CAP; i += 64) if (!(av[i] < t2)) a++;
    if (a) atomicAdd(&c[p], a);
    __syncthreads();
    const bool redo = bad[0] != 0;
    if (redo && recount) {              // block uniform
        __syncthreads();
        if (threadIdx.x < 3) c[threadIdx.x] = 0;
        __syncthreads();
        const int M = P.PWi >> 1;
        for (int q = 0; q < 3; q++) {
            const float tq = mag2_threshold(magmin * (double)med[img * 3 + q]);
            const float2* pl = stat_plane(spec, P.img_stride, img, q, P.PH, M, m2in != 0);
            const float* plm = reinterpret_cast<const float*>(pl);
            unsigned long long mine = 0;
            for (int y = 1; y < P.bh; y++) {
                if (2 * y == P.PH) continue;
                const unsigned long long yy = (unsigned long long)y * (unsigned long long)y;
                const float2* row = pl + (size_t)y * M;
                const float2* mrow = pl + (size_t)((P.PH - y) & (P.PH - 1)) * M;
                for (int x = 1 + (int)threadIdx.x; x < P.bw; x += (int)blockDim.x) {
                    if (2 * x == P.PW) continue;
                    const unsigned long long r2 = yy + (unsigned long long)x * (unsigned long long)x;
                    if (r2 < P.s_lo || r2 > P.s_hi) continue;
                    float m2;
                    if (m2in) m2 = x < M ? plm[(size_t)y * M + x] : plm[(size_t)((P.PH - y) & (P.PH - 1)) * M + (P.PW - x)];
                    else m2 = mag2_of(x < M ? row[x] : mrow[P.PW - x]);
                    if (!(m2 < tq)) mine++;
                }
            }
            if (mine) atomicAdd(&c[q], mine);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { usable[img] = c[0] / 2 + c[1] / 2 + c[2] / 2; flag[img] = (redo && !recount) ? 1u : 0u; }
}
constexpr unsigned CAPACITY_SETTLE_LDS = 64;      // c[3] and bad
// nb: partial counts per plane; recount = false: launch_capacity follows for the flagged images
static void launch_capacity_settle(const float2* spec, int n_images, const StatBufs& b, const CapParams& cap, unsigned nb, bool recount, bool m2in,
                                   hipStream_t s) {
    hipLaunchKernelGGL(k_capacity_settle, dim3(n_images), dim3(192), CAPACITY_SETTLE_LDS, s, b.st, b.med, cap.magmin, b.partial, (int)nb, b.amb, b.usable,
                       stat_flags(b.partial, n_images), spec, cap, recount ? 1 : 0, m2in ? 1 : 0);
}

// LEVEL 2: verify the bracket and pick the 2048-wide sub-bucket; LEVEL 3: the exact value.
template <int LEVEL>
__global__ void k_select_fast(SelectState* __restrict__ st, float* __restrict__ med_out) {
    SelLds& L = *reinterpret_cast<SelLds*>(tfft_smem);
    SelectState* s = st + blockIdx.x;
    if (LEVEL == 3 && s->done != 2) return;            // level 2 did not verify: leave everything to the fallback
    constexpr int NB = (LEVEL == 2) ? 1024 : 2048;
    stage_hist(s, L, NB, SEL_THREADS);
    sum_hist(L, SEL_THREADS);
    unsigned long long rank = s->rank;
    if (LEVEL == 2) {
#ifdef TFFT_DEBUG_MEDIAN
        if (threadIdx.x == 0) printf("sel2 plane %d: rank %llu below %llu total %llu lo %u hi %u n_cand %u\n", (int)blockIdx.x, rank, s->below, L.total, s->lo, s->hi, s->n_cand);
#endif
        if (threadIdx.x == 0) L.ok = bracket_holds(rank, s->below, L.total) ? 1 : 0;
        rank -= s->below;
    } else if (threadIdx.x == 0) L.ok = 1;
    __syncthreads();
    if (L.ok) {
        int b; unsigned long long before;
        find_bucket(L, rank, NB, b, before);
        if (threadIdx.x == 0) {
            if (LEVEL == 2) { s->prefix = (unsigned)b; s->rank = rank - before; s->done = 2; }
            else { med_out[blockIdx.x] = sqrtf(__uint_as_float((s->lo << 19) + (s->prefix << 11) + (unsigned)b)); s->done = 1; s->fast = 1; }
        }
    } else if (threadIdx.x == 0) {
        sel_reopen(s);
    }
    __syncthreads();
    clear_hist(s, SEL_THREADS);
}

// One level's histogram of the compacted candidates i = first, first + stride, .. < n into `hist` (LDS), weights 1 or 2:
//   CAND_LEVEL2: 1024 buckets of rel >> 11 (what k_collect_bracket builds while it stages them; the in-kernel form, COLS_STAT, does not)
//   CAND_FAST3 : 2048 buckets of rel & 2047 among the candidates whose rel >> 11 equals the level-2 bucket `want`
//   CAND_PLAIN3: the plain select's candidates c (k_collect): 512 buckets of c & 511 among those with (c >> 9) & 1023 == want
// (a kernel trace shows the values, k_hist_cand<0..2>: tools/prof_traffic.py looks for <0> and <1> -- keep the two in step)
enum { CAND_LEVEL2 = 0, CAND_FAST3 = 1, CAND_PLAIN3 = 2 };
constexpr unsigned cand_buckets(int level) { return level == CAND_LEVEL2 ? 1024u : level == CAND_FAST3 ? 2048u : 512u; }
template <int LV>
__device__ __forceinline__ void cand_hist(unsigned* hist, const unsigned* __restrict__ in, unsigned n, unsigned first, unsigned stride, unsigned want) {
    for (unsigned i = first; i < n; i += stride) {
        const unsigned c = in[i], v = c & 0x7FFFFFFFu;
        if (c == TFFT_CAND_HOLE) continue;
        const bool take = LV == CAND_LEVEL2 ? true : LV == CAND_FAST3 ? (v >> 11) == want : ((v >> 9) & 1023u) == want;
        if (take) atomicAdd(&hist[LV == CAND_LEVEL2 ? ((v >> 11) & 1023u) : (v & (cand_buckets(LV) - 1u))], (c >> 31) ? 2u : 1u);
    }
}
// ... by a grid of blocks per plane, added to the plane's global counters.  The level-3 forms return at once where they have nothing
// to do: FAST3 unless level 2 verified, PLAIN3 when the median is known.
template <int LV>
__global__ void k_hist_cand(SelectState* __restrict__ st, const unsigned* __restrict__ cand, size_t cand_stride) {
    SelectState* s = sel_of(st);
    if (LV == CAND_FAST3 && s->done != 2) return;
    if (LV == CAND_PLAIN3 && s->done != 0) return;
    constexpr int NB = (int)cand_buckets(LV);
    unsigned* hist = reinterpret_cast<unsigned*>(tfft_smem);
    for (int i = threadIdx.x; i < NB; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const unsigned want = LV == CAND_PLAIN3 ? (s->prefix & 1023u) : s->prefix;
    cand_hist<LV>(hist, cand + ((size_t)blockIdx.z * 3 + blockIdx.y) * cand_stride, s->cand_fixed + s->n_cand, blockIdx.x * blockDim.x + threadIdx.x,
                  gridDim.x * blockDim.x, want);
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += blockDim.x)
        if (hist[i]) atomicAdd(&s->hist[i], hist[i]);
}
template <int LV>
static void launch_hist_cand(unsigned blocks, int n_images, const StatBufs& b, hipStream_t s) {
    hipLaunchKernelGGL(k_hist_cand<LV>, dim3(blocks, 3, n_images), dim3(256), cand_buckets(LV) * sizeof(unsigned), s, b.st, b.cand, b.cand_stride);
}
// candidates: ~13 % of a plane; 16 blocks per plane are plenty for a batch but left one 8192^2 image with 48 blocks in all (110 us)
static unsigned cand_blocks(int n_images) {
    const int nbh = stat_fill(n_images);
    return (unsigned)(nbh < 16 ? 16 : nbh > 256 ? 256 : nbh);
}
// the fast path behind the level-2 histogram: verify + level 2, level-3 histogram, level 3
constexpr int FAST_TAIL_LAUNCHES = 3;
static void launch_fast_tail(int n_images, const StatBufs& b, hipStream_t s) {
    const dim3 gs(3 * n_images);
    hipLaunchKernelGGL(k_select_fast<2>, gs, dim3(SEL_THREADS), sizeof(SelLds), s, b.st, b.med);
    launch_hist_cand<CAND_FAST3>(cand_blocks(n_images), n_images, b, s);
    hipLaunchKernelGGL(k_select_fast<3>, gs, dim3(SEL_THREADS), sizeof(SelLds), s, b.st, b.med);
}

// |F|^2 planes (batched delta embeds): the packed column 0 travels beside the plane as complex values -- F[y][0] and F[y][M]
// (unpack_col0), one value of weight 1 each, classified like k_collect_bracket does; neither column belongs to the annulus count
// (x = 0 and 2x = PW are excluded, S:698-700)
__global__ void k_col0_stats(const float2* __restrict__ col0, int PH, SelectState* __restrict__ st, unsigned* __restrict__ cand, size_t cand_stride,
                             int with_hist) {
    SelectState* s = st + (size_t)blockIdx.z * 3 + blockIdx.y;
    const float2* cz = col0 + ((size_t)blockIdx.z * 3 + blockIdx.y) * PH;
    unsigned* out = cand + ((size_t)blockIdx.z * 3 + blockIdx.y) * cand_stride;
    const unsigned lo = s->lo, span = s->hi - lo, base_bits = lo << 19;
    unsigned below = 0;
    for (int y = blockIdx.x * blockDim.x + threadIdx.x; y < PH; y += gridDim.x * blockDim.x) {
        const float2 a = cz[y], b = cz[(PH - y) & (PH - 1)];
        const float2 f0 = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
        const float2 fm = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
        const unsigned v[2] = {__float_as_uint(mag2_of(f0)), __float_as_uint(mag2_of(fm))};
        for (int i = 0; i < 2; i++) {
            const unsigned bk = v[i] >> 19;
            if (bk < lo) below++;
            else if (bk - lo <= span) {
                const unsigned rel = v[i] - base_bits;
                out[s->cand_fixed + atomicAdd(&s->n_cand, 1u)] = rel;                           // weight 1: bit 31 clear
                if (with_hist) atomicAdd(&s->hist[rel >> 11], 1u);                              // the level-2 histogram k_collect_bracket keeps
            }
        }
    }
    if (below) atomicAdd(&s->below, (unsigned long long)below);
}

// ---- compact pipeline (planes up to TFFT_COMPACT_MAX_BINS): the three launches after the bracket pass in one, the six fallback
// launches in one.  A single image spends its time in the GPU-side latency of dependent launches (~6.7 us each: the statistics were
// 16 of the ~35 of a 1080p round trip), not in the kernels.
// k_select_fast<2> + k_hist_cand<CAND_FAST3> + k_select_fast<3> for one plane per block (1024 threads)
__global__ void __launch_bounds__(1024) k_select_finish(SelectState* __restrict__ st, const unsigned* __restrict__ cand, size_t cand_stride,
                                                        float* __restrict__ med_out, unsigned long long rank) {
    SelLds& L = *reinterpret_cast<SelLds*>(tfft_smem);
    SelectState* s = st + blockIdx.x;
    const int t = threadIdx.x;
    stage_hist(s, L, 1024, blockDim.x);
    sum_hist(L, blockDim.x);
    const unsigned long long below = s->below;
    const bool ok = bracket_holds(rank, below, L.total);       // exact result or declared failure
    clear_hist(s, blockDim.x);
    if (!ok) {
        if (t == 0) sel_reopen(s);      // k_median_fallback takes over
        return;
    }
    int b2; unsigned long long before;
    find_bucket_all(L, rank - below, 1024, b2, before);
    const unsigned long long rank3 = rank - below - before;
    for (int i = t; i < 4096; i += blockDim.x) L.h[i] = 0;
    __syncthreads();
    cand_hist<CAND_FAST3>(L.h, cand + (size_t)blockIdx.x * cand_stride, s->cand_fixed + s->n_cand, t, blockDim.x, (unsigned)b2);
    int b3;
    find_bucket_all(L, rank3, 2048, b3, before);
    if (t == 0) {
        med_out[blockIdx.x] = sqrtf(__uint_as_float((s->lo << 19) + ((unsigned)b2 << 11) + (unsigned)b3));
        s->prefix = (unsigned)b2; s->done = 1; s->fast = 1;
    }
}
// The plain three-level radix select (4096 / 1024 / 512 buckets of the float's bits, as k_select<1..3>) by ONE block per plane:
// three passes of that block over its plane.  Runs only where the fast path did not verify (or when forced): slow and rare.
__global__ void __launch_bounds__(1024) k_median_fallback(const float2* __restrict__ spec, int PH, int M, size_t img_stride, SelectState* __restrict__ st,
                                                          float* __restrict__ med_out, unsigned long long rank, int force, const float2* __restrict__ col0 = nullptr) {
    SelectState* s = st + blockIdx.x;
    if (!force && s->done) return;
    SelLds& L = *reinterpret_cast<SelLds*>(tfft_smem);
    unsigned* h = L.h;
    const int img = blockIdx.x / 3, plane = blockIdx.x - 3 * img, t = threadIdx.x;
    const float2* pl = stat_plane(spec, img_stride, img, plane, PH, M, col0 != nullptr);
    const float2* c0 = col0 ? col0 + (size_t)blockIdx.x * PH : nullptr;
    const size_t n = (size_t)PH * M;
    unsigned prefix = 0;
    for (int level = 1; level <= 3; level++) {
        for (int i = t; i < 4096; i += blockDim.x) h[i] = 0;
        __syncthreads();
        for (size_t e = t; e < n; e += blockDim.x) {
            const int y = (int)(e / M), x = (int)(e - (size_t)y * M);
            for_each_mag(pl, PH, M, y, x, [&](unsigned b, unsigned w) {
                if (level == 1) atomicAdd(&h[b >> 19], w);
                else if (level == 2) { if ((b >> 19) == prefix) atomicAdd(&h[(b >> 9) & 1023u], w); }
                else { if ((b >> 9) == prefix) atomicAdd(&h[b & 511u], w); }
            }, true, c0);
        }
        int b; unsigned long long before;
        find_bucket_all(L, rank, level == 1 ? 4096 : level == 2 ? 1024 : 512, b, before);
        rank -= before;
        prefix = (level == 1) ? (unsigned)b : (level == 2) ? ((prefix << 10) | (unsigned)b) : ((prefix << 9) | (unsigned)b);
        __syncthreads();
    }
    if (t == 0) { med_out[blockIdx.x] = sqrtf(__uint_as_float(prefix)); s->done = 1; s->fast = 0; s->n_amb = 0; }
    clear_hist(s, blockDim.x);
}
// the planes the fast path left open (force: all of them), one block each
static void launch_median_fallback(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, bool force, bool m2in,
                                   hipStream_t s) {
    hipLaunchKernelGGL(k_median_fallback, dim3(3 * n_images), dim3(1024), sizeof(SelLds), s, spec, PH, PW >> 1, img_stride, b.st, b.med,
                       median_rank(PH, PW), force ? 1 : 0, m2in ? b.col0 : (const float2*)nullptr);
}

// ---- fallback path (plain 3-level radix select; every kernel is a no-op when s->done) ---------------
template <int LEVEL>
__global__ void k_select(SelectState* __restrict__ st, float* __restrict__ med_out) {
    constexpr int NB = (LEVEL == 1) ? 4096 : (LEVEL == 2) ? 1024 : 512;
    constexpr int SHIFT = (LEVEL == 1) ? 0 : (LEVEL == 2) ? 10 : 9;
    SelLds& L = *reinterpret_cast<SelLds*>(tfft_smem);
    SelectState* s = st + blockIdx.x;
    if (s->done) return;
    stage_hist(s, L, NB, SEL_THREADS);
    int b; unsigned long long before;
    const unsigned long long rank = s->rank;
    find_bucket(L, rank, NB, b, before);
    if (threadIdx.x == 0) {
        s->rank = rank - before;
        s->prefix = (LEVEL == 1) ? (unsigned)b : ((s->prefix << SHIFT) | (unsigned)b);
        if (LEVEL == 3) med_out[blockIdx.x] = sqrtf(__uint_as_float(s->prefix));
    }
    __syncthreads();
    clear_hist(s, SEL_THREADS);
}

// Compaction of the selected level-1 bucket (candidate = low 19 bits | weight flag) + its level-2 histogram.
__global__ void k_collect(const float2* __restrict__ spec, int PH, int M, size_t img_stride,
                          SelectState* __restrict__ st, unsigned* __restrict__ cand, size_t cand_stride) {
    SelectState* s = sel_of(st);
    if (s->done) return;
    unsigned* hist = reinterpret_cast<unsigned*>(tfft_smem);      // 1024 level-2 counters
    unsigned* buf = hist + 1024;                                  // 2048 staged candidates
    unsigned* cnt = buf + 2048;                                   // [0] staged count, [1] global base
    const unsigned prefix = s->prefix;
    unsigned* out = cand + ((size_t)blockIdx.z * 3 + blockIdx.y) * cand_stride;
    const float2* pl = spec + (size_t)blockIdx.z * img_stride + (size_t)blockIdx.y * PH * M;
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) hist[i] = 0;
    if (threadIdx.x == 0) cnt[0] = 0;
    __syncthreads();
    for (int y = blockIdx.x; y < PH; y += gridDim.x) {
        for (int x0 = 0; x0 < M; x0 += 1024) {
            for (int x = x0 + threadIdx.x; x < M && x < x0 + 1024; x += blockDim.x)
                for_each_mag(pl, PH, M, y, x, [&](unsigned b, unsigned w) {
                    if ((b >> 19) == prefix) {
                        buf[atomicAdd(&cnt[0], 1u)] = (b & 0x7FFFFu) | (w == 2u ? 0x80000000u : 0u);
                        atomicAdd(&hist[(b >> 9) & 1023u], w);
                    }
                });
            __syncthreads();
            const unsigned n = cnt[0];
            if (n) {
                if (threadIdx.x == 0) cnt[1] = atomicAdd(&s->n_cand, n);
                __syncthreads();
                const unsigned base = cnt[1];
                for (unsigned i = threadIdx.x; i < n; i += blockDim.x) out[base + i] = buf[i];
                __syncthreads();
                if (threadIdx.x == 0) cnt[0] = 0;
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < 1024; i += blockDim.x)
        if (hist[i]) atomicAdd(&s->hist[i], hist[i]);
}
constexpr unsigned COLLECT_LDS = (1024 + 2048 + 2) * sizeof(unsigned);      // hist, buf, cnt
// the plain select over the spectrum: histogram, level 1, compaction + level-2 histogram, level 2, level-3 histogram, level 3
constexpr int PLAIN_SELECT_LAUNCHES = 6;
static void launch_plain_select(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, hipStream_t s) {
    const int M = PW >> 1;
    const dim3 g3(stat_blocks(PH, n_images), 3, n_images), gs(3 * n_images);
    hipLaunchKernelGGL(k_hist_spec, g3, dim3(256), HIST_SPEC_LDS, s, spec, PH, M, img_stride, b.st, 1, 1, 1, (const float2*)nullptr);
    hipLaunchKernelGGL(k_select<1>, gs, dim3(SEL_THREADS), sizeof(SelLds), s, b.st, b.med);
    hipLaunchKernelGGL(k_collect, g3, dim3(256), COLLECT_LDS, s, spec, PH, M, img_stride, b.st, b.cand, b.cand_stride);
    hipLaunchKernelGGL(k_select<2>, gs, dim3(SEL_THREADS), sizeof(SelLds), s, b.st, b.med);
    launch_hist_cand<CAND_PLAIN3>(16, n_images, b, s);
    hipLaunchKernelGGL(k_select<3>, gs, dim3(SEL_THREADS), sizeof(SelLds), s, b.st, b.med);
}

// ---------------------------------------------------------------------------
// capacity count_plane S:998-1008 over the bounding box of the annulus.
// The radius test is done on exact integers: s_lo <= y*y+x*x <= s_hi, with the
// bounds derived on the host from the reference's double comparison.  Each block
// walks rows of the box and writes ONE partial count (no global atomics).
//   grid (NB, 3, n_images)  block 256   partial[(img*3+plane)*NB + block]
// ---------------------------------------------------------------------------
// WIDE: grids beyond 32768 need 64-bit y*y+x*x
template <bool WIDE>
__global__ void __launch_bounds__(256) k_capacity(const float2* __restrict__ spec, CapParams P, const float* __restrict__ med_dev,
                           unsigned* __restrict__ partial, const unsigned* __restrict__ only_flagged) {
    if (only_flagged && !only_flagged[blockIdx.z]) return;      // batch path: only the images the bracket pass could not settle
    unsigned* blk = reinterpret_cast<unsigned*>(tfft_smem);
    if (threadIdx.x == 0) blk[0] = 0;
    __syncthreads();
    const int plane = blockIdx.y, img = blockIdx.z;
    const double thr = med_dev ? P.magmin * (double)med_dev[img * 3 + plane] : P.thr[plane];
    const float t2 = mag2_threshold(thr);
    const int M = P.PWi >> 1;
    const float2* pl = spec + (size_t)img * P.img_stride + (size_t)plane * P.PH * M;
    typedef typename std::conditional<WIDE, unsigned long long, unsigned>::type R;
    const R s_lo = (R)P.s_lo, s_hi = (R)P.s_hi;
    unsigned mine = 0;
    for (int y = blockIdx.x; y < P.bh; y += gridDim.x) {
        if (y == 0 || 2 * y == P.PH) continue;
        const R yy = (R)y * (R)y;
        const float2* row = pl + (size_t)y * M;                                  // bins x < M
        const float2* mrow = pl + (size_t)((P.PH - y) & (P.PH - 1)) * M;         // bins x > M: conj of (PH-y, PW-x), same magnitude
        // four independent loads per thread in flight
        for (int x0 = threadIdx.x; x0 < P.bw; x0 += 4 * blockDim.x) {
            float2 v[4]; bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int x = x0 + u * (int)blockDim.x;
                const R s = yy + (R)x * (R)x;
                in[u] = x < P.bw && x != 0 && 2 * x != P.PW && s >= s_lo && s <= s_hi;
                v[u] = in[u] ? (x < M ? row[x] : mrow[P.PW - x]) : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (in[u] && !(mag2_of(v[u]) < t2)) mine++;
        }
    }
    if (mine) atomicAdd(&blk[0], mine);
    __syncthreads();
    if (threadIdx.x == 0) partial[((size_t)img * 3 + plane) * gridDim.x + blockIdx.x] = blk[0];
}
// usable[img] = sum_p floor(c_p/2): one block of three waves per image, wave p sums the partials of plane p
__global__ void k_capacity_final(const unsigned* __restrict__ partial, int nb, unsigned long long* __restrict__ usable,
                                 const unsigned* __restrict__ only_flagged) {
    if (only_flagged && !only_flagged[blockIdx.x]) return;
    unsigned long long* c = reinterpret_cast<unsigned long long*>(tfft_smem);   // [3]
    const int img = blockIdx.x, p = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < 3) c[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a = 0;
    for (int i = lane; i < nb; i += 64) a += partial[((size_t)img * 3 + p) * nb + i];
    if (a) atomicAdd(&c[p], a);
    __syncthreads();
    if (threadIdx.x == 0) usable[img] = c[0] / 2 + c[1] / 2 + c[2] / 2;
}
constexpr unsigned CAPACITY_LDS = 16, CAPACITY_FINAL_LDS = 32;      // one counter; c[3]
constexpr int CAPACITY_LAUNCHES = 2;
hipError_t launch_capacity(const float2* spec, const CapParams& P, int n_images, const float* med_dev,
                           unsigned* partial, unsigned long long* usable, hipStream_t s, const unsigned* only_flagged) {
    // about a dozen rows of the box per block (plain stores of the partial counts, no atomics): long
    // enough to amortise a block's start-up (threshold search, barrier), short enough that the grid still
    // has thousands of blocks with four loads per thread in flight; a single image gets more, shorter blocks
    const int bh = P.bh > 0 ? P.bh : 1;
    int nbi = (bh + 11) / 12;
    if (nbi < stat_fill(n_images)) nbi = stat_fill(n_images);
    if (nbi > bh) nbi = bh;
    if (nbi > TFFT_STAT_MAX_BLOCKS) nbi = TFFT_STAT_MAX_BLOCKS;
    const unsigned nb = (unsigned)nbi;
    // the exact integer radius test fits 32 bits up to 32768 x 32768 and when the host bounds do
    const bool wide = P.PH > 32768 || P.PW > 32768 || P.s_hi > 0xFFFFFFFFull || P.s_lo > 0xFFFFFFFFull;
    if (wide) hipLaunchKernelGGL(k_capacity<true>, dim3(nb, 3, n_images), dim3(256), CAPACITY_LDS, s, spec, P, med_dev, partial, only_flagged);
    else hipLaunchKernelGGL(k_capacity<false>, dim3(nb, 3, n_images), dim3(256), CAPACITY_LDS, s, spec, P, med_dev, partial, only_flagged);
    hipLaunchKernelGGL(k_capacity_final, dim3(n_images), dim3(192), CAPACITY_FINAL_LDS, s, partial, (int)nb, usable, only_flagged);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// the pipelines
// ---------------------------------------------------------------------------
// Which pipeline a launch of n_images planes of PH x PW bins takes, and the kernels it launches.
//   compact: 6 dependent launches instead of 16 (a single image is bound by their latency)
//   finish1: the merged finish kernel walks a plane's candidates (~13 % of its bins) with ONE block: fine up to 2048^2 (270 k
//            candidates), too slow beyond (8 x 4K: 0.52 vs 0.43 ms for the whole statistics stage) -- and only worth it when the
//            dependent-launch latency matters, i.e. for a few images: with 96 planes in flight the three parallel kernels take 35 us,
//            the merged one 44
MedianPlan plan_medians(int PH, int PW, int n_images, const StatOpts& o) {
    const unsigned long long bins = (unsigned long long)PH * PW;
    MedianPlan p;
    p.compact = o.compact && bins <= TFFT_COMPACT_MAX_BINS;
    p.finish1 = p.compact && bins <= TFFT_FINISH1_MAX_BINS && n_images <= TFFT_FINISH1_MAX_IMAGES;
    p.launches = (!p.compact || o.force_fallback) ? 1 : 0;                                                              // k_select_init
    if (!o.force_fallback) p.launches += 1 + guess_launches(o) + 1 + (o.m2 ? 1 : 0) + (p.finish1 ? 1 : FAST_TAIL_LAUNCHES);      // sample .. fast path
    p.launches += p.compact ? 1 : PLAIN_SELECT_LAUNCHES;                                                                 // fallback
    if (o.cap) p.launches += 1 + (p.compact ? 0 : CAPACITY_LAUNCHES);                                                    // settle (+ recount)
    return p;
}
// o.cap != nullptr: also S:998-1008 for every image (magmin in cap->magmin), counted inside the full median pass.
// o.m2: `spec` holds |F|^2 planes (float) and b.col0 the packed columns 0 (the batched delta embeds store nothing else); only the
// fast path of the compact pipeline reads that form
hipError_t launch_medians(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, const StatOpts& o, hipStream_t s) {
    const MedianPlan plan = plan_medians(PH, PW, n_images, o);
    if (o.m2 && (!plan.compact || o.force_fallback)) return hipErrorInvalidValue;
    unsigned nbc = 0;
    if (!plan.compact || o.force_fallback) hipLaunchKernelGGL(k_select_init, dim3(3 * n_images), dim3(256), 0, s, b.st, median_rank(PH, PW));
    if (!o.force_fallback) {
        // fast path: sample histogram -> bracket -> one verified pass
        // sample every step-th row, 64 rows in all (65 k stored values at 2048 columns: the sample median's standard error is
        // ~0.6 % of the value, the bracket reaches 4.4 % to either side)
        const unsigned nb = stat_blocks(PH, n_images);
        launch_hist_sample(spec, PH, PW >> 1, img_stride, n_images, b.st, PH / 64, nb > 32u ? nb : 32u, 1, o.m2 ? b.col0 : nullptr, s);
        launch_guess(PH, PW, n_images, b.st, o, s);
        nbc = launch_collect_bracket(spec, PH, PW, img_stride, n_images, b, o, s);
        if (o.m2) hipLaunchKernelGGL(k_col0_stats, dim3((PH + 255) / 256, 3, n_images), dim3(256), 0, s, b.col0, PH, b.st, b.cand, b.cand_stride, 1);
        if (plan.finish1) hipLaunchKernelGGL(k_select_finish, dim3(3 * n_images), dim3(1024), sizeof(SelLds), s, b.st, b.cand, b.cand_stride, b.med, median_rank(PH, PW));
        else launch_fast_tail(n_images, b, s);
    }
    // fallback: every block returns at once where the fast path verified
    if (plan.compact) launch_median_fallback(spec, PH, PW, img_stride, n_images, b, o.force_fallback != 0, o.m2, s);
    else launch_plain_select(spec, PH, PW, img_stride, n_images, b, s);
    if (o.cap) {
        // capacity: settle the bracket pass's counts with the now known medians; images it could not settle (fallback median,
        // overflowing park list, forced fallback) are recounted -- inside the settle block (compact) or by the plain kernel
        launch_capacity_settle(spec, n_images, b, *o.cap, nbc, plan.compact, o.m2, s);
        if (!plan.compact) {
            hipError_t e = launch_capacity(spec, *o.cap, n_images, b.med, b.partial, b.usable, s, stat_flags(b.partial, n_images));
            if (e != hipSuccess) return e;
        }
    }
    return hipGetLastError();
}

// ---- statistics inside the last forward column step (COLS_STAT): the launches around it.
// (1) bracket guess from a sample of the column tiles (mini: a narrow spectrum of Ms columns written by the plain step with tile_step;
//     nullptr: the sample pass has filled the histograms itself, ColParams::hist_sel)
hipError_t launch_stat_guess(const float2* mini, int PH, int PW, int Ms, size_t mini_img_stride, int col0_packed, int n_images, const StatBufs& b,
                             const StatOpts& o, hipStream_t s) {
    hipError_t e = hipMemsetAsync(b.partial, 0, (size_t)n_images * (3 * TFFT_STAT_MAX_BLOCKS + 1) * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    // ~65 k sampled values per plane
    if (mini) launch_hist_sample(mini, PH, Ms, mini_img_stride, n_images, b.st, ((long long)PH * Ms) / 65536, 32u, col0_packed, nullptr, s);
    launch_guess(PH, PW, n_images, b.st, o, s);
    return hipGetLastError();
}
// (2) after the COLS_STAT step: the packed column 0, the candidates' level-2 histogram, the verified select
hipError_t launch_stat_select(int PH, int n_images, const StatBufs& b, hipStream_t s) {
    hipLaunchKernelGGL(k_col0_stats, dim3((PH + 255) / 256, 3, n_images), dim3(256), 0, s, b.col0, PH, b.st, b.cand, b.cand_stride, 0);
    launch_hist_cand<CAND_LEVEL2>(cand_blocks(n_images), n_images, b, s);
    launch_fast_tail(n_images, b, s);
    return hipGetLastError();
}
// (3) the planes the fast path could not settle (their spectrum has been produced by the gated plain step in between), the capacity
hipError_t launch_stat_settle(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, const StatOpts& o, hipStream_t s) {
    launch_median_fallback(spec, PH, PW, img_stride, n_images, b, false, false, s);
    if (o.cap) launch_capacity_settle(spec, n_images, b, *o.cap, TFFT_STAT_MAX_BLOCKS, true, false, s);
    return hipGetLastError();
}
// kernels of (1) without a narrow spectrum, (2) and (3) together
int stat_tile_launches(const StatOpts& o) { return guess_launches(o) + 2 + FAST_TAIL_LAUNCHES + 1 + (o.cap ? 1 : 0); }

}  // namespace tfft

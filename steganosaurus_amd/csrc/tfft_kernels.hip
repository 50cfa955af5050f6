// tfft_kernels.hip -- hand-written gfx950 kernels of the TurtleFFT hot path.
//
// Data layout in HBM (per resident image = "slot"):
//   spec[3][PH][M]  float2, M = PW/2: HALF spectrum of each colour plane.  The
//                   cover is real, so F[-ky][-kx] = conj(F[ky][kx]) and columns
//                   kx > M are never stored; column 0 holds F[.][0] and F[.][M]
//                   packed as FFT_col(X[.][0] + i*X[.][M]) (both are spectra of
//                   real columns and are separable by Hermitian symmetry).
//   tmp [3][PH][M]  float2: row-pass output / column-pass input (and reverse).
//
// A 2-D transform is: rows (real<->half-complex, length PW, done as a complex
// FFT of length M on packed even/odd samples) + columns (complex, length PH,
// on M columns).  Rows >= H of the padded image are zero and are neither
// stored nor loaded; the inverse computes only rows < H and columns < W.
//
// Reference lines (steganosaurus/src/steganosaur.cpp) replaced by each kernel
// are cited as S:<line>.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "tfft_fft.h"
#include "tfft_device.h"
#include "tfft_kernels.h"

// occupancy floor for a kernel: the register allocator must fit n waves per SIMD (512/n VGPRs)
#ifndef TFFT_WAVES_PER_EU
#define TFFT_WAVES_PER_EU(n) __attribute__((amdgpu_waves_per_eu(n)))
#endif
// Column kernels: occupancy floor handed to the register allocator (waves per SIMD) and whether the next tile is prefetched into
// registers.  Round 3 (same-box A/B, gpurun_out/r3e): from L = 256 on the kernels hold NO tile ahead (32 VGPRs less) and fit 4 waves per
// SIMD instead -- two 512-thread workgroups per CU at L = 512, four 256-thread ones at L = 256 -- so that one workgroup's loads and LDS
// exchanges run under another one's arithmetic: tile-resident extraction 0.542 -> 0.387 ms per 8 x 4K launch, 0.348 -> 0.321 per
// 32 x 1080p.  (Round 2 had measured "two workgroups per CU buy nothing" -- on kernels whose prefetch never overlapped anything
// because their predicated loads defeated s_waitcnt's counting, see load_tile.)  The variants with predicated stores (!FULL: the
// last inverse step, the row-limited extraction of small chunks) need more registers and keep a floor of two.
#ifndef TFFT_COLS_WAVES
#define TFFT_COLS_WAVES(logl) ((logl) >= 8 ? 4 : 1)
#endif
// column kernels of length <= 2^this fetch the next tile into registers while the current one is transformed
#ifndef TFFT_COLS_PF_MAXLOG
#define TFFT_COLS_PF_MAXLOG 7
#endif
#ifndef TFFT_COLS_PFEMIT
#define TFFT_COLS_PFEMIT 0      // 1: COLS_EMIT keeps the register prefetch and one wave per SIMD whatever the length (A/B)
#endif
#ifndef TFFT_ROWS_LAZY_LOG
#define TFFT_ROWS_LAZY_LOG 11
#endif
// column kernels of length >= 2^this read their inter-pass twiddles from an LDS copy of the table instead of holding them in
// registers.  Needed at 512 (no spills); measured at 256 as well (round 2 A/B, one box): final forward step 0.614 vs 0.640 ms
// per 32x1080p launch, nothing lost elsewhere; shorter lengths: no difference
// elements per thread of the one-plane row kernels for rows of 2^TFFT_ROWS_E8_LOG complex samples and more (8: twice the threads per
// row, one more LDS exchange, about half the registers); 99 = never
#ifndef TFFT_ROWS_E8_LOG
#define TFFT_ROWS_E8_LOG 99
#endif
#ifndef TFFT_COLS_LDS_TW_LOG
#define TFFT_COLS_LDS_TW_LOG 8
#endif

namespace tfft {

constexpr int rows_elems(int logm) { return logm >= TFFT_ROWS_E8_LOG ? 8 : elems_for(1 << logm); }

// XCD-aware workgroup order for the kernels whose three colour-plane workgroups share cache lines (the
// interleaved u8 rows).  Workgroups go to the 8 XCDs round robin by linear id and every XCD has its own L2,
// so the three planes of one row group are given ids 8 apart: same XCD, dispatched back to back.  With the
// natural (n2, plane, image) grid they were 256 ids apart -- same XCD but ~2 MB of other traffic later --
// and the u8 lines were written back partially three times (WRITE_SIZE 2.7x the image bytes).
//   grid.x = N2 * 3 (N2 a multiple of 8, else the natural order is kept), grid.y or .z = images
// Used by the fused kernels (N2 row groups) and by the one-plane-per-workgroup row kernels (N2 = H rows).
__device__ __forceinline__ void xcd_plane_order(int N2, int& n2, int& plane) {
    const int L = blockIdx.x;
    if (N2 & 7) { n2 = L % N2; plane = L / N2; return; }
    const int xcd = L & 7, q = L >> 3;
    plane = q % 3;
    n2 = (q / 3) * 8 + xcd;
}

// The four samples of colour plane p (0..2) in one 12-byte group of four RGB pixels a|b|c: bytes p, p+3,
// p+6, p+9.  Two byte-aligned 32-bit windows hold them at byte 0 and byte 3 (v_alignbyte_b32 takes its
// shift modulo 4, hence the select for p == 2), and byte -> float is one v_cvt_f32_ubyteN each: ~10
// instructions per group instead of ~40 for variable 64-bit shifts.
__device__ __forceinline__ void plane_samples4(uint32_t a, uint32_t b, uint32_t c, int p, float bias, float& v0, float& v1, float& v2, float& v3) {
    const uint32_t w0 = __builtin_amdgcn_alignbyte(b, a, (uint32_t)p);                         // bytes p .. p+3
    const uint32_t w1 = (p == 2) ? c : __builtin_amdgcn_alignbyte(c, b, (uint32_t)(p + 2));    // bytes p+6 .. p+9
    v0 = (float)(w0 & 0xFFu) - bias; v1 = (float)(w0 >> 24) - bias;
    v2 = (float)(w1 & 0xFFu) - bias; v3 = (float)(w1 >> 24) - bias;
}

// ---------------------------------------------------------------------------
// rows, forward: u8 RGB row -> (optional centring) -> zero-pad -> real FFT of
// length PW -> M half-spectrum bins per plane.   S:383-386, S:392, S:393-398,
// and the row loop of fft2d S:361.
// These kernels are instruction-issue bound, not bandwidth bound, so the common
// case (W % 4 == 0, 4-byte aligned image, 3 planes per workgroup) stages whole
// 4-pixel groups: one 12-byte load, twelve byte->float conversions and six 8-byte
// LDS stores per thread instead of per-byte index arithmetic.
//   grid  (H, 3/PPB, n_images)   block (T, PPB)   T = M/E
// ---------------------------------------------------------------------------
template <int LOGM, int PPB>
__global__ void __launch_bounds__((1 << LOGM) / rows_elems(LOGM) * PPB) TFFT_WAVES_PER_EU(LOGM >= TFFT_ROWS_LAZY_LOG ? 4 : 1)
k_rows_fwd(const uint8_t* __restrict__ rgb, float2* __restrict__ out, const float2* __restrict__ tw,
                           RowParams P) {
    constexpr int M = 1 << LOGM, E = rows_elems(LOGM), T = M / E;
    const int t = threadIdx.x, pb = threadIdx.y;
    int y = blockIdx.x, plane0 = blockIdx.y * PPB;
    if (PPB == 1) xcd_plane_order(P.H, y, plane0);      // grid.x = 3*H: the three planes of a row on one XCD, back to back
    const int img = blockIdx.z;
    const int tid = pb * T + t, nthr = T * PPB;
    float2* lds = reinterpret_cast<float2*>(tfft_smem);
    float* ldsf = reinterpret_cast<float*>(tfft_smem);
    LayRows lay{LayRows::padded(M)};
    using Sync = typename std::conditional<T == 64, WaveSync, BlockSync>::type;

    const int nbytes = P.W * 3;
    const uint8_t* src = rgb + ((size_t)img * P.H + y) * (size_t)nbytes;
    const bool aligned4 = ((P.W & 3) == 0) && (((uintptr_t)rgb & 3) == 0);
    const bool fast = (PPB == 3) && aligned4;

    // ---- stage the row: bytes -> floats, de-interleaved into the packed (even,odd) layout
    if (PPB == 1 && aligned4) {
        // one plane per workgroup: the same 12-byte groups, keeping the four samples of this plane
        const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
        // all loads first, then the conversions (see k_rowcol_fwd): E/2 four-pixel groups per thread
        constexpr int GMAX = (E + 1) / 2;
        const int ng = P.W >> 2;
        uint32_t ra[GMAX], rb[GMAX], rc[GMAX];
#pragma unroll
        for (int i = 0; i < GMAX; i++) {
            const int g = imin(tid + i * nthr, ng - 1);      // clamped, not predicated: a branch per load serialises them
            ra[i] = srcw[3 * g]; rb[i] = srcw[3 * g + 1]; rc[i] = srcw[3 * g + 2];
        }
#pragma unroll
        for (int i = 0; i < GMAX; i++) {
            const int g = tid + i * nthr;
            if (g < ng) {
                float v0, v1, v2, v3;
                plane_samples4(ra[i], rb[i], rc[i], plane0, P.bias, v0, v1, v2, v3);
                lds[lay.idx(2 * g, 0)] = make_float2(s0 * v0, s1 * v1);
                lds[lay.idx(2 * g + 1, 0)] = make_float2(s0 * v2, s1 * v3);
            }
        }
        for (int m = (P.W >> 1) + tid; m < M; m += nthr) lds[lay.idx(m, 0)] = make_float2(0.f, 0.f);
    } else if (fast) {
        const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;   // (-1)^(x+y), x = 4g+j
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
        for (int g = tid; g < (P.W >> 2); g += nthr) {
            const uint32_t a = srcw[3 * g], b = srcw[3 * g + 1], c = srcw[3 * g + 2];   // R0G0B0R1 G1B1R2G2 B2R3G3B3
            const int i0 = lay.idx(2 * g, 0), i1 = lay.idx(2 * g + 1, 0);
            const float bz = P.bias;
            lds[i0] = make_float2(s0 * ((float)(a & 0xFF) - bz), s1 * ((float)(a >> 24) - bz));
            lds[i1] = make_float2(s0 * ((float)((b >> 16) & 0xFF) - bz), s1 * ((float)((c >> 8) & 0xFF) - bz));
            lds[i0 + lay.pitch] = make_float2(s0 * ((float)((a >> 8) & 0xFF) - bz), s1 * ((float)(b & 0xFF) - bz));
            lds[i1 + lay.pitch] = make_float2(s0 * ((float)(b >> 24) - bz), s1 * ((float)((c >> 16) & 0xFF) - bz));
            lds[i0 + 2 * lay.pitch] = make_float2(s0 * ((float)((a >> 16) & 0xFF) - bz), s1 * ((float)((b >> 8) & 0xFF) - bz));
            lds[i1 + 2 * lay.pitch] = make_float2(s0 * ((float)(c & 0xFF) - bz), s1 * ((float)(c >> 24) - bz));
        }
        for (int m = (P.W >> 1) + tid; m < M; m += nthr) {      // zero padding W..PW-1
#pragma unroll
            for (int b = 0; b < PPB; b++) lds[lay.idx(m, b)] = make_float2(0.f, 0.f);
        }
    } else {
        const int head = (int)((4 - ((uintptr_t)src & 3)) & 3);
        auto put = [&](int off, unsigned byte) {
            const int n = off / 3, ch = off - 3 * n;
            const int b = ch - plane0;
            if (b < 0 || b >= PPB) return;
            float v = (float)byte - P.bias;
            if (P.center && ((n + y) & 1)) v = -v;
            ldsf[2 * lay.idx(n >> 1, b) + (n & 1)] = v;
        };
        for (int o = tid; o < head && o < nbytes; o += nthr) put(o, src[o]);
        const int nwords = nbytes > head ? (nbytes - head) / 4 : 0;
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src + head);
        for (int w = tid; w < nwords; w += nthr) {
            const uint32_t v = srcw[w];
            const int o = head + 4 * w;
            put(o, v & 0xFF); put(o + 1, (v >> 8) & 0xFF); put(o + 2, (v >> 16) & 0xFF); put(o + 3, v >> 24);
        }
        for (int o = head + 4 * nwords + tid; o < nbytes; o += nthr) put(o, src[o]);
        for (int n = P.W + tid; n < 2 * M; n += nthr) {   // zero padding W..PW-1
#pragma unroll
            for (int b = 0; b < PPB; b++) ldsf[2 * lay.idx(n >> 1, b) + (n & 1)] = 0.0f;
        }
    }
    // twiddles of the radix passes and of the real-FFT split (indices depend on the thread only):
    // issued before the barrier so their L2 latency overlaps the staging
    // Rows of 4096 and more samples (two or more waves per row): the prefetched pass twiddles cost 54
    // registers, which at 171 VGPRs leaves two waves per SIMD; fetched at the point of use the kernel fits
    // four, and the extra occupancy hides more latency than the prefetch did.
    constexpr bool LAZY = LOGM >= TFFT_ROWS_LAZY_LOG;
    float2 W[LAZY ? 1 : tw_regs<M, E>()];
    if (!LAZY) fft_prefetch_twiddles<M, E, +1>(W, t, tw, 2);
    constexpr int NSPLIT = (M / 2) / T + 1;
    float2 wk[NSPLIT];
#pragma unroll
    for (int j = 0; j < NSPLIT; j++) wk[j] = tw[imin(t + j * T, M / 2)];
    lds_barrier();

    // ---- complex FFT of length M on z[m] = x[2m] + i x[2m+1].  From here on a thread only touches
    // its own plane's LDS slab; when that plane is exactly one wave (T == 64) no workgroup barrier is needed.
    float2 u[E];
#pragma unroll
    for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, pb)];
    Sync::sync();
    if (LAZY) fft_block_lazy<M, E, +1, Sync>(u, lds, lay, t, pb, tw, 2);
    else fft_block<M, E, +1, Sync>(u, lds, lay, t, pb, W);
#pragma unroll
    for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, pb)] = u[m];
    Sync::sync();

    // ---- split into the spectrum of the real row: X[k] = Ev[k] + w^k Od[k], w = exp(+2 pi i/PW)
    float2* dst = out + (size_t)img * P.img_stride + ((size_t)(plane0 + pb) * P.PH + y) * M;
#pragma unroll
    for (int j = 0; j < NSPLIT; j++) {
        const int k = t + j * T;
        if (k > M / 2) break;
        const int k2 = (M - k) & (M - 1);
        const float2 zk = lds[lay.idx(k, pb)], zm = lds[lay.idx(k2, pb)];
        float2 xk, xmk;
        rsplit_fwd(zk, zm, wk[j], xk, xmk);
        if (k == 0) {
            dst[0] = make_float2(xk.x, xmk.x);               // X[0] = Ev + Od and X[M] = Ev - Od (w = 1), both real, packed
        } else {
            dst[k] = xk;
            if (k2 != k) dst[k2] = xmk;
        }
    }
}

// ---------------------------------------------------------------------------
// rows + first column step, fused (images up to 2048 wide, PH = N1*N2 with N1 = 8):
// a workgroup holds the N1 rows y = n1*N2 + n2 of one plane in LDS, one wave per row.
// Each wave does the real FFT of its row exactly like k_rows_fwd (rows >= H are zero
// and skipped), the workgroup then takes the length-N1 DFT across the rows for every
// column, multiplies by w^(n2*k1) and stores rows k1*N2 + n2: the result is what
// k_rows_fwd followed by the first k_fft_cols step leaves in `out`, without writing
// and re-reading the H x M intermediate.
//   grid (3*N2, n_images) in xcd_plane_order   block (64, N1)   M = 1024, E = 16
// ---------------------------------------------------------------------------
// LOGM = 10: images up to 2048 wide, one wave per row (wave-level exchanges, no barrier inside the row transform).
// LOGM = 11: up to 4096 wide, two waves per row, 1024-thread workgroups holding 8 x 16 KB rows (155 KB of LDS, one workgroup
//            per CU); the row transform's exchanges are workgroup barriers, which the waves of padded rows just sit out.
template <int LOGN1, int LOGM>
__global__ void __launch_bounds__(1 << (LOGM - 4 + LOGN1)) k_rowcol_fwd(const uint8_t* __restrict__ rgb, float2* __restrict__ out,
                             const float2* __restrict__ tw, const float2* __restrict__ tw_h, RowParams P) {
    constexpr int M = 1 << LOGM, E = 16, T = M / E, N1 = 1 << LOGN1;
    using Sync = typename std::conditional<T == 64, WaveSync, BlockSync>::type;
    const int t = threadIdx.x, n1 = threadIdx.y;
    const int N2 = P.PH >> LOGN1;
    int n2, plane;
    xcd_plane_order(N2, n2, plane);
    const int img = blockIdx.y;
    const int y = n1 * N2 + n2;
    float2* lds = reinterpret_cast<float2*>(tfft_smem);
    float* ldsf = reinterpret_cast<float*>(tfft_smem);
    LayRows lay{LayRows::padded(M)};
    const bool live = y < P.H;          // wave uniform: a row is one or two whole waves

    // pass twiddles exp(+2 pi i j/M), j < M, staged once per workgroup behind the row slabs: the radix
    // passes then read them with LDS latency instead of L2 latency (8 KB; two workgroups still fit a CU)
    float2* ltw = lds + (size_t)N1 * lay.pitch;
    float2* lwc = ltw + M;              // + the N1 column-step twiddles exp(+2 pi i n2 k1/PH) of this workgroup

    // ---- every global load of the prologue is issued before the first LDS store that needs one of them:
    // s_waitcnt counts in order, so a store placed between two groups of loads makes the second group
    // wait a full memory round trip for the first (table fill loop, per-iteration staging loads and the
    // column twiddles after the barrier each cost ~1 us per workgroup that way)
    constexpr int NT = M / (T * N1);
    float2 tv[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) tv[i] = tw[2 * (n1 * T + t + i * T * N1)];
    float2 cv = make_float2(0.f, 0.f);
    if (n1 == 0 && t < N1) cv = tw_h[(n2 * t) & (P.PH - 1)];
    // split twiddle exp(+2 pi i x/PW) of the column pair (x, M-x) this thread finishes in the column phase:
    // x = n1*T + t in [0, M/2); thread 0 owns the packed column 0 and the self-paired column M/2
    const int px = n1 * T + t;
    const float2 wsx = tw[px], wsh = tw[M / 2];
    const uint8_t* src = rgb + ((size_t)img * P.H + (live ? y : 0)) * (size_t)(P.W * 3);
    const bool fastp = live && ((P.W & 3) == 0) && (((uintptr_t)rgb & 3) == 0);
    constexpr int GMAX = (2 * M / 4) / T;               // 4-pixel groups per lane
    const int ng = P.W >> 2;
    uint32_t ra[GMAX], rb[GMAX], rc[GMAX];
    if (fastp) {
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
#pragma unroll
        for (int i = 0; i < GMAX; i++) {
            const int g = imin(t + i * T, ng - 1);      // clamped, not predicated: a branch per load serialises them (s_waitcnt in every arm)
            ra[i] = srcw[3 * g]; rb[i] = srcw[3 * g + 1]; rc[i] = srcw[3 * g + 2];
        }
    }
#pragma unroll
    for (int i = 0; i < NT; i++) ltw[n1 * T + t + i * T * N1] = tv[i];
    if (n1 == 0 && t < N1) lwc[t] = cv;
    if (fastp) {
        const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;
#pragma unroll
        for (int i = 0; i < GMAX; i++) {
            const int g = t + i * T;
            if (g < ng) {
                float v0, v1, v2, v3;
                plane_samples4(ra[i], rb[i], rc[i], plane, P.bias, v0, v1, v2, v3);
                lds[lay.idx(2 * g, n1)] = make_float2(s0 * v0, s1 * v1);
                lds[lay.idx(2 * g + 1, n1)] = make_float2(s0 * v2, s1 * v3);
            }
        }
        for (int m = (P.W >> 1) + t; m < M; m += T) lds[lay.idx(m, n1)] = make_float2(0.f, 0.f);
    } else if (live) {
        for (int n = t; n < 2 * M; n += T) {
            float v = 0.0f;
            if (n < P.W) { v = (float)src[3 * n + plane] - P.bias; if (P.center && ((n + y) & 1)) v = -v; }
            ldsf[2 * lay.idx(n >> 1, n1) + (n & 1)] = v;
        }
    }
    lds_barrier();                    // the twiddle table and every live row are staged
    // pass twiddles are read at the point of use from the LDS copy: prefetching them into registers
    // (54 more VGPRs) leaves room for one workgroup per CU instead of two and measured 0.87 ms against 0.66 ms
    if constexpr (T == 64) {            // one wave per row: the waves of padded rows skip the transform altogether
        if (live) {
            float2 u[E];
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, n1)];
            WaveSync::sync();
            fft_block_lazy<M, E, +1, WaveSync>(u, lds, lay, t, n1, ltw, 1);
#pragma unroll
            for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, n1)] = u[m];      // Z = FFT of the packed (even, odd) row
        } else {
#pragma unroll
            for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, n1)] = make_float2(0.f, 0.f);
        }
    } else {                            // two waves per row: everybody meets at the exchange barriers, padded rows compute nothing
        float2 u[E];
        if (live) {
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, n1)];
        }
        Sync::sync();
        fft_block_lazy<M, E, +1, Sync>(u, lds, lay, t, n1, ltw, 1, live);
#pragma unroll
        for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, n1)] = live ? u[m] : make_float2(0.f, 0.f);
    }
    lds_barrier();

    // ---- real-FFT split and length-N1 DFT across the rows in one go, per column PAIR (x, M-x): the split
    // X[x] = Ev + w^x Od, X[M-x] = conj(Ev - w^x Od) needs Z[x] and Z[M-x] of the same row, and w^x is the same for
    // all N1 rows, so the thread that owns the pair loads both columns once (a separate in-place split pass cost
    // four more LDS accesses per bin and nine twiddle registers per row thread).  M/2 threads, one pair each;
    // output row k1*N2 + n2, times exp(+2 pi i n2 k1/PH).
    static_assert(T * N1 == M / 2, "one column pair per thread");
    float2 wc[N1];                      // from the LDS copy made at the top: as global loads here they were a
#pragma unroll                          // full memory round trip between the barrier and the first store
    for (int k1 = 0; k1 < N1; k1++) wc[k1] = lwc[k1];
    float2* dst = out + (size_t)img * P.img_stride + (size_t)plane * P.PH * M + (size_t)n2 * M;
    const int xa = px, xb = (px == 0) ? M / 2 : M - px;       // thread 0: packed column 0, then the self-paired column M/2
    float2 va[N1], vb[N1];
#pragma unroll
    for (int r = 0; r < N1; r++) {
        const float2 zk = lds[lay.idx(xa, r)], zm = lds[lay.idx((M - xa) & (M - 1), r)];
        rsplit_fwd(zk, zm, wsx, va[r], vb[r]);
        if (px == 0) {
            va[r] = make_float2(va[r].x, vb[r].x);                                     // X[0] and X[M] (w = 1), both real, packed
            const float2 zh = lds[lay.idx(M / 2, r)];                                  // column M/2 pairs with itself
            const float2 ah = make_float2(zh.x, 0.0f), dh = make_float2(0.0f, 2.0f * zh.y);
            const float2 odh = make_float2(0.5f * dh.y, -0.5f * dh.x);
            vb[r] = cadd(ah, cmul(wsh, odh));
        }
    }
    DftReg<N1, +1, 0, N1>::run(va);
    DftReg<N1, +1, 0, N1>::run(vb);
#pragma unroll
    for (int k1 = 0; k1 < N1; k1++) {
        dst[(size_t)k1 * N2 * M + xa] = cmul(va[bitrev(k1, LOGN1)], wc[k1]);
        dst[(size_t)k1 * N2 * M + xb] = cmul(vb[bitrev(k1, LOGN1)], wc[k1]);
    }
}

// ---------------------------------------------------------------------------
// The same fused kernel with LIVE rows only.  Of the N1 = 8 rows n1*N2 + n2 a workgroup covers, those below the image's
// height are the first NL = ceil or floor(H / N2) (4 or 5 of 8 at 1920x1080 and 3840x2160); the others are padding.  The
// kernel above keeps a wave (pair) and an LDS slab for every one of the 8: the waves of padded rows idle at the barriers and
// their slabs hold zeros.  Here a workgroup has NL rows' worth of threads and slabs and nothing else, so a CU holds three
// workgroups instead of two at 2048 columns (43-52 KB each) and two instead of one at 4096 columns with NL <= 4 (70 KB, pass
// twiddles read from the L2-resident table instead of an LDS copy) -- the workgroups of a CU overlap each other's load,
// transform and store phases, which is where these kernels get their bandwidth from.  The column phase loops over the M/2
// column pairs with however many threads there are; rows >= NL enter the length-8 DFT as zeros.
//   launched once per value of NL: grid (3 * n2_cnt, n_images), block (T, NL), rows n2 in [n2_lo, n2_lo + n2_cnt)
// ---------------------------------------------------------------------------
template <int LOGM, int NL>
__global__ void __launch_bounds__((1 << (LOGM - 4)) * NL) k_rowcol_fwd_live(const uint8_t* __restrict__ rgb, float2* __restrict__ out,
                             const float2* __restrict__ tw, const float2* __restrict__ tw_h, RowParams P, int n2_lo, int n2_cnt) {
    constexpr int M = 1 << LOGM, E = 16, T = M / E, N1 = 8, NTHR = T * NL;
    constexpr bool LTW = (LOGM <= 10);                  // pass twiddles: LDS copy (2048 columns) or the global table (4096 columns)
    constexpr int NPAIR = ((M / 2) + NTHR - 1) / NTHR;  // column pairs per thread
    using Sync = typename std::conditional<T == 64, WaveSync, BlockSync>::type;
    const int t = threadIdx.x, n1 = threadIdx.y, tid = n1 * T + t;
    const int N2 = P.PH >> 3;
    int n2, plane;
    xcd_plane_order(n2_cnt, n2, plane);
    n2 += n2_lo;
    const int img = blockIdx.y;
    const int y = n1 * N2 + n2;
    float2* lds = reinterpret_cast<float2*>(tfft_smem);
    float* ldsf = reinterpret_cast<float*>(tfft_smem);
    LayRows lay{LayRows::padded(M)};
    const bool live = y < P.H;          // always true except for images shorter than N2 rows (NL = 1 covers their padded groups)
    float2* ltw = lds + (size_t)NL * lay.pitch;
    float2* lwc = ltw + (LTW ? M : 0);

    // ---- prologue: every global load before the first dependent LDS store (see k_rowcol_fwd)
    constexpr int NT = LTW ? (M + NTHR - 1) / NTHR : 1;
    float2 tv[NT];
    if (LTW) {
#pragma unroll
        for (int i = 0; i < NT; i++) tv[i] = tw[2 * imin(tid + i * NTHR, M - 1)];
    }
    float2 cv = make_float2(0.f, 0.f);
    if (tid < N1) cv = tw_h[(n2 * tid) & (P.PH - 1)];
    float2 wsx[NPAIR];
#pragma unroll
    for (int i = 0; i < NPAIR; i++) wsx[i] = tw[imin(tid + i * NTHR, M / 2)];      // split twiddles exp(+2 pi i x/PW) of this thread's pairs
    const float2 wsh = tw[M / 2];
    const uint8_t* src = rgb + ((size_t)img * P.H + (live ? y : 0)) * (size_t)(P.W * 3);
    const bool fastp = live && ((P.W & 3) == 0) && (((uintptr_t)rgb & 3) == 0);
    constexpr int GMAX = (2 * M / 4) / T;
    const int ng = P.W >> 2;
    uint32_t ra[GMAX], rb[GMAX], rc[GMAX];
    if (fastp) {
        const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
#pragma unroll
        for (int i = 0; i < GMAX; i++) {
            const int g = imin(t + i * T, ng - 1);
            ra[i] = srcw[3 * g]; rb[i] = srcw[3 * g + 1]; rc[i] = srcw[3 * g + 2];
        }
    }
    if (LTW) {
#pragma unroll
        for (int i = 0; i < NT; i++) if (tid + i * NTHR < M) ltw[tid + i * NTHR] = tv[i];
    }
    if (tid < N1) lwc[tid] = cv;
    if (fastp) {
        const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;
#pragma unroll
        for (int i = 0; i < GMAX; i++) {
            const int g = t + i * T;
            if (g < ng) {
                float v0, v1, v2, v3;
                plane_samples4(ra[i], rb[i], rc[i], plane, P.bias, v0, v1, v2, v3);
                lds[lay.idx(2 * g, n1)] = make_float2(s0 * v0, s1 * v1);
                lds[lay.idx(2 * g + 1, n1)] = make_float2(s0 * v2, s1 * v3);
            }
        }
        for (int m = (P.W >> 1) + t; m < M; m += T) lds[lay.idx(m, n1)] = make_float2(0.f, 0.f);
    } else if (live) {
        for (int n = t; n < 2 * M; n += T) {
            float v = 0.0f;
            if (n < P.W) { v = (float)src[3 * n + plane] - P.bias; if (P.center && ((n + y) & 1)) v = -v; }
            ldsf[2 * lay.idx(n >> 1, n1) + (n & 1)] = v;
        }
    }
    lds_barrier();
    {
        float2 u[E];
        if (live) {
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, n1)];
        }
        Sync::sync();
        if (LTW) fft_block_lazy<M, E, +1, Sync>(u, lds, lay, t, n1, ltw, 1, live);
        else fft_block_lazy<M, E, +1, Sync>(u, lds, lay, t, n1, tw, 2, live);
#pragma unroll
        for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, n1)] = live ? u[m] : make_float2(0.f, 0.f);
    }
    lds_barrier();

    // ---- real-FFT split + length-8 DFT across the rows per column pair (x, M-x); rows >= NL are zeros
    float2 wc[N1];
#pragma unroll
    for (int k1 = 0; k1 < N1; k1++) wc[k1] = lwc[k1];
    float2* dst = out + (size_t)img * P.img_stride + (size_t)plane * P.PH * M + (size_t)n2 * M;
#pragma unroll
    for (int i = 0; i < NPAIR; i++) {
        const int px = tid + i * NTHR;
        if (px >= M / 2) break;
        const int xa = px, xb = (px == 0) ? M / 2 : M - px;
        float2 va[N1], vb[N1];
#pragma unroll
        for (int r = 0; r < N1; r++) {
            if (r < NL) {
                const float2 zk = lds[lay.idx(xa, r)], zm = lds[lay.idx((M - xa) & (M - 1), r)];
                rsplit_fwd(zk, zm, wsx[i], va[r], vb[r]);
                if (px == 0) {
                    va[r] = make_float2(va[r].x, vb[r].x);                                     // X[0] and X[M] (w = 1), both real, packed
                    const float2 zh = lds[lay.idx(M / 2, r)];                                  // column M/2 pairs with itself
                    const float2 ah = make_float2(zh.x, 0.0f), dh = make_float2(0.0f, 2.0f * zh.y);
                    const float2 odh = make_float2(0.5f * dh.y, -0.5f * dh.x);
                    vb[r] = cadd(ah, cmul(wsh, odh));
                }
            } else {
                va[r] = make_float2(0.f, 0.f); vb[r] = make_float2(0.f, 0.f);
            }
        }
        DftReg<N1, +1, 0, N1>::run(va);
        DftReg<N1, +1, 0, N1>::run(vb);
#pragma unroll
        for (int k1 = 0; k1 < N1; k1++) {
            dst[(size_t)k1 * N2 * M + xa] = cmul(va[bitrev(k1, 3)], wc[k1]);
            dst[(size_t)k1 * N2 * M + xb] = cmul(vb[bitrev(k1, 3)], wc[k1]);
        }
    }
}

// clamp(round(v), 0, 255) with C round() semantics (half away from zero, S:389) for the values that
// survive the clamp: negatives go to 0 either way, so only v >= 0 needs exact half-up rounding
// (v - trunc(v) is exact in fp32, unlike v + 0.5f).
// a byte of the cover through an ALIGNED dword load (cover_word) decoded later (cover_pick): a wave's byte loads at a stride of 6
// (pixel pairs of one plane) are gathers; as dwords they coalesce
__device__ __forceinline__ uint32_t cover_word(const uint8_t* p) {
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)3);
}
__device__ __forceinline__ unsigned cover_pick(uint32_t w, const uint8_t* p) {
    return (w >> (8u * (unsigned)(reinterpret_cast<uintptr_t>(p) & 3))) & 255u;
}
__device__ __forceinline__ unsigned quantise_u8(float v) {
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    const float r = truncf(v);
    return (unsigned)r + ((v - r >= 0.5f) ? 1u : 0u);
}

// ---------------------------------------------------------------------------
// last inverse column step + rows, fused (mirror image of k_rowcol_fwd): for every
// column the length-N1 inverse DFT across the rows k1*N2 + n2 gives the rows
// n1*N2 + n2 in LDS; one wave per row then does the half-spectrum -> real row
// transform, scales, rounds and stores its plane's bytes.  Rows >= H are dropped.
// Replaces the second k_fft_cols inverse step followed by k_rows_inv.
//   grid (3*N2, n_images) in xcd_plane_order   block (64, N1)   M = 1024, E = 16
// ---------------------------------------------------------------------------
template <int LOGN1, int LOGM>
// (140 VGPRs leave one workgroup of 8 waves per CU; forcing 128 with amdgpu_waves_per_eu(4) spills 19 dwords and
// measured 0.71 ms against 0.58 ms)
__global__ void __launch_bounds__(1 << (LOGM - 4 + LOGN1)) k_colrow_inv(const float2* __restrict__ in, uint8_t* __restrict__ rgb,
                             const float2* __restrict__ tw, RowParams P) {
    constexpr int M = 1 << LOGM, E = 16, T = M / E, N1 = 1 << LOGN1;
    using Sync = typename std::conditional<T == 64, WaveSync, BlockSync>::type;
    const int t = threadIdx.x, n1 = threadIdx.y;
    const int N2 = P.PH >> LOGN1;
    int n2, plane;
    xcd_plane_order(N2, n2, plane);
    const int img = blockIdx.y;
    const int y = n1 * N2 + n2;
    float2* lds = reinterpret_cast<float2*>(tfft_smem);
    float* ldsf = reinterpret_cast<float*>(tfft_smem);
    LayRows lay{LayRows::padded(M)};

    // pass twiddles exp(+2 pi i j/M) staged in LDS behind the row slabs (as in k_rowcol_fwd): LDS reads need
    // no 64-bit address pair per twiddle, which is what kept this kernel above 128 VGPRs (one workgroup per CU)
    float2* ltw = lds + (size_t)N1 * lay.pitch;
    constexpr int NT = M / (T * N1);    // stored to LDS after the column loads have been issued (see k_rowcol_fwd)
    float2 tv[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) tv[i] = tw[2 * (n1 * T + t + i * T * N1)];

    // ---- length-N1 inverse DFT across the rows and the half-spectrum -> packed-row split in one go, per column
    // PAIR (x, M-x) (mirror image of k_rowcol_fwd): Z[x] = Ev + i Od, Z[M-x] = conj(Ev) + i conj(Od) with
    // Ev = (X[x] + conj X[M-x])/2, Od = (X[x] - conj X[M-x])/2 * w^-x, and w^x is shared by the N1 rows.  One pair
    // per thread; thread 0 owns the packed column 0 and the self-paired column M/2.  Rows >= H are not stored.
    static_assert(T * N1 == M / 2, "one column pair per thread");
    const int px = n1 * T + t;
    const int xa = px, xb = (px == 0) ? M / 2 : M - px;
    const float2 wsx = tw[px], wsh = tw[M / 2];
    const float2* src = in + (size_t)img * P.img_stride + (size_t)plane * P.PH * M + (size_t)n2 * M;
    // delta embedding: the transform is added to the cover's pixels.  Their bytes are fetched in one batch BEFORE any store (a load
    // after a store to a pointer that may alias it -- in-place embedding is allowed -- is not hoisted: 15 exposed round trips per row,
    // 0.42 -> 0.79 ms), and by the one-wave-per-row variant before its row transform, whose registers allow it
    const size_t pix0 = ((size_t)img * P.H + y) * (size_t)P.W * 3 + plane;
    const uint8_t* cov = P.cover ? P.cover + pix0 : nullptr;
    // W % 4 == 0 and an aligned cover: a thread takes groups of 4 pixels = 12 contiguous bytes = 3 coalesced dwords (its plane's 4
    // bytes are picked out of them); otherwise the two bytes of a pixel pair come out of the aligned dwords holding them
    const bool cov4 = cov && (P.W & 3) == 0 && (reinterpret_cast<uintptr_t>(P.cover) & 3) == 0;
    uint32_t cw[2 * E];                 // raw dwords (decoded where they are used)
    auto load_cover = [&]() {
        if (cov4) {
            const uint32_t* row = reinterpret_cast<const uint32_t*>(cov - plane);
            const int last = (P.W >> 2) - 1;
#pragma unroll
            for (int i = 0; i < E / 2; i++) {
                const int q = imin(t + i * T, last);                  // clamped: every load unconditional
                cw[3 * i] = row[3 * q]; cw[3 * i + 1] = row[3 * q + 1]; cw[3 * i + 2] = row[3 * q + 2];
            }
        } else {
            const int last = (P.W >> 1) - 1;
#pragma unroll
            for (int i = 0; i < E; i++) {
                const uint8_t* a = cov + 6 * imin(t + i * T, last);
                cw[2 * i] = cover_word(a);
                cw[2 * i + 1] = cover_word(a + 3);
            }
        }
    };
    float2 va[N1], vb[N1];
#pragma unroll
    for (int k1 = 0; k1 < N1; k1++) { va[k1] = src[(size_t)k1 * N2 * M + xa]; vb[k1] = src[(size_t)k1 * N2 * M + xb]; }
    if (T == 64 && y < P.H && cov && (P.W & 1) == 0) load_cover();      // behind the column loads in the queue, consumed after the row transform (there: 0.51 vs 0.48 ms)
    DftReg<N1, -1, 0, N1>::run(va);
    DftReg<N1, -1, 0, N1>::run(vb);
#pragma unroll
    for (int r = 0; r < N1; r++) {
        if (r * N2 + n2 >= P.H) continue;                     // workgroup uniform
        const float2 xk = va[bitrev(r, LOGN1)], xm = vb[bitrev(r, LOGN1)];
        if (px == 0) {
            lds[lay.idx(0, r)] = make_float2(0.5f * (xk.x + xk.y), 0.5f * (xk.x - xk.y));      // X[0], X[M] packed in bin 0
            const float2 od = cmul(make_float2(0.0f, xm.y), cconj(wsh));                       // column M/2 pairs with itself
            lds[lay.idx(M / 2, r)] = make_float2(xm.x - od.y, 0.0f + od.x);
        } else {
            float2 za, zb;
            rsplit_inv(xk, xm, wsx, za, zb);
            lds[lay.idx(xa, r)] = za;
            lds[lay.idx(xb, r)] = zb;
        }
    }
#pragma unroll
    for (int i = 0; i < NT; i++) ltw[n1 * T + t + i * T * N1] = tv[i];
    lds_barrier();
    const bool live = y < P.H;          // wave uniform (a row is one or two whole waves)
    if constexpr (T == 64) {            // one wave per row: no workgroup barrier follows, padded rows are done
        if (!live) return;
        WaveSync::sync();
        float2 u[E];
#pragma unroll
        for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, n1)];
        WaveSync::sync();
        fft_block_lazy<M, E, -1, WaveSync>(u, lds, lay, t, n1, ltw, 1);
#pragma unroll
        for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, n1)] = cscale(u[m], P.scale);
        WaveSync::sync();
    } else {                            // two waves per row: padded rows stay for the exchange barriers and compute nothing
        float2 u[E];
        if (live) {
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, n1)];
        }
        Sync::sync();
        fft_block_lazy<M, E, -1, Sync>(u, lds, lay, t, n1, ltw, 1, live);
        if (live) {
#pragma unroll
            for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, n1)] = cscale(u[m], P.scale);
        }
        Sync::sync();
        if (!live) return;
    }

    // ---- quantise and store this plane's bytes of row y
    uint8_t* dst = rgb + pix0;
    if ((P.W & 1) == 0) {
        const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;
        if (cov && T != 64) load_cover();
        if (cov4) {
            const unsigned sh = 8u * (unsigned)plane;
#pragma unroll
            for (int i = 0; i < E / 2; i++) {
                const int q = t + i * T;
                if (q < (P.W >> 2)) {
                    const uint32_t w0 = cw[3 * i], w1 = cw[3 * i + 1], w2 = cw[3 * i + 2];
                    // bytes 3j + plane of the 12: pixel j's sample of this plane
                    const uint32_t x0 = w0, x1 = (w0 >> 24) | (w1 << 8), x2 = (w1 >> 16) | (w2 << 16), x3 = w2 >> 8;
                    const float2 va = lds[lay.idx(2 * q, n1)], vb = lds[lay.idx(2 * q + 1, n1)];
                    uint8_t* d = dst + 12 * q;
                    d[0] = (uint8_t)quantise_u8(s0 * va.x + (float)((x0 >> sh) & 255u));
                    d[3] = (uint8_t)quantise_u8(s1 * va.y + (float)((x1 >> sh) & 255u));
                    d[6] = (uint8_t)quantise_u8(s0 * vb.x + (float)((x2 >> sh) & 255u));
                    d[9] = (uint8_t)quantise_u8(s1 * vb.y + (float)((x3 >> sh) & 255u));
                }
            }
        } else if (cov) {
#pragma unroll
            for (int i = 0; i < E; i++) {
                const int m = t + i * T;
                if (m < (P.W >> 1)) {
                    const float2 v = lds[lay.idx(m, n1)];
                    {
                    dst[6 * m] = (uint8_t)quantise_u8(s0 * v.x + (float)cover_pick(cw[2 * i], cov + 6 * m));
                    dst[6 * m + 3] = (uint8_t)quantise_u8(s1 * v.y + (float)cover_pick(cw[2 * i + 1], cov + 6 * m + 3));
                    }
                }
            }
        } else {
            for (int m = t; m < (P.W >> 1); m += T) {
                const float2 v = lds[lay.idx(m, n1)];
                dst[6 * m] = (uint8_t)quantise_u8(s0 * v.x + P.bias);
                dst[6 * m + 3] = (uint8_t)quantise_u8(s1 * v.y + P.bias);
            }
        }
    } else {
        for (int n = t; n < P.W; n += T) {
            float v = ldsf[2 * lay.idx(n >> 1, n1) + (n & 1)];
            if (P.center && ((n + y) & 1)) v = -v;
            dst[3 * n] = (uint8_t)quantise_u8(v + (cov ? (float)cov[3 * n] : P.bias));
        }
    }
}

// ---------------------------------------------------------------------------
// rows, inverse: M half-spectrum bins -> real row of length PW (only x < W is
// produced) -> scale -> (centring) -> round half away, clamp, interleave u8.
// The row loop of fft2d(inverse) S:361/S:357, ifft_crop S:399-403, S:1102,
// from_planes_u8 S:387-391.
//   grid  (H, 3/PPB, n_images)   block (T, PPB)
// ---------------------------------------------------------------------------
template <int LOGM, int PPB>
__global__ void __launch_bounds__((1 << LOGM) / rows_elems(LOGM) * PPB) TFFT_WAVES_PER_EU(LOGM >= TFFT_ROWS_LAZY_LOG ? 4 : 1)
k_rows_inv(const float2* __restrict__ in, uint8_t* __restrict__ rgb, const float2* __restrict__ tw,
                           RowParams P) {
    constexpr int M = 1 << LOGM, E = rows_elems(LOGM), T = M / E;
    const int t = threadIdx.x, pb = threadIdx.y;
    int y = blockIdx.x, plane0 = blockIdx.y * PPB;
    if (PPB == 1) xcd_plane_order(P.H, y, plane0);      // grid.x = 3*H: the three planes of a row on one XCD, back to back
    const int img = blockIdx.z;
    const int tid = pb * T + t, nthr = T * PPB;
    float2* lds = reinterpret_cast<float2*>(tfft_smem);
    float* ldsf = reinterpret_cast<float*>(tfft_smem);
    LayRows lay{LayRows::padded(M)};
    using Sync = typename std::conditional<T == 64, WaveSync, BlockSync>::type;

    const float2* src = in + (size_t)img * P.img_stride + ((size_t)(plane0 + pb) * P.PH + y) * M;
    // ---- Z[k] = Ev[k] + i Od[k]:  Ev = (X[k]+conj X[M-k])/2,  Od = (X[k]-conj X[M-k])/2 * w^-k, one pair (k, M-k)
    // at a time straight from global memory (Ev[M-k] = conj Ev[k], Od[M-k] = conj Od[k]; see k_colrow_inv): both
    // streams are coalesced (k ascending, M-k descending) and the packed row reaches LDS already split.
    constexpr int NSPLIT = (M / 2) / T + 1;
    float2 xk[NSPLIT], xm[NSPLIT], wk[NSPLIT];      // every load first (clamped, unpredicated), then the arithmetic
#pragma unroll
    for (int j = 0; j < NSPLIT; j++) {
        const int k = imin(t + j * T, M / 2);
        xk[j] = src[k]; xm[j] = src[(M - k) & (M - 1)]; wk[j] = tw[k];      // split twiddles exp(+2 pi i k/PW)
    }
    constexpr bool LAZY = LOGM >= TFFT_ROWS_LAZY_LOG;      // see k_rows_fwd
    float2 W[LAZY ? 1 : tw_regs<M, E>()];
    if (!LAZY) fft_prefetch_twiddles<M, E, -1>(W, t, tw, 2);
#pragma unroll
    for (int j = 0; j < NSPLIT; j++) {
        const int k = t + j * T;
        if (k <= M / 2) {
            const int k2 = (M - k) & (M - 1);
            float2 zk, zk2;
            rsplit_inv(xk[j], xm[j], wk[j], zk, zk2);
            if (k == 0) zk = make_float2(0.5f * (xk[j].x + xk[j].y), 0.5f * (xk[j].x - xk[j].y));     // X[0], X[M] packed in bin 0
            lds[lay.idx(k, pb)] = zk;
            if (k2 != k) lds[lay.idx(k2, pb)] = zk2;
        }
    }
    Sync::sync();
    float2 u[E];
#pragma unroll
    for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, pb)];
    Sync::sync();
    if (LAZY) fft_block_lazy<M, E, -1, Sync>(u, lds, lay, t, pb, tw, 2);
    else fft_block<M, E, -1, Sync>(u, lds, lay, t, pb, W);
#pragma unroll
    for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, pb)] = cscale(u[m], P.scale);
    lds_barrier();

    // ---- quantise and store
    const int nbytes = P.W * 3;
    const size_t row0 = ((size_t)img * P.H + y) * (size_t)nbytes;
    uint8_t* dst = rgb + row0;
    const uint8_t* cov = P.cover ? P.cover + row0 : nullptr;      // delta embedding: the transform is added to the cover's pixels
    const bool fast = (PPB == 3) && ((P.W & 3) == 0) && (((uintptr_t)rgb & 3) == 0) && (((uintptr_t)P.cover & 3) == 0);
    if (fast) {
        const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;
        uint32_t* dstw = reinterpret_cast<uint32_t*>(dst);
        const uint32_t* covw = reinterpret_cast<const uint32_t*>(cov);
        // the cover's words of every group this thread stores, fetched before the first store (see k_colrow_inv)
        constexpr int NG = imax(1, (M / 2 + T * PPB - 1) / (T * PPB));
        uint32_t cw[3 * NG];
        if (covw) {
#pragma unroll
            for (int i = 0; i < NG; i++) {
                const int g = imin(tid + i * nthr, (P.W >> 2) - 1);      // clamped: every load unconditional
                cw[3 * i] = covw[3 * g]; cw[3 * i + 1] = covw[3 * g + 1]; cw[3 * i + 2] = covw[3 * g + 2];
            }
        }
#pragma unroll
        for (int gi = 0; gi < NG; gi++) {
            const int g = tid + gi * nthr;
            if (g >= (P.W >> 2)) break;
            const int i0 = lay.idx(2 * g, 0), i1 = lay.idx(2 * g + 1, 0);
            const float2 r01 = lds[i0], r23 = lds[i1], g01 = lds[i0 + lay.pitch], g23 = lds[i1 + lay.pitch],
                         b01 = lds[i0 + 2 * lay.pitch], b23 = lds[i1 + 2 * lay.pitch];
            // DC removal: the constant taken out before the forward transform comes back here (or the cover's own bytes, delta embedding)
            float zR0, zG0, zB0, zR1, zG1, zB1, zR2, zG2, zB2, zR3, zG3, zB3;
            if (covw) {
                const uint32_t c0 = cw[3 * gi], c1 = cw[3 * gi + 1], c2 = cw[3 * gi + 2];
                zR0 = (float)(c0 & 255u); zG0 = (float)((c0 >> 8) & 255u); zB0 = (float)((c0 >> 16) & 255u); zR1 = (float)(c0 >> 24);
                zG1 = (float)(c1 & 255u); zB1 = (float)((c1 >> 8) & 255u); zR2 = (float)((c1 >> 16) & 255u); zG2 = (float)(c1 >> 24);
                zB2 = (float)(c2 & 255u); zR3 = (float)((c2 >> 8) & 255u); zG3 = (float)((c2 >> 16) & 255u); zB3 = (float)(c2 >> 24);
            } else {
                zR0 = zG0 = zB0 = zR1 = zG1 = zB1 = zR2 = zG2 = zB2 = zR3 = zG3 = zB3 = P.bias;
            }
            const unsigned R0 = quantise_u8(s0 * r01.x + zR0), R1 = quantise_u8(s1 * r01.y + zR1), R2 = quantise_u8(s0 * r23.x + zR2), R3 = quantise_u8(s1 * r23.y + zR3);
            const unsigned G0 = quantise_u8(s0 * g01.x + zG0), G1 = quantise_u8(s1 * g01.y + zG1), G2 = quantise_u8(s0 * g23.x + zG2), G3 = quantise_u8(s1 * g23.y + zG3);
            const unsigned B0 = quantise_u8(s0 * b01.x + zB0), B1 = quantise_u8(s1 * b01.y + zB1), B2 = quantise_u8(s0 * b23.x + zB2), B3 = quantise_u8(s1 * b23.y + zB3);
            dstw[3 * g] = R0 | (G0 << 8) | (B0 << 16) | (R1 << 24);
            dstw[3 * g + 1] = G1 | (B1 << 8) | (R2 << 16) | (G2 << 24);
            dstw[3 * g + 2] = B2 | (R3 << 8) | (G3 << 16) | (B3 << 24);
        }
    } else {
        auto get = [&](int off) -> unsigned {
            const int n = off / 3, ch = off - 3 * n;
            float v = ldsf[2 * lay.idx(n >> 1, ch - plane0) + (n & 1)];
            if (P.center && ((n + y) & 1)) v = -v;
            return quantise_u8(v + (cov ? (float)cov[off] : P.bias));
        };
        if (PPB == 3) {
            const int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
            for (int o = tid; o < head && o < nbytes; o += nthr) dst[o] = (uint8_t)get(o);
            const int nwords = nbytes > head ? (nbytes - head) / 4 : 0;
            uint32_t* dstw = reinterpret_cast<uint32_t*>(dst + head);
            for (int w = tid; w < nwords; w += nthr) {
                const int o = head + 4 * w;
                dstw[w] = get(o) | (get(o + 1) << 8) | (get(o + 2) << 16) | (get(o + 3) << 24);
            }
            for (int o = head + 4 * nwords + tid; o < nbytes; o += nthr) dst[o] = (uint8_t)get(o);
        } else if ((P.W & 1) == 0) {
            // one plane per workgroup: the packed slot m holds pixels 2m and 2m+1 of this plane (as in k_colrow_inv); the generic
            // byte loop below cost ~25 instructions per pixel (index division, single-float LDS reads) -- 30 % of this kernel's VALU work
            const float s0 = (P.center && (y & 1)) ? -1.0f : 1.0f, s1 = P.center ? -s0 : s0;
            uint8_t* d1 = dst + plane0;
            constexpr int NP = imax(1, (M + T * PPB - 1) / (T * PPB));
            uint32_t cv[2 * NP];
            if (cov) {
#pragma unroll
                for (int i = 0; i < NP; i++) {
                    const uint8_t* a = cov + plane0 + 6 * imin(tid + i * nthr, (P.W >> 1) - 1);
                    cv[2 * i] = cover_word(a);
                    cv[2 * i + 1] = cover_word(a + 3);
                }
            }
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const int m = tid + i * nthr;
                if (m >= (P.W >> 1)) break;
                const float2 v = lds[lay.idx(m, 0)];
                d1[6 * m] = (uint8_t)quantise_u8(s0 * v.x + (cov ? (float)cover_pick(cv[2 * i], cov + plane0 + 6 * m) : P.bias));
                d1[6 * m + 3] = (uint8_t)quantise_u8(s1 * v.y + (cov ? (float)cover_pick(cv[2 * i + 1], cov + plane0 + 6 * m + 3) : P.bias));
            }
        } else {
            for (int n = tid; n < P.W; n += nthr) dst[3 * n + plane0] = (uint8_t)get(3 * n + plane0);
        }
    }
}

// ---------------------------------------------------------------------------
// columns: complex FFTs of length L down a tile of 16 adjacent columns.  One
// kernel serves the direct pass (L = PH) and both steps of the two-step
// ("four-step") decomposition PH = N1*N2 used for tall images:
//   input  row of element l of group g : in_a*l  + in_b*g   (rows >= in_rows read as 0)
//   output row of element k of group g : out_a*k + out_b*g  (rows >= out_rows not stored)
//   tw_out: multiply output k of group g by exp(SIGN*2*pi*i*k*g/PH)
// The column loop of fft2d S:362-365.
//   grid (ceil(M/16), ceil(G/GPB), n_planes)   block (16, T, GPB)
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned opaque_u32(unsigned v) {
#if defined(__HIPCC__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}
constexpr int cols_threads(int logl) { return imax(256, 16 * ((1 << logl) / elems_for(1 << logl))); }
__device__ __forceinline__ int read_bit_value(float2 v, const EmbedParams& P, int p, const float* __restrict__ jitter, uint64_t j);   // defined with k_read

// MODE (the COLS_* of tfft_kernels.h, named by the caller of launch_cols in its ColStep; own symbols, so that a kernel trace tells them
// apart; which combinations with the switches below exist: cols_variant_exists):
//   COLS_PLAIN     the transform
//   COLS_ROWLIMIT  rows above *P.last_row_dev are not stored
//   COLS_READ      extraction: nothing is stored at all -- the tile is parked in LDS and the bits of the bins
//                  bucketed to it (P.rd_*) are read there (replaces the spectrum write + k_read's scattered reads)
//   COLS_EMBED     delta embedding (first inverse step): nothing is loaded -- the tile starts as zeros, receives F' - F at the bins
//                  bucketed to it (F read from `in` at those bins only) and is transformed: the stego image is cover + IFFT(F' - F),
//                  so neither k_embed's scattered read-modify-write nor this step's read of the whole spectrum takes place
//   COLS_EMIT      delta embedding (last forward step): the transform, plus the values of the listed bins written to P.em_fl
//   COLS_STAT      COLS_EMIT without any spectrum store: the statistics' bracket pass (weight below the median's bracket, its members,
//                  the capacity counts against the threshold's bracket) runs on the values in registers (ColParams::st_*).  Round 2
//                  built this on the parked tile, measured it slower and shelved it; on round 3's kernels (two workgroups per CU,
//                  no 64-byte |F|^2 stores to wait for) the step itself gets FASTER by it and the |F|^2 plane, its write and the
//                  bracket pass over it disappear
//   COLS_EMBED_D   COLS_EMBED with F' - F not computed from (F, bit, alpha) but taken as it is from P.em_fl: one value per bucket entry,
//                  in the coordinates of the stored bin -- the corrected deltas of the fitted embed (tfft_embed_stream_batch_fit_dev,
//                  DESIGN.md section 10).  One walk per image only (PI)
//   COLS_STAT_EMBED  COLS_STAT and COLS_EMBED of the same (row group, column tile) in one visit: the tile of `in` is transformed and
//                  classified as in COLS_STAT; F at the tile's listed bins is read from the parked tile (not through P.em_fl), the tile is
//                  zeroed, receives F' - F, is transformed back and stored to `out` with the inverse step's output twiddles.  The inverse
//                  step's output rows are the forward step's input rows (k + L*g), so the stores go where the loads came from, in the
//                  other buffer: `in` survives for the statistics' gated tail.  Two-step plans only (SIGN = +1 names the first half)
__device__ __forceinline__ unsigned frame_bit(const uint8_t* __restrict__ header, const uint8_t* __restrict__ payload, uint64_t i);   // defined with k_embed
// DC: the DC-removal epilogue (ColParams::dc_*) is compiled in; its own instantiation, because the kernel sits at the
// 256-VGPR cap and even the unused code costs accumulation-register spills
// TW: the output twiddles of the two-step decomposition (P.tw_out) are compiled in: 32 VGPRs the final steps do not need
// FULL: every output element of the launch exists (all columns, groups and rows < out_rows): the stores carry no predicate.  A store
//       behind an exec-mask branch may or may not have been issued, so s_waitcnt cannot count past it: the wait for the prefetched
//       tile that follows then also waits for the stores just issued (their whole latency, every tile).  The launcher picks it.
// PH: the phase options of the batched calls (ColParams::em_jp / em_med, tfft_set_phase_options) are compiled in -- COLS_EMBED and
//     COLS_READ only, their own instantiations, so that the fixed-alpha kernels stay exactly as they are (registers, occupancy)
// PI: one walk per image (tfft_*_stream_batch_walks_dev, launch_bucket_walks): image i's buckets follow image i-1's (bucket
//     ((3*i + plane)*G + g)*ntiles + tile) and hold ABSOLUTE entry indices (image i's entries at [i*n, (i+1)*n)), so em_fl / em_pb /
//     em_jp are indexed by the entry alone: the launcher passes em_n = 0.  (Written as `PI ? 0 : img*em_n` here instead, the COLS_STAT
//     step of a 1080p launch spilled a register.)
//     Bucket modes only, their own instantiations: the shared-list kernels keep their registers and occupancy
template <int LOGL, int SIGN, int MODE = COLS_PLAIN, bool DC = false, bool TW = false, bool FULL = false, bool PH = false, bool PI = false>
__global__ void __launch_bounds__(cols_threads(LOGL)) TFFT_WAVES_PER_EU((MODE == COLS_EMIT && TFFT_COLS_PFEMIT) ? 1 : (FULL ? TFFT_COLS_WAVES(LOGL) : imin(2, TFFT_COLS_WAVES(LOGL)))) k_fft_cols(const float2* in, float2* out, const float2* __restrict__ tw,
                           ColParams P) {
    constexpr int L = 1 << LOGL, E = elems_for(L), T = L / E, C = 16;
    constexpr bool STAT = stat_mode(MODE), FUSED = (MODE == COLS_STAT_EMBED);
    // (COLS_STAT_EMBED from L = 256 on: one group per workgroup -- launch_cols_t -- and said so here, the group and what follows from it
    // are scalars: left as threadIdx.z the kernel spilled 14 registers of such per-thread copies at four waves per SIMD)
    const int c = threadIdx.x, t = threadIdx.y, gl = (FUSED && T * C >= 256) ? 0 : (int)threadIdx.z;
    const int g = (MODE == COLS_PLAIN && SIGN > 0 && FULL && P.g_step > 1) ? (int)(blockIdx.y * blockDim.z + gl) * P.g_step + P.g_off      // the statistics' sample
                                                                            : (int)(blockIdx.y * blockDim.z + gl);
    const int img = blockIdx.z / 3, plane = blockIdx.z - 3 * img;      // grid.z = 3 * n_images
    const size_t plane_off = (size_t)img * P.img_stride + (size_t)plane * P.plane_stride;
    float2* lds = reinterpret_cast<float2*>(tfft_smem) + (size_t)gl * L * C;
    LayColumns lay{C};

    // A workgroup walks `tiles_per_block` adjacent 16-column tiles.  The twiddles depend on (t, g) only,
    // so they are fetched once; the next tile's data is fetched into registers while the current tile
    // is being transformed (the loads of tile i+1 overlap the LDS exchanges and stores of tile i).
    if (MODE == COLS_PLAIN && SIGN > 0 && P.gate) {      // the statistics of this image were settled without the spectrum: nothing to redo
        const SelectState* gs = P.gate + 3 * img;
        if (gs[0].fast && gs[1].fast && gs[2].fast && gs[0].n_amb <= TFFT_AMB_CAP && gs[1].n_amb <= TFFT_AMB_CAP && gs[2].n_amb <= TFFT_AMB_CAP) return;
    }
    // COLS_PLAIN forward with tile_step > 1 (the statistics' sample): tile index i stands for tile i*tile_step + tile_off of the input
    // and for column block i of a narrow output (out_M columns)
    const int ts = (MODE == COLS_PLAIN && SIGN > 0 && P.tile_step > 1) ? P.tile_step : 1;
    const int toff = ts > 1 ? P.tile_off : 0;
    const int tile0 = blockIdx.x * P.tiles_per_block;
    const int ntiles = ((P.M + C - 1) / C - toff + ts - 1) / ts;
    const int tile1 = (tile0 + P.tiles_per_block < ntiles) ? tile0 + P.tiles_per_block : ntiles;
    // The loads of a tile are UNCONDITIONAL at clamped (always valid) addresses; elements that do not exist (rows >= in_rows, the
    // columns / groups beyond the grid) are zeroed by tile_mask() when the tile is consumed.  Written as `cond ? src[i] : 0` every
    // load sat behind its own s_cbranch_execz, and a load that may or may not have been issued cannot be counted: the wait for
    // the CURRENT tile's registers at the top of its transform became s_waitcnt vmcnt(<the few unconditional loads>), i.e. it
    // also waited for the tile prefetched a moment earlier -- the one-tile-ahead prefetch never overlapped anything (rounds 1-2).
    const int rows_in_max = P.in_a * (L - 1) + P.in_b * (P.G - 1);            // highest input row any thread of the launch addresses
    const bool in_full = (rows_in_max < P.in_rows) && (P.M % C == 0) && (P.G % (int)blockDim.z == 0);
    // (opaque_u32: the value, made opaque to the optimiser inside the tile loop -- without it the per-thread part of every address
    //  is loop invariant and gets hoisted as sixteen 64-bit pairs all the same)
    // Addressing.  Element m of a thread sits m * (a * T * M) bins after its element 0 -- a workgroup-uniform stride -- and a tile
    // 16 bins after the previous one, so an access is (uniform 64-bit base of (tile, m), in SGPRs) + (ONE 32-bit byte offset per
    // thread), the form global_load / global_store take directly.  Left to the compiler, every access had its own loop-invariant
    // 64-bit address: 16 pairs for the loads, 16 per store flavour -- hoisted out of the tile loop and, at four waves per SIMD,
    // spilled (COLS_EMIT: 328 bytes of scratch).  A plane has < 2^27 bins, so byte offsets fit 32 bits.
    const unsigned voff_in = (unsigned)((P.in_a * t + P.in_b * g) * P.M + c) * 8u;
    const size_t stride_in = (size_t)P.in_a * T * P.M * sizeof(float2);
    const char* in_bytes = reinterpret_cast<const char*>(in + plane_off);
    const int oM = ts > 1 ? P.out_M : P.M;
    const unsigned voff_out = (unsigned)((P.out_a * t + P.out_b * g) * oM + c) * 8u;
    const size_t stride_out = (size_t)P.out_a * T * oM * sizeof(float2);
    char* out_bytes = reinterpret_cast<char*>(out + (ts > 1 ? (size_t)img * P.out_img_stride + (size_t)plane * P.out_plane_stride : plane_off));
    char* m2_bytes = reinterpret_cast<char*>(reinterpret_cast<float*>(out + (size_t)img * P.img_stride) + (size_t)plane * P.plane_stride);      // COLS_EMIT: the |F|^2 plane
    auto load_tile = [&](int tile, float2 (&v)[E]) {
        if (in_full) {
            const char* tb = in_bytes + (size_t)(imin(tile, ntiles - 1) * ts + toff) * (C * sizeof(float2));      // (a workgroup past the last tile loads it again)
            const unsigned vo = opaque_u32(voff_in);
#pragma unroll
            for (int m = 0; m < E; m++) v[m] = *reinterpret_cast<const float2*>(tb + m * stride_in + vo);
        } else {
            const int col = imin((tile * ts + toff) * C + c, P.M - 1);
            const float2* src = in + plane_off;
            const int gc = imin(g, P.G - 1), to = (int)opaque_u32((unsigned)t);
#pragma unroll
            for (int m = 0; m < E; m++) {
                const int row = imin(P.in_a * (to + m * T) + P.in_b * gc, P.in_rows - 1);
                v[m] = src[(unsigned)(row * P.M + col)];
            }
        }
    };
    auto tile_mask = [&](int tile, float2 (&v)[E]) {       // workgroup-uniform test first: the final steps never need it
        if (in_full) return;
        const bool active = ((tile * ts + toff) * C + c < P.M) && (g < P.G);
#pragma unroll
        for (int m = 0; m < E; m++) {
            const int row = P.in_a * (t + m * T) + P.in_b * g;
            if (!(active && row < P.in_rows)) v[m] = make_float2(0.f, 0.f);
        }
    };
    constexpr bool PF = (LOGL <= TFFT_COLS_PF_MAXLOG || (MODE == COLS_EMIT && TFFT_COLS_PFEMIT)) && !embed_mode(MODE);      // one tile ahead in registers (EMBED loads no tile: its lists always travel one tile ahead)
    float2 u[E], un[E];
    // c*A_W of the tile's column travels with the tile's loads (fetched where it is used it sat behind the prefetch of
    // the next tile in the in-order vmcnt queue and cost the overlap: 0.60 -> 0.87 ms)
    float2 awc = make_float2(0.f, 0.f), awn = make_float2(0.f, 0.f);
    auto load_aw = [&](int tile) -> float2 { const int col = (tile * ts + toff) * C + c; return (DC && col < P.M) ? P.dc_aw[col] : make_float2(0.f, 0.f); };
    // the first tile's loads go out before anything else: the tables staged below (each a global -> LDS round trip) ride behind them,
    // and ONE barrier at the end of the prologue covers them all
    if (PF) { load_tile(tile0, u); awc = load_aw(tile0); }
    const int out_rows = (MODE == COLS_ROWLIMIT) ? imin(P.out_rows, *P.last_row_dev + 1) : P.out_rows;
    // DC removal: this group's rows of c*A_H staged behind the exchange buffers (read once per tile and output)
    float2* lds_ah = reinterpret_cast<float2*>(tfft_smem) + (size_t)blockDim.z * L * C + (size_t)gl * L;
    // output twiddles of the two-step decomposition, exp(SIGN*2*pi*i*k*g/PH), k < L: staged once per workgroup behind the DC rows
    // and read back at the stores (as registers they were 32 VGPRs: the L = 256 / 512 variants spilled 26 .. 79 dwords)
    // COLS_STAT_EMBED: ONE such slot holds the DC rows while the tile is F (classification, the reads of the listed bins) and the inverse
    // step's output twiddles exp(-2*pi*i*k*g/PH) from there to the tile's stores.  Both depend on (k, g) only, a group has exactly L threads
    // (T*C = L from L = 16 on; the mode exists from L = 32), so thread (t, c) fetches entry k = t*C + c of the table that comes next (8 bytes out of L2, asked for a
    // phase ahead) and writes it into the slot where the phase changes.  (A slot of its own for the twiddles is 2 KiB at L = 256: 42 KiB
    // per workgroup, one workgroup per CU fewer than COLS_STAT; the entries kept in registers across the classification spilled there.)
    float2* lds_wo = FUSED ? lds_ah : reinterpret_cast<float2*>(tfft_smem) + (size_t)blockDim.z * L * (C + (DC ? 1 : 0)) + (size_t)gl * L;
    // (opaque: inside the tile loop these are loop-invariant loads, and hoisted they are the registers again)
    auto fu_load_wo = [&]() -> float2 { return twload<-1>(tw, (int)((opaque_u32((unsigned)(t * C + c)) * (unsigned)g) & (unsigned)(P.PH - 1))); };
    auto fu_load_ah = [&]() -> float2 { return P.dc_ah[(unsigned)P.out_a * opaque_u32((unsigned)(t * C + c)) + (unsigned)(P.out_b * g)]; };      // (FULL: every row exists)
    if (FUSED && !DC) lds_wo[t * C + c] = fu_load_wo();      // (no DC rows: the slot never changes)
    if (DC) {
        for (int k = t * C + c; k < L; k += T * C) {       // forward: rows of the outputs; inverse: rows of the inputs
            const int row = (SIGN > 0) ? P.out_a * k + P.out_b * g : P.in_a * k + P.in_b * g;
            lds_ah[k] = (g < P.G && row < P.PH) ? P.dc_ah[row] : make_float2(0.f, 0.f);
        }
    }
    if (TW) {
        for (int k = t * C + c; k < L; k += T * C) lds_wo[k] = twload<SIGN>(tw, (k * g) & (P.PH - 1));
    }
    // COLS_READ: a tile without bins (beyond the annulus: a tenth of them with rmax = 0.45) is neither loaded nor transformed.  The bucket
    // offsets of the workgroup's tiles sit in LDS (lds_eo, staged below); workgroup-uniform, so the barriers stay aligned.  The FIRST tile
    // is loaded before the offsets are there (its load must not wait for a global -> LDS round trip) and dropped afterwards if empty.
    constexpr int NOFF = 16;            // tiles per workgroup the offsets cover (the launcher caps tiles_per_block of the bucket modes)
    // inter-pass twiddles: registers (fetched once per workgroup) for short columns; from TFFT_COLS_LDS_TW_LOG on the L-entry table
    // exp(+2 pi i j/L) is staged in LDS and read at the point of use (at L = 512 they would be 46 more VGPRs in a kernel capped at 256)
    // (COLS_STAT_EMBED: always the table -- the one exp(+2 pi i j/L) serves both directions, registers would hold one sign's)
    constexpr bool TWL = (LOGL >= TFFT_COLS_LDS_TW_LOG) || FUSED;
    float2 W[TWL ? 1 : tw_regs<L, E>()];
    float2* lds_tw = reinterpret_cast<float2*>(tfft_smem) + (size_t)blockDim.z * L * (C + (DC || FUSED ? 1 : 0) + (TW ? 1 : 0));
    float2* lds_aw = lds_tw + (TWL ? L : 0) + gl * C;      // COLS_READ with DC: the current tile's 16 column factors
    if (TWL) {
        const int tws = P.PH >> LOGL;
        for (int k = (gl * T + t) * C + c; k < L; k += blockDim.z * T * C) lds_tw[k] = tw[k * tws];
    } else {
        fft_prefetch_twiddles<L, E, SIGN>(W, t, tw, P.PH >> LOGL);
    }
    // ---- delta embedding (COLS_EMIT in the last forward step, COLS_EMBED in the first inverse step) -------------------------------
    // The stego image is cover + IFFT(F' - F), and F' - F is zero but at the bins of the list.  Reading F at those bins from the
    // stored spectrum is 9 M scattered 8-byte reads per 32 x 1080p launch (0.25 ms inside the write-saturated inverse step; k_embed's
    // read-modify-write cost 0.18 ms).  The last FORWARD step has every tile in LDS, so it writes the values of the tile's bins into a
    // list in bucket order (em_fl, 8 bytes per bin per image, coalesced), k_gather_bits puts the stream bits in the same order (em_pb),
    // and the inverse step builds its tiles from the three lists: bucket entry, value and bit are all addressed by the entry index,
    // so the entries of tile i+1 are requested while tile i is transformed, like the tile loads of the other modes.
    // NE entries per thread travel in registers; a longer bucket fetches the rest in place.
    // Every fetch is UNCONDITIONAL at a clamped, always valid address, and nothing looks at a fetched word before the stage that uses
    // it: a load inside a predicated block is followed by its own s_waitcnt vmcnt(0) (32 serialised round trips were seen).
    // entries per thread that travel in registers.  4K: ~1650 entries per bucket and 512 threads, 1080p: ~240 and 256.  Four cover a
    // 4K bucket (a longer one fetches the rest in place, a dependent round trip in the middle of the tile): first inverse step
    // 0.547 -> 0.512 ms per 8 x 4K launch (round 3, gpurun_out/r3f; round 2's kernel, one workgroup per CU at 247 registers, lost by it)
#ifndef TFFT_EMBED_NE9
#ifndef TFFT_STAT_LDS_LOG
#define TFFT_STAT_LDS_LOG 9      // columns from this length on are classified from the parked tile, shorter ones in registers
#endif
#ifndef TFFT_STAT_SLOTS
#define TFFT_STAT_SLOTS 193     // staged candidates per wave (+ one spare slot), flushed once per tile
#endif
#define TFFT_EMBED_NE9 4
#endif
    constexpr int NE = (LOGL >= 9) ? (embed_mode(MODE) ? (LOGL == 9 ? TFFT_EMBED_NE9 : 2) : 4) : 2;
    struct EmEntry { TileBin tb; float2 f; unsigned bit, live; };   // bucket entry, the stored value of its bin (conjugate of the bin when
                                                                    // tb.conj) and its stream bit (2: beyond the end of the stream)
    EmEntry enC[NE], enN[NE];
    const int em_tid = t * C + c, em_nthr = T * C;
    // the bucket offsets of the workgroup's tiles (at most NOFF: the launcher sees to it) sit in LDS: read with lgkmcnt, not vmcnt,
    // and without the branch trees a register array indexed by the tile turned into
    unsigned* lds_eo = reinterpret_cast<unsigned*>(lds_tw + (TWL ? L : 0) + blockDim.z * C) + gl * (NOFF + 2);
    if (MODE == COLS_READ || embed_mode(MODE) || MODE == COLS_EMIT || STAT) {
        const unsigned b0 = (unsigned)(((PI ? (int)blockIdx.z : plane) * P.G + (g < P.G ? g : 0)) * ntiles);      // (PI: blockIdx.z = 3*img + plane)
        for (int i = em_tid; i <= NOFF; i += em_nthr) lds_eo[i] = P.rd_off[b0 + (unsigned)imin(tile0 + i, ntiles)];
    }
    unsigned* lds_hist = reinterpret_cast<unsigned*>(tfft_smem + P.hist_lds_off);
    const bool hist_on = (MODE == COLS_PLAIN && SIGN > 0 && FULL) && P.hist_sel != nullptr;      // workgroup uniform
    if (hist_on)
        for (int i = (gl * T + t) * C + c; i < 4096; i += (int)(blockDim.x * blockDim.y * blockDim.z)) lds_hist[i] = 0;
    lds_barrier();            // the tables above (DC rows, output twiddles, pass twiddles, bucket offsets)
    auto em_range = [&](int tile, unsigned& e0, unsigned& e1) {
        const int i = imin(tile - tile0, NOFF - 1);
        e0 = lds_eo[i]; e1 = lds_eo[i + 1];
        if (!(tile < tile1 && g < P.G)) e1 = e0;
    };
    auto has_bins = [&](int tile) -> bool {
        if (MODE != COLS_READ || blockDim.z > 1) return true;
        unsigned e0, e1;
        em_range(tile, e0, e1);
        return e1 > e0;
    };
    const float2* em_fl = P.em_fl + (size_t)img * P.em_n;
    const uint8_t* em_pb = P.em_pb + (size_t)img * P.em_n;
    auto em_entries = [&](int tile, EmEntry (&en)[NE], bool with_value, bool with_bit) {      // (COLS_STAT_EMBED: the bit alone, F comes out of the tile)
        unsigned e0, e1;
        em_range(tile, e0, e1);
#pragma unroll
        for (int i = 0; i < NE; i++) {
            const unsigned e = e0 + (unsigned)(em_tid + i * em_nthr);
            en[i].live = e < e1 ? 1u : 0u;
            const unsigned ec = en[i].live ? e : 0u;
            en[i].tb = P.rd_bins[ec];
            if (with_value) en[i].f = em_fl[ec];
            if (with_bit) en[i].bit = em_pb[ec];
        }
    };
    // adaptive alpha (S:704-710): this image's median of the plane (workgroup uniform)
    const float em_medp = (MODE == COLS_EMBED && PH && P.em_med) ? fmaxf(1e-12f, P.em_med[3 * img + plane]) : 1.f;
    auto em_delta = [&](float2 f, unsigned bit, unsigned conj, unsigned e) -> float2 {      // write_bit_on_bin S:712-732 minus the old value
        if (MODE == COLS_EMBED_D) return f;       // (em_fl holds the delta itself)
        const float mag = fmaxf(1e-12f, mag_of(f));
        float ca = P.em_cos, sa = P.em_sin;
        if (MODE == COLS_EMBED && PH && P.em_med) sincosf(P.em_alpha * fminf(2.f, fmaxf(0.5f, mag / em_medp)), &sa, &ca);
        float2 nv = make_float2(mag * ca, bit ? mag * sa : -mag * sa);
        if (PH && P.em_jp) nv = cmul(nv, P.em_jp[e]);     // polar(mag, +-a + jitter[bit]): the phase of +-a turned by the bin's jitter
        if (conj) nv = cconj(nv);
        return csub(nv, f);
    };
    // ---- COLS_STAT: k_collect_bracket's per-value work (see there) on this kernel's registers.  Candidates are staged per wave in LDS
    // (128 slots behind the bucket offsets; flushed with one global atomic once more than 64 are waiting: a value adds at most 64)
    const int st_lin = (gl * T + t) * C + c, st_wave = st_lin >> 6;
    unsigned* st_wbuf = lds_eo + (blockDim.z - gl) * (NOFF + 2) + st_wave * TFFT_STAT_SLOTS;
    SelectState* st_s = STAT ? P.st_sel + 3 * img + plane : nullptr;
    const unsigned st_lo = STAT ? st_s->lo : 0u, st_span = STAT ? st_s->hi - st_lo : 0u, st_base = st_lo << 19;
    // (thresholds clamped at 0 -- mag2_threshold answers -inf for "everything passes", |F|^2 is never negative -- so that -1 can stand for
    // "not a bin of the annulus" in the comparisons below)
    const float st_t2lo = STAT ? fmaxf(st_s->t2_lo, 0.f) : 0.f, st_t2hi = STAT ? fmaxf(st_s->t2_hi, 0.f) : 0.f;
    unsigned* st_out = STAT ? P.st_cand + ((size_t)img * 3 + plane) * P.st_cand_stride : nullptr;
    float* st_ambo = STAT ? P.st_amb + ((size_t)img * 3 + plane) * TFFT_AMB_CAP : nullptr;
    // per-lane counters (one LDS atomic each at the end).  The classification is written for the VECTOR unit: a compare + add-with-carry
    // per counter and two branches on VCC per value.  Its first form counted with ballots and scalar popcounts: 39 scalar
    // instructions per value, and the scalar unit is shared by the CU's four SIMDs -- 0.21 ms of a 1080p batch's 0.66 (round 3).
    unsigned st_below = 0, st_capcount = 0, st_nstaged = 0;
    // bucket in [lo, hi] <=> bits - st_base <= st_span_b; never beyond +inf, so that a negative value (column 0's stand-in) stays outside
    const unsigned st_span_raw = st_span >= 8192u ? 0xFFFFFFFFu : ((st_span << 19) | 0x7FFFFu);
    const unsigned st_span_b = st_base > 0x7F800000u ? 0u : (st_span_raw < 0x7F800000u - st_base ? st_span_raw : 0x7F800000u - st_base);
    const unsigned st_aspan = (STAT && P.st_shi >= P.st_slo) ? P.st_shi - P.st_slo : 0u;       // annulus: d1 - s_lo <= st_aspan
    const unsigned st_t2lo_b = __float_as_uint(st_t2lo), st_t2win = __float_as_uint(st_t2hi) - st_t2lo_b;  // threshold window on the bits (values >= 0)
    // Every wave of the launch owns P.st_resv slots at the head of the plane's candidate list (wave w of workgroup b: slots
    // (b * nwaves + w) * st_resv ..), fills what it does not use with TFFT_CAND_HOLE at the end (the select kernels skip those), and only a
    // wave with more candidates than that appends the rest behind the fixed part with a global atomic.  (First form: one atomic per
    // flush, whose round trip the wave sat out -- ~0.1 ms of a 1080p batch's 0.68; reserving with one atomic per wave at the start was
    // worse still, 0.99: a thousand waves per plane queue on one address at once.)
    unsigned* st_region = st_out + (size_t)(((blockIdx.y * gridDim.x + blockIdx.x) * ((blockDim.x * blockDim.y * blockDim.z + 63) >> 6)) + st_wave) * P.st_resv;
    if (STAT && blockIdx.x == 0 && blockIdx.y == 0 && st_lin == 0) st_s->cand_fixed = P.st_cand_fixed;
    unsigned st_used = 0;
    auto st_fill = [&]() {              // wave uniform
        for (unsigned i = st_used + (st_lin & 63); i < P.st_resv; i += 64) st_region[i] = TFFT_CAND_HOLE;
    };
    auto st_flush = [&]() {             // wave uniform: the wave's staged candidates go to its slots of the plane's list
        const unsigned lane = st_lin & 63;
        WaveSync::sync();
        const unsigned room = P.st_resv - st_used, n1 = st_nstaged < room ? st_nstaged : room;
        for (unsigned i = lane; i < n1; i += 64) st_region[st_used + i] = st_wbuf[i];
        st_used += n1;
        if (st_nstaged > n1) {            // rare: behind the fixed part, as k_col0_stats appends its own
            const unsigned rest = st_nstaged - n1;
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&st_s->n_cand, rest);
            base = __builtin_amdgcn_readfirstlane(base);
            if ((size_t)P.st_cand_fixed + base + rest <= P.st_cand_stride)       // (the list is sized for the worst case, tfft_capi.hip: never false)
                for (unsigned i = lane; i < rest; i += 64) st_out[(size_t)P.st_cand_fixed + base + i] = st_wbuf[n1 + i];
        }
        WaveSync::sync();
        st_nstaged = 0;
    };
    if (embed_mode(MODE)) em_entries(tile0, enC, true, true);
    if (PF && (MODE == COLS_EMIT || STAT || MODE == COLS_READ)) em_entries(tile0, enC, false, FUSED);
    for (int tile = tile0; tile < tile1; tile++) {
        if (!PF && !embed_mode(MODE)) {      // no prefetch: this tile's loads and list entries now; another resident workgroup covers the wait
            if (!has_bins(tile)) continue;
            load_tile(tile, u); awc = load_aw(tile);
            if (MODE == COLS_EMIT || MODE == COLS_READ) em_entries(tile, enC, false, false);      // (COLS_STAT: after its classification, the registers are needed there)
        }
        // the next tile's loads ALWAYS go out (a load inside a branch cannot be counted by s_waitcnt: every later wait would drain the
        // queue): past the last tile, or when the next tile has no bins to read, this tile is fetched again (cache resident, never used)
        if (PF) { const int nt = (tile + 1 < tile1 && has_bins(tile + 1)) ? tile + 1 : tile; load_tile(nt, un); awn = load_aw(nt); }
        if (PF && (MODE == COLS_EMIT || STAT || MODE == COLS_READ)) em_entries(tile + 1, enN, false, FUSED);          // travels with the next tile's loads
        if (embed_mode(MODE)) {
            // the tile of F' - F: zeros but for the bins of the list (S:712-732 per bin); a tile without bins is stored as zeros.
            // The values of tile+1's bins and the entries of tile+2 are fetched now (see em_* above the loop).
            bool hb = true;
            if (blockDim.z == 1) { unsigned e0, e1; em_range(tile, e0, e1); hb = e1 > e0; }      // workgroup-uniform: the barriers stay aligned
            em_entries(tile + 1, enN, true, true);
            if (hb) {
#pragma unroll
                for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, c)] = make_float2(0.f, 0.f);
                lds_barrier();
                unsigned pe0 = 0;       // (PH: the first entry of the tile, for the jitter phasors of the entries in registers)
                if (PH) { unsigned pe1; em_range(tile, pe0, pe1); }
#pragma unroll
                for (int i = 0; i < NE; i++)
                    if (enC[i].live && enC[i].bit < 2u)
                        lds[lay.idx(enC[i].tb.k, enC[i].tb.c)] = em_delta(enC[i].f, enC[i].bit, enC[i].tb.conj, pe0 + (unsigned)(em_tid + i * em_nthr));
                if (g < P.G) {          // a bucket with more than NE entries per thread: the rest the slow way
                    unsigned e0, e1;
                    em_range(tile, e0, e1);
                    for (unsigned e = e0 + (unsigned)(em_tid + NE * em_nthr); e < e1; e += em_nthr) {
                        const TileBin tb = P.rd_bins[e];
                        const unsigned bit = em_pb[e];
                        if (bit >= 2u) continue;
                        lds[lay.idx(tb.k, tb.c)] = em_delta(em_fl[e], bit, tb.conj, e);
                    }
                }
                lds_barrier();
#pragma unroll
                for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, c)];
                lds_barrier();            // before the first exchange of the transform overwrites the tile
                if (TWL) fft_block_lazy<L, E, SIGN>(u, lds, lay, t, c, lds_tw, 1);
                else fft_block<L, E, SIGN>(u, lds, lay, t, c, W);
            }
                const int col = tile * C + c;
            if (FULL) {
                char* ob = out_bytes + (size_t)tile * (C * sizeof(float2));
                const unsigned vo = opaque_u32(voff_out);
#pragma unroll
                for (int m = 0; m < E; m++) {
                    float2 v = hb ? u[m] : make_float2(0.f, 0.f);
                    if (TW && hb) v = cmul(v, lds_wo[t + m * T]);
                    *reinterpret_cast<float2*>(ob + m * stride_out + vo) = v;
                }
            } else if ((col < P.M) && (g < P.G)) {
                float2* dst = out + plane_off;
                const int to = (int)opaque_u32((unsigned)t);
#pragma unroll
                for (int m = 0; m < E; m++) {
                    const int k = to + m * T;
                    const int row = P.out_a * k + P.out_b * g;
                    if (row < out_rows) {
                        float2 v = hb ? u[m] : make_float2(0.f, 0.f);
                        if (TW && hb) v = cmul(v, lds_wo[k]);
                        dst[(unsigned)(row * P.M + col)] = v;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NE; i++) enC[i] = enN[i];
            continue;
        }
        if (PF && !has_bins(tile)) {
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = un[m];
            awc = awn;
#pragma unroll
            for (int i = 0; i < NE; i++) enC[i] = enN[i];
            continue;
        }
        tile_mask(tile, u);
        if (DC && SIGN < 0) {           // first inverse step: the rank-1 term leaves before the transform (the row kernel adds c back)
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = csub(u[m], cmul(lds_ah[t + m * T], awc));
        }
        // (COLS_STAT_EMBED: the thread's row made opaque per transform -- the twiddle addresses that follow from it are loop invariant, and
        // hoisted for two transforms they are 15 registers the classification between them has no room for)
        if (FUSED) fft_block_lazy<L, E, SIGN>(u, lds, lay, (int)opaque_u32((unsigned)t), c, lds_tw, 1);
        else if (TWL) fft_block_lazy<L, E, SIGN>(u, lds, lay, t, c, lds_tw, 1);
        else fft_block<L, E, SIGN>(u, lds, lay, t, c, W);
        if (MODE == COLS_READ) {
            // park the tile (row k of group g = spectrum row g + G*k) and read the bits of its bins in place
            lds_barrier();            // the last gather of fft_block has been consumed by every thread
#pragma unroll
            for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, c)] = u[m];
            // DC removal: the rank-1 term is added to the bins that are READ (a few hundred per tile), not to all 16 x L values of
            // the tile (that was 0.056 ms of the 0.50 ms launch): the tile's 16 column factors go to LDS beside the row factors
            if (DC && t == 0) lds_aw[c] = awc;
            lds_barrier();
            if (FULL || g < P.G) {
                // the tile's entries travelled with its loads (NE per thread in registers; a longer bucket fetches the rest in place)
                unsigned e0, e1;
                em_range(tile, e0, e1);
                uint8_t* bo = P.rd_bits + (size_t)img * P.rd_n;
                // read_bit_from_bin S:734-746 for an alpha in (0, pi): Im >= 0; with jitter j the targets j +- a are symmetric about j,
                // so the bit is Im(F e^{-ij}) >= 0
                auto bit_of = [&](const TileBin tb, unsigned e) -> uint8_t {
                    float2 v = lds[lay.idx(tb.k, tb.c)];
                    if (DC) v = cadd(v, cmul(lds_ah[tb.k], lds_aw[tb.c]));
                    if (PH && P.em_jp) {
                        const float2 p = P.em_jp[e];
                        if (tb.conj) v = cconj(v);
                        return (uint8_t)(v.y * p.x - v.x * p.y >= 0.0f ? 1 : 0);
                    }
                    return (uint8_t)((tb.conj ? -v.y : v.y) >= 0.0f ? 1 : 0);
                };
                // stores without a predicate (see FULL): a lane without an entry writes its byte to the context's scratch line instead
#pragma unroll
                for (int i = 0; i < NE; i++) {
                    const TileBin tb = enC[i].tb;
                    uint8_t* dst = enC[i].live ? bo + tb.bit : P.trash + em_tid;
                    *dst = bit_of(tb, enC[i].live ? e0 + (unsigned)(em_tid + i * em_nthr) : 0u);
                }
                for (unsigned e = e0 + (unsigned)(em_tid + NE * em_nthr); e < e1; e += em_nthr) { const TileBin tb = P.rd_bins[e]; bo[tb.bit] = bit_of(tb, e); }
            }
            lds_barrier();            // before the next tile's exchanges overwrite the parked values
            if (PF) {
#pragma unroll
                for (int m = 0; m < E; m++) u[m] = un[m];
                awc = awn;
#pragma unroll
                for (int i = 0; i < NE; i++) enC[i] = enN[i];
            }
            continue;
        }
        const int col = tile * C + c;
        // COLS_STAT: the bracket pass of the statistics (k_collect_bracket's classify / cap_elem) on the thread's values while they are in
        // registers -- unrolled beside the DC term, sixteen independent chains.  (Read back from the parked tile in a rolled loop the same
        // work cost 210 us of a 1080p batch's 690: one LDS round trip + a dependent chain per value, four waves per SIMD to hide it.)
        // One value = one stored bin (row, col) of weight 2; the packed column 0 is left to k_col0_stats.
        // (the launcher only picks this mode when the annulus stays left of column PW/2: the mirror bins of the stored half never count)
        const bool st_valid = col != 0;
        // (st_row0 opaque: the rows do not depend on the tile, and left visible the compiler computes every row's square and the
        // axis tests once before the tile loop -- 50 spilled dwords -- instead of two instructions per value inside it)
        const unsigned st_col2 = (unsigned)col * (unsigned)col, st_rstep = (unsigned)(P.out_a * T), st_row0 = opaque_u32((unsigned)(P.out_a * t + P.out_b * g));
        constexpr bool ST_LDS = (LOGL >= TFFT_STAT_LDS_LOG);
        unsigned st_ambflag = 0;
        auto st_value = [&](int m, float2 v) {
            const float m2 = st_valid ? fmaf(v.x, v.x, v.y * v.y) : -1.0f;
            const unsigned b = __float_as_uint(m2), rel = b - st_base, row = st_row0 + (unsigned)m * st_rstep;
            // median: values below the bracket are counted, values inside it staged for the select (lanes without one write the spare slot)
            st_below += (b < st_base) ? 1u : 0u;
            const bool cnd = rel <= st_span_b;
            const unsigned long long mk = __ballot(cnd);
            {   // straight-line on purpose: a branch per value ("any candidate in the wave?") keeps the compiler from overlapping the sixteen
                // values' LDS reads and chains, and the wave sat out each one in turn (round 3: 0.12 ms of a 1080p batch's 0.69)
                const unsigned slot = st_nstaged + wave_rank(mk), sel = (cnd && slot < (unsigned)(TFFT_STAT_SLOTS - 1)) ? 0xFFFFFFFFu : 0u;
                st_wbuf[(slot & sel) | ((unsigned)(TFFT_STAT_SLOTS - 1) & ~sel)] = rel | 0x80000000u;      // lanes without a candidate (or without room) write the spare slot
                st_nstaged += (unsigned)__popcll(mk);       // beyond the slots: the tile is staged again below, value by value
            }
            // capacity (S:998-1008): bins of the annulus at or above the threshold window are counted; a value inside the window only
            // leaves a mark (bit E-1-m of st_ambflag: rare, picked up from the parked tile below)
            const unsigned d1 = __umul24(row, row) + st_col2;           // rows < 2^13
            const float x = (d1 - P.st_slo <= st_aspan) ? m2 : -1.0f;
            st_capcount += !(x < st_t2hi) ? 1u : 0u;
            st_ambflag = st_ambflag + st_ambflag + ((__float_as_uint(x) - st_t2lo_b < st_t2win) ? 1u : 0u);
        };
        if (FULL && STAT && !ST_LDS) {
            // the DC row factors of TFFT_STAT_GROUP values are read together, ahead of those values' staging writes: the compiler cannot
            // tell the two LDS regions apart, so a read issued per value waited behind the previous value's write and out its own latency
#ifndef TFFT_STAT_GROUP
#define TFFT_STAT_GROUP 8
#endif
#pragma unroll
            for (int m0 = 0; m0 < E; m0 += TFFT_STAT_GROUP) {
                float2 ahv[TFFT_STAT_GROUP];
#pragma unroll
                for (int j = 0; j < TFFT_STAT_GROUP; j++) ahv[j] = DC ? lds_ah[t + (m0 + j) * T] : make_float2(0.f, 0.f);
#pragma unroll
                for (int j = 0; j < TFFT_STAT_GROUP; j++) {
                    float2 v = u[m0 + j];
                    if (DC) v = cadd(v, cmul(ahv[j], awc));      // the rank-1 term comes back (the same expression as in every other mode)
                    st_value(m0 + j, v);
                }
            }
        } else if (FULL) {
            char* ob = out_bytes + (size_t)tile * (C * sizeof(float2));
            char* mb = m2_bytes + (size_t)tile * (C * sizeof(float));
            const unsigned vo = opaque_u32(voff_out);
#pragma unroll
            for (int m = 0; m < E; m++) {
                float2 v = u[m];
                if (TW) v = cmul(v, lds_wo[t + m * T]);
                if (DC && SIGN > 0) v = cadd(v, cmul(lds_ah[t + m * T], awc));      // last forward step: the rank-1 term comes back
                if (STAT) {        // nothing is stored (L = 512: the values are classified from the parked tile below; shorter columns: above)
                } else if (MODE == COLS_EMIT && P.em_m2) {      // nothing but the statistics will read this: |F|^2, half the bytes (2: no statistics
                    if (P.em_m2 == 1) *reinterpret_cast<float*>(mb + m * (stride_out >> 1) + (vo >> 1)) = fmaf(v.x, v.x, v.y * v.y);      // asked for, nothing at all)
                } else if (MODE == COLS_PLAIN && SIGN > 0 && hist_on) {      // the statistics' sample: a histogram instead of the narrow spectrum
                    if ((tile * ts + toff) * C + c != 0) atomicAdd(&lds_hist[__float_as_uint(fmaf(v.x, v.x, v.y * v.y)) >> 19], 2u);
                } else *reinterpret_cast<float2*>(ob + m * stride_out + vo) = v;
            }
        } else if (((tile * ts + toff) * C + c < P.M) && (g < P.G)) {      // (the sample pass: input column tile*ts+toff, output column block tile of a narrow plane)
            float2* dst = reinterpret_cast<float2*>(out_bytes);
            float* dst_m2 = reinterpret_cast<float*>(out + (size_t)img * P.img_stride) + (size_t)plane * P.plane_stride;
            const int to = (int)opaque_u32((unsigned)t);
#pragma unroll
            for (int m = 0; m < E; m++) {
                const int k = to + m * T;
                const int row = P.out_a * k + P.out_b * g;
                if (row < out_rows) {
                    float2 v = u[m];
                    if (TW) v = cmul(v, lds_wo[k]);
                    if (DC && SIGN > 0) v = cadd(v, cmul(lds_ah[k], awc));
                    if (MODE == COLS_EMIT && P.em_m2) {
                        if (P.em_m2 == 1) dst_m2[(unsigned)(row * P.M + col)] = fmaf(v.x, v.x, v.y * v.y);
                    } else dst[(unsigned)(row * oM + col)] = v;
                }
            }
        }
        if (((MODE == COLS_EMIT && P.em_m2 == 1) || STAT) && tile == 0 && c == 0 && g < P.G) {      // the packed column 0 (its two real spectra cannot be told
            float2* col0 = P.st_col0 + ((size_t)img * 3 + plane) * P.PH;                  // apart from magnitudes) travels beside the |F|^2 plane
            const int to = (int)opaque_u32((unsigned)t);
#pragma unroll
            for (int m = 0; m < E; m++) {
                const int row = P.out_a * (to + m * T) + P.out_b * g;
                if (row < out_rows) col0[(unsigned)row] = (DC && SIGN > 0) ? cadd(u[m], cmul(lds_ah[to + m * T], awc)) : u[m];
            }
        }
        if (MODE == COLS_EMIT || STAT) {
            // park the tile (as COLS_READ does) and write the values of the listed bins, DC term included, into the list the first
            // inverse step embeds from: em_fl[entry index], coalesced
            lds_barrier();            // the last gather of fft_block has been consumed by every thread
#pragma unroll
            for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, c)] = u[m];
            if (DC && t == 0) lds_aw[c] = awc;
            lds_barrier();
            float2 fu_wo = make_float2(0.f, 0.f);
            if (FUSED && DC) fu_wo = fu_load_wo();      // needed once the tile's values have been read: the statistics' tail rides in between
            if (STAT) {
                if (ST_LDS) {
                    // L = 512: 32 values per thread -- classified in registers beside the transform's own 64 the kernel spills; from the
                    // parked tile instead, four values in flight
#pragma unroll 4
                    for (int m = 0; m < E; m++) {
                        const int k = t + m * T;
                        float2 v = lds[lay.idx(k, c)];
                        if (DC) v = cadd(v, cmul(lds_ah[k], awc));
                        st_value(m, v);
                    }
                }
                {
                    auto st_again = [&](int m, float& m2, unsigned& row) -> bool {      // value m of this thread once more, from the parked tile; in the annulus?
                        const int k = t + m * T;
                        float2 v = lds[lay.idx(k, c)];
                        if (DC) v = cadd(v, cmul(lds_ah[k], awc));
                        m2 = fmaf(v.x, v.x, v.y * v.y);
                        row = st_row0 + (unsigned)m * st_rstep;
                        return row * row + st_col2 - P.st_slo <= st_aspan;
                    };
                    // rows 0 and PH/2 are axes, outside the count (S:698-700): st_value did not test for them -- the few lanes that hold
                    // such a row take back what it counted there
                    auto st_uncount = [&](int m) {
                        float m2; unsigned row;
                        if (st_again(m, m2, row) && !(m2 < st_t2hi)) st_capcount -= 1u;
                    };
                    const unsigned half = (unsigned)P.PH >> 1, dh = half - st_row0;
                    if (st_valid && st_row0 == 0) st_uncount(0);
                    if (st_valid && half != 0 && half >= st_row0 && dh % st_rstep == 0 && dh / st_rstep < (unsigned)E) st_uncount((int)(dh / st_rstep));
                    // the staged candidates leave once per tile (a wave stages ~50 of its 1024 values; 192 fit).  A tile with more -- a
                    // bracket gone wide, a flat image -- is staged again from the parked values, flushing as it goes
                    if (st_nstaged > (unsigned)(TFFT_STAT_SLOTS - 1)) {
                        st_nstaged = 0;
                        for (int m = 0; m < E; m++) {
                            float m2; unsigned row;
                            (void)st_again(m, m2, row);
                            const unsigned rel = __float_as_uint(st_valid ? m2 : -1.0f) - st_base;
                            const bool cnd = rel <= st_span_b;
                            const unsigned long long mk = __ballot(cnd);
                            if (cnd) st_wbuf[st_nstaged + wave_rank(mk)] = rel | 0x80000000u;
                            st_nstaged += (unsigned)__popcll(mk);
                            if (st_nstaged > 64) st_flush();
                        }
                    }
                    if (st_nstaged) st_flush();
                    // values inside the threshold window: kept for k_capacity_settle, which knows the median
                    if (__ballot(st_ambflag != 0)) {
                        for (int m = 0; m < E; m++) {
                            if (!((st_ambflag >> (E - 1 - m)) & 1u)) continue;
                            float m2; unsigned row;
                            if (st_again(m, m2, row) && !(m2 < st_t2lo) && m2 < st_t2hi && row != 0 && 2u * row != (unsigned)P.PH) {
                                const unsigned slot = atomicAdd(&st_s->n_amb, 1u);
                                if (slot < TFFT_AMB_CAP) st_ambo[slot] = m2;
                            }
                        }
                    }
                }
            }
            if (!PF && STAT) em_entries(tile, enC, false, FUSED);
            // the value of a listed bin out of the parked tile, DC term included: what COLS_EMIT / COLS_STAT write to em_fl and COLS_STAT_EMBED embeds from
            auto read_listed = [&](const TileBin tb) -> float2 {
                float2 v = lds[lay.idx(tb.k, tb.c)];
                if (DC) v = cadd(v, cmul(lds_ah[tb.k], lds_aw[tb.c]));
                return v;
            };
            if constexpr (FUSED) {
                // F at the tile's listed bins out of the parked tile into registers; then the tile becomes F' - F (zeros but for those bins)
                // and goes back: COLS_EMBED's tile, built without the round trip of the values through P.em_fl.  A bucket with more than
                // NE entries per thread parks the values of the rest in P.em_fl after all: each by the thread that reads it back below
                unsigned e0, e1;
                em_range(tile, e0, e1);
                bool hb = true;
                if (blockDim.z == 1) hb = e1 > e0;      // workgroup-uniform: the barriers stay aligned
                if (hb) {
                    float2* fl = P.em_fl + (size_t)img * P.em_n;
#pragma unroll
                    for (int i = 0; i < NE; i++) {
                        const TileBin tb = enC[i].tb;
                        enC[i].f = read_listed(tb);
                    }
                    for (unsigned e = e0 + (unsigned)(em_tid + NE * em_nthr); e < e1; e += em_nthr) {
                        const TileBin tb = P.rd_bins[e];
                        fl[e] = read_listed(tb);
                    }
                    lds_barrier();            // every read of the parked tile and of the DC rows is done
#pragma unroll
                    for (int m = 0; m < E; m++) lds[lay.idx(t + m * T, c)] = make_float2(0.f, 0.f);
                    if (DC) lds_wo[t * C + c] = fu_wo;
                    lds_barrier();
#pragma unroll
                    for (int i = 0; i < NE; i++)
                        if (enC[i].live && enC[i].bit < 2u)
                            lds[lay.idx(enC[i].tb.k, enC[i].tb.c)] = em_delta(enC[i].f, enC[i].bit, enC[i].tb.conj, e0 + (unsigned)(em_tid + i * em_nthr));
                    for (unsigned e = e0 + (unsigned)(em_tid + NE * em_nthr); e < e1; e += em_nthr) {
                        const TileBin tb = P.rd_bins[e];
                        const unsigned bit = em_pb[e];
                        if (bit >= 2u) continue;
                        lds[lay.idx(tb.k, tb.c)] = em_delta(em_fl[e], bit, tb.conj, e);
                    }
                    lds_barrier();
#pragma unroll
                    for (int m = 0; m < E; m++) u[m] = lds[lay.idx(t + m * T, c)];
                    lds_barrier();            // before the first exchange of the transform overwrites the tile
                    fft_block_lazy<L, E, -1>(u, lds, lay, (int)opaque_u32((unsigned)t), c, lds_tw, 1);
                }
                // the inverse step's output rows k + L*g are this step's input rows: the same offsets, in `out`
                char* ob = out_bytes + (size_t)tile * (C * sizeof(float2));
                const unsigned vo = opaque_u32(voff_in);
                float2 fu_ah = make_float2(0.f, 0.f);
                if (DC) fu_ah = fu_load_ah();
#pragma unroll
                for (int m = 0; m < E; m++) {
                    float2 v = make_float2(0.f, 0.f);
                    if (hb) v = cmul(u[m], lds_wo[t + m * T]);
                    *reinterpret_cast<float2*>(ob + m * stride_in + vo) = v;
                }
                static_assert(!FUSED || LOGL >= TFFT_TILE_FUSE_MIN_LOG, "COLS_STAT_EMBED: from L = 32 on");
                if (DC && hb) {             // the slot goes back to the DC rows; the next tile's transform has a barrier before it reads them
                    lds_barrier();          // (L >= 32: a transform with an exchange)
                    lds_ah[t * C + c] = fu_ah;
                } else if (!hb) lds_barrier();      // before the next tile's exchanges overwrite the parked values
            } else {
                unsigned e0, e1;
                em_range(tile, e0, e1);
                float2* fl = P.em_fl + (size_t)img * P.em_n;
#pragma unroll
                for (int i = 0; i < NE; i++) {      // no predicate on the store (see FULL): lanes without an entry write to the context's scratch line
                    const TileBin tb = enC[i].tb;
                    float2* dst = enC[i].live ? fl + (e0 + (unsigned)(em_tid + i * em_nthr)) : reinterpret_cast<float2*>(P.trash) + em_tid;
                    *dst = read_listed(tb);
                }
                for (unsigned e = e0 + (unsigned)(em_tid + NE * em_nthr); e < e1; e += em_nthr) {
                    const TileBin tb = P.rd_bins[e];
                    fl[e] = read_listed(tb);
                }
                lds_barrier();            // before the next tile's exchanges overwrite the parked values
            }
            if (PF) {
#pragma unroll
                for (int i = 0; i < NE; i++) enC[i] = enN[i];
            }
        }
        if (PF) {
#pragma unroll
            for (int m = 0; m < E; m++) u[m] = un[m];
            awc = awn;
        }
    }
    if (MODE == COLS_PLAIN && SIGN > 0 && FULL) {
        if (hist_on) {
            lds_barrier();
            unsigned* gh = P.hist_sel[3 * img + plane].hist;
            for (int i = (gl * T + t) * C + c; i < 4096; i += (int)(blockDim.x * blockDim.y * blockDim.z))
                if (lds_hist[i]) atomicAdd(&gh[i], lds_hist[i]);
        }
    }
    if (STAT) {            // the workgroup's sums: one global atomic each (a per-thread atomic on one address per plane serialises)
        // (opaque: computed here, not carried through the tile loop in a register the allocator then spills)
        unsigned* st_wcnt = lds_eo + (blockDim.z - opaque_u32(threadIdx.z)) * (NOFF + 2) + ((blockDim.x * blockDim.y * blockDim.z + 63) >> 6) * TFFT_STAT_SLOTS;      // [0], [1]: the workgroup's sums
        st_fill();
        lds_barrier();
        if (threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0) { st_wcnt[0] = 0; st_wcnt[1] = 0; }
        lds_barrier();
        if (st_below) atomicAdd(&st_wcnt[0], 2u * st_below);          // a stored bin = two full-grid bins of equal magnitude
        if (st_capcount) atomicAdd(&st_wcnt[1], st_capcount);       // corrections may be negative: the sums wrap back
        lds_barrier();
        if (threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0) {
            if (st_wcnt[0]) atomicAdd(&st_s->below, (unsigned long long)st_wcnt[0]);
            if (P.st_cap && st_wcnt[1])
                atomicAdd(&P.st_partial[((size_t)img * 3 + plane) * TFFT_STAT_MAX_BLOCKS + ((blockIdx.y * gridDim.x + blockIdx.x) % TFFT_STAT_MAX_BLOCKS)], st_wcnt[1]);
        }
    }
}

// ---------------------------------------------------------------------------
// spectrum access helpers (half spectrum + packed column 0)
// ---------------------------------------------------------------------------
struct BinRef { size_t idx; bool conj; };
__device__ __forceinline__ BinRef locate(int plane, int y, int x, int PH, int PW) {
    const int M = PW >> 1;
    if (x < M) return BinRef{((size_t)plane * PH + y) * M + x, false};
    const int yy = (PH - y) & (PH - 1);
    return BinRef{((size_t)plane * PH + yy) * M + (PW - x), true};
}
__device__ __forceinline__ float2 full_bin(const float2* __restrict__ plane, int y, int x, int PH, int PW) {
    const int M = PW >> 1;
    if (x == 0 || x == M) {
        float2 f0, fm; unpack_col0(plane, y, PH, M, f0, fm);
        return x == 0 ? f0 : fm;
    }
    if (x < M) return plane[(size_t)y * M + x];
    return cconj(plane[(size_t)((PH - y) & (PH - 1)) * M + (PW - x)]);
}

// Highest row of the stored half spectrum that a bin list touches (bins with x > M live in row PH-y of
// the mirror half).  The read path lets the last forward column step skip the stores of every row above
// it: with the default annulus (rmax = 0.45) that is 55 % of the rows.
__global__ void k_bins_last_row(const tfft_bin* __restrict__ bins, uint64_t n, int PH, int PW, int* __restrict__ last_row) {
    int* blk = reinterpret_cast<int*>(tfft_smem);
    if (threadIdx.x == 0) blk[0] = 0;
    __syncthreads();
    int mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const tfft_bin bn = bins[i];
        const int x = bn.x, y = bn.y;
        if (x >= PW || y >= PH) continue;           // k_read flags these
        const int row = (x <= (PW >> 1)) ? y : ((PH - y) & (PH - 1));
        mine = row > mine ? row : mine;
    }
    if (mine) atomicMax(&blk[0], mine);
    __syncthreads();
    if (threadIdx.x == 0 && blk[0]) atomicMax(last_row, blk[0]);
}

// stream bit i of Rep-3(header, 38 bytes) || Rep-7(payload), MSB first (bits_from_bytes + rep3/rep7_encode, S:455-467, S:494-500)
__device__ __forceinline__ unsigned frame_bit(const uint8_t* __restrict__ header, const uint8_t* __restrict__ payload, uint64_t i) {
    uint64_t b; const uint8_t* src;
    if (i < 912) { b = i / 3; src = header; }
    else { b = (i - 912) / 7; src = payload; }
    return (unsigned)((src[b >> 3] >> (7 - (b & 7))) & 1);
}

// write_bit_on_bin S:712-732 over a bin list (the loop body of S:1074-1097).
__global__ void k_embed(float2* __restrict__ spec, const tfft_bin* __restrict__ bins, const uint8_t* __restrict__ bits,
                        const float* __restrict__ jitter, EmbedParams P, int* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const int img = blockIdx.y;              // images of a batch share the bin list, not the bits (unless each has its own walk: bins_stride)
    spec += (size_t)img * P.img_stride;
    if (bits) bits += (size_t)img * P.n;
    bins += (size_t)img * P.bins_stride;
    if (jitter) jitter += (size_t)img * P.bins_stride;
    const tfft_bin bn = bins[i];
    const uint64_t j = P.bit_index ? (uint64_t)P.bit_index[i] : i;      // the stream bit this bin carries
    if (j >= P.limit) return;                // the stream ends before this position of the walk (tfft_embed_stream_batch_dev)
    const int x = bn.x, y = bn.y, p = bn.plane;
    if (p > 2 || x >= P.PW || y >= P.PH || x == 0 || y == 0 || 2 * x == P.PW || 2 * y == P.PH) {
        atomicOr(err, 1);     // outside the grid or on an excluded axis (S:698-700): never produced by the walk
        return;
    }
    const BinRef r = locate(p, y, x, P.PH, P.PW);
    const float2 v = spec[r.idx];
    const float mag = fmaxf(1e-12f, mag_of(v));
    // the stream pipelines hand over packed bytes: the bit is computed from them (a few KB per image, cache resident) instead of being
    // read out of an expanded one-byte-per-bit copy at a scattered position
    const int bit = P.frame_hdr ? (int)frame_bit(P.frame_hdr + (size_t)img * 38, P.frame_pay + (size_t)img * P.frame_plen, j) : (int)bits[j];
    float2 nv;
    if (!P.generic) {
        nv = make_float2(mag * P.cos_a, bit ? mag * P.sin_a : -mag * P.sin_a);
    } else {
        double alpha = P.alpha;
        const double med = P.med_dev ? (double)P.med_dev[3 * img + p] : P.med[p];
        if (P.adaptive) alpha *= fmin(2.0, fmax(0.5, (double)mag / fmax(1e-12, med)));   // S:704-710
        const double theta = (bit ? alpha : -alpha) + (jitter ? (double)jitter[j] : 0.0);
        nv = make_float2((float)((double)mag * cos(theta)), (float)((double)mag * sin(theta)));
    }
    spec[r.idx] = r.conj ? cconj(nv) : nv;    // the Hermitian mirror is implicit in the half spectrum
}

// delta embedding: the stream bits in bucket order, one byte per bucket entry and image (2: the stream ends before this position),
// so that the first inverse column step reads entry, value and bit at the same index
__global__ void k_gather_bits(const TileBin* __restrict__ ent, const unsigned* __restrict__ n_ent, const uint8_t* __restrict__ bits,
                              const uint8_t* __restrict__ hdr, const uint8_t* __restrict__ pay, uint64_t plen, uint64_t n, uint64_t limit,
                              uint8_t* __restrict__ out) {
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= *n_ent) return;
    const int img = blockIdx.y;
    const uint64_t j = ent[e].bit;
    unsigned b = 2u;
    if (j < limit) b = hdr ? frame_bit(hdr + (size_t)img * 38, pay + (size_t)img * plen, j) : (unsigned)(bits[(size_t)img * n + j] & 1u);
    out[(size_t)img * n + e] = (uint8_t)b;
}

// jitter of the batched calls in bucket order (tfft_set_phase_options): one unit phasor per bucket entry, shared by every image
__global__ void k_gather_jitter(const TileBin* __restrict__ ent, const unsigned* __restrict__ n_ent, const float* __restrict__ jitter, uint64_t n,
                                float2* __restrict__ out) {
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= *n_ent) return;
    const uint64_t j = ent[e].bit;
    const double jt = j < n ? (double)jitter[j] : 0.0;
    out[e] = make_float2((float)cos(jt), (float)sin(jt));
}

// read_bit_from_bin S:734-746 for one (already conjugate-corrected) bin value
__device__ __forceinline__ int read_bit_value(float2 v, const EmbedParams& P, int p, const float* __restrict__ jitter, uint64_t j) {
    if (!P.generic) return (v.y >= 0.0f) ? 1 : 0;     // nearer of +a / -a for 0 < a < pi, ties -> 1
    const double PI = 3.14159265358979323846;
    const double th = atan2((double)v.y, (double)v.x);
    double alpha = P.alpha;
    if (P.adaptive) {
        const double mag = fmax(1e-12, (double)mag_of(v));
        alpha *= fmin(2.0, fmax(0.5, mag / fmax(1e-12, P.med[p])));
    }
    const double jt = jitter ? (double)jitter[j] : 0.0;
    double dp = fmod(th - (jt + alpha) + PI, 2 * PI); if (dp < 0) dp += 2 * PI; dp = fabs(dp - PI);
    double dn = fmod(th - (jt - alpha) + PI, 2 * PI); if (dn < 0) dn += 2 * PI; dn = fabs(dn - PI);
    return (dp <= dn) ? 1 : 0;
}

// read_bit_from_bin S:734-746 over a bin list.
__global__ void k_read(const float2* __restrict__ spec, const tfft_bin* __restrict__ bins,
                       const float* __restrict__ jitter, EmbedParams P, uint8_t* __restrict__ bits_out,
                       int* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const int img = blockIdx.y;
    spec += (size_t)img * P.img_stride;
    bits_out += (size_t)img * P.n;
    bins += (size_t)img * P.bins_stride;
    if (jitter) jitter += (size_t)img * P.bins_stride;
    const tfft_bin bn = bins[i];
    const uint64_t j = P.bit_index ? (uint64_t)P.bit_index[i] : i;
    const int x = bn.x, y = bn.y, p = bn.plane;
    if (p > 2 || x >= P.PW || y >= P.PH || x == 0 || y == 0 || 2 * x == P.PW || 2 * y == P.PH) {
        atomicOr(err, 1);
        bits_out[j] = 0;
        return;
    }
    const BinRef r = locate(p, y, x, P.PH, P.PW);
    float2 v = spec[r.idx];
    if (r.conj) v = cconj(v);
    bits_out[j] = (uint8_t)read_bit_value(v, P, p, jitter, j);
}

// ---------------------------------------------------------------------------
// Tile buckets for the spectrum-free extraction: the final forward column step holds a 16-column x L-row
// tile of the final spectrum in LDS (rows y = g + G*k of group g); bucket b = (plane*G + g)*ntiles + tile
// lists the bins of the walk that live in that tile, so the kernel reads their bits there and the
// spectrum is never written.  count -> exclusive scan -> fill (order inside a bucket is irrelevant).
// Invalid bins (off grid / on an excluded axis) set the error flag and are left out (their bits stay 0).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool tile_bin_of(const tfft_bin bn, int PH, int PW, int G, unsigned& bucket, TileBin& tb) {
    const int x = bn.x, y = bn.y, p = bn.plane;
    if (p > 2 || x >= PW || y >= PH || x == 0 || y == 0 || 2 * x == PW || 2 * y == PH) return false;
    const int M = PW >> 1, ntiles = (M + 15) >> 4;
    const bool conj = x > M;
    const int xs = conj ? PW - x : x, ys = conj ? ((PH - y) & (PH - 1)) : y;
    const int g = ys % G;
    bucket = (unsigned)((p * G + g) * ntiles + (xs >> 4));
    tb.k = (uint16_t)(ys / G); tb.c = (uint8_t)(xs & 15); tb.conj = conj ? 1 : 0; tb.bit = 0;
    return true;
}
// Every workgroup takes a CONTIGUOUS chunk of the list.  When the chunk's buckets span fewer than
// BUCKET_LCAP ids -- always, for a list in address order, whose neighbours share rows: that is why the bucket
// id puts the tile last -- it counts in an LDS histogram of that span and touches each global counter once.
// The first version added every bin to the global counters directly: at any moment all workgroups were on the
// same few rows, and 231 000 atomics on ~150 hot addresses took 137 us (count) + 206 us (fill) per call.
// Chunks with a wide span (a list in walk order) use global atomics, which such a list scatters by itself.
constexpr unsigned BUCKET_LCAP = 8192;
__device__ __forceinline__ bool bucket_span(const tfft_bin* __restrict__ bins, uint64_t lo, uint64_t hi, int PH, int PW, int G,
                                            unsigned* mm, unsigned& bmin, unsigned& width, int* err) {
    if (threadIdx.x == 0) { mm[0] = 0xFFFFFFFFu; mm[1] = 0u; }
    __syncthreads();
    unsigned tmin = 0xFFFFFFFFu, tmax = 0u;          // per thread first: 4096 LDS atomics on two addresses cost ~25 us per workgroup
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        unsigned b; TileBin tb;
        if (tile_bin_of(bins[i], PH, PW, G, b, tb)) { tmin = b < tmin ? b : tmin; tmax = b > tmax ? b : tmax; }
        else if (err) atomicOr(err, 1);
    }
    if (tmin <= tmax) { atomicMin(&mm[0], tmin); atomicMax(&mm[1], tmax); }
    __syncthreads();
    bmin = mm[0];
    const unsigned bmax = mm[1];
    width = (bmin <= bmax) ? bmax - bmin + 1 : 0;
    return width > 0 && width <= BUCKET_LCAP;
}
__global__ void k_bucket_count(const tfft_bin* __restrict__ bins, uint64_t n, int PH, int PW, int G, unsigned* __restrict__ cnt,
                               int* __restrict__ err, int force_global) {
    unsigned* lc = reinterpret_cast<unsigned*>(tfft_smem);        // [BUCKET_LCAP] + min/max
    unsigned* mm = lc + BUCKET_LCAP;
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x, lo = (uint64_t)blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    unsigned bmin, width;
    const bool local = bucket_span(bins, lo, hi, PH, PW, G, mm, bmin, width, err) && !force_global;
    if (local) {
        for (unsigned i = threadIdx.x; i < width; i += blockDim.x) lc[i] = 0;
        __syncthreads();
    }
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        unsigned b; TileBin tb;
        if (tile_bin_of(bins[i], PH, PW, G, b, tb)) atomicAdd(local ? &lc[b - bmin] : &cnt[b], 1u);
    }
    if (local) {
        __syncthreads();
        for (unsigned i = threadIdx.x; i < width; i += blockDim.x) if (lc[i]) atomicAdd(&cnt[bmin + i], lc[i]);
    }
}
// exclusive scan of the bucket counts in three small launches (a single workgroup walking 49 152 counters took
// 119 us): A: every workgroup scans its 1024 counters in LDS and publishes its total; B: one workgroup scans the
// <= 1024 totals; C: every workgroup adds its prefix.  cnt is reset to 0 (the fill uses it as the cursor).
__global__ void k_bucket_scan_a(unsigned* __restrict__ cnt, unsigned* __restrict__ off, unsigned* __restrict__ totals, int nb) {
    unsigned* sh = reinterpret_cast<unsigned*>(tfft_smem);        // [1024]
    const int t = threadIdx.x, i = blockIdx.x * 1024 + t;
    const unsigned v = (i < nb) ? cnt[i] : 0u;
    if (i < nb) cnt[i] = 0;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                          // Hillis-Steele inclusive scan
        const unsigned a = (t >= d) ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    if (i < nb) off[i] = sh[t] - v;
    if (t == 1023) totals[blockIdx.x] = sh[t];
}
__global__ void k_bucket_scan_b(unsigned* __restrict__ totals, int nblk, unsigned* __restrict__ off, int nb) {
    unsigned* sh = reinterpret_cast<unsigned*>(tfft_smem);
    const int t = threadIdx.x;
    const unsigned v = (t < nblk) ? totals[t] : 0u;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned a = (t >= d) ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    if (t < nblk) totals[t] = sh[t] - v;                          // exclusive prefix of the workgroup totals
    if (t == 1023) off[nb] = sh[t];
}
__global__ void k_bucket_scan_c(unsigned* __restrict__ off, const unsigned* __restrict__ totals, int nb) {
    const int i = blockIdx.x * 1024 + threadIdx.x;
    if (i < nb) off[i] += totals[blockIdx.x];
}
// same chunking as k_bucket_count: count locally, reserve one range per non-zero bucket with ONE global atomic,
// then place the chunk's bins with LDS atomics
__global__ void k_bucket_fill(const tfft_bin* __restrict__ bins, const uint32_t* __restrict__ bit_index, uint64_t n, int PH, int PW,
                              int G, unsigned* __restrict__ cursor, const unsigned* __restrict__ off, TileBin* __restrict__ out,
                              int force_global) {
    unsigned* lc = reinterpret_cast<unsigned*>(tfft_smem);        // [BUCKET_LCAP] local count, then this workgroup's cursor into the bucket
    unsigned* mm = lc + BUCKET_LCAP;
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x, lo = (uint64_t)blockIdx.x * per, hi = (lo + per < n) ? lo + per : n;
    unsigned bmin, width;
    const bool local = bucket_span(bins, lo, hi, PH, PW, G, mm, bmin, width, nullptr) && !force_global;
    if (local) {
        for (unsigned i = threadIdx.x; i < width; i += blockDim.x) lc[i] = 0;
        __syncthreads();
        for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            unsigned b; TileBin tb;
            if (tile_bin_of(bins[i], PH, PW, G, b, tb)) atomicAdd(&lc[b - bmin], 1u);
        }
        __syncthreads();
        for (unsigned i = threadIdx.x; i < width; i += blockDim.x) {
            const unsigned k = lc[i];
            if (k) lc[i] = off[bmin + i] + atomicAdd(&cursor[bmin + i], k);      // start of this workgroup's range in the bucket
        }
        __syncthreads();
    }
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        unsigned b; TileBin tb;
        if (!tile_bin_of(bins[i], PH, PW, G, b, tb)) continue;
        tb.bit = bit_index ? bit_index[i] : (uint32_t)i;
        const unsigned pos = local ? atomicAdd(&lc[b - bmin], 1u) : off[b] + atomicAdd(&cursor[b], 1u);
        out[pos] = tb;
    }
}

// One walk per image (launch_bucket_walks): image i's list is bins[i*n .. (i+1)*n) and owns buckets [i*nb, (i+1)*nb); one more bucket at
// n_images*nb collects the invalid bins of every image (the error flag is raised for them), so that after the scan image i's entries fill
// exactly [i*n, (i+1)*n) whenever its list is valid.  A workgroup takes a contiguous chunk of ONE image's list (a walk scatters its bins over
// the whole grid: no narrow span to count in, as the shared list in address order has) and counts it in an LDS histogram of the image's
// buckets (+ the invalid one) when they fit, touching each global counter once per chunk; otherwise it adds to the global counters directly.
__global__ void k_bucket_count_walks(const tfft_bin* __restrict__ bins, uint64_t n, int chunks, int PH, int PW, int G, unsigned nb,
                                     unsigned* __restrict__ cnt, int* __restrict__ err) {
    unsigned* lc = reinterpret_cast<unsigned*>(tfft_smem);        // [nb + 1] when it fits BUCKET_LCAP
    const int img = blockIdx.x / chunks, ch = blockIdx.x - img * chunks, nimg = gridDim.x / chunks;
    const uint64_t per = (n + chunks - 1) / chunks, lo = (uint64_t)ch * per, hi = (lo + per < n) ? lo + per : n;
    const bool local = nb + 1 <= BUCKET_LCAP;
    const tfft_bin* b0 = bins + (size_t)img * n;
    unsigned* gc = cnt + (size_t)img * nb;
    unsigned* gbad = cnt + (size_t)nimg * nb;
    if (local) {
        for (unsigned i = threadIdx.x; i <= nb; i += blockDim.x) lc[i] = 0;
        __syncthreads();
    }
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        unsigned b; TileBin tb;
        if (!tile_bin_of(b0[i], PH, PW, G, b, tb)) { atomicOr(err, 1); b = nb; }
        atomicAdd(local ? &lc[b] : (b < nb ? &gc[b] : gbad), 1u);
    }
    if (local) {
        __syncthreads();
        for (unsigned i = threadIdx.x; i <= nb; i += blockDim.x) if (lc[i]) atomicAdd(i < nb ? &gc[i] : gbad, lc[i]);
    }
}
__global__ void k_bucket_fill_walks(const tfft_bin* __restrict__ bins, uint64_t n, int chunks, int PH, int PW, int G, unsigned nb,
                                    unsigned* __restrict__ cursor, const unsigned* __restrict__ off, TileBin* __restrict__ out) {
    unsigned* lc = reinterpret_cast<unsigned*>(tfft_smem);
    const int img = blockIdx.x / chunks, ch = blockIdx.x - img * chunks, nimg = gridDim.x / chunks;
    const uint64_t per = (n + chunks - 1) / chunks, lo = (uint64_t)ch * per, hi = (lo + per < n) ? lo + per : n;
    const bool local = nb + 1 <= BUCKET_LCAP;
    const tfft_bin* b0 = bins + (size_t)img * n;
    auto gidx = [&](unsigned b) -> size_t { return b < nb ? (size_t)img * nb + b : (size_t)nimg * nb; };
    if (local) {
        for (unsigned i = threadIdx.x; i <= nb; i += blockDim.x) lc[i] = 0;
        __syncthreads();
        for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            unsigned b; TileBin tb;
            if (!tile_bin_of(b0[i], PH, PW, G, b, tb)) b = nb;
            atomicAdd(&lc[b], 1u);
        }
        __syncthreads();
        for (unsigned i = threadIdx.x; i <= nb; i += blockDim.x) {
            const unsigned k = lc[i];
            if (k) lc[i] = off[gidx(i)] + atomicAdd(&cursor[gidx(i)], k);      // start of this workgroup's range in the bucket
        }
        __syncthreads();
    }
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        unsigned b; TileBin tb;
        if (!tile_bin_of(b0[i], PH, PW, G, b, tb)) { b = nb; tb.k = 0; tb.c = 0; tb.conj = 0; }
        tb.bit = (uint32_t)i;
        const unsigned pos = local ? atomicAdd(&lc[b], 1u) : off[gidx(b)] + atomicAdd(&cursor[gidx(b)], 1u);
        out[pos] = tb;
    }
}
// the stream bits of the per-image entries: entry e is image e / n's (launch_bucket_walks), out[e] as k_gather_bits writes out[img*n + e]
__global__ void k_gather_bits_walks(const TileBin* __restrict__ ent, const uint8_t* __restrict__ bits, const uint8_t* __restrict__ hdr,
                                    const uint8_t* __restrict__ pay, uint64_t plen, uint64_t n, uint64_t limit, uint64_t total,
                                    uint8_t* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint64_t img = e / n;
    const uint64_t j = ent[e].bit;
    unsigned b = 2u;
    if (j < limit) b = hdr ? frame_bit(hdr + img * 38, pay + img * plen, j) : (unsigned)(bits[img * n + j] & 1u);
    out[e] = (uint8_t)b;
}
__global__ void k_gather_jitter_walks(const TileBin* __restrict__ ent, const float* __restrict__ jitter, uint64_t n, uint64_t total,
                                      float2* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint64_t j = ent[e].bit;
    const double jt = j < n ? (double)jitter[(e / n) * n + j] : 0.0;
    out[e] = make_float2((float)cos(jt), (float)sin(jt));
}

// ---- the fitted embed (tfft_embed_stream_batch_fit_dev) ------------------------------------------------------
// Per bucket entry e of a chunk's walks (image e / n): f = the stored value of its bin after a COLS_EMIT step (the bin's own value is
// conj(f) when ent[e].conj), its stream bit (2: beyond the stream) and the jitter phasor e^{ij} (or none).  For 0 < alpha < pi/2 the
// reader's decision is the side of a line: bit 1 <=> u = Im(F e^{-ij}) >= 0 (S:734-746).
__device__ __forceinline__ float fit_u(float2 f, unsigned conj, const float2* __restrict__ jp, uint64_t e) {
    const float2 v = conj ? cconj(f) : f;
    if (!jp) return v.y;
    const float2 p = jp[e];
    return v.y * p.x - v.x * p.y;
}
// from F0 (the cover's values): D0 = F' - F0 in stored coordinates (what COLS_EMBED puts into the tile) and the margin
// mu = max(tau |F0| sin(alpha_k), floor) every entry is fitted to
__global__ void k_fit_init(const TileBin* __restrict__ ent, const float2* __restrict__ fl, const uint8_t* __restrict__ pb, const float2* __restrict__ jp,
                           const tfft_bin* __restrict__ bins, const float* __restrict__ med, uint64_t n, uint64_t total, float alpha, float cos_a,
                           float sin_a, float tau, float mu_floor, float2* __restrict__ d, float* __restrict__ mu) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const unsigned bit = pb[e];
    if (bit >= 2u) { d[e] = make_float2(0.f, 0.f); mu[e] = 0.f; return; }
    const TileBin tb = ent[e];
    const float2 f = fl[e];
    const float mag = fmaxf(1e-12f, mag_of(f));
    float ca = cos_a, sa = sin_a;
    if (med) {          // adaptive alpha (S:704-710) with the image's median of the bin's plane
        const uint64_t img = e / n;
        const int plane = bins[img * n + tb.bit].plane;
        sincosf(alpha * fminf(2.f, fmaxf(0.5f, mag / fmaxf(1e-12f, med[3 * img + plane]))), &sa, &ca);
    }
    float2 nv = make_float2(mag * ca, bit ? mag * sa : -mag * sa);
    if (jp) nv = cmul(nv, jp[e]);
    if (tb.conj) nv = cconj(nv);
    d[e] = csub(nv, f);
    mu[e] = fmaxf(tau * mag * sa, mu_floor);
}
// per image: entries that read wrong, and entries below half their margin (wrong ones included).  grid (nblk, n_images): workgroup b
// counts its share of the image's n entries in LDS and writes ONE pair of partials, partial[(img*nblk + b)*2 ..] (no global atomics)
__global__ void k_fit_count(const TileBin* __restrict__ ent, const float2* __restrict__ fl, const uint8_t* __restrict__ pb,
                            const float2* __restrict__ jp, const float* __restrict__ mu, uint64_t n, unsigned* __restrict__ partial) {
    unsigned* lc = reinterpret_cast<unsigned*>(tfft_smem);
    if (threadIdx.x < 2) lc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t img = blockIdx.y, nblk = gridDim.x;
    const uint64_t per = (n + nblk - 1) / nblk, b0 = blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
    const uint64_t lo = img * n + b0, hi = img * n + b1;
    unsigned wrong = 0, weak = 0;
    for (uint64_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
        const unsigned bit = pb[e];
        if (bit >= 2u) continue;
        const float u = fit_u(fl[e], ent[e].conj, jp, e);
        const float su = bit ? u : -u;
        wrong += (bit ? u < 0.f : u >= 0.f) ? 1u : 0u;      // (the reader's tie goes to 1)
        weak += (su < 0.5f * mu[e]) ? 1u : 0u;          // (mu > 0: a wrong entry is a weak one too)
    }
    if (wrong) atomicAdd(&lc[0], wrong);
    if (weak) atomicAdd(&lc[1], weak);
    __syncthreads();
    if (threadIdx.x < 2) partial[(img * nblk + blockIdx.x) * 2 + threadIdx.x] = lc[threadIdx.x];
}
// ... summed per image: counts[2*img] wrong, counts[2*img + 1] below half the margin; wrong_out[img] (optional) = the wrong count
__global__ void k_fit_sum(const unsigned* __restrict__ partial, unsigned nblk, unsigned* __restrict__ counts, uint32_t* __restrict__ wrong_out) {
    const unsigned img = blockIdx.x;
    if (threadIdx.x != 0) return;
    unsigned wrong = 0, weak = 0;
    for (unsigned b = 0; b < nblk; b++) { wrong += partial[((size_t)img * nblk + b) * 2]; weak += partial[((size_t)img * nblk + b) * 2 + 1]; }
    counts[2 * img] = wrong; counts[2 * img + 1] = weak;
    if (wrong_out) wrong_out[img] = wrong;
}
// one correction: every entry of a not yet converged image with s*u < mu gets the smallest change of its bin that puts u at s*mu,
// i e^{ij} (s*mu - u), times `gain` (the crop keeps W*H/(PW*PH) of a bin's energy: gain = PW*PH/(W*H)), added to its delta in stored
// coordinates (conjugated for a mirror entry)
__global__ void k_fit_correct(const TileBin* __restrict__ ent, const float2* __restrict__ fl, const uint8_t* __restrict__ pb,
                              const float2* __restrict__ jp, const float* __restrict__ mu, const unsigned* __restrict__ counts, uint64_t n,
                              uint64_t total, float gain, float2* __restrict__ d) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint64_t img = e / n;
    if (counts[2 * img] == 0 && counts[2 * img + 1] == 0) return;      // converged: its stego stays as it is
    const unsigned bit = pb[e];
    if (bit >= 2u) return;
    const TileBin tb = ent[e];
    const float u = fit_u(fl[e], tb.conj, jp, e);
    const float m = mu[e], target = bit ? m : -m;
    if (bit ? u >= m : u <= -m) return;
    const float s = (target - u) * gain;
    const float2 p = jp ? jp[e] : make_float2(1.f, 0.f);
    float2 dv = make_float2(-p.y * s, p.x * s);          // i e^{ij} s
    if (tb.conj) dv = cconj(dv);
    d[e] = cadd(d[e], dv);
}

// ---------------------------------------------------------------------------
// exports for parity tests and the cover hash (S:428-436)
// ---------------------------------------------------------------------------
__global__ void k_export_full(const float2* __restrict__ spec, int PH, int PW, int PWout, float2* __restrict__ out) {
    const unsigned n = 3u * (unsigned)PH * (unsigned)PWout;              // <= 3 * 8192 * 8192
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned r = e / (unsigned)PWout;
    const int x = (int)(e - r * (unsigned)PWout), p = (int)(r / (unsigned)PH), y = (int)(r - (unsigned)p * (unsigned)PH), M = PW >> 1;
    const float2* pl = spec + (size_t)p * PH * M;
    const int ym = (PH - y) & (PH - 1);
    float2 v;
    if (x == 0 || x == M) {             // the packed column 0 (unpack_col0)
        const float2 a = pl[(size_t)y * M], b = pl[(size_t)ym * M];
        v = x == 0 ? make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)) : make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
    } else if (x < M) v = pl[(size_t)y * M + x];
    else v = cconj(pl[(size_t)ym * M + (PW - x)]);
    out[e] = v;
}
// compute_cover_hash's magnitudes (S:428-436) in fp64, straight from the pixels: |F[y][x]| for y, x < region <= 8 is a
// 3 x region x region corner of the spectrum, i.e. 192 inner products with the image -- no transform needed, and fp64
// keeps the quantiser floor(log(1+mag)/2) (S:433) on the reference's side of every bucket edge (the fp32 spectrum is
// 1e-7..1e-6 off; these values agree with the reference's fp64 FFT to ~1e-13).
//   rows: grid (H, images)  block (32, region)   rowsum[n][p][x] = sum_m s(m) pix[n][m][p] exp(+2 pi i x m/PW)
//   cols: grid (3*region*region, images)  block 256   out[p][y][x] = | sum_n s(n) rowsum[n][p][x] exp(+2 pi i y n/PH) |
//   (image i of a batch: pixels W*H*3 bytes on, rowsum rs_stride double2 on, out 3*region^2 on; the sums run in the same order)
__device__ __forceinline__ void unit_2pi(long long k, int N, double& c, double& s) {      // exp(2 pi i k/N), N a power of two
    const double t = (double)(k & (long long)(N - 1)) / (double)N;                            // exact
    sincos(6.283185307179586476925286766559 * t, &s, &c);
}
__global__ void k_lowfreq_rows_f64(const uint8_t* __restrict__ rgb, int W, int PW, int center, int region, double2* __restrict__ rowsum,
                                   size_t img_bytes, size_t rs_stride) {
    double* red = reinterpret_cast<double*>(tfft_smem);                 // [region][32][6]
    const int lane = threadIdx.x, x = threadIdx.y, n = blockIdx.x;
    rgb += (size_t)blockIdx.y * img_bytes;
    rowsum += (size_t)blockIdx.y * rs_stride;
    const uint8_t* row = rgb + (size_t)n * W * 3;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int m = lane; m < W; m += 32) {
        double c, s; unit_2pi((long long)x * m, PW, c, s);
        if (center && (m & 1)) { c = -c; s = -s; }
#pragma unroll
        for (int p = 0; p < 3; p++) { const double v = (double)row[3 * m + p]; acc[2 * p] += v * c; acc[2 * p + 1] += v * s; }
    }
    double* mine = red + ((size_t)x * 32 + lane) * 6;
#pragma unroll
    for (int i = 0; i < 6; i++) mine[i] = acc[i];
    __syncthreads();
    for (int d = 16; d >= 1; d >>= 1) {
        if (lane < d) {
#pragma unroll
            for (int i = 0; i < 6; i++) mine[i] += mine[d * 6 + i];
        }
        __syncthreads();
    }
    const double* tot = red + (size_t)x * 32 * 6;                        // lane 0's slot holds the sums of this x
    if (lane < 3) rowsum[((size_t)n * 3 + lane) * region + x] = make_double2(tot[2 * lane], tot[2 * lane + 1]);
}
__global__ void k_lowfreq_cols_f64(const double2* __restrict__ rowsum, int H, int PH, int center, int region, double* __restrict__ out,
                                   size_t rs_stride) {
    double* red = reinterpret_cast<double*>(tfft_smem);                 // [256][2]
    const int e = blockIdx.x, x = e % region, y = (e / region) % region, p = e / (region * region);
    rowsum += (size_t)blockIdx.y * rs_stride;
    out += (size_t)blockIdx.y * 3 * region * region;
    double re = 0, im = 0;
    for (int n = threadIdx.x; n < H; n += blockDim.x) {
        double c, s; unit_2pi((long long)y * n, PH, c, s);
        if (center && (n & 1)) { c = -c; s = -s; }
        const double2 r = rowsum[((size_t)n * 3 + p) * region + x];
        re += r.x * c - r.y * s; im += r.x * s + r.y * c;
    }
    red[2 * threadIdx.x] = re; red[2 * threadIdx.x + 1] = im;
    __syncthreads();
    for (int d = blockDim.x / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) { red[2 * threadIdx.x] += red[2 * (threadIdx.x + d)]; red[2 * threadIdx.x + 1] += red[2 * (threadIdx.x + d) + 1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[e] = hypot(red[0], red[1]);
}

// ---------------------------------------------------------------------------
// stream framing on the device: bits_from_bytes + rep3/rep7_encode (S:455-467, S:494-500)
// and rep3/rep7_decode + bytes_from_bits (S:447-454, S:468-474, S:501-508), MSB first, one byte per bit in
// the stream.  Only packed bytes (38-byte header, ciphertext || tag) then cross PCIe.
//   expand  : grid (ceil(n_bits/256), n_images);  majority: grid (ceil((38+plen)/256), n_images)
// ---------------------------------------------------------------------------
// one thread per FOUR stream bits (n = 912 + 56*plen is a multiple of 4): one dword store when the image's stream is 4-byte aligned
// (one-byte stores were 16-28 us per call for a few MB)
__global__ void k_frame_expand(const uint8_t* __restrict__ header, const uint8_t* __restrict__ payload, uint64_t plen,
                               uint8_t* __restrict__ bits, uint64_t stride) {
    const uint64_t n = 38ull * 24 + plen * 56;
    const uint64_t i = 4 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const uint64_t img = blockIdx.y;
    const uint8_t* h = header + img * 38;
    const uint8_t* p = payload + img * plen;
    const unsigned v = frame_bit(h, p, i) | (frame_bit(h, p, i + 1) << 8) | (frame_bit(h, p, i + 2) << 16) | (frame_bit(h, p, i + 3) << 24);
    uint8_t* dst = bits + img * stride + i;
    if (((uintptr_t)dst & 3) == 0) *reinterpret_cast<uint32_t*>(dst) = v;
    else { dst[0] = (uint8_t)v; dst[1] = (uint8_t)(v >> 8); dst[2] = (uint8_t)(v >> 16); dst[3] = (uint8_t)(v >> 24); }
}
__global__ void k_frame_majority(const uint8_t* __restrict__ bits, uint64_t plen, uint8_t* __restrict__ header,
                                 uint8_t* __restrict__ payload) {
    const uint64_t n = 38ull * 24 + plen * 56;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 38 + plen) return;
    const uint64_t img = blockIdx.y;
    const uint8_t* in = bits + img * n;
    unsigned v = 0;
    if (j < 38) {
        for (int q = 0; q < 8; q++) {
            const uint8_t* p = in + (j * 8 + q) * 3;
            v = (v << 1) | ((p[0] + p[1] + p[2]) >= 2 ? 1u : 0u);
        }
        header[img * 38 + j] = (uint8_t)v;
    } else {
        const uint64_t k = j - 38;
        for (int q = 0; q < 8; q++) {
            const uint8_t* p = in + 912 + (k * 8 + q) * 7;
            v = (v << 1) | ((p[0] + p[1] + p[2] + p[3] + p[4] + p[5] + p[6]) >= 4 ? 1u : 0u);
        }
        payload[img * plen + k] = (uint8_t)v;
    }
}

// The extractor's two phases on the device (S:1223-1264): Rep-3 majority of the first 912 raw bits -> 38 header bytes ->
// magic / version / clen -> how many bits of the SAME walk the payload takes; then Rep-7 majority of exactly those.
//   status[img] = clen (>= 0) | -1 magic not found | -2 unsupported version | -3 the bin list (n_bins) or the payload
//   buffer (max_plen) is too short for 912 + 56*(clen+16) bits (the reference would keep walking: S:1260-1264)
//   plen[img]   = clen + 16 when status >= 0, else 0
//   header: grid (n_images) block 64          payload: grid (ceil(max_plen/256), n_images) block 256
__global__ void k_stream_header(const uint8_t* __restrict__ bits, uint64_t n_bins, uint64_t max_plen, uint8_t* __restrict__ header,
                                int* __restrict__ status, unsigned* __restrict__ plen) {
    uint8_t* hb = reinterpret_cast<uint8_t*>(tfft_smem);        // [38]
    const uint64_t img = blockIdx.x;
    const uint8_t* in = bits + img * n_bins;
    const int j = threadIdx.x;
    if (j < 38) {
        unsigned v = 0;
        if (n_bins >= 912) {
            for (int q = 0; q < 8; q++) {
                const uint8_t* p = in + (j * 8 + q) * 3;
                v = (v << 1) | ((p[0] + p[1] + p[2]) >= 2 ? 1u : 0u);
            }
        }
        hb[j] = (uint8_t)v;
        header[img * 38 + j] = (uint8_t)v;
    }
    __syncthreads();
    if (j == 0) {
        int st; unsigned pl = 0;
        if (n_bins < 912) st = -3;
        else if (!(hb[0] == 'F' && hb[1] == 'T' && hb[2] == 'T' && hb[3] == 'G')) st = -1;      // S:1236
        else if (hb[4] != 2) st = -2;                                                            // S:1237
        else {
            const unsigned long long clen = ((unsigned long long)hb[34] << 24) | ((unsigned long long)hb[35] << 16) | ((unsigned long long)hb[36] << 8) | hb[37];
            const unsigned long long rest = clen + 16, need = 912ull + rest * 56ull;
            if (need > n_bins || rest > max_plen) st = -3;
            else { st = (int)clen; pl = (unsigned)rest; }
        }
        status[img] = st; plen[img] = pl;
    }
}
__global__ void k_stream_payload(const uint8_t* __restrict__ bits, uint64_t n_bins, uint64_t max_plen, const unsigned* __restrict__ plen,
                                 uint8_t* __restrict__ payload) {
    const uint64_t img = blockIdx.y, k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= plen[img]) return;
    const uint8_t* p = bits + img * n_bins + 912 + k * 56;
    unsigned v = 0;
    for (int q = 0; q < 8; q++, p += 7)
        v = (v << 1) | ((p[0] + p[1] + p[2] + p[3] + p[4] + p[5] + p[6]) >= 4 ? 1u : 0u);
    payload[img * max_plen + k] = (uint8_t)v;
}

// ===========================================================================
// launchers
// ===========================================================================
hipError_t launch_frame_expand(const uint8_t* header, const uint8_t* payload, uint64_t plen, int n_images, uint8_t* bits,
                               uint64_t stride, hipStream_t s) {
    const uint64_t n = 38ull * 24 + plen * 56;
    if (stride < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_frame_expand, dim3((unsigned)((n / 4 + 255) / 256), n_images), dim3(256), 0, s, header, payload, plen, bits, stride);
    return hipGetLastError();
}
hipError_t launch_frame_majority(const uint8_t* bits, uint64_t plen, int n_images, uint8_t* header, uint8_t* payload,
                                 hipStream_t s) {
    hipLaunchKernelGGL(k_frame_majority, dim3((unsigned)((38 + plen + 255) / 256), n_images), dim3(256), 0, s, bits, plen, header, payload);
    return hipGetLastError();
}
hipError_t launch_stream_decode(const uint8_t* bits, uint64_t n_bins, uint64_t max_plen, int n_images, uint8_t* header, uint8_t* payload,
                                int* status, unsigned* plen, hipStream_t s) {
    if (n_images == 0) return hipSuccess;
    hipLaunchKernelGGL(k_stream_header, dim3(n_images), dim3(64), 64, s, bits, n_bins, max_plen, header, status, plen);
    if (max_plen)
        hipLaunchKernelGGL(k_stream_payload, dim3((unsigned)((max_plen + 255) / 256), n_images), dim3(256), 0, s, bits, n_bins, max_plen, plen, payload);
    return hipGetLastError();
}

#define TFFT_DISPATCH_LOG(n, F)                                                                   \
    switch (n) {                                                                                  \
        case 0: F(0); break; case 1: F(1); break; case 2: F(2); break; case 3: F(3); break;       \
        case 4: F(4); break; case 5: F(5); break; case 6: F(6); break; case 7: F(7); break;       \
        case 8: F(8); break; case 9: F(9); break; case 10: F(10); break; case 11: F(11); break;   \
        case 12: F(12); break; case 13: F(13); break;                                             \
        default: return hipErrorInvalidValue;                                                     \
    }

constexpr int rows_ppb(int logm) { return logm <= 10 ? 3 : 1; }   // wide rows: one plane (few waves) per workgroup   // 3 planes/block while 3*M*8 B fits LDS comfortably

template <int LOGM, int PPB, bool FWD>
static hipError_t launch_rows_t(const void* in, void* out, const float2* tw, const RowParams& P, int n_images,
                                hipStream_t s) {
    constexpr int M = 1 << LOGM, E = rows_elems(LOGM), T = M / E;
    const size_t lds = (size_t)PPB * LayRows::padded(M) * sizeof(float2);
    dim3 grid(PPB == 1 ? P.H * 3 : P.H, PPB == 1 ? 1 : 3 / PPB, n_images), block(T, PPB, 1);
    if (FWD) {
        auto k = k_rows_fwd<LOGM, PPB>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k, grid, block, lds, s, (const uint8_t*)in, (float2*)out, tw, P);
    } else {
        auto k = k_rows_inv<LOGM, PPB>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k, grid, block, lds, s, (const float2*)in, (uint8_t*)out, tw, P);
    }
    return hipGetLastError();
}

hipError_t launch_rows_fwd(const uint8_t* rgb, float2* out, const float2* tw_pw, const RowParams& P, int n_images,
                           hipStream_t s) {
    const int logm = ilog2(P.PW >> 1);
#define F(n) return launch_rows_t<n, rows_ppb(n), true>(rgb, out, tw_pw, P, n_images, s)
    TFFT_DISPATCH_LOG(logm, F)
#undef F
    return hipSuccess;
}
template <int LOGM>
static hipError_t launch_rowcol_fwd_t(const uint8_t* rgb, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P,
                                      int n_images, hipStream_t s) {
    constexpr int LOGN1 = 3, M = 1 << LOGM;
    const size_t lds = ((size_t)(1 << LOGN1) * LayRows::padded(M) + M + (1 << LOGN1)) * sizeof(float2);    // row slabs + twiddle tables
    auto k = k_rowcol_fwd<LOGN1, LOGM>;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((P.PH >> LOGN1) * 3, n_images), dim3(M / 16, 1 << LOGN1), lds, s, rgb, out, tw_pw, tw_ph, P);
    return hipGetLastError();
}
hipError_t launch_rowcol_fwd(const uint8_t* rgb, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P,
                             int n_images, hipStream_t s) {
    if (P.PW == 2048) return launch_rowcol_fwd_t<10>(rgb, out, tw_pw, tw_ph, P, n_images, s);
    if (P.PW == 4096) return launch_rowcol_fwd_t<11>(rgb, out, tw_pw, tw_ph, P, n_images, s);
    return hipErrorInvalidValue;
}
template <int LOGM>
static hipError_t launch_colrow_inv_t(const float2* in, uint8_t* rgb, const float2* tw_pw, const RowParams& P, int n_images, hipStream_t s) {
    constexpr int LOGN1 = 3, M = 1 << LOGM;
    const size_t lds = ((size_t)(1 << LOGN1) * LayRows::padded(M) + M) * sizeof(float2);    // row slabs + twiddle table
    auto k = k_colrow_inv<LOGN1, LOGM>;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((P.PH >> LOGN1) * 3, n_images), dim3(M / 16, 1 << LOGN1), lds, s, in, rgb, tw_pw, P);
    return hipGetLastError();
}
hipError_t launch_colrow_inv(const float2* in, uint8_t* rgb, const float2* tw_pw, const RowParams& P, int n_images, hipStream_t s) {
    if (P.PW == 2048) return launch_colrow_inv_t<10>(in, rgb, tw_pw, P, n_images, s);
    if (P.PW == 4096) return launch_colrow_inv_t<11>(in, rgb, tw_pw, P, n_images, s);
    return hipErrorInvalidValue;
}
// live-rows-only forward: one launch per distinct number of live rows NL among the groups n2 (at most two values).  (The inverse
// was tried the same way and is no faster -- 0.623 vs 0.613 ms per 8 x 4K launch, 0.416 vs 0.407 per 32 x 1080p: its column phase
// comes first and is all loads, for which the waves of the padded rows are useful help before they exit.)
template <int LOGM, int NL>
static hipError_t launch_fwd_live_t(const uint8_t* in, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P, int n_images,
                                    int n2_lo, int n2_cnt, hipStream_t s) {
    constexpr int M = 1 << LOGM;
    const size_t lds = ((size_t)NL * LayRows::padded(M) + (LOGM <= 10 ? M : 0) + 8) * sizeof(float2);
    auto k = k_rowcol_fwd_live<LOGM, NL>;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(n2_cnt * 3, n_images), dim3(M / 16, NL), lds, s, in, out, tw_pw, tw_ph, P, n2_lo, n2_cnt);
    return hipGetLastError();
}
template <int LOGM>
static hipError_t launch_fwd_live_nl(int nl, const uint8_t* in, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P, int n_images,
                                     int n2_lo, int n2_cnt, hipStream_t s) {
    // PH = next_pow2(H) < 2H and N2 = PH/8, so 4 < H/N2 <= 8: a group has 4 .. 8 live rows
    switch (nl) {
        case 4: return launch_fwd_live_t<LOGM, 4>(in, out, tw_pw, tw_ph, P, n_images, n2_lo, n2_cnt, s);
        case 5: return launch_fwd_live_t<LOGM, 5>(in, out, tw_pw, tw_ph, P, n_images, n2_lo, n2_cnt, s);
        case 6: return launch_fwd_live_t<LOGM, 6>(in, out, tw_pw, tw_ph, P, n_images, n2_lo, n2_cnt, s);
        case 7: return launch_fwd_live_t<LOGM, 7>(in, out, tw_pw, tw_ph, P, n_images, n2_lo, n2_cnt, s);
        default: return launch_fwd_live_t<LOGM, 8>(in, out, tw_pw, tw_ph, P, n_images, n2_lo, n2_cnt, s);
    }
}
// groups n2 < H mod N2 have ceil(H/N2) live rows, the others floor(H/N2)
hipError_t launch_rowcol_fwd_live(const uint8_t* rgb, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P, int n_images, hipStream_t s) {
    const int N2 = P.PH >> 3, hi = P.H / N2, rem = P.H % N2;
    hipError_t e = hipSuccess;
    for (int part = 0; part < 2 && e == hipSuccess; part++) {
        const int lo = part ? rem : 0, cnt = part ? N2 - rem : rem;
        int nl = part ? hi : hi + 1;
        if (cnt == 0) continue;
        if (nl < 4) nl = 4;
        if (nl > 8) nl = 8;
        if (P.PW == 2048) e = launch_fwd_live_nl<10>(nl, rgb, out, tw_pw, tw_ph, P, n_images, lo, cnt, s);
        else if (P.PW == 4096) e = launch_fwd_live_nl<11>(nl, rgb, out, tw_pw, tw_ph, P, n_images, lo, cnt, s);
        else e = hipErrorInvalidValue;
    }
    return e;
}
hipError_t launch_rows_inv(const float2* in, uint8_t* rgb, const float2* tw_pw, const RowParams& P, int n_images,
                           hipStream_t s) {
    const int logm = ilog2(P.PW >> 1);
#define F(n) return launch_rows_t<n, rows_ppb(n), false>(in, rgb, tw_pw, P, n_images, s)
    TFFT_DISPATCH_LOG(logm, F)
#undef F
    return hipSuccess;
}

template <int LOGL, int SIGN, int MODE = COLS_PLAIN, bool DC = false, bool TW = false, bool FULL = false, bool PH = false, bool PI = false>
static hipError_t launch_cols_t(const float2* in, float2* out, const float2* tw, const ColParams& P, int n_planes,
                                hipStream_t s) {
    constexpr int L = 1 << LOGL, E = elems_for(L), T = L / E, C = 16;
    // (the statistics' sample pass may walk every g_step-th row group only)
    const bool gsample = (MODE == COLS_PLAIN && SIGN > 0 && P.hist_sel && P.g_step > 1);
    const int Geff = gsample ? (P.G - P.g_off + P.g_step - 1) / P.g_step : P.G;
    int gpb = 256 / (T * C);
    if (gpb < 1) gpb = 1;
    if (gpb > Geff) gpb = Geff;
    if constexpr (!FULL && (LOGL >= 6 || stat_mode(MODE) || (MODE == COLS_PLAIN && SIGN > 0 && !TW)) && MODE != COLS_ROWLIMIT) {
        // every output element exists: the variant whose stores carry no predicate (ROWLIMIT cuts rows by definition; short columns
        // only for the statistics, whose classification / histogram live in that store loop)
        const int rows_out_max = P.out_a * (L - 1) + P.out_b * (P.G - 1);
        if ((LOGL >= 6 || stat_mode(MODE) || P.hist_sel) && rows_out_max < P.out_rows && P.M % C == 0 && Geff % gpb == 0)
            return launch_cols_t<LOGL, SIGN, MODE, DC, TW, true, PH, PI>(in, out, tw, P, n_planes, s);
        if (stat_mode(MODE)) return hipErrorInvalidValue;      // the in-register classification lives in the unpredicated store loop only
    }
    const size_t lds0 = (size_t)gpb * L * C * sizeof(float2) + (DC || MODE == COLS_STAT_EMBED ? (size_t)gpb * L * sizeof(float2) : 0) + (TW ? (size_t)gpb * L * sizeof(float2) : 0) +
                       (LOGL >= TFFT_COLS_LDS_TW_LOG || MODE == COLS_STAT_EMBED ? (size_t)L * sizeof(float2) : 0);      // (COLS_STAT_EMBED: see the kernel's lds_wo, TWL)
    int ntiles = (P.M + C - 1) / C;
    if (MODE == COLS_PLAIN && SIGN > 0 && P.tile_step > 1) ntiles = (ntiles - P.tile_off + P.tile_step - 1) / P.tile_step;      // the statistics' sample: every tile_step-th tile
    int tpb = P.tiles_per_block > 0 ? P.tiles_per_block : 1;
    ColParams Q = P;
    constexpr bool BUCKETS = (MODE == COLS_READ || embed_mode(MODE) || MODE == COLS_EMIT || stat_mode(MODE));
    if (BUCKETS) {          // the bucket offsets of a workgroup's tiles are staged in LDS: 16 tiles + sentinel per group
        if (tpb > 16) tpb = 16;
        if (tpb > ntiles) tpb = ntiles;      // a grid narrower than the request: COLS_STAT's reservations (st_resv) go with the tiles a workgroup really has
        Q.tiles_per_block = tpb;
    }
    const size_t nwaves = ((size_t)C * T * gpb + 63) / 64;
    const size_t lds = lds0 + (BUCKETS ? (size_t)gpb * (C * sizeof(float2) + 18 * sizeof(unsigned)) : 0) +
                       (stat_mode(MODE) ? (nwaves * (TFFT_STAT_SLOTS + 1) + 2) * sizeof(unsigned) : 0);
    size_t lds_total = lds;
    if (MODE == COLS_PLAIN && SIGN > 0 && P.hist_sel) {
        if (!FULL) return hipErrorInvalidValue;      // the histogram lives in the unpredicated store loop only
        Q.hist_lds_off = (unsigned)((lds + 15) & ~(size_t)15);
        lds_total = Q.hist_lds_off + 4096 * sizeof(unsigned);
    }
    if (gsample && (!FULL || P.g_off + (Geff - 1) * P.g_step >= P.G)) return hipErrorInvalidValue;
    dim3 grid((ntiles + tpb - 1) / tpb, (Geff + gpb - 1) / gpb, n_planes), block(C, T, gpb);      // n_planes = 3 * n_images
    if (stat_mode(MODE)) {
        Q.st_resv = 64u * (unsigned)tpb;        // a wave stages ~45 of a tile's 1024 values (three sixteenth-octave buckets around the median)
        const size_t fixed = (size_t)grid.x * grid.y * nwaves * Q.st_resv;
        if (fixed + (size_t)P.PH * (P.M + 1) > P.st_cand_stride) return hipErrorInvalidValue;
        Q.st_cand_fixed = (unsigned)fixed;
    }
    if constexpr (MODE == COLS_STAT_EMBED && !FULL) return hipErrorInvalidValue;      // (never reached: the predicated form is not even built)
    else {
        auto k = k_fft_cols<LOGL, SIGN, MODE, DC, TW, FULL, PH, PI>;
        if (lds_total > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_total);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k, grid, block, lds_total, s, in, out, tw, Q);
        return hipGetLastError();
    }
}
// Which instantiations of k_fft_cols exist (FULL aside, which launch_cols_t picks): the guard of the dispatch below, so also what
// launch_cols accepts.  The inverse knows the plain step and the first step of a delta embed (no DC term: the tile holds F' - F);
// every other mode belongs to the final forward step (no output twiddles), the plain forward step is the final one (DC) or the
// first of two (TW).  PH: COLS_EMBED and COLS_READ only; PI: the bucket modes, COLS_EMBED_D in no other form
constexpr bool cols_variant_exists(int mode, int sign, bool dc, bool tw, bool ph, bool pi) {
    if (sign < 0) return mode == COLS_PLAIN ? !ph && !pi : mode == COLS_EMBED ? !dc : mode == COLS_EMBED_D ? !dc && !ph && pi : false;
    switch (mode) {
        case COLS_PLAIN: return !(dc && tw) && !ph && !pi;
        case COLS_ROWLIMIT: return !tw && !ph && !pi;
        case COLS_READ: return !tw;
        case COLS_EMIT: case COLS_STAT: return !tw && !ph;
        case COLS_STAT_EMBED: return !tw;      // (jitter: PH, as COLS_EMBED; the output twiddles are the inverse half's own, always on)
        default: return false;
    }
}
// a run-time value lo <= v <= hi as a compile-time one: f(std::integral_constant<int, v>).  launch_cols nests four of these, so the
// innermost body exists 10 x 2 x 8 x 16 times on the host; where cols_variant_exists says no, that body is `return hipErrorInvalidValue`
// alone and names no kernel, so only the existing forms are instantiated.  (The row launchers' sizes go through TFFT_DISPATCH_LOG.)
template <int LO, int HI, class F>
static hipError_t with_constant(int v, const F& f) {
    if constexpr (LO > HI) return hipErrorInvalidValue;
    else return v == LO ? f(std::integral_constant<int, LO>{}) : with_constant<LO + 1, HI>(v, f);
}
hipError_t launch_cols(const float2* in, float2* out, const float2* tw_ph, const ColParams& P, const ColStep& step, int n_planes, hipStream_t s) {
    const int mode = step.mode;
    const bool fwd = step.sign > 0, emit = mode == COLS_EMIT || stat_mode(mode), buckets = emit || embed_mode(mode) || mode == COLS_READ;
    if (step.logl > 9) return hipErrorInvalidValue;      // 512 x 16 x 8 B tiles: two workgroups per CU; plan_cols never asks for more
    // what the mode reads (the bucket modes redirect the stores of idle lanes to the context's scratch line)
    if (buckets && (!P.rd_bins || !P.trash)) return hipErrorInvalidValue;
    if ((emit || embed_mode(mode)) && !P.em_fl) return hipErrorInvalidValue;
    if (mode == COLS_ROWLIMIT && !P.last_row_dev) return hipErrorInvalidValue;
    if (mode == COLS_STAT_EMBED && (!fwd || !P.em_pb || P.em_m2 || in == out || P.in_a != 1 || P.in_b != (1 << step.logl) || P.out_b != 1)) return hipErrorInvalidValue;      // the last step of a two-step plan
    if (stat_mode(mode) && (step.logl < 4 || !P.st_sel || !P.st_cand || !P.st_col0 || (P.st_cap && (!P.st_partial || !P.st_amb)))) return hipErrorInvalidValue;
    // fields that change what a launch does, in the one mode that honours them
    if (P.em_m2 && fwd && !(emit && P.st_col0)) return hipErrorInvalidValue;      // |F|^2 planes: COLS_EMIT (COLS_STAT stores nothing, the inverse step ignores it)
    if ((P.tile_step > 1 || P.gate) && !(mode == COLS_PLAIN && fwd && !P.tw_out)) return hipErrorInvalidValue;      // plain final forward step only
    if (P.em_med && mode != COLS_EMBED) return hipErrorInvalidValue;      // adaptive alpha: the embedding step only (COLS_READ knows the jitter alone)
    // DC: ColParams::dc_ah, TW: tw_out, PH: the phase options, PI: one walk per image
    const int sw = (P.dc_ah ? 1 : 0) | (P.tw_out ? 2 : 0) | (P.em_jp || P.em_med ? 4 : 0) | (step.walks ? 8 : 0);
    return with_constant<0, 9>(step.logl, [&](auto logl) {
        return with_constant<0, 1>(fwd ? 1 : 0, [&](auto f) {
            return with_constant<COLS_PLAIN, COLS_STAT_EMBED>(mode, [&](auto m) {
                return with_constant<0, 15>(sw, [&](auto w) {
                    constexpr int LOGL = decltype(logl)::value, SIGN = decltype(f)::value ? +1 : -1, MODE = decltype(m)::value, SW = decltype(w)::value;
                    constexpr bool DC = SW & 1, TW = SW & 2, PH = SW & 4, PI = SW & 8;
                    if constexpr (cols_variant_exists(MODE, SIGN, DC, TW, PH, PI) && !(MODE == COLS_STAT_EMBED && LOGL < TFFT_TILE_FUSE_MIN_LOG)) return launch_cols_t<LOGL, SIGN, MODE, DC, TW, false, PH, PI>(in, out, tw_ph, P, n_planes, s);
                    else return hipErrorInvalidValue;
                });
            });
        });
    });
}

hipError_t launch_bucket_bins(const tfft_bin* bins, const uint32_t* bit_index, uint64_t n, int PH, int PW, int G,
                              unsigned* cnt, unsigned* off, TileBin* out, int* err, int force_global, hipStream_t s) {
    const int M = PW >> 1, ntiles = (M + 15) >> 4, nb = 3 * ntiles * G;
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)nb * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    unsigned blocks = (unsigned)((n + 2047) / 2048);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    const size_t lds = (BUCKET_LCAP + 2) * sizeof(unsigned);
    hipLaunchKernelGGL(k_bucket_count, dim3(blocks), dim3(256), lds, s, bins, n, PH, PW, G, cnt, err, force_global);
    const int nblk = (nb + 1023) / 1024;                          // <= 1024 for every grid up to 16384^2 (3*512*64 buckets / 1024 = 96)
    if (nblk > 1024) return hipErrorInvalidValue;
    unsigned* totals = off + nb + 1;                              // the offsets buffer holds nb + 1 + nblk words
    hipLaunchKernelGGL(k_bucket_scan_a, dim3(nblk), dim3(1024), 1024 * sizeof(unsigned), s, cnt, off, totals, nb);
    hipLaunchKernelGGL(k_bucket_scan_b, dim3(1), dim3(1024), 1024 * sizeof(unsigned), s, totals, nblk, off, nb);
    hipLaunchKernelGGL(k_bucket_scan_c, dim3(nblk), dim3(1024), 0, s, off, totals, nb);
    hipLaunchKernelGGL(k_bucket_fill, dim3(blocks), dim3(256), lds, s, bins, bit_index, n, PH, PW, G, cnt, off, out, force_global);
    return hipGetLastError();
}
hipError_t launch_bucket_walks(const tfft_bin* bins, uint64_t n, int n_images, int PH, int PW, int G, unsigned* cnt, unsigned* off, TileBin* out,
                               int* err, hipStream_t s) {
    if (n == 0 || n_images <= 0) return hipErrorInvalidValue;
    const int M = PW >> 1, ntiles = (M + 15) >> 4;
    const unsigned nb = 3u * (unsigned)ntiles * (unsigned)G, nbi = nb + 1;
    const uint64_t nbt = (uint64_t)nb * (uint64_t)n_images + 1;      // + the invalid bins' bucket
    if (nbt > 1024ull * 1024ull || (uint64_t)n * (uint64_t)n_images > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)nbt * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    // chunks of at least 8192 bins per workgroup: the flush of an LDS histogram costs up to nb + 1 global atomics
    int chunks = (int)((n + 8191) / 8192);
    if (chunks < 1) chunks = 1;
    if ((uint64_t)chunks * (uint64_t)n_images > 65535ull) chunks = 65535 / n_images > 0 ? 65535 / n_images : 1;
    const size_t lds = nbi <= BUCKET_LCAP ? (size_t)nbi * sizeof(unsigned) : 16;
    hipLaunchKernelGGL(k_bucket_count_walks, dim3((unsigned)(chunks * n_images)), dim3(256), lds, s, bins, n, chunks, PH, PW, G, nb, cnt, err);
    const int nblk = (int)((nbt + 1023) / 1024);
    unsigned* totals = off + nbt + 1;                             // the offsets buffer holds nbt + 1 + nblk words
    hipLaunchKernelGGL(k_bucket_scan_a, dim3(nblk), dim3(1024), 1024 * sizeof(unsigned), s, cnt, off, totals, (int)nbt);
    hipLaunchKernelGGL(k_bucket_scan_b, dim3(1), dim3(1024), 1024 * sizeof(unsigned), s, totals, nblk, off, (int)nbt);
    hipLaunchKernelGGL(k_bucket_scan_c, dim3(nblk), dim3(1024), 0, s, off, totals, (int)nbt);
    hipLaunchKernelGGL(k_bucket_fill_walks, dim3((unsigned)(chunks * n_images)), dim3(256), lds, s, bins, n, chunks, PH, PW, G, nb, cnt, off, out);
    return hipGetLastError();
}
hipError_t launch_gather_bits_walks(const TileBin* ent, const uint8_t* bits, const uint8_t* hdr, const uint8_t* pay, uint64_t plen, uint64_t n,
                                    uint64_t limit, int n_images, uint8_t* out, hipStream_t s) {
    if (n == 0 || n_images <= 0) return hipSuccess;
    const uint64_t total = n * (uint64_t)n_images;
    hipLaunchKernelGGL(k_gather_bits_walks, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ent, bits, hdr, pay, plen, n, limit, total, out);
    return hipGetLastError();
}
hipError_t launch_gather_jitter_walks(const TileBin* ent, const float* jitter, uint64_t n, int n_images, float2* out, hipStream_t s) {
    if (n == 0 || n_images <= 0) return hipSuccess;
    const uint64_t total = n * (uint64_t)n_images;
    hipLaunchKernelGGL(k_gather_jitter_walks, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ent, jitter, n, total, out);
    return hipGetLastError();
}
hipError_t launch_fit_init(const TileBin* ent, const float2* fl, const uint8_t* pb, const float2* jp, const tfft_bin* bins, const float* med,
                           uint64_t n, int n_images, double alpha, double tau, double mu_floor, float2* d, float* mu, hipStream_t s) {
    if (n == 0 || n_images <= 0) return hipSuccess;
    const uint64_t total = n * (uint64_t)n_images;
    hipLaunchKernelGGL(k_fit_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ent, fl, pb, jp, bins, med, n, total, (float)alpha,
                       (float)cos(alpha), (float)sin(alpha), (float)tau, (float)mu_floor, d, mu);
    return hipGetLastError();
}
hipError_t launch_fit_count(const TileBin* ent, const float2* fl, const uint8_t* pb, const float2* jp, const float* mu, uint64_t n, int n_images,
                            unsigned nblk, unsigned* partial, unsigned* counts, uint32_t* wrong_out, hipStream_t s) {
    if (n == 0 || n_images <= 0 || nblk == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_count, dim3(nblk, (unsigned)n_images), dim3(256), 2 * sizeof(unsigned), s, ent, fl, pb, jp, mu, n, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fit_sum, dim3((unsigned)n_images), dim3(64), 0, s, partial, nblk, counts, wrong_out);
    return hipGetLastError();
}
hipError_t launch_fit_correct(const TileBin* ent, const float2* fl, const uint8_t* pb, const float2* jp, const float* mu, const unsigned* counts,
                              uint64_t n, int n_images, double gain, float2* d, hipStream_t s) {
    if (n == 0 || n_images <= 0) return hipSuccess;
    const uint64_t total = n * (uint64_t)n_images;
    hipLaunchKernelGGL(k_fit_correct, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ent, fl, pb, jp, mu, counts, n, total, (float)gain, d);
    return hipGetLastError();
}
hipError_t launch_gather_bits(const TileBin* ent, const unsigned* n_ent, const uint8_t* bits, const uint8_t* hdr, const uint8_t* pay, uint64_t plen,
                              uint64_t n, uint64_t limit, int n_images, uint8_t* out, hipStream_t s) {
    if (n == 0 || n_images == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_bits, dim3((unsigned)((n + 255) / 256), n_images), dim3(256), 0, s, ent, n_ent, bits, hdr, pay, plen, n, limit, out);
    return hipGetLastError();
}
hipError_t launch_gather_jitter(const TileBin* ent, const unsigned* n_ent, const float* jitter, uint64_t n, float2* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_jitter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ent, n_ent, jitter, n, out);
    return hipGetLastError();
}
hipError_t launch_bins_last_row(const tfft_bin* bins, uint64_t n, int PH, int PW, int* last_row, hipStream_t s) {
    hipError_t e = hipMemsetAsync(last_row, 0, sizeof(int), s);
    if (e != hipSuccess || n == 0) return e;
    unsigned nb = (unsigned)((n + 2047) / 2048);
    if (nb > 512) nb = 512;
    hipLaunchKernelGGL(k_bins_last_row, dim3(nb), dim3(256), 16, s, bins, n, PH, PW, last_row);
    return hipGetLastError();
}
hipError_t launch_embed(float2* spec, const tfft_bin* bins, const uint8_t* bits, const float* jitter,
                        const EmbedParams& P, int n_images, int* err, hipStream_t s) {
    if (P.n == 0 || n_images == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((P.n + 255) / 256);
    hipLaunchKernelGGL(k_embed, dim3(blocks, n_images), dim3(256), 0, s, spec, bins, bits, jitter, P, err);
    return hipGetLastError();
}
hipError_t launch_read(const float2* spec, const tfft_bin* bins, const float* jitter, const EmbedParams& P,
                       int n_images, uint8_t* bits_out, int* err, hipStream_t s) {
    if (P.n == 0 || n_images == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((P.n + 255) / 256);
    hipLaunchKernelGGL(k_read, dim3(blocks, n_images), dim3(256), 0, s, spec, bins, jitter, P, bits_out, err);
    return hipGetLastError();
}

hipError_t launch_export_full(const float2* spec, int PH, int PW, int PWout, float2* out, hipStream_t s) {
    const size_t n = (size_t)3 * PH * PWout;
    hipLaunchKernelGGL(k_export_full, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, spec, PH, PW, PWout, out);
    return hipGetLastError();
}
hipError_t launch_lowfreq_f64(const uint8_t* rgb, int W, int H, int PW, int PH, int center, int region, double2* rowsum, double* out,
                              hipStream_t s) {
    return launch_lowfreq_f64_batch(rgb, W, H, PW, PH, center, region, 1, rowsum, 0, out, s);
}
hipError_t launch_lowfreq_f64_batch(const uint8_t* rgb, int W, int H, int PW, int PH, int center, int region, int n_images, double2* rowsum,
                                    size_t rowsum_stride, double* out, hipStream_t s) {
    if (region < 1 || region > 8 || n_images < 1 || n_images > 65535) return hipErrorInvalidValue;
    const size_t img_bytes = (size_t)W * H * 3;
    hipLaunchKernelGGL(k_lowfreq_rows_f64, dim3(H, n_images), dim3(32, region), (size_t)region * 32 * 6 * sizeof(double), s, rgb, W, PW, center, region,
                       rowsum, img_bytes, rowsum_stride);
    hipLaunchKernelGGL(k_lowfreq_cols_f64, dim3(3 * region * region, n_images), dim3(256), 512 * sizeof(double), s, rowsum, H, PH, center, region, out,
                       rowsum_stride);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// stego analysis
// ---------------------------------------------------------------------------
// Annulus phase histograms: the bins count_plane (S:998-1008) counts -- the box and the exact integer radius test of k_capacity, its
// fp32 magnitude test -- binned by theta = atan2(Im F, Re F) of the FULL-plane coefficient (x > M: the conjugate of the stored mirror).
// Each wave counts into its own copy of the histogram in LDS while there is room for four (fewer LDS atomics on the same word); the
// block writes one partial histogram and k_phase_hist_sum adds the NB partials of a bin in block order (integers: no order effects).
//   grid (NB, 3, n_images)  block 256  LDS copies * nbins words   partial[((img*3 + plane)*NB + block)*nbins + bin]
__device__ __forceinline__ int phase_bin(float im, float re, double scale, int nbins) {
    const double t = ((double)atan2f(im, re) + 3.14159265358979323846) * scale;      // (theta + pi) * nbins / (2 pi)
    int b = (int)floor(t);
    if (b < 0) b = 0;                    // theta = -pi in fp32 lies a hair below -pi: bin 0, as theta = +pi (b = nbins) is
    return b & (nbins - 1);
}
template <bool WIDE>
__global__ void __launch_bounds__(256) k_phase_hist(const float2* __restrict__ spec, PhaseHistParams P, unsigned* __restrict__ partial) {
    unsigned* hist = reinterpret_cast<unsigned*>(tfft_smem);
    const int nbins = 1 << P.log_bins;
    const int copies = P.log_bins >= 12 ? 1 : (P.log_bins == 11 ? 2 : 4);
    for (int i = threadIdx.x; i < copies * nbins; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    unsigned* h = hist + (int)((threadIdx.x >> 6) % (unsigned)copies) * nbins;
    const int plane = blockIdx.y, img = blockIdx.z;
    const CapParams& cp = P.cap;
    const float t2 = P.t2[plane];
    const double scale = (double)nbins * 0.15915494309189533577;      // nbins / (2 pi)
    const int M = cp.PWi >> 1;
    const float2* pl = spec + (size_t)img * cp.img_stride + (size_t)plane * cp.PH * M;
    typedef typename std::conditional<WIDE, unsigned long long, unsigned>::type R;
    const R s_lo = (R)cp.s_lo, s_hi = (R)cp.s_hi;
    for (int y = blockIdx.x; y < cp.bh; y += gridDim.x) {
        if (y == 0 || 2 * y == cp.PH) continue;
        const R yy = (R)y * (R)y;
        const float2* row = pl + (size_t)y * M;                                  // bins x < M
        const float2* mrow = pl + (size_t)((cp.PH - y) & (cp.PH - 1)) * M;         // bins x > M: conj of (PH-y, PW-x)
        for (int x0 = threadIdx.x; x0 < cp.bw; x0 += 4 * blockDim.x) {
            float2 v[4]; bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int x = x0 + u * (int)blockDim.x;
                const R s = yy + (R)x * (R)x;
                in[u] = x < cp.bw && x != 0 && 2 * x != cp.PW && s >= s_lo && s <= s_hi;
                v[u] = in[u] ? (x < M ? row[x] : cconj(mrow[cp.PW - x])) : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (in[u] && !(mag2_of(v[u]) < t2)) atomicAdd(&h[phase_bin(v[u].y, v[u].x, scale, nbins)], 1u);
        }
    }
    __syncthreads();
    unsigned* out = partial + (((size_t)img * 3 + plane) * gridDim.x + blockIdx.x) * (size_t)nbins;
    for (int i = threadIdx.x; i < nbins; i += blockDim.x) {
        unsigned s = 0;
        for (int c = 0; c < copies; c++) s += hist[c * nbins + i];
        out[i] = s;
    }
}
//   grid (ceil(nbins/256), 3*n_images)  block 256: hist[z*nbins + i] = sum over blocks b of partial[(z*nb + b)*nbins + i]
__global__ void __launch_bounds__(256) k_phase_hist_sum(const unsigned* __restrict__ partial, int nb, int nbins, uint32_t* __restrict__ hist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (i >= nbins) return;
    const unsigned* p = partial + (size_t)z * nb * nbins + i;
    unsigned s = 0;
    for (int b = 0; b < nb; b++) s += p[(size_t)b * nbins];
    hist[(size_t)z * nbins + i] = s;
}

// Cover / stego quality: per tile of TFFT_QA_TX x TFFT_QA_TY window positions, both images' bytes of the tile and its 10-pixel halo in LDS (all three
// planes), then per plane the separable 11-tap Gaussian of the five moments of x = a - 128, y = b - 128 (x, y, x^2, y^2, xy): the
// horizontal pass writes them to LDS (a thread filters 8 adjacent columns of one row, every pixel's products formed once), the vertical
// pass keeps 8 outputs of one column in registers.  SSE over the tile's own pixels in integers; the SSIM of the tile's windows added in
// fp64.  Partials per (image, plane, tile); k_quality_sum adds them in a fixed order.
//   grid (ceil(W/TFFT_QA_TX), ceil(H/TFFT_QA_TY), n_images)  block 256
template <bool SSIM>
__global__ void __launch_bounds__(256) k_quality(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, QualityParams P,
                                                 unsigned long long* __restrict__ sse_part, double* __restrict__ ssim_part) {
    constexpr int RX = TFFT_QA_TX + 10, RY = TFFT_QA_TY + 10, PLN = RY * RX;
    uint8_t* la = reinterpret_cast<uint8_t*>(tfft_smem);                      // [3][RY][RX]
    uint8_t* lb = la + 3 * PLN;                                               // [3][RY][RX]
    float* hs = reinterpret_cast<float*>(tfft_smem + TFFT_QA_LDS_OFF);       // [5][RY][TFFT_QA_TX]
    // block sums: after the filters over the moments (SSIM), at the start of the LDS otherwise (SSE only: no tile is kept)
    constexpr size_t RED_OFF = SSIM ? TFFT_QA_LDS_OFF : 0;
    unsigned long long* red = reinterpret_cast<unsigned long long*>(tfft_smem + RED_OFF);                          // [3][256]
    double* redd = reinterpret_cast<double*>(tfft_smem + RED_OFF + 3 * 256 * sizeof(unsigned long long));     // [3][256], SSIM only
    const int tid = threadIdx.x, img = blockIdx.z;
    const int x0 = blockIdx.x * TFFT_QA_TX, y0 = blockIdx.y * TFFT_QA_TY;
    const size_t img_bytes = (size_t)P.W * P.H * 3;
    const uint8_t* ia = a + (size_t)img * img_bytes;
    const uint8_t* ib = b + (size_t)img * img_bytes;
    // load the tile + halo (zeros outside the image) into LDS; SSE of the tile's own pixels.  SSE only: just the own pixels, no LDS
    unsigned long long sse[3] = {0, 0, 0};
    const int rx = (P.W - x0 < RX ? P.W - x0 : RX), ry = (P.H - y0 < RY ? P.H - y0 : RY);
    const int own_x = (P.W - x0 < TFFT_QA_TX ? P.W - x0 : TFFT_QA_TX), own_y = (P.H - y0 < TFFT_QA_TY ? P.H - y0 : TFFT_QA_TY);
    constexpr int LX = SSIM ? RX : TFFT_QA_TX, LY = SSIM ? RY : TFFT_QA_TY;
    for (int e = tid; e < LY * 3 * LX; e += blockDim.x) {
        const int r = e / (3 * LX), k = e - r * 3 * LX, c = k / 3, p = k - 3 * c;
        uint8_t va = 0, vb = 0;
        if (r < (SSIM ? ry : own_y) && c < (SSIM ? rx : own_x)) {
            const size_t o = ((size_t)(y0 + r) * P.W + (x0 + c)) * 3 + p;
            va = ia[o]; vb = ib[o];
            if (r < own_y && c < own_x) { const int d = (int)va - (int)vb; sse[p] += (unsigned)(d * d); }
        }
        if (SSIM) { la[p * PLN + r * RX + c] = va; lb[p * PLN + r * RX + c] = vb; }
    }
    double ssum[3] = {0.0, 0.0, 0.0};
    if (SSIM) {
        __syncthreads();
        const int nwx = P.W - 10 - x0, nwy = P.H - 10 - y0;                     // window positions of this tile: x < nwx, y < nwy
        for (int p = 0; p < 3; p++) {
            // horizontal: item (row r, columns 8*cg .. 8*cg+7)
            for (int it = tid; it < RY * (TFFT_QA_TX / 8); it += blockDim.x) {
                const int r = it / (TFFT_QA_TX / 8), c0 = (it - r * (TFFT_QA_TX / 8)) * 8;
                float acc[8][5];
#pragma unroll
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int m = 0; m < 5; m++) acc[j][m] = 0.f;
                const uint8_t* pa = la + p * PLN + r * RX + c0;
                const uint8_t* pb = lb + p * PLN + r * RX + c0;
#pragma unroll
                for (int i = 0; i < 18; i++) {
                    const float x = (float)((int)pa[i] - 128), y = (float)((int)pb[i] - 128);
                    const float v[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (i - j < 0 || i - j > 10) continue;
#pragma unroll
                        for (int m = 0; m < 5; m++) acc[j][m] = fmaf(P.g[i - j], v[m], acc[j][m]);
                    }
                }
#pragma unroll
                for (int m = 0; m < 5; m++)
#pragma unroll
                    for (int j = 0; j < 8; j++) hs[(m * RY + r) * TFFT_QA_TX + c0 + j] = acc[j][m];
            }
            __syncthreads();
            // vertical: item (column c, output rows 8*rg .. 8*rg+7)
            for (int it = tid; it < TFFT_QA_TX * (TFFT_QA_TY / 8); it += blockDim.x) {
                const int c = it % TFFT_QA_TX, r0 = (it / TFFT_QA_TX) * 8;
                float acc[8][5];
#pragma unroll
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int m = 0; m < 5; m++) acc[j][m] = 0.f;
#pragma unroll
                for (int i = 0; i < 18; i++) {
                    float v[5];
#pragma unroll
                    for (int m = 0; m < 5; m++) v[m] = hs[(m * RY + r0 + i) * TFFT_QA_TX + c];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (i - j < 0 || i - j > 10) continue;
#pragma unroll
                        for (int m = 0; m < 5; m++) acc[j][m] = fmaf(P.g[i - j], v[m], acc[j][m]);
                    }
                }
                if (c < nwx) {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        if (r0 + j >= nwy) continue;
                        const float mx = acc[j][0] + 128.f, my = acc[j][1] + 128.f;      // the means of the pixels themselves
                        const float sx = acc[j][2] - acc[j][0] * acc[j][0], sy = acc[j][3] - acc[j][1] * acc[j][1];
                        const float sxy = acc[j][4] - acc[j][0] * acc[j][1];
                        const float num = (2.f * mx * my + TFFT_QA_C1) * (2.f * sxy + TFFT_QA_C2);
                        const float den = (mx * mx + my * my + TFFT_QA_C1) * (sx + sy + TFFT_QA_C2);
                        ssum[p] += (double)(num / den);
                    }
                }
            }
            __syncthreads();
        }
    } else {
        __syncthreads();
    }
    // block sums in a fixed order
    for (int p = 0; p < 3; p++) { red[p * 256 + tid] = sse[p]; if (SSIM) redd[p * 256 + tid] = ssum[p]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int p = 0; p < 3; p++) { red[p * 256 + tid] += red[p * 256 + tid + s]; if (SSIM) redd[p * 256 + tid] += redd[p * 256 + tid + s]; }
        __syncthreads();
    }
    if (tid < 3) {
        const size_t ntiles = (size_t)gridDim.x * gridDim.y, t = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        sse_part[((size_t)img * 3 + tid) * ntiles + t] = red[tid * 256];
        if (SSIM) ssim_part[((size_t)img * 3 + tid) * ntiles + t] = redd[tid * 256];
    }
}
//   grid (3*n_images)  block 256: the tiles' partials of (image, plane) z added in a fixed order; SSIM = sum / windows, 1 where SSE = 0
__global__ void __launch_bounds__(256) k_quality_sum(const unsigned long long* __restrict__ sse_part, const double* __restrict__ ssim_part,
                                                     int ntiles, double n_windows, unsigned long long* __restrict__ sse_out, double* __restrict__ ssim_out) {
    unsigned long long* red = reinterpret_cast<unsigned long long*>(tfft_smem);
    double* redd = reinterpret_cast<double*>(tfft_smem + 256 * sizeof(unsigned long long));
    const int tid = threadIdx.x, z = blockIdx.x;
    unsigned long long s = 0; double d = 0.0;
    for (int t = tid; t < ntiles; t += blockDim.x) { s += sse_part[(size_t)z * ntiles + t]; if (ssim_out) d += ssim_part[(size_t)z * ntiles + t]; }
    red[tid] = s; redd[tid] = d;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) { red[tid] += red[tid + k]; redd[tid] += redd[tid + k]; }
        __syncthreads();
    }
    if (tid == 0) {
        sse_out[z] = red[0];
        if (ssim_out) ssim_out[z] = red[0] == 0 ? 1.0 : redd[0] / n_windows;
    }
}

int phase_hist_blocks(const CapParams& cp, int log_bins, int n_images) {
    // rows of the box per block: about a dozen as k_capacity, more when the flush of the partial histogram would cost more than an
    // eighth of the block's reads; at least ~1024 blocks per launch, and at most TFFT_PH_PARTIAL_WORDS partial words per plane
    const int nbins = 1 << log_bins, bh = cp.bh > 0 ? cp.bh : 1, bw = cp.bw > 0 ? cp.bw : 1;
    int rows = (4 * nbins + bw - 1) / bw;
    if (rows < 12) rows = 12;
    int nb = (bh + rows - 1) / rows;
    const int fill = (1024 + 3 * n_images - 1) / (3 * n_images);
    if (nb < fill) nb = fill;
    if (nb > bh) nb = bh;
    if (nb > TFFT_STAT_MAX_BLOCKS) nb = TFFT_STAT_MAX_BLOCKS;
    if (nb > TFFT_PH_PARTIAL_WORDS / nbins) nb = TFFT_PH_PARTIAL_WORDS / nbins;
    return nb < 1 ? 1 : nb;
}

hipError_t launch_phase_hist(const float2* spec, const PhaseHistParams& P, int n_images, unsigned* partial, uint32_t* hist_out, hipStream_t s) {
    if (P.log_bins < 3 || P.log_bins > 12 || n_images < 1 || n_images > 65535) return hipErrorInvalidValue;
    const int nbins = 1 << P.log_bins, nb = phase_hist_blocks(P.cap, P.log_bins, n_images);
    const int copies = P.log_bins >= 12 ? 1 : (P.log_bins == 11 ? 2 : 4);
    const size_t lds = (size_t)copies * nbins * sizeof(unsigned);
    const CapParams& cp = P.cap;
    const bool wide = cp.PH > 32768 || cp.PW > 32768 || cp.s_hi > 0xFFFFFFFFull || cp.s_lo > 0xFFFFFFFFull;
    if (wide) hipLaunchKernelGGL(k_phase_hist<true>, dim3(nb, 3, n_images), dim3(256), lds, s, spec, P, partial);
    else hipLaunchKernelGGL(k_phase_hist<false>, dim3(nb, 3, n_images), dim3(256), lds, s, spec, P, partial);
    hipLaunchKernelGGL(k_phase_hist_sum, dim3((nbins + 255) / 256, 3 * n_images), dim3(256), 0, s, partial, nb, nbins, hist_out);
    return hipGetLastError();
}

size_t quality_partials(int W, int H) {
    return (size_t)((W + TFFT_QA_TX - 1) / TFFT_QA_TX) * (size_t)((H + TFFT_QA_TY - 1) / TFFT_QA_TY);
}

hipError_t launch_quality(const uint8_t* a, const uint8_t* b, const QualityParams& P, int n_images, unsigned long long* sse_part, double* ssim_part,
                          unsigned long long* sse_out, double* ssim_out, hipStream_t s) {
    if (P.W < 1 || P.H < 1 || n_images < 1 || n_images > 65535 || (ssim_out && (P.W < 11 || P.H < 11))) return hipErrorInvalidValue;
    const unsigned tx = (unsigned)((P.W + TFFT_QA_TX - 1) / TFFT_QA_TX), ty = (unsigned)((P.H + TFFT_QA_TY - 1) / TFFT_QA_TY);
    if (ty > 65535) return hipErrorInvalidValue;
    const size_t lds = TFFT_QA_LDS;
    if (ssim_out) {
        hipError_t e = hipFuncSetAttribute((const void*)k_quality<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_quality<true>, dim3(tx, ty, n_images), dim3(256), lds, s, a, b, P, sse_part, ssim_part);
    } else {
        hipLaunchKernelGGL(k_quality<false>, dim3(tx, ty, n_images), dim3(256), 3 * 256 * sizeof(unsigned long long), s, a, b, P,
                           sse_part, ssim_part);
    }
    const double n_windows = ssim_out ? (double)(P.W - 10) * (double)(P.H - 10) : 1.0;
    hipLaunchKernelGGL(k_quality_sum, dim3(3 * n_images), dim3(256), 256 * (sizeof(unsigned long long) + sizeof(double)), s, sse_part, ssim_part,
                       (int)(tx * ty), n_windows, sse_out, ssim_out);
    return hipGetLastError();
}

// ===========================================================================
// robustness analysis: channels and error counts
// ===========================================================================
// splitmix64 (Steele, Lea, Flood 2014; the public-domain reference of S. Vigna, prng.di.unimi.it/splitmix64.c)
#define TFFT_GOLDEN64 0x9E3779B97F4A7C15ull
__device__ __forceinline__ uint64_t splitmix64(uint64_t k) {
    uint64_t z = k + TFFT_GOLDEN64;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// One noisy byte: Box-Muller on the two 24-bit uniforms of the counter's hash, u = (a + 0.5) / 2^24.  Both are formed exactly in fp32: a + 0.5
// has 25 bits from a = 2^23 on, so the upper half of u1 goes through its complement (-log1p(-(1 - u1)), 1 - u1 exact) -- that is where
// sqrt(-2 ln u1) is small and a rounded u1 would show (2.4e-4 at u1 = 1 - 2^-25) -- and u2 only sets an angle (its rounding: 4e-7 rad)
__device__ __forceinline__ unsigned awgn_byte(unsigned pix, uint64_t k, float sigma) {
    const uint64_t z = splitmix64(k);
    const unsigned a = (unsigned)(z >> 40), b = (unsigned)(z >> 16) & 0xFFFFFFu;
    const float e = a < (1u << 23) ? -logf(((float)a + 0.5f) * (1.0f / 16777216.0f))
                                   : -log1pf(-(((float)(16777216u - a) - 0.5f) * (1.0f / 16777216.0f)));
    const float g = sqrtf(2.0f * e) * cosf(6.283185307179586f * (((float)b + 0.5f) * (1.0f / 16777216.0f)));
    const float v = rintf((float)pix + sigma * g);
    return (unsigned)fminf(fmaxf(v, 0.0f), 255.0f);
}
//   grid (ceil((n_bytes/4 + 1)/256))  block 256: a thread owns four bytes -- one aligned dword where input and output share their
//   alignment (the bytes before the first and after the last aligned dword go to the first threads), four single bytes otherwise
__global__ void __launch_bounds__(256) k_channel_awgn(const uint8_t* in, uint8_t* out, size_t n_bytes, uint64_t k0, float sigma) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto one = [&](size_t j) { out[j] = (uint8_t)awgn_byte(in[j], k0 + TFFT_GOLDEN64 * (uint64_t)j, sigma); };
    if ((((uintptr_t)in ^ (uintptr_t)out) & 3) != 0) {
        for (size_t j = 4 * gid; j < n_bytes && j < 4 * gid + 4; j++) one(j);
        return;
    }
    size_t head = (size_t)((4 - ((uintptr_t)in & 3)) & 3);
    if (head > n_bytes) head = n_bytes;
    const size_t nw = (n_bytes - head) / 4, tail = n_bytes - head - 4 * nw;
    if (gid < head) one(gid);
    if (gid < tail) one(head + 4 * nw + gid);
    if (gid >= nw) return;
    const size_t j = head + 4 * gid;
    const uint32_t v = *reinterpret_cast<const uint32_t*>(in + j);
    uint32_t r = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) r |= awgn_byte((v >> (8 * t)) & 0xFFu, k0 + TFFT_GOLDEN64 * (uint64_t)(j + t), sigma) << (8 * t);
    *reinterpret_cast<uint32_t*>(out + j) = r;
}

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural (row-major) order
__device__ const uint8_t k_jpeg_base[128] = {
    16, 11, 10, 16, 24, 40, 51, 61,      12, 12, 14, 19, 26, 58, 60, 55,      14, 13, 16, 24, 40, 57, 69, 56,      14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,    24, 35, 55, 64, 81, 104, 113, 92,    49, 64, 78, 87, 103, 121, 120, 101,  72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99, 99, 99, 99,      18, 21, 26, 66, 99, 99, 99, 99,      24, 26, 56, 99, 99, 99, 99, 99,      47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,      99, 99, 99, 99, 99, 99, 99, 99,      99, 99, 99, 99, 99, 99, 99, 99,      99, 99, 99, 99, 99, 99, 99, 99};

// orthonormal 8-point DCT-II and its inverse, in place, by the even / odd split: s = x[n] + x[7-n] feeds the even outputs, d = x[n] - x[7-n]
// the odd ones (22 multiplies each way).  cK = cos(K pi/16) / 2; X[0] carries sqrt(1/8) = c4 / 2 * ... = JC4 per sample
#define TFFT_JC1 0.49039264020161522f
#define TFFT_JC2 0.46193976625564337f
#define TFFT_JC3 0.41573480615127262f
#define TFFT_JC4 0.35355339059327376f
#define TFFT_JC5 0.27778511650980111f
#define TFFT_JC6 0.19134171618254489f
#define TFFT_JC7 0.09754516100806413f
__device__ __forceinline__ void dct8(float (&x)[8]) {
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float p = s0 + s3, q = s1 + s2, m = s0 - s3, n = s1 - s2;
    x[0] = TFFT_JC4 * (p + q);
    x[4] = TFFT_JC4 * (p - q);
    x[2] = TFFT_JC2 * m + TFFT_JC6 * n;
    x[6] = TFFT_JC6 * m - TFFT_JC2 * n;
    x[1] = TFFT_JC1 * d0 + TFFT_JC3 * d1 + TFFT_JC5 * d2 + TFFT_JC7 * d3;
    x[3] = TFFT_JC3 * d0 - TFFT_JC7 * d1 - TFFT_JC1 * d2 - TFFT_JC5 * d3;
    x[5] = TFFT_JC5 * d0 - TFFT_JC1 * d1 + TFFT_JC7 * d2 + TFFT_JC3 * d3;
    x[7] = TFFT_JC7 * d0 - TFFT_JC5 * d1 + TFFT_JC3 * d2 - TFFT_JC1 * d3;
}
__device__ __forceinline__ void idct8(float (&x)[8]) {
    const float a = TFFT_JC4 * (x[0] + x[4]), b = TFFT_JC4 * (x[0] - x[4]);
    const float c = TFFT_JC2 * x[2] + TFFT_JC6 * x[6], d = TFFT_JC6 * x[2] - TFFT_JC2 * x[6];
    const float e0 = a + c, e1 = b + d, e2 = b - d, e3 = a - c;
    const float o0 = TFFT_JC1 * x[1] + TFFT_JC3 * x[3] + TFFT_JC5 * x[5] + TFFT_JC7 * x[7];
    const float o1 = TFFT_JC3 * x[1] - TFFT_JC7 * x[3] - TFFT_JC1 * x[5] - TFFT_JC5 * x[7];
    const float o2 = TFFT_JC5 * x[1] - TFFT_JC1 * x[3] + TFFT_JC7 * x[5] + TFFT_JC3 * x[7];
    const float o3 = TFFT_JC7 * x[1] - TFFT_JC5 * x[3] + TFFT_JC3 * x[5] - TFFT_JC1 * x[7];
    x[0] = e0 + o0; x[7] = e0 - o0;
    x[1] = e1 + o1; x[6] = e1 - o1;
    x[2] = e2 + o2; x[5] = e2 - o2;
    x[3] = e3 + o3; x[4] = e3 - o3;
}

// JPEG quantisation.  A workgroup owns a strip of 8 image rows x TFFT_JQ_COLS pixel columns = 32 blocks; thread (block b = tid / 8, line
// r = tid % 8) holds line r of block b for all three components in registers: first a pixel row (colour transform, row DCT), after a
// transpose through LDS a coefficient column (column DCT, quantise, dequantise, inverse column DCT), after the transpose back the pixel row
// again (inverse row DCT, colour transform, rounding).
// The bytes travel as aligned dwords: the strip's rows are staged in LDS dword for dword as they lie in memory (rows are 3*W bytes
// apart, so every row has its own byte shift; the dwords that straddle the strip's ends are read byte by byte -- nothing outside the
// strip's own bytes is touched, which is also what makes in == out safe), a thread cuts its 24 bytes out of seven of them with
// v_alignbyte_b32, and the results go back the same way through a second strip.  Rows past H and columns past W are the last row /
// column again (loaded twice; replicated in LDS) and are not stored.
//   grid (ceil(W/TFFT_JQ_COLS), ceil(H/8), n_images)  block 256   LDS TFFT_JQ_LDS
__global__ void __launch_bounds__(256) k_channel_jpeg(const uint8_t* in, uint8_t* out, int W, int H, int quality) {
    uint32_t* sin = reinterpret_cast<uint32_t*>(tfft_smem);                   // [8][TFFT_JQ_IN_PITCH]
    uint32_t* sout = sin + 8 * TFFT_JQ_IN_PITCH;                              // [8][TFFT_JQ_OUT_PITCH], the strip's dword d at [1 + d]
    float* tr = reinterpret_cast<float*>(sout + 8 * TFFT_JQ_OUT_PITCH);       // [32][3][8][9]
    float* ql = tr + TFFT_JQ_TR;                                              // [2][64]
    uint8_t* sinb = reinterpret_cast<uint8_t*>(sin);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TFFT_JQ_COLS, y0 = blockIdx.y * 8;
    const int ncols = W - x0 < TFFT_JQ_COLS ? W - x0 : TFFT_JQ_COLS, nb = 3 * ncols;
    const size_t img_off = (size_t)blockIdx.z * (size_t)W * (size_t)H * 3;
    // the quantiser of this quality (IJG scaling), as floats
    if (tid < 128) {
        const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        int q = ((int)k_jpeg_base[tid] * s + 50) / 100;
        q = q < 1 ? 1 : (q > 255 ? 255 : q);
        ql[tid] = (float)q;
    }
    // ---- stage the 8 rows
    constexpr int ND = (3 + 3 * TFFT_JQ_COLS + 3) / 4;      // dwords a row of the strip can touch
    for (int e = tid; e < 8 * ND; e += 256) {
        const int r = e / ND, d = e - r * ND;
        const int y = y0 + r < H ? y0 + r : H - 1;
        const uint8_t* row = in + img_off + ((size_t)y * W + x0) * 3;
        const int sh = (int)((uintptr_t)row & 3), lo = 4 * d - sh;      // the dword holds bytes lo .. lo+3 of the row
        if (lo >= 0 && lo + 4 <= nb) sin[r * TFFT_JQ_IN_PITCH + d] = *reinterpret_cast<const uint32_t*>(row + lo);
        else
            for (int t = 0; t < 4; t++)
                if (lo + t >= 0 && lo + t < nb) sinb[4 * (r * TFFT_JQ_IN_PITCH + d) + t] = row[lo + t];
    }
    __syncthreads();
    const int full = (ncols + 7) & ~7;
    if (full != ncols) {      // the last column again, up to the end of its block
        for (int e = tid; e < 8 * 21; e += 256) {
            const int r = e / 21, j = e - r * 21, px = ncols + j / 3, ch = j % 3;
            const int y = y0 + r < H ? y0 + r : H - 1;
            const int sh = (int)((uintptr_t)(in + img_off + ((size_t)y * W + x0) * 3) & 3);
            if (px < full) sinb[4 * r * TFFT_JQ_IN_PITCH + sh + 3 * px + ch] = sinb[4 * r * TFFT_JQ_IN_PITCH + sh + 3 * (ncols - 1) + ch];
        }
        __syncthreads();
    }
    const int b = tid >> 3, r = tid & 7;
    const bool active = 8 * b < ncols;
    float* tb = tr + b * (3 * 8 * 9);
    float Y[8], Cb[8], Cr[8];
    if (active) {
        const int y = y0 + r < H ? y0 + r : H - 1;
        const int sh = (int)((uintptr_t)(in + img_off + ((size_t)y * W + x0) * 3) & 3);
        const int o = sh + 24 * b;
        const uint32_t* w = sin + r * TFFT_JQ_IN_PITCH + (o >> 2);
        uint32_t v[6];
#pragma unroll
        for (int i = 0; i < 6; i++) v[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], (uint32_t)(o & 3));
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float R = (float)((v[(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 0xFFu);
            const float G = (float)((v[(3 * j + 1) >> 2] >> (8 * ((3 * j + 1) & 3))) & 0xFFu);
            const float B = (float)((v[(3 * j + 2) >> 2] >> (8 * ((3 * j + 2) & 3))) & 0xFFu);
            // JFIF full-range BT.601
            Y[j] = 0.299f * R + 0.587f * G + 0.114f * B - 128.0f;
            Cb[j] = -0.168736f * R - 0.331264f * G + 0.5f * B;
            Cr[j] = 0.5f * R - 0.418688f * G - 0.081312f * B;
        }
        dct8(Y); dct8(Cb); dct8(Cr);
#pragma unroll
        for (int u = 0; u < 8; u++) { tb[(0 * 8 + r) * 9 + u] = Y[u]; tb[(1 * 8 + r) * 9 + u] = Cb[u]; tb[(2 * 8 + r) * 9 + u] = Cr[u]; }
    }
    __syncthreads();
    if (active) {      // column r of the block: coefficients (v, u = r), quantiser ql[8*v + r]
#pragma unroll
        for (int k = 0; k < 8; k++) { Y[k] = tb[(0 * 8 + k) * 9 + r]; Cb[k] = tb[(1 * 8 + k) * 9 + r]; Cr[k] = tb[(2 * 8 + k) * 9 + r]; }
        dct8(Y); dct8(Cb); dct8(Cr);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float qy = ql[8 * k + r], qc = ql[64 + 8 * k + r];
            Y[k] = rintf(Y[k] / qy) * qy; Cb[k] = rintf(Cb[k] / qc) * qc; Cr[k] = rintf(Cr[k] / qc) * qc;
        }
        idct8(Y); idct8(Cb); idct8(Cr);
    }
    __syncthreads();      // every column has been read: the buffer takes the half-inverted block
    if (active) {
#pragma unroll
        for (int k = 0; k < 8; k++) { tb[(0 * 8 + k) * 9 + r] = Y[k]; tb[(1 * 8 + k) * 9 + r] = Cb[k]; tb[(2 * 8 + k) * 9 + r] = Cr[k]; }
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int u = 0; u < 8; u++) { Y[u] = tb[(0 * 8 + r) * 9 + u]; Cb[u] = tb[(1 * 8 + r) * 9 + u]; Cr[u] = tb[(2 * 8 + r) * 9 + u]; }
        idct8(Y); idct8(Cb); idct8(Cr);
        uint32_t v[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float yy = Y[j] + 128.0f;
            const float R = yy + 1.402f * Cr[j];
            const float G = yy - 0.344136f * Cb[j] - 0.714136f * Cr[j];
            const float B = yy + 1.772f * Cb[j];
            v[(3 * j) >> 2] |= (uint32_t)fminf(fmaxf(rintf(R), 0.0f), 255.0f) << (8 * ((3 * j) & 3));
            v[(3 * j + 1) >> 2] |= (uint32_t)fminf(fmaxf(rintf(G), 0.0f), 255.0f) << (8 * ((3 * j + 1) & 3));
            v[(3 * j + 2) >> 2] |= (uint32_t)fminf(fmaxf(rintf(B), 0.0f), 255.0f) << (8 * ((3 * j + 2) & 3));
        }
#pragma unroll
        for (int i = 0; i < 6; i++) sout[r * TFFT_JQ_OUT_PITCH + 1 + 6 * b + i] = v[i];
    }
    __syncthreads();
    // ---- store the rows < H: aligned dword d of a row holds the strip's bytes 4d - sh .. 4d - sh + 3
    for (int e = tid; e < 8 * ND; e += 256) {
        const int rr = e / ND, d = e - rr * ND;
        if (y0 + rr >= H) break;
        uint8_t* row = out + img_off + ((size_t)(y0 + rr) * W + x0) * 3;
        const int sh = (int)((uintptr_t)row & 3), lo = 4 * d - sh;
        if (lo >= nb) continue;
        const uint32_t hi = sout[rr * TFFT_JQ_OUT_PITCH + 1 + d], low = sout[rr * TFFT_JQ_OUT_PITCH + d];
        const uint32_t val = sh ? __builtin_amdgcn_alignbyte(hi, low, (uint32_t)(4 - sh)) : hi;
        if (lo >= 0 && lo + 4 <= nb) *reinterpret_cast<uint32_t*>(row + lo) = val;
        else
            for (int t = 0; t < 4; t++)
                if (lo + t >= 0 && lo + t < nb) row[lo + t] = (uint8_t)(val >> (8 * t));
    }
}

// The error counts of one attacked batch.  A thread takes one byte of the frame (38 header bytes, then plen payload bytes): the 24 or
// 56 raw bits that carry its 8 bits three or seven times over (Rep-3 / Rep-7, MSB first: frame_bit's layout) are compared with those bits,
// their majorities with the byte.  Counts are integers: block sums in LDS, then one atomic add per counter and block.
//   grid (ceil((38 + plen)/256) capped at 64, n_images)  block 256
__global__ void __launch_bounds__(256) k_robust_count(const uint8_t* __restrict__ raw, uint64_t n_bins, const uint8_t* __restrict__ header,
                                                      const uint8_t* __restrict__ payload, uint64_t plen, const int* __restrict__ status,
                                                      uint32_t* __restrict__ result) {
    unsigned* red = reinterpret_cast<unsigned*>(tfft_smem);      // [3][256]
    const int tid = threadIdx.x;
    const uint64_t img = blockIdx.y;
    const uint8_t* in = raw + img * n_bins;
    unsigned n_raw = 0, n_hdr = 0, n_pay = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + tid; j < 38 + plen; j += (uint64_t)gridDim.x * 256) {
        const bool hd = j < 38;
        const int rep = hd ? 3 : 7;
        const uint8_t* p = hd ? in + j * 24 : in + 912 + (j - 38) * 56;
        const unsigned want = hd ? header[img * 38 + j] : payload[img * plen + (j - 38)];
        unsigned v = 0;
        for (int q = 0; q < 8; q++, p += rep) {
            unsigned ones = 0;
            for (int t = 0; t < rep; t++) ones += p[t] ? 1u : 0u;
            n_raw += ((want >> (7 - q)) & 1u) ? rep - ones : ones;
            v = (v << 1) | (2 * ones > (unsigned)rep ? 1u : 0u);
        }
        if (v != want) { if (hd) n_hdr++; else n_pay++; }
    }
    red[tid] = n_raw; red[256 + tid] = n_hdr; red[512 + tid] = n_pay;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[tid] += red[tid + s]; red[256 + tid] += red[256 + tid + s]; red[512 + tid] += red[512 + tid + s]; }
        __syncthreads();
    }
    if (tid < 3 && red[256 * tid]) atomicAdd(result + 4 * img + tid, red[256 * tid]);
    if (tid == 3 && blockIdx.x == 0) result[4 * img + 3] = (uint32_t)status[img];
}

hipError_t launch_channel_awgn(const uint8_t* in, uint8_t* out, size_t n_bytes, uint64_t seed, uint64_t index0, float sigma, hipStream_t s) {
    if (n_bytes == 0) return hipSuccess;
    const size_t blocks = (n_bytes / 4 + 1 + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_channel_awgn, dim3((unsigned)blocks), dim3(256), 0, s, in, out, n_bytes, seed + TFFT_GOLDEN64 * index0, sigma);
    return hipGetLastError();
}

hipError_t launch_channel_jpeg(const uint8_t* in, uint8_t* out, int W, int H, int n_images, int quality, hipStream_t s) {
    if (W < 1 || H < 1 || n_images < 1 || n_images > 65535 || quality < 1 || quality > 100) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((W + TFFT_JQ_COLS - 1) / TFFT_JQ_COLS), gy = (unsigned)((H + 7) / 8);
    if (gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_channel_jpeg, dim3(gx, gy, n_images), dim3(256), TFFT_JQ_LDS, s, in, out, W, H, quality);
    return hipGetLastError();
}

hipError_t launch_robust_count(const uint8_t* raw, uint64_t n_bins, const uint8_t* header, const uint8_t* payload, uint64_t plen,
                               const int* status, int n_images, uint32_t* result, hipStream_t s) {
    if (n_images < 1 || n_images > 65535 || n_bins < 912 + 56 * plen) return hipErrorInvalidValue;
    uint64_t nb = (38 + plen + 255) / 256;
    if (nb > 64) nb = 64;
    hipLaunchKernelGGL(k_robust_count, dim3((unsigned)nb, n_images), dim3(256), 3 * 256 * sizeof(unsigned), s, raw, n_bins, header, payload, plen,
                       status, result);
    return hipGetLastError();
}

// ===========================================================================
// SPAM steganalysis features: second-order co-occurrences of clamped pixel differences
// ===========================================================================
// For every pixel p of a plane and each of the directions d = (dy, dx) = (0,1), (1,0), (1,1), (1,-1) with p + 3d inside the image:
//   e_k = clamp(I[p + (k-1)d] - I[p + kd], -T, T), k = 1..3;   counts[image][plane][dir][((e1+T) n + (e2+T)) n + (e3+T)] += 1,  n = 2T + 1.
// A workgroup owns TFFT_SP_COLS pixel columns of a band of rows, all three planes, and walks the band TFFT_SP_ROWS rows at a time: the rows and
// their halo (3 rows below, 3 pixels left and right) are staged in LDS dword for dword as they lie in memory (rows are 3*W bytes apart, so
// every row has its own byte shift; a dword that straddles the end of what the tile needs is read byte by byte -- nothing outside the tile's own
// bytes, all of them inside the image, is touched).  A thread then takes bytes tid, tid + 256, tid + 512 of each row of the tile (the planes
// (tid + k) mod 3): 13 LDS bytes and four triples per byte.
// Histograms: [3][4][n^3] words in LDS, two copies: measured on 32 x 1080p, four copies (two workgroups per CU) cost 0.83 ms, two (three
// workgroups) 0.65, one (five) 0.69 -- the kernel waits on LDS latency more than on contention.  What contention costs
// is equal indices inside ONE ds_add_u32 -- the LDS takes a wave's atomic apart by address -- so the copy is chosen by lane (tid mod
// copies; the copies lie 12 n^3 words apart, in different banks), not by wave: lanes that meet on an index are spread over the copies
// (5 % faster than per-wave copies at four copies).  The index every flat or smooth region hits,
// (0, 0, 0), is not sent to LDS at all: a thread counts it in registers (a compare and an add per value, no scalar instruction, no atomic)
// and adds its twelve counters once at the end, so a flat image costs no contended atomic.  A block adds its non-zero counters to the
// zeroed result with one integer atomic each (integers: no order effects, repeated calls return identical bytes).
#ifndef TFFT_SP_COPY_BY_LANE
#define TFFT_SP_COPY_BY_LANE 1           // 0: one copy per wave (A/B builds only, `make variant`)
#endif
#ifndef TFFT_SP_COPIES
#define TFFT_SP_COPIES 2                 // histogram copies of a workgroup (a power of two; A/B builds: 1, 4 -- T = 4 takes at most two)
#endif
//   grid (ceil(W/TFFT_SP_COLS), bands, n_images)  block 256   LDS tile + copies * 12 n^3 words
template <int T>
__device__ __forceinline__ int spam_index(int p0, int p1, int p2, int p3) {
    constexpr int N = 2 * T + 1;
    auto cl = [](int v) { return (v < -T ? -T : (v > T ? T : v)) + T; };
    return (cl(p0 - p1) * N + cl(p1 - p2)) * N + cl(p2 - p3);
}
template <int T>
__global__ void __launch_bounds__(256) k_spam(const uint8_t* __restrict__ rgb, int W, int H, int band_rows, int copies, uint32_t* __restrict__ counts) {
    constexpr int N = 2 * T + 1, N3 = N * N * N, HL = 12 * N3, CENTRE = (T * N + T) * N + T;
    constexpr int ND = TFFT_SP_PITCH;                                         // dwords a row of the tile can touch: 3 + 3*(COLS + 6) bytes
    uint32_t* tile = reinterpret_cast<uint32_t*>(tfft_smem);                  // [TFFT_SP_STAGE_ROWS][TFFT_SP_PITCH]; byte 9 + shift of a row = pixel x0
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
    unsigned* hist = reinterpret_cast<unsigned*>(tile + TFFT_SP_STAGE_ROWS * TFFT_SP_PITCH);      // [copies][3][4][N3]
    const int tid = threadIdx.x;
    for (int i = tid; i < copies * HL; i += 256) hist[i] = 0;
    unsigned* h = hist + (int)((unsigned)(TFFT_SP_COPY_BY_LANE ? tid : tid >> 6) % (unsigned)copies) * HL;
    const int x0 = blockIdx.x * TFFT_SP_COLS, yb = blockIdx.y * band_rows;
    const int ye = yb + band_rows < H ? yb + band_rows : H;
    const int ncols = W - x0 < TFFT_SP_COLS ? W - x0 : TFFT_SP_COLS;                    // own pixel columns
    const int lcols = W - x0 < TFFT_SP_COLS + 3 ? W - x0 : TFFT_SP_COLS + 3;            // with the halo to the right
    const int vlo = x0 ? 0 : 9, vhi = 9 + 3 * lcols;                                    // the tile's bytes that exist, counted from pixel x0 - 3
    const uint8_t* img = rgb + (size_t)blockIdx.z * (size_t)W * (size_t)H * 3;
    const unsigned row_step = (3u * (unsigned)W) & 3u;
    unsigned cz[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int d = 0; d < 4; d++) cz[k][d] = 0;
    for (int yc = yb; yc < ye; yc += TFFT_SP_ROWS) {
        const int own = ye - yc < TFFT_SP_ROWS ? ye - yc : TFFT_SP_ROWS;
        const int staged = H - yc < own + 3 ? H - yc : own + 3;
        const uint8_t* row0 = img + ((size_t)yc * W + x0) * 3;                          // pixel (yc, x0)
        const unsigned s0 = (unsigned)(((uintptr_t)row0 - 9) & 3);                      // byte shift of the first staged row
        __syncthreads();                                                                // the zeroing; the readers of the last chunk
        for (int e = tid; e < staged * ND; e += 256) {
            const int r = e / ND, d = e - r * ND;
            const uint8_t* row = row0 + (size_t)r * W * 3;
            const int sh = (int)((s0 + (unsigned)r * row_step) & 3u), lo = 4 * d - sh;  // the dword holds the tile's bytes lo .. lo+3 of the row
            if (lo >= vlo && lo + 4 <= vhi) tile[r * TFFT_SP_PITCH + d] = *reinterpret_cast<const uint32_t*>(row + (lo - 9));
            else
                for (int t = 0; t < 4; t++)
                    if (lo + t >= vlo && lo + t < vhi) tb[4 * (r * TFFT_SP_PITCH + d) + t] = row[lo + t - 9];
        }
        __syncthreads();
        for (int r = 0; r < own; r++) {
            const bool down = yc + r + 3 < H;
            int o[4];                                                                   // LDS byte of pixel x0, plane 0 in rows r .. r+3
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = 4 * (r + q) * TFFT_SP_PITCH + (int)((s0 + (unsigned)(r + q) * row_step) & 3u) + 9;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int b = tid + 256 * k, j = b / 3;
                if (j >= ncols) continue;
                // what lies beside or below the image is read from the tile all the same (stale bytes, inside the tile) and not counted
                const bool right = x0 + j + 3 < W, left = x0 + j >= 3;
                const int p0 = tb[o[0] + b];
                const int i0 = spam_index<T>(p0, tb[o[0] + b + 3], tb[o[0] + b + 6], tb[o[0] + b + 9]);
                const int i1 = spam_index<T>(p0, tb[o[1] + b], tb[o[2] + b], tb[o[3] + b]);
                const int i2 = spam_index<T>(p0, tb[o[1] + b + 3], tb[o[2] + b + 6], tb[o[3] + b + 9]);
                const int i3 = spam_index<T>(p0, tb[o[1] + b - 3], tb[o[2] + b - 6], tb[o[3] + b - 9]);
                const bool ok0 = right, ok1 = down, ok2 = down && right, ok3 = down && left;
                unsigned* hp = h + (b - 3 * j) * 4 * N3;
                cz[k][0] += (ok0 && i0 == CENTRE) ? 1u : 0u;
                cz[k][1] += (ok1 && i1 == CENTRE) ? 1u : 0u;
                cz[k][2] += (ok2 && i2 == CENTRE) ? 1u : 0u;
                cz[k][3] += (ok3 && i3 == CENTRE) ? 1u : 0u;
                if (ok0 && i0 != CENTRE) atomicAdd(&hp[0 * N3 + i0], 1u);
                if (ok1 && i1 != CENTRE) atomicAdd(&hp[1 * N3 + i1], 1u);
                if (ok2 && i2 != CENTRE) atomicAdd(&hp[2 * N3 + i2], 1u);
                if (ok3 && i3 != CENTRE) atomicAdd(&hp[3 * N3 + i3], 1u);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int plane = (tid + 256 * k) % 3;
#pragma unroll
        for (int d = 0; d < 4; d++)
            if (cz[k][d]) atomicAdd(&h[(plane * 4 + d) * N3 + CENTRE], cz[k][d]);
    }
    __syncthreads();
    uint32_t* out = counts + (size_t)blockIdx.z * HL;
    for (int i = tid; i < HL; i += 256) {
        unsigned s = 0;
        for (int c = 0; c < copies; c++) s += hist[c * HL + i];
        if (s) atomicAdd(&out[i], s);
    }
}

int spam_bands(int W, int H, int t, int n_images, int* band_rows) {
    // rows of a band: a block's flush (12 n^3 atomics of 4 bytes) costs at most about an eighth of its reads (3 * TFFT_SP_COLS bytes per row),
    // the k_phase_hist rule; fewer rows where that leaves a launch under ~1024 blocks
    const int n = 2 * t + 1, n3 = n * n * n;
    const int tx = (W + TFFT_SP_COLS - 1) / TFFT_SP_COLS;
    int rows = (8 * 4 * 12 * n3 + 3 * TFFT_SP_COLS - 1) / (3 * TFFT_SP_COLS);
    rows = (rows + TFFT_SP_ROWS - 1) / TFFT_SP_ROWS * TFFT_SP_ROWS;
    int nb = (H + rows - 1) / rows;
    const int fill = (1024 + tx * n_images - 1) / (tx * n_images);
    if (nb < fill) nb = fill;
    const int most = (H + TFFT_SP_ROWS - 1) / TFFT_SP_ROWS;
    if (nb > most) nb = most;
    if (nb > 65535) nb = 65535;
    rows = ((H + nb - 1) / nb + TFFT_SP_ROWS - 1) / TFFT_SP_ROWS * TFFT_SP_ROWS;
    *band_rows = rows;
    return (H + rows - 1) / rows;
}

template <int T>
static hipError_t launch_spam_t(const uint8_t* rgb, int W, int H, int n_images, uint32_t* counts, hipStream_t s) {
    constexpr int N = 2 * T + 1, HL = 12 * N * N * N;
    constexpr int copies = (T <= 3 || TFFT_SP_COPIES < 2) ? TFFT_SP_COPIES : 2;      // T = 4: four copies (140 KB) and the tile do not fit
    constexpr size_t lds = (size_t)TFFT_SP_STAGE_ROWS * TFFT_SP_PITCH * 4 + (size_t)copies * HL * sizeof(unsigned);
    int band_rows = 0;
    const int nb = spam_bands(W, H, T, n_images, &band_rows);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k_spam<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_spam<T>, dim3((unsigned)((W + TFFT_SP_COLS - 1) / TFFT_SP_COLS), (unsigned)nb, (unsigned)n_images), dim3(256), lds, s, rgb, W, H,
                       band_rows, copies, counts);
    return hipGetLastError();
}

hipError_t launch_spam(const uint8_t* rgb, int W, int H, int n_images, int t, uint32_t* counts, hipStream_t s) {
    if (W < 1 || H < 1 || n_images < 1 || n_images > 65535 || t < 1 || t > 4) return hipErrorInvalidValue;
    const int n = 2 * t + 1;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_images * 12 * n * n * n * sizeof(uint32_t), s);      // every entry is written
    if (e != hipSuccess) return e;
    switch (t) {
        case 1: return launch_spam_t<1>(rgb, W, H, n_images, counts, s);
        case 2: return launch_spam_t<2>(rgb, W, H, n_images, counts, s);
        case 3: return launch_spam_t<3>(rgb, W, H, n_images, counts, s);
        default: return launch_spam_t<4>(rgb, W, H, n_images, counts, s);
    }
}

}  // namespace tfft

// tfft_stats.hip is a unit of its own: hipcc compiles it apart (csrc/Makefile), and so does the CPU emulation of the tests
// (tests/emu/Makefile names it and sets TFFT_STATS_OWN_UNIT).  Only an emulation build that does neither gets it from here.  That is the
// tests directory of the revision before the split: laid over these sources, as a regression run of the old tests over the new code does
// it, its Makefile names the old units alone, and without this the library it builds fails to load for want of every launcher that moved.
#if !defined(__HIPCC__) && !defined(TFFT_STATS_OWN_UNIT)
#include "tfft_stats.hip"
#endif

// tfft_device.h -- device helpers that tfft_kernels.hip and tfft_stats.hip both need: one definition each, so that the transform,
// the embed and the statistics agree bit for bit on what a magnitude is and on how the packed column 0 comes apart.
#pragma once
#include <hip/hip_runtime.h>

namespace tfft {

// the dynamic LDS of every kernel of the library
extern __shared__ __attribute__((aligned(16))) unsigned char tfft_smem[];

// |F| exactly as every kernel of this library computes it (one definition so
// that medians, capacity and embed agree bit for bit)
__device__ __forceinline__ float mag_of(float2 v) { return sqrtf(fmaf(v.x, v.x, v.y * v.y)); }
// The statistics work on |F|^2 (the argument of mag_of's square root): sqrtf is monotone, so the element at
// a given rank is the same and the median is the square root of the selected value -- one sqrt per plane
// instead of one per bin.
__device__ __forceinline__ float mag2_of(float2 v) { return fmaf(v.x, v.x, v.y * v.y); }

// F[y][0] and F[y][M] out of the packed column 0
__device__ __forceinline__ void unpack_col0(const float2* __restrict__ plane, int y, int PH, int M, float2& f0,
                                            float2& fm) {
    const float2 a = plane[(size_t)y * M], b = plane[(size_t)((PH - y) & (PH - 1)) * M];
    f0 = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));           // (a + conj b)/2
    fm = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));          // (a - conj b)/(2i)
}

// rank of this lane among the set bits of a wave mask (v_mbcnt_lo/hi)
__device__ __forceinline__ unsigned wave_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

}  // namespace tfft

// geom_common.h -- device helpers shared by the geometric-verification kernels (kernels_homography.hip, kernels_fundamental.hip,
// kernels_fundrefit.hip): the wave sum whose order the refits' rules fix, and the record load, count clamp, Sampson test and
// 3 x 3 product of the fundamental matrix.  Every file that includes it is built with -ffp-contract=off.
#pragma once
#include "hak_internal.h"

// xor butterfly over 32, 16, .., 1: every lane returns the same total
__device__ __forceinline__ double hg_wsum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int hg_wsum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the last 16 bytes of a hak_match_pair; a record with a non-finite coordinate gets x1 = NaN, which fails every test below
__device__ __forceinline__ float4 fd_load(const hak_match_pair* m, int i)
{
    float4 r = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(m + i) + 16);
    if (!(__builtin_isfinite(r.x) && __builtin_isfinite(r.y) && __builtin_isfinite(r.z) && __builtin_isfinite(r.w)))
        r.x = __builtin_nanf("");
    return r;
}

__device__ __forceinline__ int fd_count(const int* counts, int pair, int n_host, long stride)
{
    long n = counts ? counts[pair] : n_host;
    return (int)(n < 0 ? 0 : (n > stride ? stride : n));
}

// Sampson distance below the threshold (t2 = threshold^2); NaN fails
__device__ __forceinline__ bool fd_inlier(const float F[9], const float4 r, const float t2)
{
    const float a = (F[0] * r.x + F[1] * r.y) + F[2];
    const float b = (F[3] * r.x + F[4] * r.y) + F[5];
    const float c = (F[6] * r.x + F[7] * r.y) + F[8];
    const float e = (a * r.z + b * r.w) + c;
    const float p = (F[0] * r.z + F[3] * r.w) + F[6];
    const float q = (F[1] * r.z + F[4] * r.w) + F[7];
    const float den = (a * a + b * b) + (p * p + q * q);
    return e * e < t2 * den;
}

__device__ __forceinline__ void fd_mul3(const double A[9], const double B[9], double C[9])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

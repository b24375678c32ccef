// geom_common.h -- device arithmetic shared by the geometric-verification kernels (kernels_homography.hip, kernels_fundamental.hip,
// kernels_fundrefit.hip, kernels_pose.hip, kernels_poserefit.hip, kernels_pnp.hip, kernels_pnprefit.hip,
// kernels_triangulate.hip): the wave sum whose order the refits' rules fix,
// the match-list record load and count clamp of all of them, the 3 x 3 product, the transfer-error test of the homography and the
// Sampson test of the fundamental matrix, the real roots of a monic cubic by bracketing and bisection (step 5 of
// hak_find_fundamental, also the critical points of hak_solve_pnp's quartic), and the 3 x 3 cyclic Jacobi of the refit's rule.
// The RANSAC scaffold of the three estimators is ransac_common.h, which includes this and holds the views hg_est and fd_est; the
// refit scaffold (inlier count, Hartley passes, normal equations, elimination, round loop) is refit_common.h on top of that.
// What the two point kernels share (kernels_pose.hip, kernels_triangulate.hip) is points_common.h, which also includes this.
// Every file that includes it is built with -ffp-contract=off.
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

// the count of list `pair`, clamped to 0 .. stride: counts[pair * step], or counts = NULL: n_host
__device__ __forceinline__ int fd_count(const int* counts, int pair, int step, int n_host, long stride)
{
    long n = counts ? counts[(long)pair * step] : n_host;
    return (int)(n < 0 ? 0 : (n > stride ? stride : n));
}

// transfer error of the homography H (H[8] = 1) below the threshold in front of the camera (t2 = threshold^2); NaN fails
__device__ __forceinline__ bool hg_inlier(const float H[9], const float4 r, const float t2)
{
    const float wz = (H[6] * r.x + H[7] * r.y) + 1.0f;
    const float u = (H[0] * r.x + H[1] * r.y) + H[2];
    const float v = (H[3] * r.x + H[4] * r.y) + H[5];
    const float ex = u - r.z * wz, ey = v - r.w * wz;
    return wz > 0.0f && ex * ex + ey * ey < t2 * (wz * wz);
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

// the monic cubic ((a + b2) a + b1) a + b0
__device__ __forceinline__ double fd_q(double a, double b2, double b1, double b0) { return ((a + b2) * a + b1) * a + b0; }

// 64 bisections of [lo, hi]; *has = the ends differ in the sign test
__device__ __forceinline__ double fd_bisect(double lo, double hi, double b2, double b1, double b0, bool* has)
{
    const bool neg = fd_q(lo, b2, b1, b0) < 0.0;
    *has = neg != (fd_q(hi, b2, b1, b0) < 0.0);
#pragma unroll 1
    for (int it = 0; it < 64; it++) {
        const double mid = 0.5 * (lo + hi);
        const bool left = (fd_q(mid, b2, b1, b0) < 0.0) == neg;
        lo = left ? mid : lo;
        hi = left ? hi : mid;
    }
    return 0.5 * (lo + hi);
}

// step 5 of hak_find_fundamental from the monic coefficients on: the real roots of ((a + b2) a + b1) a + b0 in bracket order to
// av[0 .. *count); false if a coefficient or the bound is non-finite.  Shared with the quartic's critical points of hak_solve_pnp.
__device__ __forceinline__ bool fd_cubic_roots(double b2, double b1, double b0, double av[3], int* count)
{
    double mx = fabs(b2);
    if (fabs(b1) > mx) mx = fabs(b1);
    if (fabs(b0) > mx) mx = fabs(b0);
    const double bound = 1.0 + mx;
    if (!(__builtin_isfinite(b2) && __builtin_isfinite(b1) && __builtin_isfinite(b0) && __builtin_isfinite(bound))) return false;
    const double D = b2 * b2 - 3.0 * b1;
    const bool three = D > 0.0;
    const double sq = sqrt(three ? D : 0.0);
    const double t1 = (-b2 - sq) / 3.0, t2 = (-b2 + sq) / 3.0;
    double root[3];
    bool has[3];
    root[0] = fd_bisect(-bound, three ? t1 : bound, b2, b1, b0, &has[0]);
    root[1] = fd_bisect(t1, t2, b2, b1, b0, &has[1]);
    root[2] = fd_bisect(t2, bound, b2, b1, b0, &has[2]);
    has[1] = has[1] && three;
    has[2] = has[2] && three;
    // roots are numbered in bracket order: compact them (selects)
    *count = (int)has[0] + (int)has[1] + (int)has[2];
    av[0] = has[0] ? root[0] : (has[1] ? root[1] : root[2]);
    av[1] = (has[0] && has[1]) ? root[1] : root[2];
    av[2] = root[2];
    return true;
}

// the rotation that annihilates apq (step 5 of hak_refine_fundamental)
__device__ __forceinline__ void fr_angle(double app, double aqq, double apq, double& t, double& c, double& sn)
{
    const double th = (aqq - app) / (2.0 * apq);
    const double sg = th >= 0.0 ? 1.0 : -1.0;
    t = sg / (fabs(th) + sqrt(th * th + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    sn = t * c;
}

// the sweeps of jacobi(G, 3, sweeps) of that rule, every lane the whole problem: G is left with the eigenvalues on its diagonal,
// V gets the eigenvectors as columns
__device__ __forceinline__ void fd_jacobi3(double G[3][3], double V[3][3], const int sweeps)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < sweeps; sweep++)
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                const double apq = G[p][q];
                if (apq == 0.0) continue;
                double t, c, sn;
                fr_angle(G[p][p], G[q][q], apq, t, c, sn);
                const int k = 3 - p - q;                            // the one index that is neither p nor q
                const double x = G[k][p], y = G[k][q];
                G[k][p] = G[p][k] = c * x - sn * y;
                G[k][q] = G[q][k] = sn * x + c * y;
                G[p][p] = G[p][p] - t * apq;
                G[q][q] = G[q][q] + t * apq;
                G[p][q] = G[q][p] = 0.0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - sn * vq;
                    V[i][q] = sn * vp + c * vq;
                }
            }
}

// the column of the smallest eigenvalue (<, ties to the smallest j)
__device__ __forceinline__ int fd_jacobi3_smallest(const double G[3][3])
{
    int best = 0;
    double dbest = G[0][0];
#pragma unroll
    for (int j = 1; j < 3; j++)
        if (G[j][j] < dbest) { dbest = G[j][j]; best = j; }
    return best;
}

// kernels_pnprefit.hip -- Gauss-Newton refit of an absolute pose over its inliers, iterated (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_refine_pnp) so that the numpy reference tests/pnp_refit_ref.py agrees bit for
// bit: per round the inliers of the current pose, their reprojection residuals and Jacobian rows under the left perturbation
// Xc' = Xc + w x Xc + dt, the 21 upper-triangle sums of the 6 x 6 normal matrix and the 6 of its right-hand side in the homography
// refit's summation order, Gaussian elimination with partial pivoting, the Cayley update and float32 re-scoring; the round is kept
// when it scores at least as well.  float64, + - * / only; the file is built with -ffp-contract=off: no FMA is formed, so every
// rounding is the one the reference makes.
//
// k_pnp_refit: one wave per list, refit_record of refit_common.h: the record's check, the round loop, the mask (written once, after
//   the last round) and the record (lane 0 rewrites it in place) are that header's.  pr_refit::round is this rule's round: one
//   streaming pass over the list accumulates the inlier count and the 27 sums in registers (rf_tri_add) and closes them with the
//   xor butterfly (rf_system), so every lane holds the same system; the 6 x 7 elimination (rf_solve, the one the homography's
//   refit runs at 8 x 9: fully unrolled, row exchanges as selects on compile-time indices) and the update run redundantly in every
//   lane; the loop's second pass counts the candidate's inliers.  No LDS, no scratch.
#include "refit_common.h"
#include "pnp_common.h"

// the refit scaffold's view (refit_common.h)
struct pr_refit : pn_est {
    static constexpr int MIN_INLIERS = 4, REFINED = 4;              // REFINED: hak_abs_pose.solution of a refitted record
    __device__ bool round(const hak_corr3d* c, int n, const float cur[12], int* cnt, float cand[12]) const;
};

// steps 1-5 of the rule up to the scoring, from the pose cur: *cnt = the inliers of cur; true and cand = the updated pose, false
// when the round fails.  Every lane computes the same.
__device__ bool pr_refit::round(const hak_corr3d* c, int n, const float cur[12], int* cnt, float cand[12]) const
{
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = (double)cur[k];
    const double fx = K.fx, fy = K.fy, cx = K.cx, cy = K.cy;
    int m = 0;
    double N[21], g[6];
    rf_tri_zero(N);
    rf_tri_zero(g);
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) {
        const pn_rec r = pn_load(c, i);
        if (!inlier(cur, r)) continue;
        m++;
        const double X = r.a.x, Y = r.a.y, Z = r.a.z;
        const double xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[9];
        const double yc = ((M[3] * X + M[4] * Y) + M[5] * Z) + M[10];
        const double zc = ((M[6] * X + M[7] * Y) + M[8] * Z) + M[11];
        const double iz = 1.0 / zc;
        const double a = xc * iz, b = yc * iz;
        const double rx = (fx * a + cx) - (double)r.a.w, ry = (fy * b + cy) - (double)r.v;
        const double px = fx * iz, py = fy * iz;
        const double jx[6] = {-((px * a) * yc), px * zc + (px * a) * xc, -(px * yc), px, 0.0, -(px * a)};
        const double jy[6] = {(-(py * zc)) - (py * b) * yc, (py * b) * xc, py * xc, 0.0, py, -(py * b)};
        rf_tri_add<6>(N, jx, jy);
#pragma unroll
        for (int p = 0; p < 6; p++) g[p] = g[p] + (-(jx[p] * rx + jy[p] * ry));
    }
    m = hg_wsum(m);
    *cnt = m;
    if (m < MIN_INLIERS) return false;                              // (wave-uniform, as every exit below)
    double S[6][7], d[6];
    rf_system<6>(N, g, S);
    if (!rf_solve<6>(S, d)) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && __builtin_isfinite(d[i]);
    if (!ok) return false;
    // step 5: the Cayley map of w = d[0..2] / 2, applied on the left
    const double w0 = 0.5 * d[0], w1 = 0.5 * d[1], w2 = 0.5 * d[2];
    const double ww = (w0 * w0 + w1 * w1) + w2 * w2;
    const double k1 = 1.0 - ww, den = 1.0 + ww;
    const double C[9] = {(k1 + 2.0 * (w0 * w0)) / den, (2.0 * (w0 * w1 - w2)) / den, (2.0 * (w0 * w2 + w1)) / den,
                         (2.0 * (w0 * w1 + w2)) / den, (k1 + 2.0 * (w1 * w1)) / den, (2.0 * (w1 * w2 - w0)) / den,
                         (2.0 * (w0 * w2 - w1)) / den, (2.0 * (w1 * w2 + w0)) / den, (k1 + 2.0 * (w2 * w2)) / den};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) cand[3 * i + j] = (float)((C[3 * i] * M[j] + C[3 * i + 1] * M[3 + j]) + C[3 * i + 2] * M[6 + j]);
        cand[9 + i] = (float)(((C[3 * i] * M[9] + C[3 * i + 1] * M[10]) + C[3 * i + 2] * M[11]) + d[3 + i]);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) ok = ok && __builtin_isfinite(cand[k]);
    return ok;
}

__global__ __launch_bounds__(HAK_WAVE) void k_pnp_refit(const hak_corr3d* __restrict__ base, long stride,
                                                        const int* __restrict__ counts, int n_host, hak_intrinsics K, int rounds,
                                                        float t2, hak_abs_pose* inout, unsigned char* __restrict__ masks,
                                                        long mask_stride)
{
    const int pair = blockIdx.x;
    refit_record(pr_refit{{K, t2}}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), rounds, inout, masks,
                 mask_stride);
}

void hak_launch_pnp_refit(hipStream_t st, const hak_corr3d* corr, long stride, const int* counts, int n_host, int npairs,
                          const hak_intrinsics& K, float threshold, int rounds, hak_abs_pose* inout, unsigned char* masks,
                          long mask_stride)
{
    k_pnp_refit<<<npairs, HAK_WAVE, 0, st>>>(corr, stride, counts, n_host, K, rounds, threshold * threshold, inout, masks, mask_stride);
}

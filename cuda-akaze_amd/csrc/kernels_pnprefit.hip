// kernels_pnprefit.hip -- Gauss-Newton refit of an absolute pose over its inliers, iterated (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_refine_pnp) so that the numpy reference tests/pnp_refit_ref.py agrees bit for
// bit: per round the inliers of the current pose, their reprojection residuals and Jacobian rows under the left perturbation
// Xc' = Xc + w x Xc + dt, the 21 upper-triangle sums of the 6 x 6 normal matrix and the 6 of its right-hand side in the homography
// refit's summation order, Gaussian elimination with partial pivoting, the Cayley update and float32 re-scoring; the round is kept
// when it scores at least as well.  float64, + - * / only; the file is built with -ffp-contract=off: no FMA is formed, so every
// rounding is the one the reference makes.
//
// k_pnp_refit: one wave per list.  One streaming pass over the list per round accumulates the inlier count and the 27 sums in
//   registers and closes them with the xor butterfly, so every lane holds the same system; the 6 x 7 elimination, fully unrolled
//   with its row exchanges as selects on compile-time indices, and the update run redundantly in every lane; a second pass counts
//   the candidate's inliers.  No LDS, no scratch.  The mask is written once, after the last round; lane 0 rewrites the record in
//   place.
#include "hak_internal.h"
#include "geom_common.h"
#include "pnp_common.h"

#define PR_MIN_INLIERS 4
#define PR_REFINED_SOLUTION 4

// inliers of M over the list (every lane returns the total)
__device__ int pr_count_inliers(const hak_corr3d* c, int n, const float M[12], const hak_intrinsics K, float t2)
{
    int k = 0;
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) {
        const pn_rec r = pn_load(c, i);
        k += pn_inlier(M, r.a, r.v, K, t2) ? 1 : 0;
    }
    return hg_wsum(k);
}

// step 4 of the rule: S = [N | g] is destroyed, d = the solution; false when a pivot is 0 or non-finite or d is not finite
__device__ __forceinline__ bool pr_solve(double S[6][7], double d[6])
{
#pragma unroll
    for (int c = 0; c < 6; c++) {
        int piv = c;
        double best = fabs(S[c][c]);
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            const double v = fabs(S[r][c]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > 0.0) || !__builtin_isfinite(best)) return false;
#pragma unroll
        for (int r = c + 1; r < 6; r++) {                           // (selects, no dynamic register indexing)
            const bool swap = r == piv;
#pragma unroll
            for (int q = c; q < 7; q++) {
                const double top = S[c][q], low = S[r][q];
                S[c][q] = swap ? low : top;
                S[r][q] = swap ? top : low;
            }
        }
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            const double f = S[r][c] / S[c][c];
#pragma unroll
            for (int q = c + 1; q < 7; q++) S[r][q] = S[r][q] - f * S[c][q];
        }
    }
    bool ok = true;
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double acc = S[i][6];
#pragma unroll
        for (int j = i + 1; j < 6; j++) acc = acc - S[i][j] * d[j];
        d[i] = acc / S[i][i];
        ok = ok && __builtin_isfinite(d[i]);
    }
    return ok;
}

// steps 1-5 of the rule up to the scoring, from the pose cur: *cnt = the inliers of cur; true and cand = the updated pose, false
// when the round fails.  Every lane computes the same.
__device__ bool pr_round(const hak_corr3d* c, int n, const float cur[12], const hak_intrinsics K, float t2, int* cnt, float cand[12])
{
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = (double)cur[k];
    const double fx = K.fx, fy = K.fy, cx = K.cx, cy = K.cy;
    int m = 0;
    double N[21], g[6];
#pragma unroll
    for (int k = 0; k < 21; k++) N[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) g[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) {
        const pn_rec r = pn_load(c, i);
        if (!pn_inlier(cur, r.a, r.v, K, t2)) continue;
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
        int k = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++, k++) N[k] = N[k] + (jx[p] * jx[q] + jy[p] * jy[q]);
#pragma unroll
        for (int p = 0; p < 6; p++) g[p] = g[p] + (-(jx[p] * rx + jy[p] * ry));
    }
    m = hg_wsum(m);
    *cnt = m;
    if (m < PR_MIN_INLIERS) return false;                           // (wave-uniform, as every exit below)
    double S[6][7];
    {
        int k = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++, k++) { const double v = hg_wsum(N[k]); S[p][q] = v; S[q][p] = v; }
#pragma unroll
        for (int p = 0; p < 6; p++) S[p][6] = hg_wsum(g[p]);
    }
    double d[6];
    if (!pr_solve(S, d)) return false;
    // step 5: the Cayley map of w = d[0..2] / 2, applied on the left
    const double w0 = 0.5 * d[0], w1 = 0.5 * d[1], w2 = 0.5 * d[2];
    const double ww = (w0 * w0 + w1 * w1) + w2 * w2;
    const double k1 = 1.0 - ww, den = 1.0 + ww;
    const double C[9] = {(k1 + 2.0 * (w0 * w0)) / den, (2.0 * (w0 * w1 - w2)) / den, (2.0 * (w0 * w2 + w1)) / den,
                         (2.0 * (w0 * w1 + w2)) / den, (k1 + 2.0 * (w1 * w1)) / den, (2.0 * (w1 * w2 - w0)) / den,
                         (2.0 * (w0 * w2 - w1)) / den, (2.0 * (w1 * w2 + w0)) / den, (k1 + 2.0 * (w2 * w2)) / den};
    bool ok = true;
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
    const int pair = blockIdx.x, l = threadIdx.x;
    const hak_corr3d* c = base + (long)pair * stride;
    const int n = fd_count(counts, pair, n_host, stride);
    const hak_abs_pose in = inout[pair];
    float cur[12];
    bool model = in.hypothesis >= 0;
#pragma unroll
    for (int k = 0; k < 9; k++) { cur[k] = in.R[k]; model = model && __builtin_isfinite(cur[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { cur[9 + k] = in.t[k]; model = model && __builtin_isfinite(cur[9 + k]); }
    int cnt = 0, solution = in.solution;
    if (model) {
#pragma unroll 1
        for (int r = 0; r < rounds; r++) {
            float cand[12];
            if (!pr_round(c, n, cur, K, t2, &cnt, cand)) break;
            const int k = pr_count_inliers(c, n, cand, K, t2);
            if (k < cnt) break;
#pragma unroll
            for (int q = 0; q < 12; q++) cur[q] = cand[q];
            cnt = k;
            solution = PR_REFINED_SOLUTION;
        }
    }
    if (masks) {
        unsigned char* mk = masks + (long)pair * mask_stride;
        for (int i = l; i < n; i += HAK_WAVE) {
            const pn_rec r = pn_load(c, i);
            mk[i] = (model && pn_inlier(cur, r.a, r.v, K, t2)) ? 1 : 0;
        }
    }
    if (l == 0) {
        hak_abs_pose o;
#pragma unroll
        for (int k = 0; k < 9; k++) o.R[k] = model ? cur[k] : (k % 4 == 0 ? 1.0f : 0.0f);
#pragma unroll
        for (int k = 0; k < 3; k++) o.t[k] = model ? cur[9 + k] : 0.0f;
        o.inliers = model ? cnt : 0; o.hypothesis = model ? in.hypothesis : -1; o.solution = model ? solution : 0; o.n = n;
        inout[pair] = o;
    }
}

// the record of a hak_refine_pnp call that has no context: a device global, so that the call allocates nothing
__device__ hak_abs_pose g_pnp_refit_record;

hak_abs_pose* hak_pnp_refit_record()
{
    void* p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(g_pnp_refit_record)) == hipSuccess ? static_cast<hak_abs_pose*>(p) : nullptr;
}

void hak_launch_pnp_refit(hipStream_t st, const hak_corr3d* corr, long stride, const int* counts, int n_host, int npairs,
                          const hak_intrinsics& K, float threshold, int rounds, hak_abs_pose* inout, unsigned char* masks,
                          long mask_stride)
{
    k_pnp_refit<<<npairs, HAK_WAVE, 0, st>>>(corr, stride, counts, n_host, K, rounds, threshold * threshold, inout, masks, mask_stride);
}

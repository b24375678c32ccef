// refit_common.h -- the least-squares refit scaffold of the estimators (kernels_homography.hip, kernels_fundrefit.hip,
// kernels_pnprefit.hip, kernels_poserefit.hip): what is not an estimator's own algebra, stated once.  One wave per list; every
// lane ends with the same values, so every exit is wave-uniform.  float64 sums in the one order the rules fix: lane l takes records i = l mod 64 in ascending i, then
// hg_wsum's xor butterfly.  Every loop over a system is fully unrolled (compile-time register indices; no LDS, no scratch).
// A refit estimator E is a view of ransac_common.h that adds REFINED (the tag of a record that a round improved) and
// round(list, n, cur, &cnt, cand) const: *cnt = the inliers of cur; true and cand = the refitted model, false when the round fails
// (fewer inliers than the rule's minimum among the reasons).  Every file that includes this is built with -ffp-contract=off.
#pragma once
#include "ransac_common.h"

// inliers of M over the list (one wave, every lane returns the total)
template <class E>
__device__ __forceinline__ int rf_count_inliers(const E est, const typename E::list_t* m, int n, const float M[E::NW])
{
    int c = 0;
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) c += est.inlier(M, E::load(m, i)) ? 1 : 0;
    return hg_wsum(c);
}

struct rf_norm {
    int m;                                                          // inliers
    double c1x, c1y, c2x, c2y, q1, q2, s1, s2;                      // centroids, sums of squares about them, scales
};

// Hartley normalisation over the inliers of M on a match list, two streaming passes.  No exit of its own: what a rule makes of a
// small count, q <= 0 or a non-finite scale is the caller's to check
template <class E>
__device__ __forceinline__ rf_norm rf_hartley(const E est, const hak_match_pair* m, int n, const float M[E::NW])
{
    const int l = threadIdx.x;
    rf_norm h;
    int cnt = 0;
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
    for (int i = l; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!est.inlier(M, r)) continue;
        cnt++;
        sx1 = sx1 + (double)r.x; sy1 = sy1 + (double)r.y; sx2 = sx2 + (double)r.z; sy2 = sy2 + (double)r.w;
    }
    h.m = hg_wsum(cnt);
    const double mm = (double)h.m;
    h.c1x = hg_wsum(sx1) / mm; h.c1y = hg_wsum(sy1) / mm; h.c2x = hg_wsum(sx2) / mm; h.c2y = hg_wsum(sy2) / mm;
    double q1 = 0.0, q2 = 0.0;
    for (int i = l; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!est.inlier(M, r)) continue;
        const double dx1 = (double)r.x - h.c1x, dy1 = (double)r.y - h.c1y, dx2 = (double)r.z - h.c2x, dy2 = (double)r.w - h.c2y;
        q1 = q1 + (dx1 * dx1 + dy1 * dy1);
        q2 = q2 + (dx2 * dx2 + dy2 * dy2);
    }
    h.q1 = hg_wsum(q1); h.q2 = hg_wsum(q2);
    h.s1 = sqrt((2.0 * mm) / h.q1); h.s2 = sqrt((2.0 * mm) / h.q2);
    return h;
}

// the normal equations of N unknowns: N (N + 1) / 2 upper-triangle sums, row-major, from two rows or one per record, closed by the
// butterfly and mirrored with the right-hand side into S = [N | g]; then the elimination
template <int N>
constexpr int rf_tri() { return N * (N + 1) / 2; }

template <int K>
__device__ __forceinline__ void rf_tri_zero(double (&T)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) T[k] = 0.0;
}

// T += a^T a + b^T b (upper triangle)
template <int N>
__device__ __forceinline__ void rf_tri_add(double (&T)[rf_tri<N>()], const double (&a)[N], const double (&b)[N])
{
    int k = 0;
#pragma unroll
    for (int p = 0; p < N; p++)
#pragma unroll
        for (int q = p; q < N; q++, k++) T[k] = T[k] + (a[p] * a[q] + b[p] * b[q]);
}

// T += w^T w (upper triangle)
template <int N>
__device__ __forceinline__ void rf_tri_add(double (&T)[rf_tri<N>()], const double (&w)[N])
{
    int k = 0;
#pragma unroll
    for (int p = 0; p < N; p++)
#pragma unroll
        for (int q = p; q < N; q++, k++) T[k] = T[k] + w[p] * w[q];
}

// S = [N | g] from the lanes' partial sums
template <int N>
__device__ __forceinline__ void rf_system(const double (&T)[rf_tri<N>()], const double (&g)[N], double (&S)[N][N + 1])
{
    int k = 0;
#pragma unroll
    for (int p = 0; p < N; p++)
#pragma unroll
        for (int q = p; q < N; q++, k++) { const double v = hg_wsum(T[k]); S[p][q] = v; S[q][p] = v; }
#pragma unroll
    for (int p = 0; p < N; p++) S[p][N] = hg_wsum(g[p]);
}

// S is destroyed, d = the solution; false when a pivot is 0 or non-finite.  A row exchange is a chain of selects.
template <int N>
__device__ __forceinline__ bool rf_solve(double (&S)[N][N + 1], double (&d)[N])
{
#pragma unroll
    for (int c = 0; c < N; c++) {
        int piv = c;
        double best = fabs(S[c][c]);
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const double v = fabs(S[r][c]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > 0.0) || !__builtin_isfinite(best)) return false;
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const bool swap = r == piv;
#pragma unroll
            for (int q = c; q < N + 1; q++) {
                const double top = S[c][q], low = S[r][q];
                S[c][q] = swap ? low : top;
                S[r][q] = swap ? top : low;
            }
        }
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const double f = S[r][c] / S[c][c];
#pragma unroll
            for (int q = c + 1; q < N + 1; q++) S[r][q] = S[r][q] - f * S[c][q];
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double acc = S[i][N];
#pragma unroll
        for (int j = i + 1; j < N; j++) acc = acc - S[i][j] * d[j];
        d[i] = acc / S[i][i];
    }
    return true;
}

// up to `rounds` rounds from the model cur with cnt inliers (has: there is one; else the record gets no_model): a round is kept
// when its candidate scores at least as well, the first one that fails or scores worse ends the loop.  Then the mask of what is
// left and the pair's record, tagged REFINED if a round was kept.
template <class E>
__device__ __forceinline__ void refit_iterate(const E est, const typename E::list_t* m, int n, int rounds, float (&cur)[E::NW],
                                              bool has, int cnt, int hypothesis, int tag, typename E::out_t* out,
                                              unsigned char* masks, long mask_stride)
{
    if (has) {
#pragma unroll 1
        for (int r = 0; r < rounds; r++) {
            float cand[E::NW];
            if (!est.round(m, n, cur, &cnt, cand)) break;
            const int c = rf_count_inliers(est, m, n, cand);
            if (c < cnt) break;
#pragma unroll
            for (int k = 0; k < E::NW; k++) cur[k] = cand[k];
            cnt = c;
            tag = E::REFINED;
        }
    } else {
        E::no_model(cur); cnt = 0; hypothesis = -1; tag = 0;
    }
    rs_write_result(est, m, n, cur, cnt, hypothesis, tag, out, masks, mask_stride);
}

// the body of a refit kernel: the pair's record is read, refitted and rewritten in place
template <class E>
__device__ __forceinline__ void refit_record(const E est, const typename E::list_t* m, int n, int rounds, typename E::out_t* inout,
                                             unsigned char* masks, long mask_stride)
{
    const typename E::out_t in = inout[blockIdx.x];
    float cur[E::NW];
    const bool has = E::load_model(in, cur);
    refit_iterate(est, m, n, rounds, cur, has, 0, in.hypothesis, E::tag(in), inout, masks, mask_stride);
}

// kernels_poserefit.hip -- calibrated Gauss-Newton refit of a relative pose over the matches that count under it, iterated
// (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_refine_pose) so that the numpy reference tests/pose_refit_ref.py agrees bit
// for bit: the float32 F of a pose (E = [t]x R between the closed-form inverses of the two zero-skew K), the matches that count
// under it (Sampson inliers of that F in front of both cameras by the two-ray solve of hak_recover_pose), per round their Sampson
// residuals with the denominator frozen, the Jacobian rows under a left perturbation of R and a tangent step of t, the 15
// upper-triangle sums of the 5 x 5 normal matrix and the 5 of its right-hand side in the homography refit's summation order,
// Gaussian elimination with partial pivoting, the Cayley update of R and the renormalised step of t, both rounded to float32; the
// round is kept when as many matches count.  float64, + - * / sqrt only; the file is built with -ffp-contract=off: no FMA is
// formed, so every rounding is the one the reference makes.
//
// k_pose_refit: one wave per list.  The record's check, the round loop and the record (lane 0 rewrites it in place) are
//   refit_iterate's of refit_common.h; the model words are {R, t, the pose's float32 F}, so F is computed once per pose and the
//   counting test reads it beside R and t.  pz_refit::round is this rule's round: one streaming pass over the list accumulates the
//   count and the 20 sums in registers (rf_tri_add) and closes them with the xor butterfly (rf_system), so every lane holds the
//   same system; the 5 x 6 elimination (rf_solve, fully unrolled, row exchanges as selects) and the update run redundantly in
//   every lane; the loop's second pass counts the matches under the candidate.  No LDS, no scratch.
// k_pose_refit_points: the mask and point pass under the pose that is left, a second launch of k_pose's shape (one block of PZ_BLOCK
//   threads per list) that reads the rewritten record: it recomputes the pose's F, streams the list once, writes mask bytes and
//   points as k_pose's pass 2 does, counts the Sampson inliers of that F (an integer count, closed by pt_block_sum: one LDS int per
//   wave) and thread 0 completes the record with it.  The same pass at the end of k_pose_refit's one wave measured slower
//   (DESIGN.md 8k): 64 lanes writing 13 bytes per match cost more than a launch.
#include "refit_common.h"
#include "points_common.h"

#define PZ_R 0                   // model words: R row-major, t, F
#define PZ_T 9
#define PZ_F 12
#define PZ_BLOCK 512             // the point pass: k_pose's block
#define PZ_WAVES (PZ_BLOCK / HAK_WAVE)

__device__ __forceinline__ void pz_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// step 2 of the rule: M[PZ_F ..] = the float32 F of the pose M[0 .. 12); false = no model
__device__ __forceinline__ bool pz_pose_F(float M[21], const pt_K& k1, const pt_K& k2)
{
    double R[9], t[3], F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (double)M[PZ_R + k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (double)M[PZ_T + k];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double e0 = t[1] * R[6 + j] - t[2] * R[3 + j];           // column j of E = [t]x R
        const double e1 = t[2] * R[j] - t[0] * R[6 + j];
        const double e2 = t[0] * R[3 + j] - t[1] * R[j];
        F[j] = e0; F[3 + j] = e1; F[6 + j] = e2;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {                                       // E K1^-1, row by row
        const double g0 = F[3 * i] / k1.fx, g1 = F[3 * i + 1] / k1.fy;
        F[3 * i + 2] = (F[3 * i + 2] - g0 * k1.cx) - g1 * k1.cy;
        F[3 * i] = g0; F[3 * i + 1] = g1;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {                                       // K2^-T (.), column by column
        const double f0 = F[j] / k2.fx, f1 = F[3 + j] / k2.fy;
        F[6 + j] = (F[6 + j] - f0 * k2.cx) - f1 * k2.cy;
        F[j] = f0; F[3 + j] = f1;
    }
    double d = F[0];
#pragma unroll
    for (int k = 1; k < 9; k++) d = fabs(F[k]) > fabs(d) ? F[k] : d;
#pragma unroll
    for (int k = 0; k < 9; k++) M[PZ_F + k] = (float)(F[k] / d);
    return d != 0.0 && __builtin_isfinite(d);
}

// step 1 of the rule: the model words of a record; false = no model (candidate < 0, a non-finite R or t, a pose without an F)
__device__ __forceinline__ bool pz_load(const hak_pose& in, float M[21], const pt_K& k1, const pt_K& k2)
{
    bool has = in.candidate >= 0;
#pragma unroll
    for (int k = 0; k < 9; k++) { M[PZ_R + k] = in.R[k]; has = has && __builtin_isfinite(in.R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { M[PZ_T + k] = in.t[k]; has = has && __builtin_isfinite(in.t[k]); }
    return pz_pose_F(M, k1, k2) && has;
}

// the refit scaffold's view (refit_common.h) of a relative pose on a match list
struct pz_refit : rs_match_records {
    static constexpr int NW = 21, MIN_COUNT = 5, REFINED = 4;          // REFINED: hak_pose.candidate of a refitted record
    typedef hak_pose out_t;
    pt_K k1, k2;
    float t2;
    double md;
    // a match counts: a Sampson inlier of the pose's F, in front of both cameras
    __device__ __forceinline__ bool inlier(const float M[21], const float4 r) const
    {
        if (!fd_inlier(M + PZ_F, r, t2)) return false;
        double R[9], t[3], z;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = (double)M[PZ_R + k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = (double)M[PZ_T + k];
        const double b[3] = {k2.x(r.z), k2.y(r.w), 1.0};
        return pt_front(R, t, k1.x(r.x), k1.y(r.y), b, pt_dot(b, b), md, &z);
    }
    // the record's third int is the tag and says whether there is a model; `inliers` is k_pose_refit_points' to fill
    static __device__ __forceinline__ void store(hak_pose& o, const float M[21], int count, int hypothesis, int tag, int n)
    {
#pragma unroll
        for (int k = 0; k < 9; k++) o.R[k] = M[PZ_R + k];
#pragma unroll
        for (int k = 0; k < 3; k++) o.t[k] = M[PZ_T + k];
        o.inliers = 0; o.in_front = count; o.candidate = hypothesis >= 0 ? tag : -1; o.n = n;
    }
    static __device__ __forceinline__ void no_model(float M[21])
    {
#pragma unroll
        for (int k = 0; k < 21; k++) M[k] = (k < 9 && k % 4 == 0) ? 1.0f : 0.0f;
    }
    __device__ bool round(const hak_match_pair* m, int n, const float cur[21], int* cnt, float cand[21]) const;
};

// step 3 of the rule up to the scoring, from the pose cur: *cnt = the matches that count under cur; true and cand = the updated
// pose with its F, false when the round fails.  Every lane computes the same.
__device__ bool pz_refit::round(const hak_match_pair* m, int n, const float cur[21], int* cnt, float cand[21]) const
{
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (double)cur[PZ_R + k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (double)cur[PZ_T + k];
    // the tangent basis of t: e_k of the smallest |t_k| (ties to the smallest k)
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    const int kk = (a1 < a0) ? (a2 < a1 ? 2 : 1) : (a2 < a0 ? 2 : 0);
    const double nv[3] = {kk == 0 ? 0.0 : (kk == 1 ? -t[2] : t[1]), kk == 0 ? t[2] : (kk == 1 ? 0.0 : -t[0]),
                          kk == 0 ? -t[1] : (kk == 1 ? t[0] : 0.0)};   // cross(t, e_k)
    const double ln = sqrt(pt_dot(nv, nv));
    const double b1[3] = {nv[0] / ln, nv[1] / ln, nv[2] / ln};
    double b2[3];
    pz_cross(t, b1, b2);
    int cn = 0;
    double N[15], g[5];
    rf_tri_zero(N);
    rf_tri_zero(g);
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!fd_inlier(cur + PZ_F, r, t2)) continue;
        const double x = k1.x(r.x), y = k1.y(r.y);
        const double b[3] = {k2.x(r.z), k2.y(r.w), 1.0};
        double q[3], z;
        pt_rotate(R, x, y, q);
        if (!pt_front_rays(q, t, b, pt_dot(b, b), md, &z)) continue;
        cn++;
        double c[3], v[3], jw[3], h[3];
        pz_cross(t, q, c);
        const double e = pt_dot(b, c);
        pz_cross(b, t, v);
        const double u0 = (R[0] * v[0] + R[3] * v[1]) + R[6] * v[2];
        const double u1 = (R[1] * v[0] + R[4] * v[1]) + R[7] * v[2];
        const double p0 = c[0] / k2.fx, p1 = c[1] / k2.fy, p2 = u0 / k1.fx, p3 = u1 / k1.fy;
        const double s = sqrt((p0 * p0 + p1 * p1) + (p2 * p2 + p3 * p3));
        const double res = e / s;
        pz_cross(q, v, jw);
        pz_cross(q, b, h);
        const double w[5] = {jw[0] / s, jw[1] / s, jw[2] / s, pt_dot(h, b1) / s, pt_dot(h, b2) / s};
        rf_tri_add<5>(N, w);
#pragma unroll
        for (int p = 0; p < 5; p++) g[p] = g[p] + (-(w[p] * res));
    }
    cn = hg_wsum(cn);
    *cnt = cn;
    if (cn < MIN_COUNT) return false;                                   // (wave-uniform, as every exit below)
    double S[5][6], d[5];
    rf_system<5>(N, g, S);
    if (!rf_solve<5>(S, d)) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 5; i++) ok = ok && __builtin_isfinite(d[i]);
    if (!ok) return false;
    // the Cayley map of w = d[0..2] / 2, applied on the left (as hak_refine_pnp)
    const double w0 = 0.5 * d[0], w1 = 0.5 * d[1], w2 = 0.5 * d[2];
    const double ww = (w0 * w0 + w1 * w1) + w2 * w2;
    const double kc = 1.0 - ww, den = 1.0 + ww;
    const double C[9] = {(kc + 2.0 * (w0 * w0)) / den, (2.0 * (w0 * w1 - w2)) / den, (2.0 * (w0 * w2 + w1)) / den,
                         (2.0 * (w0 * w1 + w2)) / den, (kc + 2.0 * (w1 * w1)) / den, (2.0 * (w1 * w2 - w0)) / den,
                         (2.0 * (w0 * w2 - w1)) / den, (2.0 * (w1 * w2 + w0)) / den, (kc + 2.0 * (w2 * w2)) / den};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            cand[PZ_R + 3 * i + j] = (float)((C[3 * i] * R[j] + C[3 * i + 1] * R[3 + j]) + C[3 * i + 2] * R[6 + j]);
    double tn[3];
#pragma unroll
    for (int i = 0; i < 3; i++) tn[i] = (t[i] + d[3] * b1[i]) + d[4] * b2[i];
    const double len = sqrt(pt_dot(tn, tn));
#pragma unroll
    for (int i = 0; i < 3; i++) cand[PZ_T + i] = (float)(tn[i] / len);
    ok = __builtin_isfinite(len);
#pragma unroll
    for (int k = 0; k < 12; k++) ok = ok && __builtin_isfinite(cand[k]);
    return pz_pose_F(cand, k1, k2) && ok;
}

__global__ __launch_bounds__(HAK_WAVE) void k_pose_refit(const hak_match_pair* __restrict__ base, long stride,
                                                         const int* __restrict__ counts, int n_host, const hak_intrinsics K1,
                                                         const hak_intrinsics K2, float t2, float max_depth, int rounds,
                                                         hak_pose* inout)
{
    const int pair = blockIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    const pz_refit est{{}, pt_K(K1), pt_K(K2), t2, (double)max_depth};
    const hak_pose in = inout[pair];
    float cur[21];
    const bool has = pz_load(in, cur, est.k1, est.k2);                  // (wave-uniform)
    // the loop writes the record but no mask: k_pose_refit_points writes it with the points
    refit_iterate(est, m, n, rounds, cur, has, 0, has ? 0 : -1, in.candidate, inout, nullptr, 0);
}

// the mask and the points under the record's pose, and the Sampson inliers of its F (a record the loop left without a pose has
// t = 0 and candidate < 0: all zeros)
__global__ __launch_bounds__(PZ_BLOCK) void k_pose_refit_points(const hak_match_pair* __restrict__ base, long stride,
                                                                const int* __restrict__ counts, int n_host,
                                                                const hak_intrinsics K1, const hak_intrinsics K2, float t2,
                                                                float max_depth, hak_pose* inout,
                                                                unsigned char* __restrict__ masks, float* __restrict__ xyz)
{
    __shared__ int part[PZ_WAVES][1];
    const int pair = blockIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    const pt_K k1(K1), k2(K2);
    const double md = (double)max_depth;
    float cur[21];
    const bool has = pz_load(inout[pair], cur, k1, k2);
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (double)cur[PZ_R + k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (double)cur[PZ_T + k];
    const pt_out o(masks, xyz, pair, stride);
    int c[1] = {0};
    for (int i = threadIdx.x; i < n; i += PZ_BLOCK) {
        bool front = false;
        double x = 0.0, y = 0.0, z = 0.0;
        if (has) {
            const float4 r = fd_load(m, i);
            if (fd_inlier(cur + PZ_F, r, t2)) {
                c[0]++;
                x = k1.x(r.x);
                y = k1.y(r.y);
                const double b[3] = {k2.x(r.z), k2.y(r.w), 1.0};
                front = pt_front(R, t, x, y, b, pt_dot(b, b), md, &z);
            }
        }
        o.store(i, front, (float)(z * x), (float)(z * y), (float)z);
    }
    pt_block_sum<1, PZ_WAVES>(c, part);
    if (threadIdx.x == 0) inout[pair].inliers = c[0];
}

void hak_launch_pose_refit(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                           const hak_intrinsics& K1, const hak_intrinsics& K2, float threshold, float max_depth, int rounds,
                           hak_pose* inout, unsigned char* masks, float* xyz)
{
    const float t2 = threshold * threshold;
    k_pose_refit<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, K1, K2, t2, max_depth, rounds, inout);
    k_pose_refit_points<<<npairs, PZ_BLOCK, 0, st>>>(matches, stride, counts, n_host, K1, K2, t2, max_depth, inout, masks, xyz);
}

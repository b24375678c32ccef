// kernels_fundrefit.hip -- rank-2 least-squares refit of a fundamental matrix over its inliers, iterated (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_refine_fundamental) so that the numpy reference
// tests/fundamental_refit_ref.py agrees bit for bit: per round the inliers of the current F, Hartley normalisation and the 45
// upper-triangle sums of the 9 x 9 normal matrix in the homography refit's summation order, the eigenvector of its smallest
// eigenvalue by eight sweeps of cyclic Jacobi, the closest rank-2 matrix by a 3 x 3 Jacobi, denormalisation and float32 Sampson
// re-scoring; the round is kept when it scores at least as well.  float64, + - * / sqrt only; the file is built with
// -ffp-contract=off: no FMA is formed, so every rounding is the one the reference makes.
//
// k_fund_refit: one wave per pair.  Three streaming passes over the list per round (count and centroids, scales, the 45 sums in
//   registers), each closed by the xor butterfly, so every lane holds the same normal matrix.
//   The 9 x 9 Jacobi is a chain of 288 dependent rotations.  Lane k < 9 owns row k of A and row k of V in registers (the other
//   lanes shadow lane 0); the (p, q) loops are fully unrolled, so every register index and every lane number is a compile-time
//   constant.  A rotation reads A[p][p], A[q][q], A[p][q] and rows p and q from lanes p and q with v_readlane (17 64-bit lane
//   reads), every lane computes t, c and sn redundantly, lane k updates its entries of columns p and q, lanes p and q rebuild
//   their own rows from the two broadcast rows -- by the symmetry of A these are the bits the column update gives -- and V's
//   rotation needs no other lane.  No LDS, no scratch.
//   The 3 x 3 Jacobi of the rank-2 step and the denormalisation run redundantly in every lane.  The mask is written once, after
//   the last round; lane 0 rewrites the record in place.
#include "hak_internal.h"
#include "geom_common.h"

#define FR_SWEEPS9 8
#define FR_SWEEPS3 6
#define FR_MIN_INLIERS 8
#define FR_REFINED_ROOT 3

// v of lane `lane` in every lane; `lane` is wave-uniform (a constant after unrolling)
__device__ __forceinline__ double fr_lane(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// rotation (p, q) of the lane-distributed 9 x 9 problem: A = this lane's row `row` of A, V = its row of V
__device__ __forceinline__ void fr_rotate9(double (&A)[9], double (&V)[9], const int row, const int p, const int q)
{
    const double apq = fr_lane(A[q], p);
    if (apq == 0.0) return;                                         // (wave-uniform)
    const double app = fr_lane(A[p], p), aqq = fr_lane(A[q], q);
    double t, c, sn;
    fr_angle(app, aqq, apq, t, c, sn);
    const bool isp = row == p, isq = row == q;
    const double x = A[p], y = A[q];                                // A[row][p], A[row][q]
#pragma unroll
    for (int k = 0; k < 9; k++) {
        if (k == p || k == q) continue;
        const double bp = fr_lane(A[k], p), bq = fr_lane(A[k], q);  // A[p][k] = A[k][p], A[q][k] = A[k][q]
        const double rp = c * bp - sn * bq, rq = sn * bp + c * bq;
        A[k] = isp ? rp : (isq ? rq : A[k]);
    }
    const double np = c * x - sn * y, nq = sn * x + c * y;
    A[p] = isp ? app - t * apq : (isq ? 0.0 : np);
    A[q] = isp ? 0.0 : (isq ? aqq + t * apq : nq);
    const double vp = V[p], vq = V[q];
    V[p] = c * vp - sn * vq;
    V[q] = sn * vp + c * vq;
}

// jacobi(N, 9, 8) of the rule: Nf = the 45 upper-triangle entries, row-major, the same in every lane; f = the eigenvector in
// every lane
__device__ void fr_jacobi9(const double Nf[45], double f[9])
{
    const int row = threadIdx.x < 9 ? threadIdx.x : 0;
    double A[9], V[9];
#pragma unroll
    for (int j = 0; j < 9; j++) { A[j] = 0.0; V[j] = row == j ? 1.0 : 0.0; }
    {
        int k = 0;
#pragma unroll
        for (int p = 0; p < 9; p++)
#pragma unroll
            for (int q = p; q < 9; q++, k++) {
                A[q] = row == p ? Nf[k] : A[q];                     // N[p][q] to lane p
                A[p] = row == q ? Nf[k] : A[p];                     // and its mirror to lane q
            }
    }
#pragma unroll 1
    for (int sweep = 0; sweep < FR_SWEEPS9; sweep++)
#pragma unroll
        for (int p = 0; p < 8; p++)
#pragma unroll
            for (int q = p + 1; q < 9; q++) fr_rotate9(A, V, row, p, q);
    int best = 0;
    double dbest = fr_lane(A[0], 0);
#pragma unroll
    for (int j = 1; j < 9; j++) {
        const double d = fr_lane(A[j], j);
        if (d < dbest) { dbest = d; best = j; }
    }
    double col = V[0];
#pragma unroll
    for (int j = 1; j < 9; j++) col = best == j ? V[j] : col;       // V[row][best]
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = fr_lane(col, k);
}

// jacobi(G, 3, 6) of the rule, every lane the whole problem; G is destroyed
__device__ void fr_jacobi3(double G[3][3], double v[3])
{
    double V[3][3];
    fd_jacobi3(G, V, FR_SWEEPS3);
    const int best = fd_jacobi3_smallest(G);
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = best == 0 ? V[i][0] : (best == 1 ? V[i][1] : V[i][2]);
}

// inliers of F over the pair (every lane returns the total)
__device__ int fr_count_inliers(const hak_match_pair* m, int n, const float F[9], float t2)
{
    int c = 0;
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) c += fd_inlier(F, fd_load(m, i), t2) ? 1 : 0;
    return hg_wsum(c);
}

// steps 1-7 of the rule up to the scoring, from the model F: *cnt = the inliers of F; true and R = the refitted model, false
// when the round fails.  Every lane computes the same.
__device__ bool fr_round(const hak_match_pair* m, int n, const float F[9], float t2, int* cnt, float R[9])
{
    const int l = threadIdx.x;
    int c = 0;
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
    for (int i = l; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!fd_inlier(F, r, t2)) continue;
        c++;
        sx1 = sx1 + (double)r.x; sy1 = sy1 + (double)r.y; sx2 = sx2 + (double)r.z; sy2 = sy2 + (double)r.w;
    }
    c = hg_wsum(c);
    *cnt = c;
    if (c < FR_MIN_INLIERS) return false;
    const double mm = (double)c;
    const double c1x = hg_wsum(sx1) / mm, c1y = hg_wsum(sy1) / mm, c2x = hg_wsum(sx2) / mm, c2y = hg_wsum(sy2) / mm;
    double q1 = 0.0, q2 = 0.0;
    for (int i = l; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!fd_inlier(F, r, t2)) continue;
        const double dx1 = (double)r.x - c1x, dy1 = (double)r.y - c1y, dx2 = (double)r.z - c2x, dy2 = (double)r.w - c2y;
        q1 = q1 + (dx1 * dx1 + dy1 * dy1);
        q2 = q2 + (dx2 * dx2 + dy2 * dy2);
    }
    q1 = hg_wsum(q1);
    q2 = hg_wsum(q2);
    const double s1 = sqrt((2.0 * mm) / q1), s2 = sqrt((2.0 * mm) / q2);
    if (!(q1 > 0.0 && q2 > 0.0 && __builtin_isfinite(s1) && __builtin_isfinite(s2))) return false;
    double N[45];
#pragma unroll
    for (int k = 0; k < 45; k++) N[k] = 0.0;
    for (int i = l; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!fd_inlier(F, r, t2)) continue;
        const double x = s1 * ((double)r.x - c1x), y = s1 * ((double)r.y - c1y);
        const double u = s2 * ((double)r.z - c2x), v = s2 * ((double)r.w - c2y);
        const double w[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int k = 0;
#pragma unroll
        for (int p = 0; p < 9; p++)
#pragma unroll
            for (int q = p; q < 9; q++, k++) N[k] = N[k] + w[p] * w[q];
    }
#pragma unroll
    for (int k = 0; k < 45; k++) N[k] = hg_wsum(N[k]);
    double Fn[9];
    fr_jacobi9(N, Fn);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && __builtin_isfinite(Fn[k]);
    if (!ok) return false;
    // rank 2: subtract the smallest singular triplet, v = the eigenvector of Fn^T Fn's smallest eigenvalue
    double G[3][3], v[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = (Fn[i] * Fn[j] + Fn[3 + i] * Fn[3 + j]) + Fn[6 + i] * Fn[6 + j];
    fr_jacobi3(G, v);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double g = (Fn[3 * i] * v[0] + Fn[3 * i + 1] * v[1]) + Fn[3 * i + 2] * v[2];
#pragma unroll
        for (int j = 0; j < 3; j++) Fn[3 * i + j] = Fn[3 * i + j] - g * v[j];
    }
    // step 6 of hak_find_fundamental
    const double T1[9] = {s1, 0.0, -(s1 * c1x), 0.0, s1, -(s1 * c1y), 0.0, 0.0, 1.0};
    const double T2t[9] = {s2, 0.0, 0.0, 0.0, s2, 0.0, -(s2 * c2x), -(s2 * c2y), 1.0};
    double H[9], D[9];
    fd_mul3(Fn, T1, H);
    fd_mul3(T2t, H, D);
    double d = D[0];
#pragma unroll
    for (int k = 1; k < 9; k++) d = fabs(D[k]) > fabs(d) ? D[k] : d;
    ok = d != 0.0 && __builtin_isfinite(d);
#pragma unroll
    for (int k = 0; k < 9; k++) { R[k] = (float)(D[k] / d); ok = ok && __builtin_isfinite(R[k]); }
    return ok;
}

__global__ __launch_bounds__(HAK_WAVE) void k_fund_refit(const hak_match_pair* __restrict__ base, long stride,
                                                         const int* __restrict__ counts, int n_host, int rounds, float t2,
                                                         hak_fundamental* inout, unsigned char* __restrict__ masks,
                                                         long mask_stride)
{
    const int pair = blockIdx.x, l = threadIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, n_host, stride);
    const hak_fundamental in = inout[pair];
    float cur[9];
    bool model = in.hypothesis >= 0;
#pragma unroll
    for (int k = 0; k < 9; k++) { cur[k] = in.F[k]; model = model && __builtin_isfinite(cur[k]); }
    int cnt = 0, root = in.root;
    if (model) {
#pragma unroll 1
        for (int r = 0; r < rounds; r++) {
            float R[9];
            if (!fr_round(m, n, cur, t2, &cnt, R)) break;
            const int c = fr_count_inliers(m, n, R, t2);
            if (c < cnt) break;
#pragma unroll
            for (int k = 0; k < 9; k++) cur[k] = R[k];
            cnt = c;
            root = FR_REFINED_ROOT;
        }
    }
    if (masks) {
        unsigned char* mk = masks + (long)pair * mask_stride;
        for (int i = l; i < n; i += HAK_WAVE) mk[i] = (model && fd_inlier(cur, fd_load(m, i), t2)) ? 1 : 0;
    }
    if (l == 0) {
        hak_fundamental o;
#pragma unroll
        for (int k = 0; k < 9; k++) o.F[k] = model ? cur[k] : 0.0f;
        o.inliers = model ? cnt : 0; o.hypothesis = model ? in.hypothesis : -1; o.root = model ? root : 0; o.n = n;
        inout[pair] = o;
    }
}

// the record of a hak_refine_fundamental call that has no context: a device global, so that the call allocates nothing
__device__ hak_fundamental g_refit_record;

hak_fundamental* hak_fundamental_refit_record()
{
    void* p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(g_refit_record)) == hipSuccess ? static_cast<hak_fundamental*>(p) : nullptr;
}

void hak_launch_fundamental_refit(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host,
                                  int npairs, float threshold, int rounds, hak_fundamental* inout, unsigned char* masks,
                                  long mask_stride)
{
    k_fund_refit<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, rounds, threshold * threshold, inout, masks,
                                              mask_stride);
}

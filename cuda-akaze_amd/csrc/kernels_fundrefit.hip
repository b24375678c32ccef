// kernels_fundrefit.hip -- rank-2 least-squares refit of a fundamental matrix over its inliers, iterated (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_refine_fundamental) so that the numpy reference
// tests/fundamental_refit_ref.py agrees bit for bit: per round the inliers of the current F, Hartley normalisation and the 45
// upper-triangle sums of the 9 x 9 normal matrix in the homography refit's summation order, the eigenvector of its smallest
// eigenvalue by eight sweeps of cyclic Jacobi, the closest rank-2 matrix by a 3 x 3 Jacobi, denormalisation and float32 Sampson
// re-scoring; the round is kept when it scores at least as well.  float64, + - * / sqrt only; the file is built with
// -ffp-contract=off: no FMA is formed, so every rounding is the one the reference makes.
//
// k_fund_refit: one wave per pair, refit_record of refit_common.h: the record's check, the round loop, the mask (written once, after
//   the last round) and the record (lane 0 rewrites it in place) are that header's, as are the pieces of a round it shares with the
//   homography's and the pose's.  fr_refit::round is this rule's round:
//   Three streaming passes over the list (rf_hartley's count and centroids, then scales; the 45 sums in registers by rf_tri_add),
//   each closed by the xor butterfly, so every lane holds the same normal matrix.
//   The 9 x 9 Jacobi is a chain of 288 dependent rotations.  Lane k < 9 owns row k of A and row k of V in registers (the other
//   lanes shadow lane 0); the (p, q) loops are fully unrolled, so every register index and every lane number is a compile-time
//   constant.  A rotation reads A[p][p], A[q][q], A[p][q] and rows p and q from lanes p and q with v_readlane (17 64-bit lane
//   reads), every lane computes t, c and sn redundantly, lane k updates its entries of columns p and q, lanes p and q rebuild
//   their own rows from the two broadcast rows -- by the symmetry of A these are the bits the column update gives -- and V's
//   rotation needs no other lane.  No LDS, no scratch.
//   The 3 x 3 Jacobi of the rank-2 step and the denormalisation run redundantly in every lane.
#include "refit_common.h"

#define FR_SWEEPS9 8
#define FR_SWEEPS3 6

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

// the refit scaffold's view (refit_common.h)
struct fr_refit : fd_est {
    static constexpr int MIN_INLIERS = 8, REFINED = 3;              // REFINED: hak_fundamental.root of a refitted record
    __device__ bool round(const hak_match_pair* m, int n, const float F[9], int* cnt, float R[9]) const;
};

// steps 1-7 of the rule up to the scoring, from the model F: *cnt = the inliers of F; true and R = the refitted model, false
// when the round fails.  Every lane computes the same.
__device__ bool fr_refit::round(const hak_match_pair* m, int n, const float F[9], int* cnt, float R[9]) const
{
    const rf_norm h = rf_hartley(*this, m, n, F);
    *cnt = h.m;
    if (h.m < MIN_INLIERS) return false;
    const double s1 = h.s1, s2 = h.s2, c1x = h.c1x, c1y = h.c1y, c2x = h.c2x, c2y = h.c2y;
    if (!(h.q1 > 0.0 && h.q2 > 0.0 && __builtin_isfinite(s1) && __builtin_isfinite(s2))) return false;
    double N[45];
    rf_tri_zero(N);
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) {
        const float4 r = fd_load(m, i);
        if (!inlier(F, r)) continue;
        const double x = s1 * ((double)r.x - c1x), y = s1 * ((double)r.y - c1y);
        const double u = s2 * ((double)r.z - c2x), v = s2 * ((double)r.w - c2y);
        const double w[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        rf_tri_add<9>(N, w);
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
    const int pair = blockIdx.x;
    refit_record(fr_refit{{{}, t2}}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), rounds, inout, masks,
                 mask_stride);
}

// the one record of the synchronous one-list calls that own none (hak_internal.h): a device global, so such a call allocates nothing
__device__ __attribute__((aligned(16))) char g_shared_record[HAK_REC_BYTES];

void* hak_shared_record()
{
    void* p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(g_shared_record)) == hipSuccess ? p : nullptr;
}

void hak_launch_fundamental_refit(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host,
                                  int npairs, float threshold, int rounds, hak_fundamental* inout, unsigned char* masks,
                                  long mask_stride)
{
    k_fund_refit<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, rounds, threshold * threshold, inout, masks,
                                              mask_stride);
}

// kernels_pnp.hip -- track linking and RANSAC absolute pose (P3P) behind hak_recover_pose (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_link_tracks, hak_solve_pnp) so that the numpy references tests/link_ref.py and
// tests/pnp_ref.py agree byte for byte.  The file is built with -ffp-contract=off: no FMA is formed, so every rounding is the one
// the reference makes.
//
// Link: the table train -> smallest a of list A is cleared by a memset node (0x7F7F7F7F = none), then
// k_link_scatter: grid (pair, blocks over A), atomicMin of a into the table entry of A[a].train;
// k_link_gather: k_knn2_finish's shape, one 1024-thread block per pair walks B in chunks and appends a correspondence per linked
//   match at the running base through a ballot/popcount block scan: ascending m, deterministic.
//
// PnP, on the scaffold of ransac_common.h:
// k_pnp_models: grid (pair, hypothesis block of 64), one hypothesis per thread through the whole float64 solve (three points from 16
//   draws, Grunert's quartic, its critical points by fd_cubic_roots, up to four brackets of 64 bisections, a pose per root).
//   Output to the models scratch: the float32 models of solutions 0..3 (12 words each: R row-major, t) and the mask of the solutions
//   that gave one.
// k_pnp_score: rs_score_block on the hypothesis' up to four models read back from scratch; a chunk is staged as {X, Y, Z, u} + {v}
//   (20 KB).
// k_pnp_finish: rs_finish: one wave per pair reduces the slots, reads the winner's model back from scratch, writes the mask and the
//   record.
#include "pnp_common.h"          // pn_rec, pn_load, pn_inlier and the view pn_est: shared with the refit (kernels_pnprefit.hip)

#define LK_NONE 0x7F7F7F7F       // the table's cleared entry (memset byte 0x7F): above every index

__device__ __forceinline__ double pn_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void pn_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// step 5's triad of three points; false if a norm is 0 or non-finite
__device__ __forceinline__ bool pn_triad(const double P1[3], const double P2[3], const double P3[3], double e1[3], double e2[3],
                                         double e3[3])
{
    double d1[3], d2[3], nv[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { d1[i] = P2[i] - P1[i]; d2[i] = P3[i] - P1[i]; }
    const double l1 = sqrt(pn_dot(d1, d1));
#pragma unroll
    for (int i = 0; i < 3; i++) e1[i] = d1[i] / l1;
    pn_cross(d1, d2, nv);
    const double ln = sqrt(pn_dot(nv, nv));
#pragma unroll
    for (int i = 0; i < 3; i++) e3[i] = nv[i] / ln;
    pn_cross(e3, e1, e2);
    return __builtin_isfinite(l1) && l1 > 0.0 && __builtin_isfinite(ln) && ln > 0.0;
}

// the monic quartic (((v + b3) v + b2) v + b1) v + b0
__device__ __forceinline__ double pn_q(double v, double b3, double b2, double b1, double b0)
{
    return (((v + b3) * v + b2) * v + b1) * v + b0;
}

// hypothesis h of list `pair` with n correspondences, steps 1-5 of the rule: the float32 models of its solutions go to the models
// scratch (zeros where solution s gave none), returns the mask of the solutions that gave one (0 = degenerate)
__device__ int pn_hypothesis(const hak_corr3d* c, int n, const hak_intrinsics K, unsigned seed, int h, unsigned* models, int pair,
                             int iterations)
{
    int valid = 0, nsol = 0;
    bool ok = n >= 3;
    int idx[3];
    ok = ok && rs_sample<3, 16>(seed, h, n, idx);
    if (ok) {
        const double fx = K.fx, fy = K.fy, cx = K.cx, cy = K.cy;
        double X[3][3], b[3][3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const pn_rec r = pn_load(c, idx[q]);
            X[q][0] = r.a.x; X[q][1] = r.a.y; X[q][2] = r.a.z;
            const double x = ((double)r.a.w - cx) / fx, y = ((double)r.v - cy) / fy;
            const double nrm = sqrt((x * x + y * y) + 1.0);
            b[q][0] = x / nrm; b[q][1] = y / nrm; b[q][2] = 1.0 / nrm;
        }
        double da[3], db[3], dc[3];
#pragma unroll
        for (int i = 0; i < 3; i++) { da[i] = X[1][i] - X[2][i]; db[i] = X[0][i] - X[2][i]; dc[i] = X[0][i] - X[1][i]; }
        const double a2 = pn_dot(da, da), b2 = pn_dot(db, db), c2 = pn_dot(dc, dc);
        const double ca = pn_dot(b[1], b[2]), cb = pn_dot(b[0], b[2]), cg = pn_dot(b[0], b[1]);
        ok = b2 != 0.0 && __builtin_isfinite(a2) && __builtin_isfinite(b2) && __builtin_isfinite(c2) && __builtin_isfinite(ca) &&
             __builtin_isfinite(cb) && __builtin_isfinite(cg);
        // step 3
        const double p = (a2 - c2) / b2, q = (a2 + c2) / b2;
        const double rab = a2 / b2, rcb = c2 / b2, rbc = (b2 - c2) / b2, rba = (b2 - a2) / b2;
        const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
        const double pm = p - 1.0, pp = p * p, pq = 1.0 + p;
        const double A4 = pm * pm - 4.0 * (rcb * ca2);
        const double A3 = 4.0 * (((p * (1.0 - p)) * cb - ((1.0 - q) * ca) * cg) + 2.0 * ((rcb * ca2) * cb));
        const double A2 = 2.0 * (((((pp - 1.0) + 2.0 * (pp * cb2)) + 2.0 * (rbc * ca2)) - 4.0 * (((q * ca) * cb) * cg)) + 2.0 * (rba * cg2));
        const double A1 = 4.0 * (((-(p * pq)) * cb + 2.0 * ((rab * cg2) * cb)) - ((1.0 - q) * ca) * cg);
        const double A0 = pq * pq - 4.0 * (rab * cg2);
        ok = ok && A4 != 0.0 && __builtin_isfinite(A4) && __builtin_isfinite(A3) && __builtin_isfinite(A2) && __builtin_isfinite(A1) &&
             __builtin_isfinite(A0);
        // step 4
        const double b3 = A3 / A4, bb2 = A2 / A4, b1 = A1 / A4, b0 = A0 / A4;
        double mx = fabs(b3);
        if (fabs(bb2) > mx) mx = fabs(bb2);
        if (fabs(b1) > mx) mx = fabs(b1);
        if (fabs(b0) > mx) mx = fabs(b0);
        const double bound = 1.0 + mx;
        ok = ok && __builtin_isfinite(b3) && __builtin_isfinite(bb2) && __builtin_isfinite(b1) && __builtin_isfinite(b0) &&
             __builtin_isfinite(bound);
        double crit[3];
        int ccount = 0;
        ok = fd_cubic_roots(0.75 * b3, 0.5 * bb2, 0.25 * b1, crit, &ccount) && ok;
        double f1[3], f2[3], f3[3];
        ok = pn_triad(X[0], X[1], X[2], f1, f2, f3) && ok;
        if (ok) {
            // the bracket ends: 0, the critical points inside (0, bound) in order, bound (selects, no dynamic register indexing)
            double pt1 = bound, pt2 = bound, pt3 = bound;
            int m = 1;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double cr = crit[r];
                const bool keep = r < ccount && cr > 0.0 && cr < bound;
                pt1 = (keep && m == 1) ? cr : pt1;
                pt2 = (keep && m == 2) ? cr : pt2;
                pt3 = (keep && m == 3) ? cr : pt3;
                m += keep ? 1 : 0;
            }
#pragma unroll 1
            for (int j = 0; j < m; j++) {
                double lo = j == 0 ? 0.0 : (j == 1 ? pt1 : (j == 2 ? pt2 : pt3));
                double hi = j == 0 ? pt1 : (j == 1 ? pt2 : (j == 2 ? pt3 : bound));
                const bool neg = pn_q(lo, b3, bb2, b1, b0) < 0.0;
                if (neg == (pn_q(hi, b3, bb2, b1, b0) < 0.0)) continue;
#pragma unroll 1
                for (int it = 0; it < 64; it++) {
                    const double mid = 0.5 * (lo + hi);
                    const bool left = (pn_q(mid, b3, bb2, b1, b0) < 0.0) == neg;
                    lo = left ? mid : lo;
                    hi = left ? hi : mid;
                }
                const double v = 0.5 * (lo + hi);
                // step 5
                const double vv = v * v;
                const double den = 2.0 * (cg - v * ca);
                const double w = (1.0 + vv) - (2.0 * v) * cb;
                const double u = ((pm * vv - ((2.0 * p) * cb) * v) + pq) / den;
                const double s1 = sqrt(b2 / w);
                const double s2 = u * s1, s3 = v * s1;
                bool good = den != 0.0 && w > 0.0 && __builtin_isfinite(s1) && s1 > 0.0 && __builtin_isfinite(s2) && s2 > 0.0 &&
                            __builtin_isfinite(s3) && s3 > 0.0;
                double P1[3], P2[3], P3[3], e1[3], e2[3], e3[3];
#pragma unroll
                for (int i = 0; i < 3; i++) { P1[i] = s1 * b[0][i]; P2[i] = s2 * b[1][i]; P3[i] = s3 * b[2][i]; }
                good = pn_triad(P1, P2, P3, e1, e2, e3) && good;
                float M[12];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    double R[3];
#pragma unroll
                    for (int jj = 0; jj < 3; jj++) R[jj] = (e1[i] * f1[jj] + e2[i] * f2[jj]) + e3[i] * f3[jj];
                    const double t = P1[i] - pn_dot(R, X[0]);
#pragma unroll
                    for (int jj = 0; jj < 3; jj++) M[3 * i + jj] = (float)R[jj];
                    M[9 + i] = (float)t;
                }
#pragma unroll
                for (int q2 = 0; q2 < 12; q2++) good = good && __builtin_isfinite(M[q2]);
#pragma unroll
                for (int q2 = 0; q2 < 12; q2++) M[q2] = good ? M[q2] : 0.0f;
                rs_write_model<pn_est>(models, pair, iterations, h, nsol, M);
                valid |= good ? 1 << nsol : 0;
                nsol++;
            }
        }
    }
    const float none[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = nsol; s < 4; s++) rs_write_model<pn_est>(models, pair, iterations, h, s, none);
    return valid;
}

__global__ __launch_bounds__(RS_MTHREADS) void k_pnp_models(const hak_corr3d* __restrict__ base, long stride,
                                                            const int* __restrict__ counts, int n_host, hak_intrinsics K,
                                                            int iterations, unsigned seed, unsigned* __restrict__ models)
{
    const int pair = blockIdx.x;
    const int h = blockIdx.y * RS_MTHREADS + threadIdx.x;
    if (h >= iterations) return;
    const hak_corr3d* c = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    rs_write_valid<pn_est>(models, pair, iterations, h, pn_hypothesis(c, n, K, seed, h, models, pair, iterations));
}

__global__ __launch_bounds__(RS_THREADS) void k_pnp_score(const hak_corr3d* __restrict__ base, long stride,
                                                          const int* __restrict__ counts, int n_host, hak_intrinsics K,
                                                          int iterations, int hp, float t2, const unsigned* __restrict__ models,
                                                          unsigned long long* __restrict__ slots)
{
    const int pair = blockIdx.x;
    float M[4][12];
    const int valid = rs_read_models<pn_est>(models, pair, iterations, rs_block_hypothesis(hp), M);
    rs_score_block(pn_est{K, t2}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), hp, M, valid, slots);
}

__global__ __launch_bounds__(HAK_WAVE) void k_pnp_finish(const hak_corr3d* __restrict__ base, long stride,
                                                         const int* __restrict__ counts, int n_host, hak_intrinsics K, int iterations,
                                                         int hblocks, float t2, const unsigned* __restrict__ models,
                                                         const unsigned long long* __restrict__ slots,
                                                         hak_abs_pose* __restrict__ out, unsigned char* __restrict__ masks,
                                                         long mask_stride)
{
    const int pair = blockIdx.x;
    rs_finish(pn_est{K, t2}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), iterations, hblocks, models, slots,
              out, masks, mask_stride);
}

long hak_pnp_words(int npairs, int iterations) { return (long)npairs * rs_words<pn_est>() * iterations; }

void hak_launch_pnp(hipStream_t st, const hak_corr3d* corr, long stride, const int* counts, int n_host, int npairs,
                    const hak_intrinsics& K, int iterations, float threshold, unsigned seed, unsigned* models,
                    unsigned long long* slots, hak_abs_pose* out, unsigned char* masks, long mask_stride)
{
    int hp = 0;
    const int hblocks = hak_homography_blocks(npairs, iterations, &hp);
    const float t2 = threshold * threshold;
    k_pnp_models<<<dim3(npairs, (iterations + RS_MTHREADS - 1) / RS_MTHREADS), RS_MTHREADS, 0, st>>>(corr, stride, counts, n_host, K,
                                                                                                    iterations, seed, models);
    k_pnp_score<<<dim3(npairs, hblocks), RS_THREADS, 0, st>>>(corr, stride, counts, n_host, K, iterations, hp, t2, models, slots);
    k_pnp_finish<<<npairs, HAK_WAVE, 0, st>>>(corr, stride, counts, n_host, K, iterations, hblocks, t2, models, slots, out, masks,
                                              mask_stride);
}

// ------------------------------------------------------------------------------------------------------------------ link
__device__ __forceinline__ int lk_count(const int* counts, int pair, int step, int n_host, long cap)
{
    long n = counts ? counts[(long)pair * step] : n_host;
    return (int)(n < 0 ? 0 : (n > cap ? cap : n));
}

__global__ __launch_bounds__(256) void k_link_scatter(const hak_match_pair* __restrict__ A_base, long strideA,
                                                      const int* __restrict__ countsA, int stepA, int nA_host,
                                                      const unsigned char* __restrict__ masks, int max_index, int* __restrict__ table)
{
    const int pair = blockIdx.x;
    const hak_match_pair* A = A_base + (long)pair * strideA;
    const unsigned char* mk = masks ? masks + (long)pair * strideA : nullptr;
    const int nA = lk_count(countsA, pair, stepA, nA_host, strideA);
    int* tab = table + (long)pair * max_index;
    for (int a = blockIdx.y * 256 + threadIdx.x; a < nA; a += gridDim.y * 256) {
        const int tr = A[a].train;
        if (tr >= 0 && tr < max_index && (!mk || mk[a] != 0)) atomicMin(tab + tr, a);
    }
}

__global__ __launch_bounds__(1024) void k_link_gather(const hak_match_pair* __restrict__ B_base, long strideB,
                                                      const int* __restrict__ countsB, int stepB, int nB_host,
                                                      const float* __restrict__ xyz_base, long strideA, int max_index,
                                                      const int* __restrict__ table, hak_corr3d* __restrict__ out_base,
                                                      long out_stride, int* __restrict__ out_count)
{
    __shared__ int wsum[16];
    __shared__ int sbase;
    const int pair = blockIdx.x;
    const hak_match_pair* B = B_base + (long)pair * strideB;
    const float* xyz = xyz_base + 3 * (long)pair * strideA;
    const int nB = lk_count(countsB, pair, stepB, nB_host, strideB < out_stride ? strideB : out_stride);
    const int* tab = table + (long)pair * max_index;
    hak_corr3d* out = out_base + (long)pair * out_stride;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) sbase = 0;
    __syncthreads();
    for (int m0 = 0; m0 < nB; m0 += 1024) {
        const int m = m0 + threadIdx.x;
        int a = LK_NONE;
        float4 tail = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < nB) {
            const int q = B[m].query;
            tail = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(B + m) + 16);
            if (q >= 0 && q < max_index) a = tab[q];
        }
        const bool ok = a != LK_NONE;
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        int before = sbase;
        for (int t = 0; t < wv; t++) before += wsum[t];
        if (ok) {
            const float* p = xyz + 3 * (long)a;
            float4* o = reinterpret_cast<float4*>(out + before + __popcll(bal & ((1ull << lane) - 1ull)));
            o[0] = make_float4(p[0], p[1], p[2], tail.z);
            o[1] = make_float4(tail.w, __int_as_float(a), __int_as_float(m), __int_as_float(0));
        }
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int t = 0; t < 16; t++) tot += wsum[t]; sbase += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out_count[pair] = sbase;
}

void hak_launch_link(hipStream_t st, const hak_match_pair* A, long strideA, const int* countsA, int stepA, int nA_host,
                     const unsigned char* masksA, const float* xyzA, const hak_match_pair* B, long strideB, const int* countsB,
                     int stepB, int nB_host, int npairs, int max_index, int* table, hak_corr3d* out, long out_stride, int* out_counts)
{
    (void)hipMemsetAsync(table, 0x7F, sizeof(int) * (size_t)npairs * (size_t)max_index, st);
    long most = countsA ? strideA : nA_host;
    int blocks = (int)((most + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 64 ? 64 : blocks);
    k_link_scatter<<<dim3(npairs, blocks), 256, 0, st>>>(A, strideA, countsA, stepA, nA_host, masksA, max_index, table);
    k_link_gather<<<npairs, 1024, 0, st>>>(B, strideB, countsB, stepB, nB_host, xyzA, strideA, max_index, table, out, out_stride,
                                           out_counts);
}

// kernels_fundamental.hip -- RANSAC fundamental matrix over the match lists of hak_match_knn2(_batch) (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_find_fundamental) so that the numpy reference tests/fundamental_ref.py
// agrees bit for bit: the counter-based sample generator of the homography (splitmix64 of seed, hypothesis and draw; seven
// points from 32 draws), a float64 seven-point solve (Hartley normalisation, a 7 x 9 elimination with row pivoting on fixed
// pivot columns, the cubic det(a A + B) = 0 solved by bracketing and 64 bisections: + - * / sqrt only) and float32 Sampson
// scoring in one fixed expression.  No refit.  The file is built with -ffp-contract=off: no FMA is formed, so every rounding
// is the one the reference makes.
//
// k_fund_models: grid (pair, hypothesis block of 64), one hypothesis per thread through the whole float64 solve.  The 7 x 9
//   system lives in registers: every loop over it is unrolled with compile-time indices, a row swap is a chain of selects.
//   Output to the models scratch of ransac_common.h: the float32 models of roots 0, 1, 2 (9 words each) and the mask of the roots
//   that gave one.
// k_fund_score: rs_score_block on the hypothesis' up to three models read back from scratch.
// k_fund_finish: rs_finish: one wave per pair reduces the slots, reads the winner's model back from scratch, writes the mask and
//   the record.
// The Sampson test fd_inlier is in geom_common.h, the scaffold's view fd_est in ransac_common.h.
#include "ransac_common.h"

__device__ __forceinline__ double fd_det(const double m[9])
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// det of P with row i taken from Q
__device__ __forceinline__ double fd_det_row(const double P[9], const double Q[9], int i)
{
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = (k / 3 == i) ? Q[k] : P[k];
    return fd_det(m);
}

// Hartley normalisation of seven points, in place: centroid (cx, cy), s = sqrt(14 / sum r^2); false if the sum is 0 or s is
// non-finite
__device__ __forceinline__ bool fd_normalise(double x[7], double y[7], double& cx, double& cy, double& s)
{
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) { sx = sx + x[k]; sy = sy + y[k]; }
    cx = sx / 7.0;
    cy = sy / 7.0;
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        x[k] = x[k] - cx;
        y[k] = y[k] - cy;
        q = q + (x[k] * x[k] + y[k] * y[k]);
    }
    s = sqrt(14.0 / q);
#pragma unroll
    for (int k = 0; k < 7; k++) { x[k] = s * x[k]; y[k] = s * y[k]; }
    return q != 0.0 && __builtin_isfinite(s);
}

// hypothesis h of a pair with n matches, steps 1-6 of the rule: up to three float32 models to Fo[3][9], returns the mask of
// the roots that gave one (0 = degenerate)
__device__ int fd_hypothesis(const hak_match_pair* m, int n, unsigned seed, int h, float Fo[3][9])
{
    if (n < 7) return 0;
    int idx[7];
    if (!rs_sample<7, 32>(seed, h, n, idx)) return 0;
    double x[7], y[7], u[7], v[7];
#pragma unroll
    for (int q = 0; q < 7; q++) {
        const float4 r = fd_load(m, idx[q]);
        x[q] = r.x; y[q] = r.y; u[q] = r.z; v[q] = r.w;
    }
    double cx1, cy1, s1, cx2, cy2, s2;
    const bool ok1 = fd_normalise(x, y, cx1, cy1, s1);
    const bool ok2 = fd_normalise(u, v, cx2, cy2, s2);
    if (!(ok1 && ok2)) return 0;
    double M[7][9];
#pragma unroll
    for (int q = 0; q < 7; q++) {
        M[q][0] = u[q] * x[q]; M[q][1] = u[q] * y[q]; M[q][2] = u[q];
        M[q][3] = v[q] * x[q]; M[q][4] = v[q] * y[q]; M[q][5] = v[q];
        M[q][6] = x[q]; M[q][7] = y[q]; M[q][8] = 1.0;
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        int piv = c;
        double best = fabs(M[c][c]);
#pragma unroll
        for (int r = c + 1; r < 7; r++) {
            const double a = fabs(M[r][c]);
            if (a > best) { best = a; piv = r; }
        }
        ok = ok && best > 0.0 && __builtin_isfinite(best);
#pragma unroll
        for (int r = c + 1; r < 7; r++) {                           // (selects, no dynamic register indexing)
            const bool sw = r == piv;
#pragma unroll
            for (int q = c; q < 9; q++) {
                const double a = M[c][q], b = M[r][q];
                M[c][q] = sw ? b : a;
                M[r][q] = sw ? a : b;
            }
        }
#pragma unroll
        for (int r = c + 1; r < 7; r++) {
            const double f = M[r][c] / M[c][c];
#pragma unroll
            for (int q = c + 1; q < 9; q++) M[r][q] = M[r][q] - f * M[c][q];
        }
    }
    if (!ok) return 0;
    double A[9], B[9];
    A[7] = 1.0; A[8] = 0.0; B[7] = 0.0; B[8] = 1.0;
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double acc = -M[i][7], bcc = -M[i][8];
#pragma unroll
        for (int j = i + 1; j < 7; j++) { acc = acc - M[i][j] * A[j]; bcc = bcc - M[i][j] * B[j]; }
        A[i] = acc / M[i][i];
        B[i] = bcc / M[i][i];
    }
    const double c3 = fd_det(A), c0 = fd_det(B);
    const double c2 = (fd_det_row(A, B, 0) + fd_det_row(A, B, 1)) + fd_det_row(A, B, 2);
    const double c1 = (fd_det_row(B, A, 0) + fd_det_row(B, A, 1)) + fd_det_row(B, A, 2);
    if (!(c3 != 0.0) || !__builtin_isfinite(c3) || !__builtin_isfinite(c2) || !__builtin_isfinite(c1) || !__builtin_isfinite(c0))
        return 0;
    const double b2 = c2 / c3, b1 = c1 / c3, b0 = c0 / c3;
    double av[3];
    int count;
    if (!fd_cubic_roots(b2, b1, b0, av, &count)) return 0;
    const double T1[9] = {s1, 0.0, -(s1 * cx1), 0.0, s1, -(s1 * cy1), 0.0, 0.0, 1.0};
    const double T2t[9] = {s2, 0.0, 0.0, 0.0, s2, 0.0, -(s2 * cx2), -(s2 * cy2), 1.0};
    int valid = 0;
#pragma unroll 1
    for (int r = 0; r < 3; r++) {
        const double a = r == 0 ? av[0] : (r == 1 ? av[1] : av[2]);
        double Fn[9], G[9], F[9];
#pragma unroll
        for (int q = 0; q < 9; q++) Fn[q] = a * A[q] + B[q];
        fd_mul3(Fn, T1, G);
        fd_mul3(T2t, G, F);
        double d = F[0];
#pragma unroll
        for (int q = 1; q < 9; q++) d = fabs(F[q]) > fabs(d) ? F[q] : d;
        bool good = r < count && d != 0.0 && __builtin_isfinite(d);
        float f[9];
#pragma unroll
        for (int q = 0; q < 9; q++) { f[q] = (float)(F[q] / d); good = good && __builtin_isfinite(f[q]); }
#pragma unroll
        for (int q = 0; q < 9; q++) {
            const float w = good ? f[q] : 0.0f;
            if (r == 0) Fo[0][q] = w; else if (r == 1) Fo[1][q] = w; else Fo[2][q] = w;
        }
        valid |= good ? 1 << r : 0;
    }
    return valid;
}

__global__ __launch_bounds__(RS_MTHREADS) void k_fund_models(const hak_match_pair* __restrict__ base, long stride,
                                                             const int* __restrict__ counts, int n_host, int iterations,
                                                             unsigned seed, unsigned* __restrict__ models)
{
    const int pair = blockIdx.x;
    const int h = blockIdx.y * RS_MTHREADS + threadIdx.x;
    if (h >= iterations) return;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    float F[3][9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 9; q++) F[r][q] = 0.0f;
    const int valid = fd_hypothesis(m, n, seed, h, F);
#pragma unroll
    for (int r = 0; r < 3; r++) rs_write_model<fd_est>(models, pair, iterations, h, r, F[r]);
    rs_write_valid<fd_est>(models, pair, iterations, h, valid);
}

__global__ __launch_bounds__(RS_THREADS) void k_fund_score(const hak_match_pair* __restrict__ base, long stride,
                                                           const int* __restrict__ counts, int n_host, int iterations, int hp,
                                                           float t2, const unsigned* __restrict__ models,
                                                           unsigned long long* __restrict__ slots)
{
    const int pair = blockIdx.x;
    float F[3][9];
    const int valid = rs_read_models<fd_est>(models, pair, iterations, rs_block_hypothesis(hp), F);
    rs_score_block(fd_est{{}, t2}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), hp, F, valid, slots);
}

__global__ __launch_bounds__(HAK_WAVE) void k_fund_finish(const hak_match_pair* __restrict__ base, long stride,
                                                          const int* __restrict__ counts, int n_host, int iterations, int hblocks,
                                                          float t2, const unsigned* __restrict__ models,
                                                          const unsigned long long* __restrict__ slots,
                                                          hak_fundamental* __restrict__ out, unsigned char* __restrict__ masks,
                                                          long mask_stride)
{
    const int pair = blockIdx.x;
    rs_finish(fd_est{{}, t2}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), iterations, hblocks, models, slots,
              out, masks, mask_stride);
}

long hak_fundamental_words(int npairs, int iterations) { return (long)npairs * rs_words<fd_est>() * iterations; }

void hak_launch_fundamental(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                            int iterations, float threshold, unsigned seed, unsigned* models, unsigned long long* slots,
                            hak_fundamental* out, unsigned char* masks, long mask_stride)
{
    int hp = 0;
    const int hblocks = hak_homography_blocks(npairs, iterations, &hp);
    const float t2 = threshold * threshold;
    k_fund_models<<<dim3(npairs, (iterations + RS_MTHREADS - 1) / RS_MTHREADS), RS_MTHREADS, 0, st>>>(matches, stride, counts, n_host,
                                                                                                      iterations, seed, models);
    k_fund_score<<<dim3(npairs, hblocks), RS_THREADS, 0, st>>>(matches, stride, counts, n_host, iterations, hp, t2, models, slots);
    k_fund_finish<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, iterations, hblocks, t2, models, slots, out, masks,
                                               mask_stride);
}

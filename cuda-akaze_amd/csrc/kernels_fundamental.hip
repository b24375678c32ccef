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
//   Output to context scratch, word-major so that both kernels touch it coalesced: words [pair][w][iterations], w = 0..26 the
//   float32 models of roots 0, 1, 2 (9 each), w = 27 a mask of the roots that gave a model (bit r = root r).
// k_fund_score: k_hom_score's shape: grid (pair, hypothesis block), 256 threads; a block owns `hp` hypotheses (16 .. 256) and
//   256 / hp match slices; the pair's records stream through LDS in chunks of FD_CHUNK float4 {x1, y1, x2, y2}.  A thread
//   counts the inliers of its hypothesis' up to three models; each block writes its best key
//   (inliers << 32 | ~(4 h + root), 0 = none) to its own slot [pair][block]: no atomics and nothing to clear before a call.
// k_fund_finish: one wave per pair: reduces the slots, reads the winner's model back from scratch, writes the mask and the
//   record.
#include "hak_internal.h"
#include "geom_common.h"

#define FD_CHUNK 1024            // records per LDS chunk: 16 KB, so that several blocks share a CU
#define FD_THREADS 256
#define FD_MTHREADS 64           // k_fund_models: one wave per block (1024 hypotheses of one pair spread over 16 CUs)
#define FD_WORDS 28              // scratch words per hypothesis
#define FD_DRAWS 32

__device__ __forceinline__ unsigned long long fd_mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

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
    int i0 = -1, i1 = -1, i2 = -1, i3 = -1, i4 = -1, i5 = -1, i6 = -1, k = 0;
#pragma unroll 1
    for (int d = 0; d < FD_DRAWS && k < 7; d++) {
        const unsigned long long r =
            fd_mix64((unsigned long long)seed + (unsigned long long)(FD_DRAWS * (unsigned)h + d + 1) * 0x9E3779B97F4A7C15ull);
        const int j = (int)(((r >> 32) * (unsigned long long)n) >> 32);
        if (j != i0 && j != i1 && j != i2 && j != i3 && j != i4 && j != i5) {
            if (k == 0) i0 = j; else if (k == 1) i1 = j; else if (k == 2) i2 = j; else if (k == 3) i3 = j;
            else if (k == 4) i4 = j; else if (k == 5) i5 = j; else i6 = j;
            k++;
        }
    }
    if (k < 7) return 0;
    const int idx[7] = {i0, i1, i2, i3, i4, i5, i6};
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

__global__ __launch_bounds__(FD_MTHREADS) void k_fund_models(const hak_match_pair* __restrict__ base, long stride,
                                                             const int* __restrict__ counts, int n_host, int iterations,
                                                             unsigned seed, unsigned* __restrict__ models)
{
    const int pair = blockIdx.x;
    const int h = blockIdx.y * FD_MTHREADS + threadIdx.x;
    if (h >= iterations) return;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, n_host, stride);
    float F[3][9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 9; q++) F[r][q] = 0.0f;
    const int valid = fd_hypothesis(m, n, seed, h, F);
    unsigned* o = models + (long)pair * FD_WORDS * iterations + h;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 9; q++) o[(long)(9 * r + q) * iterations] = __float_as_uint(F[r][q]);
    o[(long)27 * iterations] = (unsigned)valid;
}

__global__ __launch_bounds__(FD_THREADS) void k_fund_score(const hak_match_pair* __restrict__ base, long stride,
                                                           const int* __restrict__ counts, int n_host, int iterations, int hp,
                                                           float t2, const unsigned* __restrict__ models,
                                                           unsigned long long* __restrict__ slots)
{
    __shared__ float4 rec[FD_CHUNK];
    __shared__ int part[3][FD_THREADS];
    __shared__ unsigned long long wbest[FD_THREADS / HAK_WAVE];
    const int pair = blockIdx.x, t = threadIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, n_host, stride);
    const int h = blockIdx.y * hp + (t & (hp - 1));
    const int slice = t / hp, nslice = FD_THREADS / hp;
    float F0[9], F1[9], F2[9];
    int valid = 0;
    if (h < iterations) {
        const unsigned* o = models + (long)pair * FD_WORDS * iterations + h;
        valid = (int)o[(long)27 * iterations];
#pragma unroll
        for (int q = 0; q < 9; q++) {
            F0[q] = __uint_as_float(o[(long)q * iterations]);
            F1[q] = __uint_as_float(o[(long)(9 + q) * iterations]);
            F2[q] = __uint_as_float(o[(long)(18 + q) * iterations]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 9; q++) F0[q] = F1[q] = F2[q] = 0.0f;
    }
    int c0 = 0, c1 = 0, c2 = 0;
    for (int b0 = 0; b0 < n; b0 += FD_CHUNK) {
        const int len = min(FD_CHUNK, n - b0);
        __syncthreads();                                            // the previous chunk is consumed
        for (int j = t; j < len; j += FD_THREADS) rec[j] = fd_load(m, b0 + j);
        __syncthreads();
        if (valid) {
#pragma unroll 2
            for (int j = slice; j < len; j += nslice) {
                const float4 r = rec[j];
                c0 += fd_inlier(F0, r, t2) ? 1 : 0;
                c1 += fd_inlier(F1, r, t2) ? 1 : 0;
                c2 += fd_inlier(F2, r, t2) ? 1 : 0;
            }
        }
    }
    part[0][t] = c0; part[1][t] = c1; part[2][t] = c2;
    __syncthreads();
    unsigned long long key = 0;
    if (t < hp) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            int s = 0;
            for (int k = 0; k < nslice; k++) s += part[r][t + k * hp];
            const unsigned long long kr = ((unsigned long long)s << 32) | (unsigned)~(4u * (unsigned)h + (unsigned)r);
            if ((valid >> r & 1) && kr > key) key = kr;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    if ((t & (HAK_WAVE - 1)) == 0) wbest[t / HAK_WAVE] = key;
    __syncthreads();
    if (t == 0) {
        unsigned long long b = wbest[0];
#pragma unroll
        for (int w = 1; w < FD_THREADS / HAK_WAVE; w++) b = wbest[w] > b ? wbest[w] : b;
        slots[(long)pair * gridDim.y + blockIdx.y] = b;
    }
}

__global__ __launch_bounds__(HAK_WAVE) void k_fund_finish(const hak_match_pair* __restrict__ base, long stride,
                                                          const int* __restrict__ counts, int n_host, int iterations, int hblocks,
                                                          float t2, const unsigned* __restrict__ models,
                                                          const unsigned long long* __restrict__ slots,
                                                          hak_fundamental* __restrict__ out, unsigned char* __restrict__ masks,
                                                          long mask_stride)
{
    const int pair = blockIdx.x, l = threadIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, n_host, stride);
    unsigned long long key = 0;
    for (int k = l; k < hblocks; k += HAK_WAVE) {
        const unsigned long long v = slots[(long)pair * hblocks + k];
        key = v > key ? v : key;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int inl = 0, hyp = -1, root = 0;
    if (key != 0) {
        const unsigned id = ~(unsigned)key;                         // 4 h + root, h < iterations: its model is in scratch
        hyp = (int)(id >> 2);
        root = (int)(id & 3u);
        inl = (int)(key >> 32);
        const unsigned* o = models + (long)pair * FD_WORDS * iterations + hyp;
#pragma unroll
        for (int q = 0; q < 9; q++) F[q] = __uint_as_float(o[(long)(9 * root + q) * iterations]);
    }
    if (masks) {
        unsigned char* mk = masks + (long)pair * mask_stride;
        for (int i = l; i < n; i += HAK_WAVE) mk[i] = (hyp >= 0 && fd_inlier(F, fd_load(m, i), t2)) ? 1 : 0;
    }
    if (l == 0) {
        hak_fundamental o;
#pragma unroll
        for (int q = 0; q < 9; q++) o.F[q] = F[q];
        o.inliers = inl; o.hypothesis = hyp; o.root = root; o.n = n;
        out[pair] = o;
    }
}

long hak_fundamental_words(int npairs, int iterations) { return (long)npairs * FD_WORDS * iterations; }

void hak_launch_fundamental(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                            int iterations, float threshold, unsigned seed, unsigned* models, unsigned long long* slots,
                            hak_fundamental* out, unsigned char* masks, long mask_stride)
{
    int hp = 0;
    const int hblocks = hak_homography_blocks(npairs, iterations, &hp);
    const float t2 = threshold * threshold;
    k_fund_models<<<dim3(npairs, (iterations + FD_MTHREADS - 1) / FD_MTHREADS), FD_MTHREADS, 0, st>>>(matches, stride, counts, n_host,
                                                                                                      iterations, seed, models);
    k_fund_score<<<dim3(npairs, hblocks), FD_THREADS, 0, st>>>(matches, stride, counts, n_host, iterations, hp, t2, models, slots);
    k_fund_finish<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, iterations, hblocks, t2, models, slots, out, masks,
                                               mask_stride);
}

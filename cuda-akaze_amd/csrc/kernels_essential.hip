// kernels_essential.hip -- five-point RANSAC essential matrix over the match lists of hak_match_knn2(_batch) (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_find_essential) so that the numpy reference tests/essential_ref.py agrees bit
// for bit: the counter-based sample generator of the other estimators (five points from 32 draws), Nister's five-point solver in
// float64 (bearings, a 5 x 9 elimination with complete pivoting, the mixed null-space basis, the ten cubic constraints, a 10 x 10
// Gauss-Jordan, det B(z) of degree 10, its real roots by a derivative chain of bisections, three Newton steps per root: + - * /
// only) and the float32 Sampson scoring of the fundamental matrix.  The file is built with -ffp-contract=off: no FMA is formed, so
// every rounding is the one the reference makes.
//
// k_ess_models: grid (pair, block of six hypotheses), one wave; ten lanes per hypothesis, lanes 60..63 idle.  One thread cannot hold
//   the 10 x 20 float64 constraint matrix, so lane q of a hypothesis builds and owns row q (20 doubles): the four null vectors lie in
//   LDS, where the row's (i, j) may index them; the Gauss-Jordan broadcasts the scaled pivot row with __shfl and moves no row; in the
//   root stage lane q owns bracket q of every derivative level (ten levels of 64 bisections, not 55 brackets in turn); lane q then
//   finishes the model of bracket q.  The 5 x 9 elimination and det B(z) are small and every lane of the hypothesis repeats them, which
//   costs a wave nothing.  Every lane runs every step with fixed trip counts and carries a flag, so the wave never diverges around a
//   shuffle.  All register arrays are indexed by compile-time values.
//   Output to the models scratch of ransac_common.h as three VIRTUAL hypotheses 3 h + g per hypothesis h, g = 0..2, of four models
//   each: model r (0..9, the roots in ascending order) is model r mod 4 of virtual hypothesis 3 h + r / 4, so that the scaffold's key
//   4 (3 h + g) + r' = 12 h + r keeps its order and ransac_common.h stays as it is.  Slots 10 and 11 never hold a model.
// k_ess_score: rs_score_block over 3 * iterations virtual hypotheses.
// k_ess_finish: one wave per pair reduces the slots, decodes h = h' / 3, r = 4 (h' mod 3) + r', reads the winner back from scratch
//   and writes the mask and the hak_fundamental record with root = 16 + r.
#include "ransac_common.h"

#define ES_LANES 10              // lanes per hypothesis
#define ES_GROUPS 6              // hypotheses per wave
#define ES_POLISH 3              // Newton steps per root
#define ES_ROOT_BASE 16          // hak_fundamental.root = 16 + r

// the scaffold's view: the fundamental matrix's record, test and staging with four models per (virtual) hypothesis
struct es_est : fd_est {
    static constexpr int NM = 4;
};

// monomials over v = (x, y, z, 1): degree 2 as the pairs i <= j and degree 3 as the triples i <= j <= k, both in lexicographic order
__device__ __forceinline__ constexpr int es_m2(int i, int j)
{
    constexpr int T[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    return T[i][j];
}
// (pair a) * v_k
__device__ __forceinline__ constexpr int es_m3(int a, int k)
{
    constexpr int T[10][4] = {{0, 1, 2, 3},     {1, 4, 5, 6},     {2, 5, 7, 8},     {3, 6, 8, 9},     {4, 10, 11, 12},
                              {5, 11, 13, 14},  {6, 12, 14, 15},  {7, 13, 16, 17},  {8, 14, 17, 18},  {9, 15, 18, 19}};
    return T[a][k];
}
// column c of the constraint matrix (x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1) in that order
__device__ __forceinline__ constexpr int es_nister(int c)
{
    constexpr int T[20] = {0, 10, 1, 4, 2, 3, 11, 12, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 19};
    return T[c];
}
__device__ __forceinline__ constexpr double es_binom(int n, int k)
{
    double b = 1.0;
    for (int i = 1; i <= k; i++) b = b * (double)(n - k + i) / (double)i;   // exact: every prefix is a binomial coefficient
    return b;
}

// out += a * b, linear times linear, in ascending (i, j)
__device__ __forceinline__ void es_pmul11(double out[10], const double a[4], const double b[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) out[es_m2(i, j)] = out[es_m2(i, j)] + a[i] * b[j];
}

// out += A * b, quadratic times linear, in ascending (a, k)
__device__ __forceinline__ void es_pmul21(double out[20], const double A[10], const double b[4])
{
#pragma unroll
    for (int a = 0; a < 10; a++)
#pragma unroll
        for (int k = 0; k < 4; k++) out[es_m3(a, k)] = out[es_m3(a, k)] + A[a] * b[k];
}

// the null vectors of one hypothesis in LDS: [X', Y', Z', W][9]
typedef double es_null[4][9];

// entry (i, j) of E as a polynomial over (x, y, z, 1); i and j may be run-time values
__device__ __forceinline__ void es_entry(const es_null& N, int i, int j, double e[4])
{
#pragma unroll
    for (int v = 0; v < 4; v++) e[v] = N[v][3 * i + j];
}

// a b - c d of four entries of E
__device__ __forceinline__ void es_minor(const es_null& N, int ai, int aj, int bi, int bj, int ci, int cj, int di, int dj, double out[10])
{
    double a[4], b[4], p[10], q[10];
#pragma unroll
    for (int k = 0; k < 10; k++) p[k] = q[k] = 0.0;
    es_entry(N, ai, aj, a);
    es_entry(N, bi, bj, b);
    es_pmul11(p, a, b);
    es_entry(N, ci, cj, a);
    es_entry(N, di, dj, b);
    es_pmul11(q, a, b);
#pragma unroll
    for (int k = 0; k < 10; k++) out[k] = p[k] - q[k];
}

// row 0: det E
__device__ __forceinline__ void es_row_det(const es_null& N, double row[20])
{
    double c[10], e[4];
    es_minor(N, 1, 1, 2, 2, 1, 2, 2, 1, c);
    es_entry(N, 0, 0, e);
    es_pmul21(row, c, e);
    es_minor(N, 1, 2, 2, 0, 1, 0, 2, 2, c);
    es_entry(N, 0, 1, e);
    es_pmul21(row, c, e);
    es_minor(N, 1, 0, 2, 1, 1, 1, 2, 0, c);
    es_entry(N, 0, 2, e);
    es_pmul21(row, c, e);
}

// L[i][k] = sum over l of E[i][l] E[k][l]
__device__ __forceinline__ void es_gram(const es_null& N, int i, int k, double L[10])
{
#pragma unroll
    for (int m = 0; m < 10; m++) L[m] = 0.0;
#pragma unroll
    for (int l = 0; l < 3; l++) {
        double a[4], b[4];
        es_entry(N, i, l, a);
        es_entry(N, k, l, b);
        es_pmul11(L, a, b);
    }
}

// row 1 + 3 i + j: entry (i, j) of 2 E E^T E - tr(E E^T) E = sum over k of A[i][k] E[k][j], A = 2 L - tr(L) I
__device__ __forceinline__ void es_row_trace(const es_null& N, int i, int j, double row[20])
{
    double t[10], L[10];
    {
        double L1[10], L2[10];
        es_gram(N, 0, 0, L);
        es_gram(N, 1, 1, L1);
        es_gram(N, 2, 2, L2);
#pragma unroll
        for (int m = 0; m < 10; m++) t[m] = (L[m] + L1[m]) + L2[m];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double e[4];
        es_gram(N, i, k, L);
#pragma unroll
        for (int m = 0; m < 10; m++) L[m] = i == k ? 2.0 * L[m] - t[m] : 2.0 * L[m];
        es_entry(N, k, j, e);
        es_pmul21(row, L, e);
    }
}

// polynomial product, coefficients ascending: out[i + j] += a[i] * b[j] in ascending (i, j), from 0
template <int NA, int NB>
__device__ __forceinline__ void es_conv(const double (&a)[NA], const double (&b)[NB], double (&out)[NA + NB - 1])
{
#pragma unroll
    for (int k = 0; k < NA + NB - 1; k++) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; i++)
#pragma unroll
        for (int j = 0; j < NB; j++) out[i + j] = out[i + j] + a[i] * b[j];
}

// a b - c d of polynomials
template <int NA, int NB>
__device__ __forceinline__ void es_conv_diff(const double (&a)[NA], const double (&b)[NB], const double (&c)[NB], const double (&d)[NA],
                                             double (&out)[NA + NB - 1])
{
    double p[NA + NB - 1], q[NA + NB - 1];
    es_conv(a, b, p);
    es_conv(c, d, q);
#pragma unroll
    for (int k = 0; k < NA + NB - 1; k++) out[k] = p[k] - q[k];
}

// ((a_d z + a_(d-1)) z + ..) + a_0
template <int NA>
__device__ __forceinline__ double es_horner(const double (&a)[NA], double z)
{
    double acc = a[NA - 1];
#pragma unroll
    for (int k = NA - 2; k >= 0; k--) acc = acc * z + a[k];
    return acc;
}

// the derivative's coefficients
template <int NA>
__device__ __forceinline__ void es_derive(const double (&a)[NA], double (&d)[NA - 1])
{
#pragma unroll
    for (int k = 1; k < NA; k++) d[k - 1] = (double)k * a[k];
}

// one row of B(z): the polynomials in front of x, y and 1, and their derivatives
struct es_brow {
    double x[4], y[4], o[5];
    // e - z f of the right halves (xz^2 xz x yz^2 yz y z^3 z^2 z 1) of two reduced rows
    __device__ __forceinline__ void set(const double e[10], const double f[10])
    {
        x[0] = e[2]; x[1] = e[1] - f[2]; x[2] = e[0] - f[1]; x[3] = -f[0];
        y[0] = e[5]; y[1] = e[4] - f[5]; y[2] = e[3] - f[4]; y[3] = -f[3];
        o[0] = e[9]; o[1] = e[8] - f[9]; o[2] = e[7] - f[8]; o[3] = e[6] - f[7]; o[4] = -f[6];
    }
    __device__ __forceinline__ void at(double z, double v[3]) const
    {
        v[0] = es_horner(x, z); v[1] = es_horner(y, z); v[2] = es_horner(o, z);
    }
    // the row's residual at (x, y, z) and its gradient
    __device__ __forceinline__ void newton(double px, double py, double z, double& r, double J[3]) const
    {
        double dx[3], dy[3], dz[4], v[3];
        es_derive(x, dx);
        es_derive(y, dy);
        es_derive(o, dz);
        at(z, v);
        r = (v[0] * px + v[1] * py) + v[2];
        J[0] = v[0];
        J[1] = v[1];
        J[2] = (es_horner(dx, z) * px + es_horner(dy, z) * py) + es_horner(dz, z);
    }
};

__device__ __forceinline__ double es_det(const double m[9])
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// level D of the derivative chain: a_j = C(j + s, s) b[j + s], s = 10 - D, the (10 - D)-th derivative over (10 - D)!.  Lane q < D
// owns bracket q: [q == 0 ? -bound : the point of lane q - 1, q == D - 1 ? bound : its own point]; its new point is the root, or
// the bracket's upper end if the ends do not differ in sign.
template <int D>
__device__ __forceinline__ void es_level(const double (&b)[11], double bound, int lane, int q, double& pt, bool& has)
{
    constexpr int s = 10 - D;
    double a[D + 1];
#pragma unroll
    for (int j = 0; j <= D; j++) a[j] = es_binom(j + s, s) * b[j + s];
    const double below = __shfl(pt, lane - 1);
    double lo = q == 0 ? -bound : below;
    double hi = q < D - 1 ? pt : bound;
    if (q >= D) lo = hi = bound;
    const double top = hi;
    const bool neg = es_horner(a, lo) < 0.0;
    has = neg != (es_horner(a, hi) < 0.0);
#pragma unroll 1
    for (int it = 0; it < 64; it++) {
        const double mid = 0.5 * (lo + hi);
        const bool left = (es_horner(a, mid) < 0.0) == neg;
        lo = left ? mid : lo;
        hi = left ? hi : mid;
    }
    pt = has ? 0.5 * (lo + hi) : top;
}

__global__ __launch_bounds__(RS_MTHREADS) void k_ess_models(const hak_match_pair* __restrict__ base, long stride,
                                                            const int* __restrict__ counts, int n_host, int iterations,
                                                            unsigned seed, hak_intrinsics K1, hak_intrinsics K2,
                                                            unsigned* __restrict__ models)
{
    __shared__ es_null nsp[ES_GROUPS + 1];                          // (+ 1: lanes 60..63 run the same code on a row of their own)
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int g = lane / ES_LANES, q = lane - ES_LANES * g, gb = ES_LANES * g;
    const int h = blockIdx.y * ES_GROUPS + g;
    const bool live = g < ES_GROUPS && h < iterations;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    const double fx1 = K1.fx, fy1 = K1.fy, cx1 = K1.cx, cy1 = K1.cy, fx2 = K2.fx, fy2 = K2.fy, cx2 = K2.cx, cy2 = K2.cy;

    // steps 1-3, every lane of the hypothesis alike: sample, bearings, the 5 x 9 elimination with complete pivoting
    int idx[5];
    bool ok = live && n >= 5;
    ok = rs_sample<5, 32>(seed, live ? h : 0, ok ? n : 0, idx) && ok;
    double M[5][9];
#pragma unroll
    for (int p = 0; p < 5; p++) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) r = fd_load(m, idx[p]);
        const double x = ((double)r.x - cx1) / fx1, y = ((double)r.y - cy1) / fy1;
        const double u = ((double)r.z - cx2) / fx2, v = ((double)r.w - cy2) / fy2;
        ok = ok && __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(u) && __builtin_isfinite(v);
        M[p][0] = u * x; M[p][1] = u * y; M[p][2] = u;
        M[p][3] = v * x; M[p][4] = v * y; M[p][5] = v;
        M[p][6] = x; M[p][7] = y; M[p][8] = 1.0;
    }
    int perm[9];
#pragma unroll
    for (int p = 0; p < 9; p++) perm[p] = p;
#pragma unroll
    for (int c = 0; c < 5; c++) {
        int pr = c, pc = c;
        double best = fabs(M[c][c]);
#pragma unroll
        for (int r = c; r < 5; r++)
#pragma unroll
            for (int p = c; p < 9; p++) {
                const double a = fabs(M[r][p]);
                if (a > best) { best = a; pr = r; pc = p; }
            }
        ok = ok && best > 0.0 && __builtin_isfinite(best);
#pragma unroll
        for (int r = c + 1; r < 5; r++) {                           // (selects, no dynamic register indexing)
            const bool sw = r == pr;
#pragma unroll
            for (int p = c; p < 9; p++) {
                const double a = M[c][p], b = M[r][p];
                M[c][p] = sw ? b : a;
                M[r][p] = sw ? a : b;
            }
        }
#pragma unroll
        for (int p = c + 1; p < 9; p++) {
            const bool sw = p == pc;
#pragma unroll
            for (int r = 0; r < 5; r++) {
                const double a = M[r][c], b = M[r][p];
                M[r][c] = sw ? b : a;
                M[r][p] = sw ? a : b;
            }
            const int a = perm[c], b = perm[p];
            perm[c] = sw ? b : a;
            perm[p] = sw ? a : b;
        }
#pragma unroll
        for (int r = c + 1; r < 5; r++) {
            const double f = M[r][c] / M[c][c];
#pragma unroll
            for (int p = c + 1; p < 9; p++) M[r][p] = M[r][p] - f * M[c][p];
        }
    }
    {
        // four null vectors by back substitution, the identity on the free columns 5..8, then the mix; lane k writes vector k
        double f[4][9];
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int j = 0; j < 4; j++) f[k][5 + j] = j == k ? 1.0 : 0.0;
#pragma unroll
            for (int i = 4; i >= 0; i--) {
                double acc = -M[i][5 + k];
#pragma unroll
                for (int j = i + 1; j < 5; j++) acc = acc - M[i][j] * f[k][j];
                f[k][i] = acc / M[i][i];
            }
        }
        const double mix[3] = {1.125, -0.625, 0.875};
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int p = 0; p < 9; p++) f[k][p] = f[k][p] - mix[k] * f[3][p];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (q == k) {
#pragma unroll
                for (int p = 0; p < 9; p++) nsp[g][k][perm[p]] = f[k][p];
            }
    }
    __syncthreads();
    const es_null& N = nsp[g];

    // step 4: lane q builds row q of the constraints and the ten lanes run the Gauss-Jordan on the left 10 x 10 block
    double row[20];
    {
        double lex[20];
#pragma unroll
        for (int k = 0; k < 20; k++) lex[k] = 0.0;
        if (q == 0) es_row_det(N, lex);
        else es_row_trace(N, (q - 1) / 3, (q - 1) % 3, lex);
#pragma unroll
        for (int c = 0; c < 20; c++) row[c] = lex[es_nister(c)];
    }
    bool used = false;
    int owner[10];
#pragma unroll
    for (int c = 0; c < 10; c++) {
        // the pivot of column c: the largest |entry| among the rows that hold no pivot yet, ties to the smallest row
        const double mine = used ? -2.0 : fabs(row[c]);
        double best = -1.0;
        int piv = 0;
#pragma unroll
        for (int r = 0; r < ES_LANES; r++) {
            const double a = __shfl(mine, gb + r);
            if (a > best) { best = a; piv = r; }
        }
        ok = ok && best > 0.0 && __builtin_isfinite(best);
        used = used || q == piv;
        owner[c] = piv;
        const double f = row[c], p = row[c];
#pragma unroll
        for (int k = c + 1; k < 20; k++) {
            const double v = __shfl(row[k] / p, gb + piv);
            row[k] = q == piv ? v : row[k] - f * v;
        }
    }

    // step 5: B(z) from the rows of x^2z, x^2, y^2z, y^2, xyz, xy, and det B(z)
    es_brow B[3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
        double e[10], f[10];
#pragma unroll
        for (int k = 0; k < 10; k++) {
            e[k] = __shfl(row[10 + k], gb + owner[4 + 2 * s]);
            f[k] = __shfl(row[10 + k], gb + owner[5 + 2 * s]);
        }
        B[s].set(e, f);
    }
    double b[11];
    {
        double c0[8], c1[8], c2[7], t0[11], t1[11], t2[11];
        es_conv_diff(B[1].y, B[2].o, B[1].o, B[2].y, c0);
        es_conv_diff(B[1].o, B[2].x, B[1].x, B[2].o, c1);
        es_conv_diff(B[1].x, B[2].y, B[1].y, B[2].x, c2);
        es_conv(B[0].x, c0, t0);
        es_conv(B[0].y, c1, t1);
        es_conv(B[0].o, c2, t2);
#pragma unroll
        for (int k = 0; k < 11; k++) b[k] = (t0[k] + t1[k]) + t2[k];
    }

    // step 6: monic, the bound, the derivative chain
    ok = ok && b[10] != 0.0;
#pragma unroll
    for (int k = 0; k < 11; k++) ok = ok && __builtin_isfinite(b[k]);
    const double lead = b[10];
#pragma unroll
    for (int k = 0; k < 10; k++) b[k] = b[k] / lead;
    b[10] = 1.0;
    double mx = fabs(b[0]);
#pragma unroll
    for (int k = 1; k < 10; k++) mx = fabs(b[k]) > mx ? fabs(b[k]) : mx;
    const double bound = 1.0 + mx;
#pragma unroll
    for (int k = 0; k < 10; k++) ok = ok && __builtin_isfinite(b[k]);
    ok = ok && __builtin_isfinite(bound);
    double z = bound;
    bool has = false;
    es_level<1>(b, bound, lane, q, z, has);
    es_level<2>(b, bound, lane, q, z, has);
    es_level<3>(b, bound, lane, q, z, has);
    es_level<4>(b, bound, lane, q, z, has);
    es_level<5>(b, bound, lane, q, z, has);
    es_level<6>(b, bound, lane, q, z, has);
    es_level<7>(b, bound, lane, q, z, has);
    es_level<8>(b, bound, lane, q, z, has);
    es_level<9>(b, bound, lane, q, z, has);
    es_level<10>(b, bound, lane, q, z, has);
    has = has && ok;

    // step 7: lane q finishes the model of bracket q
    double x, y;
    bool good = has;
    {
        double r0[3], r1[3], r2[3];
        B[0].at(z, r0);
        B[1].at(z, r1);
        B[2].at(z, r2);
        // (x, y, 1) is orthogonal to the rows of B(z): the cross product of the pair of rows whose third component is largest
        double w = r0[0] * r1[1] - r0[1] * r1[0];
        double cx = r0[1] * r1[2] - r0[2] * r1[1], cy = r0[2] * r1[0] - r0[0] * r1[2];
        const double w02 = r0[0] * r2[1] - r0[1] * r2[0];
        const double cx02 = r0[1] * r2[2] - r0[2] * r2[1], cy02 = r0[2] * r2[0] - r0[0] * r2[2];
        if (fabs(w02) > fabs(w)) { w = w02; cx = cx02; cy = cy02; }
        const double w12 = r1[0] * r2[1] - r1[1] * r2[0];
        const double cx12 = r1[1] * r2[2] - r1[2] * r2[1], cy12 = r1[2] * r2[0] - r1[0] * r2[2];
        if (fabs(w12) > fabs(w)) { w = w12; cx = cx12; cy = cy12; }
        x = cx / w;
        y = cy / w;
        good = good && w != 0.0 && __builtin_isfinite(w);
    }
#pragma unroll 1
    for (int it = 0; it < ES_POLISH; it++) {
        // a Newton step on B(z) (x, y, 1)^T = 0 in (x, y, z), by Cramer's rule
        double r[3], J[9];
#pragma unroll
        for (int i = 0; i < 3; i++) B[i].newton(x, y, z, r[i], &J[3 * i]);
        const double det = es_det(J);
        const double Jx[9] = {r[0], J[1], J[2], r[1], J[4], J[5], r[2], J[7], J[8]};
        const double Jy[9] = {J[0], r[0], J[2], J[3], r[1], J[5], J[6], r[2], J[8]};
        const double Jz[9] = {J[0], J[1], r[0], J[3], J[4], r[1], J[6], J[7], r[2]};
        x = x - es_det(Jx) / det;
        y = y - es_det(Jy) / det;
        z = z - es_det(Jz) / det;
    }
    float f[9];
    {
        double E[9], G[9], F[9];
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = ((x * N[0][k] + y * N[1][k]) + z * N[2][k]) + N[3][k];
        const double K1i[9] = {1.0 / fx1, 0.0, -(cx1 / fx1), 0.0, 1.0 / fy1, -(cy1 / fy1), 0.0, 0.0, 1.0};
        const double K2it[9] = {1.0 / fx2, 0.0, 0.0, 0.0, 1.0 / fy2, 0.0, -(cx2 / fx2), -(cy2 / fy2), 1.0};
        fd_mul3(E, K1i, G);
        fd_mul3(K2it, G, F);
        double d = F[0];
#pragma unroll
        for (int k = 1; k < 9; k++) d = fabs(F[k]) > fabs(d) ? F[k] : d;
        good = good && d != 0.0 && __builtin_isfinite(d);
#pragma unroll
        for (int k = 0; k < 9; k++) { f[k] = (float)(F[k] / d); good = good && __builtin_isfinite(f[k]); }
#pragma unroll
        for (int k = 0; k < 9; k++) f[k] = good ? f[k] : 0.0f;
    }

    // roots are numbered in ascending bracket order: the model of bracket q is model r = the brackets with a root below q
    const unsigned hasm = (unsigned)(__ballot(has) >> gb) & 0x3ffu, goodm = (unsigned)(__ballot(good) >> gb) & 0x3ffu;
    const int r = __popc(hasm & ((1u << q) - 1u)), count = __popc(hasm);
    unsigned valid = 0;
    {
        int k = 0;
#pragma unroll
        for (int bq = 0; bq < ES_LANES; bq++) {
            valid |= (hasm >> bq & 1u) ? (goodm >> bq & 1u) << k : 0u;
            k += (int)(hasm >> bq & 1u);
        }
    }
    if (!live) return;
    const int vit = 3 * iterations;
    const float zero[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (has) rs_write_model<es_est>(models, pair, vit, 3 * h + (r >> 2), r & 3, f);
    if (q >= count) rs_write_model<es_est>(models, pair, vit, 3 * h + (q >> 2), q & 3, zero);
    if (q < 2) rs_write_model<es_est>(models, pair, vit, 3 * h + 2, 2 + q, zero);
    if (q < 3) rs_write_valid<es_est>(models, pair, vit, 3 * h + q, (int)(valid >> (4 * q) & 0xfu));
}

__global__ __launch_bounds__(RS_THREADS) void k_ess_score(const hak_match_pair* __restrict__ base, long stride,
                                                          const int* __restrict__ counts, int n_host, int iterations, int hp,
                                                          float t2, const unsigned* __restrict__ models,
                                                          unsigned long long* __restrict__ slots)
{
    const int pair = blockIdx.x;
    float F[4][9];
    const int valid = rs_read_models<es_est>(models, pair, 3 * iterations, rs_block_hypothesis(hp), F);
    rs_score_block(es_est{{{}, t2}}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), hp, F, valid, slots);
}

__global__ __launch_bounds__(HAK_WAVE) void k_ess_finish(const hak_match_pair* __restrict__ base, long stride,
                                                         const int* __restrict__ counts, int n_host, int iterations, int hblocks,
                                                         float t2, const unsigned* __restrict__ models,
                                                         const unsigned long long* __restrict__ slots,
                                                         hak_fundamental* __restrict__ out, unsigned char* __restrict__ masks,
                                                         long mask_stride)
{
    const int pair = blockIdx.x;
    float F[9];
    es_est::no_model(F);
    int inl, vh, rv, hyp = -1, tag = 0;
    if (rs_decode(rs_best_slot(slots, hblocks), inl, vh, rv)) {
        rs_read_model<es_est>(models, pair, 3 * iterations, vh, rv, F);
        hyp = vh / 3;
        tag = ES_ROOT_BASE + 4 * (vh % 3) + rv;
    }
    rs_write_result(es_est{{{}, t2}}, base + (long)pair * stride, fd_count(counts, pair, 1, n_host, stride), F, inl, hyp, tag, out,
                    masks, mask_stride);
}

long hak_essential_words(int npairs, int iterations) { return (long)npairs * rs_words<es_est>() * 3 * iterations; }
int hak_essential_blocks(int npairs, int iterations) { return hak_homography_blocks(npairs, 3 * iterations, nullptr); }

void hak_launch_essential(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                          const hak_intrinsics& K1, const hak_intrinsics& K2, int iterations, float threshold, unsigned seed,
                          unsigned* models, unsigned long long* slots, hak_fundamental* out, unsigned char* masks, long mask_stride)
{
    int hp = 0;
    const int hblocks = hak_homography_blocks(npairs, 3 * iterations, &hp);
    const float t2 = threshold * threshold;
    k_ess_models<<<dim3(npairs, (iterations + ES_GROUPS - 1) / ES_GROUPS), RS_MTHREADS, 0, st>>>(matches, stride, counts, n_host,
                                                                                                 iterations, seed, K1, K2, models);
    k_ess_score<<<dim3(npairs, hblocks), RS_THREADS, 0, st>>>(matches, stride, counts, n_host, iterations, hp, t2, models, slots);
    k_ess_finish<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, iterations, hblocks, t2, models, slots, out, masks,
                                              mask_stride);
}

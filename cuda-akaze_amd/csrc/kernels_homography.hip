// kernels_homography.hip -- RANSAC homography over the match lists of hak_match_knn2(_batch) (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_find_homography) so that the numpy reference tests/homography_ref.py
// agrees bit for bit: a counter-based sample generator (splitmix64 of seed, hypothesis and draw), a float64 closed-form solve
// through two square-to-quad maps, float32 scoring in one fixed expression, and a float64 least-squares refit whose sums have
// a fixed order (lane l of one wave takes matches i = l mod 64 in ascending i, then an xor butterfly over 32 .. 1).
// The file is built with -ffp-contract=off: no FMA is formed, so every rounding is the one the reference makes.
//
// k_hom_score: rs_score_block's shape (ransac_common.h) with one model per hypothesis: every thread draws and solves its hypothesis
//   in registers (no models kernel, no scratch), then the scaffold counts its inliers and writes the block's slot.
// k_hom_finish: one wave per pair: reduces the slots, re-derives the winner through the same device function and hands it to
//   refit_iterate (refit_common.h) for at most one round of hg_refit::round: refit, re-score, keep if not worse, mask and record.
//   The round's Hartley passes, normal equations and elimination are that header's; its rows and the denormalisation are here.
// The inlier test hg_inlier is in geom_common.h, the scaffold's view hg_est in ransac_common.h.
#include "refit_common.h"

// the closed-form map of the unit square (0,0) (1,0) (1,1) (0,1) onto the quad x[0..3], y[0..3] (Heckbert), S[8] = 1
__device__ __forceinline__ void hg_square_to_quad(const double x[4], const double y[4], double S[9])
{
    const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], dx3 = ((x[0] - x[1]) + x[2]) - x[3];
    const double dy1 = y[1] - y[2], dy2 = y[3] - y[2], dy3 = ((y[0] - y[1]) + y[2]) - y[3];
    const double den = dx1 * dy2 - dx2 * dy1;
    const double g = (dx3 * dy2 - dx2 * dy3) / den;
    const double h = (dx1 * dy3 - dx3 * dy1) / den;
    S[0] = (x[1] - x[0]) + g * x[1]; S[1] = (x[3] - x[0]) + h * x[3]; S[2] = x[0];
    S[3] = (y[1] - y[0]) + g * y[1]; S[4] = (y[3] - y[0]) + h * y[3]; S[5] = y[0];
    S[6] = g; S[7] = h; S[8] = 1.0;
}

// divide by [2][2] and round to float32 with H[8] = 1; false if [2][2] is 0 or anything is non-finite
__device__ __forceinline__ bool hg_to_float(const double F[9], float H[9])
{
    const double d = F[8];
    if (!(d != 0.0) || !__builtin_isfinite(d)) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) { H[k] = (float)(F[k] / d); ok = ok && __builtin_isfinite(H[k]); }
    H[8] = 1.0f;
    return ok;
}

__device__ __forceinline__ double hg_cross(const double x[4], const double y[4], int a, int b, int c)
{
    return (x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a]);
}

// hypothesis h of a pair with n matches: false when it is degenerate (no four distinct indices within 16 draws, a triple with
// |cross| <= 1 px^2 or a flipped orientation in either image, a non-finite or singular solve)
__device__ bool hg_hypothesis(const hak_match_pair* m, int n, unsigned seed, int h, float H[9])
{
    if (n < 4) return false;
    int idx[4];
    if (!rs_sample<4, 16>(seed, h, n, idx)) return false;
    double ax[4], ay[4], bx[4], by[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 r = fd_load(m, idx[q]);
        ax[q] = r.x; ay[q] = r.y; bx[q] = r.z; by[q] = r.w;
    }
    const int T[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const double c1 = hg_cross(ax, ay, T[t][0], T[t][1], T[t][2]);
        const double c2 = hg_cross(bx, by, T[t][0], T[t][1], T[t][2]);
        if (!(fabs(c1) > 1.0 && fabs(c2) > 1.0 && ((c1 > 0.0) == (c2 > 0.0)))) return false;   // (NaN fails)
    }
    double S1[9], S2[9], A[9], F[9];
    hg_square_to_quad(ax, ay, S1);
    hg_square_to_quad(bx, by, S2);
    // adj(S1)
    A[0] = S1[4] * S1[8] - S1[5] * S1[7]; A[1] = S1[2] * S1[7] - S1[1] * S1[8]; A[2] = S1[1] * S1[5] - S1[2] * S1[4];
    A[3] = S1[5] * S1[6] - S1[3] * S1[8]; A[4] = S1[0] * S1[8] - S1[2] * S1[6]; A[5] = S1[2] * S1[3] - S1[0] * S1[5];
    A[6] = S1[3] * S1[7] - S1[4] * S1[6]; A[7] = S1[1] * S1[6] - S1[0] * S1[7]; A[8] = S1[0] * S1[4] - S1[1] * S1[3];
    fd_mul3(S2, A, F);
    return hg_to_float(F, H);
}

// the refit scaffold's view (refit_common.h).  A round is the least-squares refit of H's inliers (one wave; every lane computes the
// same): Hartley normalisation, 8x8 normal equations with h22 = 1, Gaussian elimination with partial pivoting, all in float64.
// False below four inliers, when the system is singular or the result is not finite.
struct hg_refit : hg_est {
    static constexpr int MIN_INLIERS = 4, REFINED = 1;
    __device__ bool round(const hak_match_pair* m, int n, const float H[9], int* cnt, float R[9]) const
    {
        const rf_norm h = rf_hartley(*this, m, n, H);
        *cnt = h.m;
        if (h.m < MIN_INLIERS) return false;
        const double s1 = h.s1, s2 = h.s2, c1x = h.c1x, c1y = h.c1y, c2x = h.c2x, c2y = h.c2y;
        // rows a = [X, Y, 1, 0, 0, 0, -X U, -Y U] (target U), b = [0, 0, 0, X, Y, 1, -X V, -Y V] (target V); N = upper triangle of
        // sum a^T a + b^T b, row-major; g = sum a U + b V
        double N[36], g[8];
        rf_tri_zero(N);
        rf_tri_zero(g);
        for (int i = threadIdx.x; i < n; i += HAK_WAVE) {
            const float4 r = fd_load(m, i);
            if (!inlier(H, r)) continue;
            const double X = s1 * ((double)r.x - c1x), Y = s1 * ((double)r.y - c1y);
            const double U = s2 * ((double)r.z - c2x), V = s2 * ((double)r.w - c2y);
            const double a[8] = {X, Y, 1.0, 0.0, 0.0, 0.0, -(X * U), -(Y * U)};
            const double b[8] = {0.0, 0.0, 0.0, X, Y, 1.0, -(X * V), -(Y * V)};
            rf_tri_add<8>(N, a, b);
#pragma unroll
            for (int p = 0; p < 8; p++) g[p] = g[p] + (a[p] * U + b[p] * V);
        }
        double S[8][9], d[8], Hn[9];
        rf_system<8>(N, g, S);
        if (!rf_solve<8>(S, d)) return false;
#pragma unroll
        for (int k = 0; k < 8; k++) Hn[k] = d[k];
        Hn[8] = 1.0;
        const double is2 = 1.0 / s2;
        const double T1[9] = {s1, 0.0, -(s1 * c1x), 0.0, s1, -(s1 * c1y), 0.0, 0.0, 1.0};
        const double T2i[9] = {is2, 0.0, c2x, 0.0, is2, c2y, 0.0, 0.0, 1.0};
        double G[9], F[9];
        fd_mul3(Hn, T1, G);
        fd_mul3(T2i, G, F);
        return hg_to_float(F, R);
    }
};

__global__ __launch_bounds__(RS_THREADS) void k_hom_score(const hak_match_pair* __restrict__ base, long stride,
                                                          const int* __restrict__ counts, int n_host, int iterations, int hp,
                                                          float t2, unsigned seed, unsigned long long* __restrict__ slots)
{
    const int pair = blockIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    const int h = rs_block_hypothesis(hp);
    float H[1][9];
    const bool ok = h < iterations && hg_hypothesis(m, n, seed, h, H[0]);
    rs_score_block(hg_est{{}, t2}, m, n, hp, H, ok ? 1 : 0, slots);
}

__global__ __launch_bounds__(HAK_WAVE) void k_hom_finish(const hak_match_pair* __restrict__ base, long stride,
                                                         const int* __restrict__ counts, int n_host, int hblocks, float t2,
                                                         unsigned seed, int refine, const unsigned long long* __restrict__ slots,
                                                         hak_homography* __restrict__ out, unsigned char* __restrict__ masks,
                                                         long mask_stride)
{
    const int pair = blockIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    float H[9];
    hg_est::no_model(H);
    int inl, hyp, model;
    const bool has = rs_decode(rs_best_slot(slots, hblocks), inl, hyp, model);
    if (has) hg_hypothesis(m, n, seed, hyp, H);                     // non-degenerate: its key was written by the same function
    // one round at most, from the winner and its decoded count: the score kernel counted the same test on the same records
    refit_iterate(hg_refit{{{}, t2}}, m, n, refine ? 1 : 0, H, has, inl, hyp, 0, out, masks, mask_stride);
}

// hypotheses per score block: the largest power of two in 16 .. 256 that still gives >= 64 blocks over all pairs (a single pair
// with 1024 hypotheses: 64 blocks of 16; 256 pairs: 4 blocks of 256 per pair)
int hak_homography_blocks(int npairs, int iterations, int* hp_out)
{
    int hp = 256;
    while (hp > 16 && (long)npairs * ((iterations + hp - 1) / hp) < 64) hp >>= 1;
    if (hp_out) *hp_out = hp;
    return (iterations + hp - 1) / hp;
}

void hak_launch_homography(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                           int iterations, float threshold, unsigned seed, int refine, unsigned long long* slots,
                           hak_homography* out, unsigned char* masks, long mask_stride)
{
    int hp = 0;
    const int hblocks = hak_homography_blocks(npairs, iterations, &hp);
    const float t2 = threshold * threshold;
    k_hom_score<<<dim3(npairs, hblocks), RS_THREADS, 0, st>>>(matches, stride, counts, n_host, iterations, hp, t2, seed, slots);
    k_hom_finish<<<npairs, HAK_WAVE, 0, st>>>(matches, stride, counts, n_host, hblocks, t2, seed, refine, slots, out, masks,
                                              mask_stride);
}

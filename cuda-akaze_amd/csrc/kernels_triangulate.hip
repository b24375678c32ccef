// kernels_triangulate.hip -- 3-D points of a match list under two known views (gfx950, wave64): the stage that carries the
// geometric chain past the third image.
//
// The semantics are fixed in include/hipakaze.h (hak_triangulate) so that the numpy reference tests/triangulate_ref.py agrees bit
// for bit: the two camera centres, per match the two bearings turned into the common frame, the least-squares two-ray solve in
// the form of step 5 of hak_recover_pose, a parallax gate, a depth gate, the midpoint of the common perpendicular rounded to
// float32, and the float32 reprojection test of hak_solve_pnp (pn_inlier) under both views.  float64, + - * / only, except where
// float32 is named; the file is built with -ffp-contract=off: no FMA is formed, so every rounding is the one the reference makes.
//
// k_triangulate: k_pose's launch shape, one block of TR_BLOCK threads (TR_WAVES waves) per list, one match per thread per step.
//   The per-block setup (the two views, their centres, the no-model test) is a few dozen operations on block-uniform values; every
//   lane computes it redundantly, so nothing is broadcast.  One pass: nothing about a match depends on the other matches, so the
//   list is streamed once, mask and point are written as they are decided, and four integer counters per lane (kept, and the
//   first gate failed) are closed by the xor butterfly per wave and one LDS row per wave (TR_WAVES x 4 ints, the only LDS).  The
//   sums are integer counts, so neither the wave a match falls to nor the order of the combine can change a bit of the result.  No
//   atomics, no memset, no scratch, vector stores only; thread 0 writes the record.
#include "hak_internal.h"
#include "pnp_common.h"
#include "points_common.h"

#define TR_BLOCK 512
#define TR_WAVES (TR_BLOCK / HAK_WAVE)

typedef pt_cameras<24> TriCameras;                                      // model: the views A, B of a call that keeps them on the host
// (step 1 of the rule for one view: pt_view, points_common.h)

// step 2: the view widened to float64 and its centre
__device__ __forceinline__ void tr_centre(const float M[12], double R[9], double c[3])
{
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = (double)M[k];
    const double t0 = (double)M[9], t1 = (double)M[10], t2 = (double)M[11];
#pragma unroll
    for (int j = 0; j < 3; j++) c[j] = -((R[j] * t0 + R[3 + j] * t1) + R[6 + j] * t2);
}

// step 3: the bearing (x, y, 1) turned into the common frame
__device__ __forceinline__ void tr_ray(const double R[9], double x, double y, double a[3])
{
#pragma unroll
    for (int j = 0; j < 3; j++) a[j] = (R[j] * x + R[3 + j] * y) + R[6 + j];
}

__global__ __launch_bounds__(TR_BLOCK) void k_triangulate(const hak_match_pair* __restrict__ base, long stride,
                                                          const int* __restrict__ counts, int count_step, int n_host,
                                                          const void* __restrict__ viewsA, int kindA, int stepA,
                                                          const void* __restrict__ viewsB, int kindB, int stepB,
                                                          const TriCameras cam, float t2, float max_depth, float min_sin,
                                                          hak_triangulation* __restrict__ out, unsigned char* __restrict__ masks,
                                                          float* __restrict__ xyz)
{
    __shared__ int part[TR_WAVES][4];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, count_step, n_host, stride);
    float MA[12], MB[12];
    const bool modelA = pt_view(viewsA, kindA, stepA, pair, cam.model, MA);
    const bool modelB = pt_view(viewsB, kindB, stepB, pair, cam.model + 12, MB);
    const bool model = modelA && modelB;                                // (block-uniform)
    double RA[9], RB[9], cA[3], cB[3], w[3];
    tr_centre(MA, RA, cA);
    tr_centre(MB, RB, cB);
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = cA[j] - cB[j];
    const pt_K kA(cam.K1), kB(cam.K2);
    const double md = (double)max_depth;
    const double s2 = (double)min_sin * (double)min_sin;
    const pt_out o(masks, xyz, pair, stride);

    int c[4] = {0, 0, 0, 0};                                            // kept, rejected[0 .. 2]
    for (int i = tid; i < n; i += TR_BLOCK) {
        bool keep = false;
        float P[3] = {0.0f, 0.0f, 0.0f};
        if (model) {
            const float4 r = fd_load(m, i);
            double a[3], b[3];
            tr_ray(RA, kA.x(r.x), kA.y(r.y), a);
            tr_ray(RB, kB.x(r.z), kB.y(r.w), b);
            const double aa = pt_dot(a, a), bb = pt_dot(b, b);
            const pt_depths d = pt_two_rays(a, aa, b, bb, w);
            int gate = 3;                                               // the first gate failed; 3 = none
            if (!(d.det > 0.0 && d.det >= s2 * (aa * bb))) gate = 0;
            else if (!(d.z1 > 0.0 && d.z1 < md && d.z2 > 0.0 && d.z2 < md)) gate = 1;
            else {
#pragma unroll
                for (int j = 0; j < 3; j++) P[j] = (float)(0.5 * ((cA[j] + d.z1 * a[j]) + (cB[j] + d.z2 * b[j])));
                if (!(pn_inlier(MA, make_float4(P[0], P[1], P[2], r.x), r.y, cam.K1, t2) &&
                      pn_inlier(MB, make_float4(P[0], P[1], P[2], r.z), r.w, cam.K2, t2)))
                    gate = 2;
            }
            keep = gate == 3;
            c[0] += keep ? 1 : 0;
            c[1] += gate == 0 ? 1 : 0;
            c[2] += gate == 1 ? 1 : 0;
            c[3] += gate == 2 ? 1 : 0;
        }
        o.store(i, keep, P[0], P[1], P[2]);
    }
    pt_block_sum<4, TR_WAVES>(c, part);
    if (tid == 0) {
        hak_triangulation t;
        t.n = n; t.kept = c[0]; t.rejected[0] = c[1]; t.rejected[1] = c[2]; t.rejected[2] = c[3]; t.model = model ? 1 : 0;
        t.pad[0] = t.pad[1] = 0;
        out[pair] = t;
    }
}

void hak_launch_triangulate(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int count_step, int n_host,
                            int npairs, const void* viewsA, int kindA, int stepA, const float* h_A, const void* viewsB, int kindB,
                            int stepB, const float* h_B, const hak_intrinsics& KA, const hak_intrinsics& KB, float threshold,
                            float max_depth, float min_sin, hak_triangulation* out, unsigned char* masks, float* xyz)
{
    TriCameras cam;
    cam.K1 = KA;
    cam.K2 = KB;
    cam.put(0, h_A, 12);
    cam.put(12, h_B, 12);
    k_triangulate<<<npairs, TR_BLOCK, 0, st>>>(matches, stride, counts, count_step, n_host, viewsA, h_A ? PT_VIEW_HOST : kindA, stepA,
                                               viewsB, h_B ? PT_VIEW_HOST : kindB, stepB, cam, threshold * threshold, max_depth,
                                               min_sin, out, masks, xyz);
}

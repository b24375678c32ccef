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

#define TR_BLOCK 512
#define TR_WAVES (TR_BLOCK / HAK_WAVE)
#define TR_VIEW_HOST 3                                                  // launcher-only kind: the view is a kernel argument

struct TriCameras {
    hak_intrinsics KA, KB;
    float A[12], B[12];                                                 // the views of a call that keeps them on the host
};

__device__ __forceinline__ double tr_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// step 1 of the rule for one view: M = {R row-major, t}; false = no model.  hak_pose and hak_abs_pose both begin with R[9], t[3];
// the word that says whether there is a model is `candidate` (word 14) of the one and `hypothesis` (word 13) of the other.
__device__ __forceinline__ bool tr_view(const void* views, int kind, int step, int pair, const float host[12], float M[12])
{
    bool model = true;
    if (kind == HAK_VIEW_IDENTITY) {
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = (k < 9 && k % 4 == 0) ? 1.0f : 0.0f;
    } else if (kind == TR_VIEW_HOST) {
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = host[k];
    } else {
        const float* rec = reinterpret_cast<const float*>(static_cast<const char*>(views) + 64 * ((long)pair * step));
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = rec[k];
        model = reinterpret_cast<const int*>(rec)[kind == HAK_VIEW_RELATIVE ? 14 : 13] >= 0;
    }
#pragma unroll
    for (int k = 0; k < 12; k++) model = model && __builtin_isfinite(M[k]);
    return model;
}

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
    const int n = fd_count(counts ? counts + (long)pair * count_step : nullptr, 0, n_host, stride);
    float MA[12], MB[12];
    const bool modelA = tr_view(viewsA, kindA, stepA, pair, cam.A, MA);
    const bool modelB = tr_view(viewsB, kindB, stepB, pair, cam.B, MB);
    const bool model = modelA && modelB;                                // (block-uniform)
    double RA[9], RB[9], cA[3], cB[3], w[3];
    tr_centre(MA, RA, cA);
    tr_centre(MB, RB, cB);
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = cA[j] - cB[j];
    const double fxA = (double)cam.KA.fx, fyA = (double)cam.KA.fy, cxA = (double)cam.KA.cx, cyA = (double)cam.KA.cy;
    const double fxB = (double)cam.KB.fx, fyB = (double)cam.KB.fy, cxB = (double)cam.KB.cx, cyB = (double)cam.KB.cy;
    const double md = (double)max_depth;
    const double s2 = (double)min_sin * (double)min_sin;
    unsigned char* mk = masks ? masks + (long)pair * stride : nullptr;
    float* pz = xyz ? xyz + 3 * ((long)pair * stride) : nullptr;

    int c[4] = {0, 0, 0, 0};                                            // kept, rejected[0 .. 2]
    for (int i = tid; i < n; i += TR_BLOCK) {
        bool keep = false;
        float P[3] = {0.0f, 0.0f, 0.0f};
        if (model) {
            const float4 r = fd_load(m, i);
            double a[3], b[3];
            tr_ray(RA, ((double)r.x - cxA) / fxA, ((double)r.y - cyA) / fyA, a);
            tr_ray(RB, ((double)r.z - cxB) / fxB, ((double)r.w - cyB) / fyB, b);
            const double aa = tr_dot(a, a), bb = tr_dot(b, b), ab = tr_dot(a, b), aw = tr_dot(a, w), bw = tr_dot(b, w);
            const double det = aa * bb - ab * ab;
            const double z1 = (ab * bw - bb * aw) / det;
            const double z2 = (aa * bw - ab * aw) / det;
            int gate = 3;                                               // the first gate failed; 3 = none
            if (!(det > 0.0 && det >= s2 * (aa * bb))) gate = 0;
            else if (!(z1 > 0.0 && z1 < md && z2 > 0.0 && z2 < md)) gate = 1;
            else {
#pragma unroll
                for (int j = 0; j < 3; j++) P[j] = (float)(0.5 * ((cA[j] + z1 * a[j]) + (cB[j] + z2 * b[j])));
                if (!(pn_inlier(MA, make_float4(P[0], P[1], P[2], r.x), r.y, cam.KA, t2) &&
                      pn_inlier(MB, make_float4(P[0], P[1], P[2], r.z), r.w, cam.KB, t2)))
                    gate = 2;
            }
            keep = gate == 3;
            c[0] += keep ? 1 : 0;
            c[1] += gate == 0 ? 1 : 0;
            c[2] += gate == 1 ? 1 : 0;
            c[3] += gate == 2 ? 1 : 0;
        }
        if (mk) mk[i] = keep ? 1 : 0;
        if (pz) {
            pz[3 * (long)i] = keep ? P[0] : 0.0f;
            pz[3 * (long)i + 1] = keep ? P[1] : 0.0f;
            pz[3 * (long)i + 2] = keep ? P[2] : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        c[k] = hg_wsum(c[k]);
        if ((tid & (HAK_WAVE - 1)) == 0) part[tid / HAK_WAVE][k] = c[k];
    }
    __syncthreads();
    if (tid == 0) {
        hak_triangulation o;
        int s[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            s[k] = 0;
#pragma unroll
            for (int wv = 0; wv < TR_WAVES; wv++) s[k] += part[wv][k];
        }
        o.n = n; o.kept = s[0]; o.rejected[0] = s[1]; o.rejected[1] = s[2]; o.rejected[2] = s[3]; o.model = model ? 1 : 0;
        o.pad[0] = o.pad[1] = 0;
        out[pair] = o;
    }
}

// the record of a hak_triangulate call: a device global, so that the call allocates nothing
__device__ hak_triangulation g_triangulation_record;

hak_triangulation* hak_triangulation_record()
{
    void* p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(g_triangulation_record)) == hipSuccess ? static_cast<hak_triangulation*>(p) : nullptr;
}

void hak_launch_triangulate(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int count_step, int n_host,
                            int npairs, const void* viewsA, int kindA, int stepA, const float* h_A, const void* viewsB, int kindB,
                            int stepB, const float* h_B, const hak_intrinsics& KA, const hak_intrinsics& KB, float threshold,
                            float max_depth, float min_sin, hak_triangulation* out, unsigned char* masks, float* xyz)
{
    TriCameras cam;
    cam.KA = KA;
    cam.KB = KB;
    for (int k = 0; k < 12; k++) {
        cam.A[k] = h_A ? h_A[k] : 0.0f;
        cam.B[k] = h_B ? h_B[k] : 0.0f;
    }
    k_triangulate<<<npairs, TR_BLOCK, 0, st>>>(matches, stride, counts, count_step, n_host, viewsA, h_A ? TR_VIEW_HOST : kindA, stepA,
                                               viewsB, h_B ? TR_VIEW_HOST : kindB, stepB, cam, threshold * threshold, max_depth,
                                               min_sin, out, masks, xyz);
}

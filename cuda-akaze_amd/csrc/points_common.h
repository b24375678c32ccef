// points_common.h -- what the point kernels share (kernels_pose.hip, kernels_poserefit.hip, kernels_triangulate.hip; the view of a
// list also serves kernels_projected.hip): the 3-vector dot product, the
// least-squares two-ray solve of step 5 of hak_recover_pose (also the solve of hak_triangulate, include/hipakaze.h) and that
// step's front test, the intrinsics
// widened to float64, the kernel argument of two cameras and a model kept on the host, the close of the per-lane integer counters
// and the store of a match's mask byte and point.  The gates on the solve stay with the kernels: they differ.
// Every file that includes it is built with -ffp-contract=off, so one source expression gives one rounding in both kernels.
#pragma once
#include "geom_common.h"

__device__ __forceinline__ double pt_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the depths z1 along ray a and z2 along ray b at which the two rays, their origins w = (origin of a) - (origin of b) apart, come
// closest; aa = a.a and bb = b.b are the caller's, which may hold one of them for several solves.  det <= 0: no solve
struct pt_depths { double det, z1, z2; };
__device__ __forceinline__ pt_depths pt_two_rays(const double a[3], double aa, const double b[3], double bb, const double w[3])
{
    const double ab = pt_dot(a, b), aw = pt_dot(a, w), bw = pt_dot(b, w);
    pt_depths d;
    d.det = aa * bb - ab * ab;
    d.z1 = (ab * bw - bb * aw) / d.det;
    d.z2 = (aa * bw - ab * aw) / d.det;
    return d;
}

// step 5 of hak_recover_pose for one match (also the front test of hak_refine_pose): a = R (x, y, 1), the first image's ray in
// the second camera's frame
__device__ __forceinline__ void pt_rotate(const double R[9], double x, double y, double a[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) a[i] = (R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2];
}
// ... and its gates on the rays a and b of the two images under the baseline t; true = in front, *z1 = the depth along the first
// camera's ray
__device__ __forceinline__ bool pt_front_rays(const double a[3], const double t[3], const double b[3], double bb, double md,
                                              double* z1)
{
    const pt_depths d = pt_two_rays(a, pt_dot(a, a), b, bb, t);
    *z1 = d.z1;
    return d.det > 0.0 && d.z1 > 0.0 && d.z1 < md && d.z2 > 0.0 && d.z2 < md;
}
// both, for the normalised point (x, y, 1) of image 1 and b of image 2 under (R, t)
__device__ __forceinline__ bool pt_front(const double R[9], const double t[3], double x, double y, const double b[3], double bb,
                                         double md, double* z1)
{
    double a[3];
    pt_rotate(R, x, y, a);
    return pt_front_rays(a, t, b, bb, md, z1);
}

// a camera's intrinsics widened to float64; x, y: a pixel coordinate normalised
struct pt_K {
    double fx, fy, cx, cy;
    __device__ __forceinline__ explicit pt_K(const hak_intrinsics& K) : fx((double)K.fx), fy((double)K.fy), cx((double)K.cx), cy((double)K.cy) {}
    __device__ __forceinline__ double x(float px) const { return ((double)px - cx) / fx; }
    __device__ __forceinline__ double y(float py) const { return ((double)py - cy) / fy; }
};

// the kernel argument of a call: the two cameras and W model words that a call may keep on the host
template <int W>
struct pt_cameras {
    hak_intrinsics K1, K2;
    float model[W];
    // (host) words at .. at + count - 1 from h, zeros without one
    void put(int at, const float* h, int count)
    {
        for (int k = 0; k < count; k++) model[at + k] = h ? h[k] : 0.0f;
    }
};

// a view Xc = R X + t of list `pair` as M = {R row-major, t}; false = no model (step 1 of hak_triangulate, step 7 of
// hak_match_projected).  kind: HAK_VIEW_*, or PT_VIEW_HOST (launcher-only): the view is the kernel argument `host`.  hak_pose and
// hak_abs_pose both begin with R[9], t[3]; the word that says whether there is a model is `candidate` (word 14) of the one and
// `hypothesis` (word 13) of the other.
#define PT_VIEW_HOST 3
__device__ __forceinline__ bool pt_view(const void* views, int kind, int step, int pair, const float host[12], float M[12])
{
    bool model = true;
    if (kind == HAK_VIEW_IDENTITY) {
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = (k < 9 && k % 4 == 0) ? 1.0f : 0.0f;
    } else if (kind == PT_VIEW_HOST) {
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

// closes N per-lane integer counters over a block of WAVES waves: the xor butterfly per wave, one row of part per wave, and the
// sum over the rows; every thread returns with the block's totals in c (k_pose chooses its winner from them in every thread;
// k_triangulate uses them in thread 0 only, and summing there alone measured the same).  The sums are integer counts, so no
// order changes a bit.  (block-uniform: holds a __syncthreads)
template <int N, int WAVES>
__device__ __forceinline__ void pt_block_sum(int c[N], int part[WAVES][N])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; k++) {
        c[k] = hg_wsum(c[k]);
        if ((tid & (HAK_WAVE - 1)) == 0) part[tid / HAK_WAVE][k] = c[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += part[w][k];
        c[k] = s;
    }
}

// where list `pair` of `stride` records writes its mask bytes and its points (3 floats per record); either array may be NULL
struct pt_out {
    unsigned char* mk;
    float* pz;
    __device__ __forceinline__ pt_out(unsigned char* masks, float* xyz, int pair, long stride)
        : mk(masks ? masks + (long)pair * stride : nullptr), pz(xyz ? xyz + 3 * ((long)pair * stride) : nullptr) {}
    // record i: the mask byte, and the point or zeros unless kept
    __device__ __forceinline__ void store(int i, bool keep, float X, float Y, float Z) const
    {
        if (mk) mk[i] = keep ? 1 : 0;
        if (pz) {
            pz[3 * (long)i] = keep ? X : 0.0f;
            pz[3 * (long)i + 1] = keep ? Y : 0.0f;
            pz[3 * (long)i + 2] = keep ? Z : 0.0f;
        }
    }
};

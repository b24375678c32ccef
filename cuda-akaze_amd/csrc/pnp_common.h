// pnp_common.h -- what the absolute-pose kernels share (kernels_pnp.hip, kernels_pnprefit.hip): the correspondence record as the
// kernels load it, the reprojection test of step 6 of hak_solve_pnp (include/hipakaze.h) and the estimator's view for the scaffolds
// of ransac_common.h and refit_common.h.
// kernels_triangulate.hip takes the reprojection test from here as gate 2 of hak_triangulate.
// Every file that includes it is built with -ffp-contract=off.
#pragma once
#include "ransac_common.h"

struct pn_rec { float4 a; float v; };                                 // a = {X, Y, Z, u}

// the first 20 bytes of a hak_corr3d; a record with a non-finite field gets X = NaN, which fails every test below
__device__ __forceinline__ pn_rec pn_load(const hak_corr3d* c, int i)
{
    const float4* p = reinterpret_cast<const float4*>(c + i);
    pn_rec r;
    r.a = p[0];
    r.v = p[1].x;
    if (!(__builtin_isfinite(r.a.x) && __builtin_isfinite(r.a.y) && __builtin_isfinite(r.a.z) && __builtin_isfinite(r.a.w) &&
          __builtin_isfinite(r.v)))
        r.a.x = __builtin_nanf("");
    return r;
}

// step 6: the reprojection test of model M = {R row-major, t}; NaN fails
__device__ __forceinline__ bool pn_inlier(const float M[12], const float4 a, const float v, const hak_intrinsics K, const float t2)
{
    const float xc = ((M[0] * a.x + M[1] * a.y) + M[2] * a.z) + M[9];
    const float yc = ((M[3] * a.x + M[4] * a.y) + M[5] * a.z) + M[10];
    const float zc = ((M[6] * a.x + M[7] * a.y) + M[8] * a.z) + M[11];
    const float ex = (K.fx * xc + K.cx * zc) - a.w * zc;
    const float ey = (K.fy * yc + K.cy * zc) - v * zc;
    return zc > 0.f && ex * ex + ey * ey < t2 * (zc * zc);
}

// the scaffolds' view of the estimator: four models (the quartic's roots) of 12 words per hypothesis, {R row-major, t}
struct pn_est {
    typedef hak_corr3d list_t;
    typedef pn_rec rec_t;
    typedef hak_abs_pose out_t;
    struct lds {
        float4 a[RS_CHUNK];
        float v[RS_CHUNK];
        __device__ __forceinline__ void put(int j, const pn_rec r) { a[j] = r.a; v[j] = r.v; }
        __device__ __forceinline__ pn_rec get(int j) const { return pn_rec{a[j], v[j]}; }
    };
    static constexpr int NM = 4, NW = 12, UNROLL = 2;
    hak_intrinsics K;
    float t2;
    static __device__ __forceinline__ pn_rec load(const hak_corr3d* c, int i) { return pn_load(c, i); }
    __device__ __forceinline__ bool inlier(const float M[12], const pn_rec r) const { return pn_inlier(M, r.a, r.v, K, t2); }
    static __device__ __forceinline__ bool load_model(const hak_abs_pose& o, float M[12])
    {
        bool model = o.hypothesis >= 0;
#pragma unroll
        for (int k = 0; k < 9; k++) { M[k] = o.R[k]; model = model && __builtin_isfinite(M[k]); }
#pragma unroll
        for (int k = 0; k < 3; k++) { M[9 + k] = o.t[k]; model = model && __builtin_isfinite(M[9 + k]); }
        return model;
    }
    static __device__ __forceinline__ int tag(const hak_abs_pose& o) { return o.solution; }
    static __device__ __forceinline__ void store(hak_abs_pose& o, const float M[12], int inliers, int hypothesis, int tag, int n)
    {
#pragma unroll
        for (int k = 0; k < 9; k++) o.R[k] = M[k];
#pragma unroll
        for (int k = 0; k < 3; k++) o.t[k] = M[9 + k];
        o.inliers = inliers; o.hypothesis = hypothesis; o.solution = tag; o.n = n;
    }
    static __device__ __forceinline__ void no_model(float M[12])
    {
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = (k < 9 && k % 4 == 0) ? 1.0f : 0.0f;
    }
};

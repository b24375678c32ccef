// pnp_common.h -- what the absolute-pose kernels share (kernels_pnp.hip, kernels_pnprefit.hip): the correspondence record as the
// kernels load it and the reprojection test of step 6 of hak_solve_pnp (include/hipakaze.h).
// Every file that includes it is built with -ffp-contract=off.
#pragma once
#include "hak_internal.h"

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

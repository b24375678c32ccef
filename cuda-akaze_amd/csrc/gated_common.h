// gated_common.h -- what the three gated searches (k_guided_search of kernels_guided.hip, k_epipolar_search of kernels_epipolar.hip,
// k_projected_search of kernels_projected.hip) do alike, stated once: the grid and a pair's view of the scratch k_guided_bin fills,
// a query's state, the step a candidate that passed the gate goes through, the walk of a disc gate, the model of a pair, and the
// launch sequence bin -> search -> reverse step.  The gates themselves, and the epipolar walk with its proof, stay in their files.
#pragma once
#include "hak_internal.h"

#define GD_N 64                  // cells per axis at most: 4096 LDS counters
// the grid of one pair, written by k_guided_bin and read by the searches
struct GdGrid {
    float ox, oy, inv;
    int nx, ny;
    int pad[3];
};
// the cell of a coordinate on one axis: non-decreasing in x for inv > 0; NaN lands in cell 0 (fmaxf drops it): listed there, and in
// no gate
__device__ __forceinline__ int gd_cell(float x, float o, float inv, int n)
{
    return (int)fminf(fmaxf(floorf((x - o) * inv), 0.f), (float)(n - 1));
}

// Pair `pair`'s part of the scratch: the lists k_guided_bin writes and the searches read, the reverse words both write ...
struct GdLists {
    int* idx;
    float2* xy;
    int* off;
    int4* rev;
};
__device__ __forceinline__ GdLists gd_lists(const HakGuidedScratch& sc, int pair)
{
    return {sc.idx + (long)pair * sc.pts_cap, sc.xy + (long)pair * sc.pts_cap, sc.off + (long)pair * (GD_N * GD_N + 1),
            sc.rev + (long)pair * sc.rev_stride};
}
__device__ __forceinline__ GdGrid* gd_grid_slot(const HakGuidedScratch& sc, int pair)
{
    return reinterpret_cast<GdGrid*>(sc.grid + (long)pair * 8);
}
// ... and a search's view of it: the lists with the grid the bin step left
struct GdView : GdLists {
    GdGrid g;
};
__device__ __forceinline__ GdView gd_view(const HakGuidedScratch& sc, int pair)
{
    GdView v;
    static_cast<GdLists&>(v) = gd_lists(sc, pair);
    v.g = *gd_grid_slot(sc, pair);
    return v;
}

// a query's state: its descriptor (loaded by the kernel once it knows that the query searches) and its two smallest keys so far
struct GdQuery {
    unsigned int qd[16];
    unsigned best = HAK_MKEY_EMPTY, second = HAK_MKEY_EMPTY;
};

// The passer step: list entry k passed the query's exact gate.  16 x (v_xor, v_bcnt) against the train descriptor, the two
// smallest hak_mkey(d, j) forward and, cross != 0, an atomicMin of hak_mkey(d, self) on the train point's reverse word.
__device__ __forceinline__ void gd_pass(GdQuery& q, const GdView& v, const hak_point* __restrict__ pts2, int k, int cross, int self)
{
    const int j = v.idx[k];
    unsigned int td[16];
    hak_desc_load(pts2 + j, td);
    unsigned d = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) d = hak_bcnt_acc(q.qd[w] ^ td[w], d);
    hak_mkey_two_smallest(q.best, q.second, hak_mkey(d, (unsigned)j));
    if (cross) atomicMin(reinterpret_cast<unsigned*>(&v.rev[j].x), hak_mkey(d, (unsigned)self));
}

// The disc search: every train point j with G = (dx dx) + (dy dy) < r2 around (px, py) goes through the passer step, once.
// rp = fl(radius * 1.0001f), r2 = fl(radius radius); (px, py) is finite.
//
// The conservative window.  G implies fl(dx dx) < r2 = fl(radius radius) (the other square is >= 0 and rounding is
// monotone), hence dx dx < radius radius (rounding is monotone), hence |dx| < radius.  dx = fl(x2 - px) is within 2^-24 relative
// of x2 - px (a float32 difference is exact where it is subnormal), so |x2 - px| < radius (1 + 2^-23) <= r' = fl(radius * 1.0001f).
// x2 is a float32 and rounding is monotone, so fl(px - r') <= x2 <= fl(px + r').  The cell function of an axis,
// cell(x) = clamp(floor(fl(fl(x - o) * inv)), 0, N - 1), is a composition of non-decreasing maps (inv > 0), so
// cell(fl(px - r')) <= cell(x2) <= cell(fl(px + r')): the search walks exactly that range on each axis -- whatever the grid's
// origin and cell side are, and wherever the points lie (points outside the box fall into border cells).  With a cell side of
// at least r' that is at most 3 x 3 cells, up to rounding of the cell coordinate far from the origin (then a few more: the loop
// bounds are the two cell numbers, not a constant).
__device__ __forceinline__ void gd_disc(GdQuery& q, const GdView& v, const hak_point* __restrict__ pts2, float px, float py, float rp,
                                        float r2, int cross, int self)
{
    const GdGrid& g = v.g;
    const int cx0 = gd_cell(px - rp, g.ox, g.inv, g.nx), cx1 = gd_cell(px + rp, g.ox, g.inv, g.nx);
    const int cy0 = gd_cell(py - rp, g.oy, g.inv, g.ny), cy1 = gd_cell(py + rp, g.oy, g.inv, g.ny);
    for (int cy = cy0; cy <= cy1; cy++) {
        // cells cx0 .. cx1 of a row are consecutive in the sorted list
        const int kend = v.off[cy * g.nx + cx1 + 1];
        for (int k = v.off[cy * g.nx + cx0]; k < kend; k++) {
            const float2 t = v.xy[k];
            const float dx = t.x - px, dy = t.y - py;
            if ((dx * dx) + (dy * dy) < r2) gd_pass(q, v, pts2, k, cross, self);      // the exact gate
        }
    }
}

// The model of a pair is its device record (batch) or the by-value copy (single call): `d_M ? d_M[pair] : Mval` in the kernel.
// A pair has no model when the record says so or any of its nine entries is non-finite.
__device__ __forceinline__ bool gd_model(const float (&m)[9], int hypothesis)
{
    bool model = hypothesis >= 0;
#pragma unroll
    for (int k = 0; k < 9; k++) model = model && fabsf(m[k]) < INFINITY;     // (false for NaN)
    return model;
}

// The launch sequence of a gated matcher: the bin step over cells of side >= rp, the matcher's search kernel -- search(grid): one
// thread per query of at most nq_host, blockIdx.y = pair -- and, cross != 0, the reverse step.  count_step as hak_launch_guided_bin.
template <typename Search>
static inline void gd_launch(hipStream_t st, const hak_point* pts2, const int* n2_dev, int n2_host, long stride2, int count_step,
                             int npairs, float rp, int cross, const HakGuidedScratch& sc, int nq_host, Search search)
{
    hak_launch_guided_bin(st, pts2, n2_dev, n2_host, stride2, npairs, rp, sc, count_step);
    search(dim3(hak_grid_x((nq_host + 255) / 256), npairs));
    if (cross) hak_launch_guided_rev(st, n2_dev, n2_host, npairs, sc, count_step);
}

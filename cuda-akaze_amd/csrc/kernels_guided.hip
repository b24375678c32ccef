// kernels_guided.hip -- guided matching: re-match a pair under its estimated homography (hak_match_guided, gfx950, wave64).
//
// The rule is the contract in include/hipakaze.h (numpy statement: tests/guided_match_ref.py): query i is projected through H and
// searched only among the train points within `radius` of the projection; 2-NN ratio test and cross-check inside that gate.
// A gated search computes a small, data-dependent subset of the n1 x n2 distances, so it cannot ride the dense matrix-core
// matcher; it is spatially binned instead:
//   k_guided_bin     one block per pair: bounding box of the train points -> a uniform grid of at most 64 x 64 cells whose
//                    counters live in LDS -> histogram, exclusive scan, scatter of {index, x, y} into a list sorted by cell;
//                    it also resets the pair's reverse keys
//   k_guided_search  one query per thread: projection, the cells its gate can reach, the exact gate on every listed candidate,
//                    16 x (v_xor, v_bcnt) per passer; the two smallest packed keys (hak_mkey(d, j), hak_internal.h) give j1, d1, d2,
//                    and an atomicMin of hak_mkey(d, i) on the train point's word gives rev(j) in the same pass
//   k_guided_rev     reverse keys -> indices, the form k_knn2_finish reads
// The bin and the reverse step are launchers of their own (hak_launch_guided_bin / _rev): the searches of kernels_epipolar.hip and
// kernels_projected.hip share them, the scratch carve and the grid.  What a search does once its gate has passed, the walk of a
// disc gate and the launch sequence are in gated_common.h, for all three.
// The accept rule and the compaction are the 2-NN matcher's own finish kernels (kernels_match.hip), unchanged.
//
// Why the result does not depend on the binning.  The grid only decides WHICH candidates a query looks at; whether a candidate
// counts is the exact gate, evaluated on the same float32 words the rule names.  So it is enough that every j with G(i, j) is
// visited (the conservative window, beside gd_disc in gated_common.h) -- and the order in which a cell lists its points (atomics)
// cannot show: the forward result is the two smallest of a set of distinct keys, the reverse one an atomicMin, both order-free.
#include "gated_common.h"
#include <cstddef>

#define GD_THREADS 1024          // k_guided_bin's block
#define GD_BOX 1048576.f         // |coordinate| beyond 2^20 does not stretch the box (such points sit in border cells)

__global__ __launch_bounds__(GD_THREADS) void k_guided_bin(const hak_point* __restrict__ pts2_base, const int* __restrict__ n2_dev, int n2_host,
                                                            long stride2, int count_stride, float rp, HakGuidedScratch sc)
{
    __shared__ int cnt[GD_N * GD_N];
    __shared__ float red[4][GD_THREADS / 64];
    __shared__ int wtot[GD_THREADS / 64];
    __shared__ GdGrid sg;
    const int pair = blockIdx.x;
    const int cap = (int)sc.pts_cap;
    const int n2 = min(max(n2_dev ? n2_dev[pair * count_stride] : n2_host, 0), cap);
    const hak_point* pts2 = pts2_base + (long)pair * stride2;
    const GdLists l = gd_lists(sc, pair);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

    // ---- bounding box of the finite train points
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int j = threadIdx.x; j < n2; j += GD_THREADS) {
        const float x = pts2[j].x, y = pts2[j].y;
        if (fabsf(x) <= GD_BOX && fabsf(y) <= GD_BOX) {               // (false for NaN and inf)
            x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
        }
        l.rev[j] = hak_knn_none();                                    // .x: the reverse key, HAK_MKEY_EMPTY = no query gates this point
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, o)); x1 = fmaxf(x1, __shfl_xor(x1, o));
        y0 = fminf(y0, __shfl_xor(y0, o)); y1 = fmaxf(y1, __shfl_xor(y1, o));
    }
    if (lane == 0) { red[0][wv] = x0; red[1][wv] = x1; red[2][wv] = y0; red[3][wv] = y1; }
    for (int c = threadIdx.x; c < GD_N * GD_N; c += GD_THREADS) cnt[c] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 0; t < GD_THREADS / 64; t++) {
            x0 = fminf(x0, red[0][t]); x1 = fmaxf(x1, red[1][t]); y0 = fminf(y0, red[2][t]); y1 = fmaxf(y1, red[3][t]);
        }
        GdGrid g{};
        const bool any = x0 <= x1;
        const float ex = any ? x1 - x0 : 0.f, ey = any ? y1 - y0 : 0.f;
        // cell side = max(r', extent / 64): a gate reaches at most three cells per axis, and the grid has at most 64 x 64
        const float side = fmaxf(rp, fmaxf(ex, ey) * (1.f / GD_N));
        g.ox = any ? x0 : 0.f;
        g.oy = any ? y0 : 0.f;
        g.inv = 1.f / side;
        g.nx = (int)fminf(floorf(ex * g.inv) + 1.f, (float)GD_N);
        g.ny = (int)fminf(floorf(ey * g.inv) + 1.f, (float)GD_N);
        sg = g;
        *gd_grid_slot(sc, pair) = g;
    }
    __syncthreads();
    const GdGrid g = sg;
    const int ncell = g.nx * g.ny;

    // ---- histogram
    for (int j = threadIdx.x; j < n2; j += GD_THREADS) {
        const int c = gd_cell(pts2[j].y, g.oy, g.inv, g.ny) * g.nx + gd_cell(pts2[j].x, g.ox, g.inv, g.nx);
        atomicAdd(&cnt[c], 1);
    }
    __syncthreads();

    // ---- exclusive scan: thread t owns cells 4 t .. 4 t + 3
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const int c = 4 * threadIdx.x + k; v[k] = c < ncell ? cnt[c] : 0; s += v[k]; }
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    int base = inc - s;
    for (int t = 0; t < wv; t++) base += wtot[t];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = 4 * threadIdx.x + k;
        if (c < ncell) { l.off[c] = base; cnt[c] = base; }            // cnt becomes the cell's write cursor
        base += v[k];
    }
    if (threadIdx.x == 0) l.off[ncell] = n2;
    __syncthreads();

    // ---- scatter (the order inside a cell is arbitrary; see the file header)
    for (int j = threadIdx.x; j < n2; j += GD_THREADS) {
        const float x = pts2[j].x, y = pts2[j].y;
        const int c = gd_cell(y, g.oy, g.inv, g.ny) * g.nx + gd_cell(x, g.ox, g.inv, g.nx);
        const int pos = atomicAdd(&cnt[c], 1);
        if (pos < cap) { l.idx[pos] = j; l.xy[pos] = make_float2(x, y); }   // (pos < n2 <= cap always)
    }
}

__global__ __launch_bounds__(256) void k_guided_search(const hak_point* __restrict__ pts1_base, const hak_point* __restrict__ pts2_base,
                                                        const int* __restrict__ n1_dev, int n1_host, long stride1, long stride2,
                                                        int count_stride, const hak_homography* __restrict__ d_H, hak_homography Hval,
                                                        float rp, float r2, int cross, HakGuidedScratch sc, int4* __restrict__ fwd_base,
                                                        long fwd_stride)
{
    const int pair = blockIdx.y;
    const int n1 = n1_dev ? min(n1_dev[pair * count_stride], n1_host) : n1_host;     // (device counts: n1_host is the capacity)
    const hak_point* pts1 = pts1_base + (long)pair * stride1;
    const hak_point* pts2 = pts2_base + (long)pair * stride2;
    int4* fwd = fwd_base + (long)pair * fwd_stride;
    const GdView view = gd_view(sc, pair);
    const hak_homography hr = d_H ? d_H[pair] : Hval;
    const bool model = gd_model(hr.H, hr.hypothesis);

    for (int i = blockIdx.x * 256 + threadIdx.x; i < n1; i += gridDim.x * 256) {
        const float x = pts1[i].x, y = pts1[i].y;
        // projection: float32, no FMA (the library is built with -ffp-contract=off), correctly rounded division
        const float wz = (hr.H[6] * x + hr.H[7] * y) + hr.H[8];
        const float u = (hr.H[0] * x + hr.H[1] * y) + hr.H[2];
        const float v = (hr.H[3] * x + hr.H[4] * y) + hr.H[5];
        const float px = u / wz, py = v / wz;
        GdQuery q;
        // a non-finite projection is in no gate (every compare of the walk would be false): it does not search
        if (model && wz > 0.f && fabsf(px) < INFINITY && fabsf(py) < INFINITY) {
            hak_desc_load(pts1 + i, q.qd);
            gd_disc(q, view, pts2, px, py, rp, r2, cross, i);
        }
        fwd[i] = hak_knn_record(q.best, q.second);
    }
}

// reverse keys -> {rev(j), its distance, 512, 0}: what k_knn2_finish's cross-check reads (.x)
__global__ __launch_bounds__(256) void k_guided_rev(const int* __restrict__ n2_dev, int n2_host, int count_stride, HakGuidedScratch sc)
{
    const int pair = blockIdx.y;
    const int n2 = min(max(n2_dev ? n2_dev[pair * count_stride] : n2_host, 0), (int)sc.pts_cap);
    int4* rev = sc.rev + (long)pair * sc.rev_stride;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n2; j += gridDim.x * 256) {
        const unsigned key = (unsigned)rev[j].x;
        if (key != HAK_MKEY_EMPTY) rev[j] = hak_knn_record(key, HAK_MKEY_EMPTY);
    }
}

size_t hak_guided_scratch_bytes(long npairs, long pts_cap)
{
    return (size_t)npairs * ((size_t)pts_cap * (sizeof(int) + sizeof(float2)) + (GD_N * GD_N + 1) * sizeof(int) + 8 * sizeof(int));
}
// carve `base` (16-byte aligned, hak_guided_scratch_bytes(npairs, pts_cap) bytes)
HakGuidedScratch hak_guided_scratch_carve(void* base, long npairs, long pts_cap, int4* rev, long rev_stride)
{
    HakGuidedScratch sc{};
    char* p = static_cast<char*>(base);
    sc.xy = reinterpret_cast<float2*>(p); p += (size_t)npairs * pts_cap * sizeof(float2);
    sc.grid = reinterpret_cast<int*>(p); p += (size_t)npairs * 8 * sizeof(int);
    sc.idx = reinterpret_cast<int*>(p); p += (size_t)npairs * pts_cap * sizeof(int);
    sc.off = reinterpret_cast<int*>(p);
    sc.pts_cap = pts_cap;
    sc.rev = rev;
    sc.rev_stride = rev_stride;
    return sc;
}

void hak_launch_guided_bin(hipStream_t st, const hak_point* pts2, const int* n2_dev, int n2_host, long stride2, int npairs, float rp,
                           const HakGuidedScratch& sc, int count_step)
{
    k_guided_bin<<<npairs, GD_THREADS, 0, st>>>(pts2, n2_dev, n2_host, stride2, count_step, rp, sc);
}
void hak_launch_guided_rev(hipStream_t st, const int* n2_dev, int n2_host, int npairs, const HakGuidedScratch& sc, int count_step)
{
    k_guided_rev<<<dim3(hak_grid_x((n2_host + 255) / 256), npairs), 256, 0, st>>>(n2_dev, n2_host, count_step, sc);
}

// the forward search of npairs pairs into fwd ({j1, d1, d2, 0} per query) and, cross != 0, rev(j) into sc.rev ({i, d, 512, 0}).
// With device-side counts (pair k: n1_dev / n2_dev[k * count_step]) n1_host / n2_host carry the capacity of the sets.  d_H: one
// record per pair on the device, or NULL: h_H[9] (host) serves the only pair.
void hak_launch_guided(hipStream_t st, const hak_point* pts1, const hak_point* pts2, const int* n1_dev, const int* n2_dev, int count_step,
                       int n1_host, int n2_host, long stride1, long stride2, int npairs, const hak_homography* d_H, const float* h_H,
                       float radius, int cross, const HakGuidedScratch& sc, int4* fwd, long fwd_stride)
{
    const float rp = radius * 1.0001f, r2 = radius * radius;
    hak_homography hv{};
    if (!d_H)
        for (int k = 0; k < 9; k++) hv.H[k] = h_H[k];
    gd_launch(st, pts2, n2_dev, n2_host, stride2, count_step, npairs, rp, cross, sc, n1_host, [&](dim3 grid) {
        k_guided_search<<<grid, 256, 0, st>>>(pts1, pts2, n1_dev, n1_host, stride1, stride2, count_step, d_H, hv, rp, r2, cross, sc, fwd,
                                              fwd_stride);
    });
}

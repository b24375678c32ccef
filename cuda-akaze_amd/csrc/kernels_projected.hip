// kernels_projected.hip -- projection-guided matching: re-match 3-D points under a known pose (hak_match_projected, gfx950, wave64).
//
// The rule is the contract in include/hipakaze.h (numpy statement: tests/projected_match_ref.py): landmark m of list A -- the point
// xyz[3m ..] with the descriptor of keypoint A[m].train -- is projected through a view Xc = R X + t and the intrinsics K, and is
// searched only among the keypoints of the new image within `radius` of the projection; 2-NN ratio test and cross-check inside
// that gate.  The train points are binned by kernels_guided.hip's k_guided_bin and the reverse keys are turned into records by its
// k_guided_rev (hak_launch_guided_bin / _rev: the same grid of at most 64 x 64 cells, the same scratch).  New here:
//   k_projected_search  one landmark per thread on k_guided_search's grid: eligibility (mask, train index), the float32 projection,
//                       the cells its gate can reach, the exact gate on every listed candidate, 16 x (v_xor, v_bcnt) per passer;
//                       the two smallest hak_mkey(d, j) forward, an atomicMin of hak_mkey(d, m) on the train point's word.  The
//                       landmark's descriptor is loaded once, through the indirection desc[A[m].train]; the view comes from the
//                       64-byte device record (pt_view, points_common.h) or, for the one-list call, by value
//   k_projected_finish  one block per list walks it in chunks of its block size, as k_link_gather compacts: hak_knn2_rule as it
//                       stands, then an ordered compaction of the accepted landmarks into hak_corr3d records in ascending m.  No
//                       atomics on the output, so the list does not depend on scheduling; it writes the count and nothing past it
// The gate is the guided matcher's gate in (px, py) and the walk is the same function, gd_disc (gated_common.h, with its
// conservative-window argument), so the result does not depend on the binning for the reasons given in the header of
// kernels_guided.hip.
#include "gated_common.h"
#include "points_common.h"

#define PJ_FINISH 1024           // k_projected_finish's block

// what a call passes by value: the camera and the view of a call that keeps it on the host
struct PjCamera {
    hak_intrinsics K;
    float view[12];
};

__global__ __launch_bounds__(256) void k_projected_search(const hak_match_pair* __restrict__ A_base, long strideA,
                                                           const int* __restrict__ countsA, int stepA, int nA_host, long capA,
                                                           const unsigned char* __restrict__ masks, const float* __restrict__ xyz_base,
                                                           const hak_point* __restrict__ desc_base, long desc_stride,
                                                           const int* __restrict__ desc_counts, int desc_step, int nD_host, long capD,
                                                           const hak_point* __restrict__ pts2_base, long stride2,
                                                           const void* __restrict__ views, int kind, int view_step, const PjCamera cam,
                                                           float rp, float r2, int cross, HakGuidedScratch sc, int4* __restrict__ fwd_base,
                                                           long fwd_stride)
{
    const int pair = blockIdx.y;
    const int nA = fd_count(countsA, pair, stepA, nA_host, capA);
    const int nD = fd_count(desc_counts, pair, desc_step, nD_host, capD);
    const hak_match_pair* A = A_base + (long)pair * strideA;
    const unsigned char* mk = masks ? masks + (long)pair * strideA : nullptr;
    const float* xyz = xyz_base + 3 * ((long)pair * strideA);
    const hak_point* desc = desc_base + (long)pair * desc_stride;
    const hak_point* pts2 = pts2_base + (long)pair * stride2;
    int4* fwd = fwd_base + (long)pair * fwd_stride;
    const GdView view = gd_view(sc, pair);
    float M[12];
    const bool model = pt_view(views, kind, view_step, pair, cam.view, M);      // (block-uniform)
    const hak_intrinsics K = cam.K;

    for (int m = blockIdx.x * 256 + threadIdx.x; m < nA; m += gridDim.x * 256) {
        GdQuery q;
        const int e = A[m].train;
        if (model && e >= 0 && e < nD && (!mk || mk[m] != 0)) {
            const float X = xyz[3 * (long)m], Y = xyz[3 * (long)m + 1], Z = xyz[3 * (long)m + 2];
            // projection: float32, no FMA (the library is built with -ffp-contract=off), correctly rounded division; xc, yc, zc
            // are the expressions of pn_inlier (pnp_common.h)
            const float xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[9];
            const float yc = ((M[3] * X + M[4] * Y) + M[5] * Z) + M[10];
            const float zc = ((M[6] * X + M[7] * Y) + M[8] * Z) + M[11];
            const float px = (K.fx * (xc / zc)) + K.cx;
            const float py = (K.fy * (yc / zc)) + K.cy;
            // a non-finite projection is in no gate (every compare of the walk would be false): it does not search
            if (zc > 0.f && fabsf(px) < INFINITY && fabsf(py) < INFINITY) {
                hak_desc_load(desc + e, q.qd);
                gd_disc(q, view, pts2, px, py, rp, r2, cross, m);
            }
        }
        fwd[m] = hak_knn_record(q.best, q.second);
    }
}

// accept rule + ordered compaction of list `pair`: chunk by chunk, a ballot per wave, the waves' counts through LDS, the running
// base in LDS.  out_base == nullptr: the count alone
__global__ __launch_bounds__(PJ_FINISH) void k_projected_finish(const int* __restrict__ countsA, int stepA, int nA_host, long capA,
                                                                 const float* __restrict__ xyz_base, long strideA,
                                                                 const hak_point* __restrict__ pts2_base, long stride2,
                                                                 const int4* __restrict__ fwd_base, long fwd_stride,
                                                                 const int4* __restrict__ rev_base, long rev_stride, int ratio_num,
                                                                 int ratio_den, int cross, int max_dist,
                                                                 hak_corr3d* __restrict__ out_base, long out_stride,
                                                                 int* __restrict__ out_count)
{
    __shared__ int wsum[PJ_FINISH / HAK_WAVE];
    __shared__ int sbase;
    const int pair = blockIdx.x;
    const int nA = fd_count(countsA, pair, stepA, nA_host, capA);
    const float* xyz = xyz_base + 3 * ((long)pair * strideA);
    const hak_point* pts2 = pts2_base + (long)pair * stride2;
    const int4* fwd = fwd_base + (long)pair * fwd_stride;
    const int4* rev = rev_base + (long)pair * rev_stride;
    hak_corr3d* out = out_base ? out_base + (long)pair * out_stride : nullptr;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) sbase = 0;
    __syncthreads();
    for (int m0 = 0; m0 < nA; m0 += PJ_FINISH) {
        const int m = m0 + threadIdx.x;
        int4 f;
        const bool ok = hak_knn2_rule(m, nA, fwd, rev, ratio_num, ratio_den, cross, max_dist, f);
        const unsigned long long bal = __ballot(ok);
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        int before = sbase;
        for (int t = 0; t < wv; t++) before += wsum[t];
        if (ok && out) {
            const float* p = xyz + 3 * (long)m;
            const hak_point* t = pts2 + f.x;
            float4* o = reinterpret_cast<float4*>(out + before + __popcll(bal & ((1ull << lane) - 1ull)));
            o[0] = make_float4(p[0], p[1], p[2], t->x);
            o[1] = make_float4(t->y, __int_as_float(m), __int_as_float(f.x), __int_as_float(0));
        }
        __syncthreads();
        if (threadIdx.x == 0) { int tot = 0; for (int t = 0; t < PJ_FINISH / HAK_WAVE; t++) tot += wsum[t]; sbase += tot; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out_count[pair] = sbase;
}

void hak_launch_projected(hipStream_t st, const hak_match_pair* A, long strideA, const int* countsA, int stepA, int nA_host, long capA,
                          const unsigned char* masksA, const float* xyzA, const hak_point* desc, long desc_stride,
                          const int* desc_counts, int desc_step, int nD_host, long capD, const hak_point* pts2, long stride2,
                          const int* counts2, int step2, int n2_host, int npairs, const void* views, int kind, int view_step,
                          const float* h_view, const hak_intrinsics& K, float radius, int ratio_num, int ratio_den, int cross,
                          int max_dist, const HakGuidedScratch& sc, int4* fwd, long fwd_stride, hak_corr3d* out, long out_stride,
                          int* out_counts)
{
    const float rp = radius * 1.0001f, r2 = radius * radius;
    PjCamera cam;
    cam.K = K;
    for (int k = 0; k < 12; k++) cam.view[k] = h_view ? h_view[k] : 0.f;
    const int most = (int)(countsA ? capA : nA_host);                 // (device counts: the capacity of a list)
    gd_launch(st, pts2, counts2, n2_host, stride2, step2, npairs, rp, cross, sc, most, [&](dim3 grid) {
        k_projected_search<<<grid, 256, 0, st>>>(A, strideA, countsA, stepA, nA_host, capA, masksA, xyzA, desc, desc_stride, desc_counts,
                                                 desc_step, nD_host, capD, pts2, stride2, views, h_view ? PT_VIEW_HOST : kind, view_step,
                                                 cam, rp, r2, cross, sc, fwd, fwd_stride);
    });
    k_projected_finish<<<npairs, PJ_FINISH, 0, st>>>(countsA, stepA, nA_host, capA, xyzA, strideA, pts2, stride2, fwd, fwd_stride, sc.rev,
                                                     sc.rev_stride, ratio_num, ratio_den, cross, max_dist, out, out_stride, out_counts);
}

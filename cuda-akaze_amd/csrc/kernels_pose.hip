// kernels_pose.hip -- relative pose, front mask and first 3-D points of a match list from its fundamental matrix and the two
// cameras' intrinsics (gfx950, wave64).
//
// The semantics are fixed in include/hipakaze.h (hak_recover_pose) so that the numpy reference tests/pose_ref.py agrees bit for
// bit: E = K2^T (F K1) scaled by its largest entry, the right singular vectors by the 3 x 3 cyclic Jacobi of the refit's rule on
// E^T E, the left ones by Gram-Schmidt, the four (R, t) candidates, and per Sampson inlier of F a linear two-ray depth solve under
// each candidate.  float64, + - * / sqrt only; the file is built with -ffp-contract=off: no FMA is formed, so every rounding is
// the one the reference makes.
//
// k_pose: one block of PO_BLOCK threads (PO_WAVES waves) per pair.  The decomposition is a chain of a few hundred dependent
//   float64 operations; every lane of every wave computes it redundantly, so nothing is broadcast.  Pass 1 streams the list once
//   and counts, per inlier, the four candidates in front: five integer counters per lane, closed by the xor butterfly per wave
//   and one LDS row per wave (PO_WAVES x 5 ints, the only LDS).  The sums are integer counts, so neither the wave a match falls
//   to nor the order of the combine can change a bit of the result.  Pass 2 re-reads the list and writes the mask and the points
//   under the winner.  No scratch, vector stores only; thread 0 writes the record.
#include "hak_internal.h"
#include "points_common.h"

#define PO_BLOCK 512
#define PO_WAVES (PO_BLOCK / HAK_WAVE)
#define PO_SWEEPS3 6

typedef pt_cameras<9> PoseCameras;                                      // model: the F of a call that keeps it on the host

__device__ __forceinline__ void po_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void po_matvec(const double E[9], const double v[3], double o[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (E[3 * i] * v[0] + E[3 * i + 1] * v[1]) + E[3 * i + 2] * v[2];
}

// steps 2-4 of the rule: Ra, Rb and u3 from F; false = no pose
__device__ bool po_decompose(const float F[9], const hak_intrinsics& K1, const hak_intrinsics& K2, double Ra[9], double Rb[9],
                             double u3[3])
{
    double Fd[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Fd[k] = (double)F[k];
    const double Km[9] = {(double)K1.fx, 0.0, (double)K1.cx, 0.0, (double)K1.fy, (double)K1.cy, 0.0, 0.0, 1.0};
    const double K2t[9] = {(double)K2.fx, 0.0, 0.0, 0.0, (double)K2.fy, 0.0, (double)K2.cx, (double)K2.cy, 1.0};
    double H[9], E[9];
    fd_mul3(Fd, Km, H);
    fd_mul3(K2t, H, E);
    double d = E[0];
#pragma unroll
    for (int k = 1; k < 9; k++) d = fabs(E[k]) > fabs(d) ? E[k] : d;
    if (!(d != 0.0 && __builtin_isfinite(d))) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = E[k] / d;
    double G[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    fd_jacobi3(G, V, PO_SWEEPS3);
    const int j3 = fd_jacobi3_smallest(G);
    double v1[3], v2[3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        v1[i] = j3 == 0 ? V[i][1] : V[i][0];                            // the other two columns, ascending
        v2[i] = j3 == 2 ? V[i][1] : V[i][2];
    }
    po_cross(v1, v2, v3);
    double x[3], y[3], u1[3], u2[3], w[3];
    po_matvec(E, v1, x);
    const double l1 = sqrt(pt_dot(x, x));
#pragma unroll
    for (int i = 0; i < 3; i++) u1[i] = x[i] / l1;
    po_matvec(E, v2, y);
    const double dd = pt_dot(u1, y);
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = y[i] - dd * u1[i];
    const double l2 = sqrt(pt_dot(w, w));
#pragma unroll
    for (int i = 0; i < 3; i++) u2[i] = w[i] / l2;
    po_cross(u1, u2, u3);
    if (!(__builtin_isfinite(l1) && l1 > 0.0 && __builtin_isfinite(l2) && l2 > 0.0)) return false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Ra[3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
            Rb[3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
        }
    return true;
}

__global__ __launch_bounds__(PO_BLOCK) void k_pose(const hak_match_pair* __restrict__ base, long stride,
                                                   const int* __restrict__ counts, int n_host,
                                                   const hak_fundamental* __restrict__ d_F, const PoseCameras cam, float t2,
                                                   float max_depth, hak_pose* __restrict__ out, unsigned char* __restrict__ masks,
                                                   float* __restrict__ xyz)
{
    __shared__ int part[PO_WAVES][5];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const hak_match_pair* m = base + (long)pair * stride;
    const int n = fd_count(counts, pair, 1, n_host, stride);
    float F[9];
    bool model = true;
    if (d_F) {
        const hak_fundamental in = d_F[pair];
        model = in.hypothesis >= 0;
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = in.F[k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = cam.model[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) model = model && __builtin_isfinite(F[k]);
    double Ra[9], Rb[9], u3[3], nu3[3];
    if (model) model = po_decompose(F, cam.K1, cam.K2, Ra, Rb, u3);     // (block-uniform)
    if (!model) {
#pragma unroll
        for (int k = 0; k < 9; k++) Ra[k] = Rb[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) u3[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) nu3[k] = -u3[k];
    const pt_K k1(cam.K1), k2(cam.K2);
    const double md = (double)max_depth;

    // pass 1: the inliers of F and, of those, the matches in front under each candidate
    int c[5] = {0, 0, 0, 0, 0};
    if (model)
        for (int i = tid; i < n; i += PO_BLOCK) {
            const float4 r = fd_load(m, i);
            if (!fd_inlier(F, r, t2)) continue;
            const double x = k1.x(r.x), y = k1.y(r.y);
            const double b[3] = {k2.x(r.z), k2.y(r.w), 1.0};
            const double bb = pt_dot(b, b);
            double z;
            c[0] += pt_front(Ra, u3, x, y, b, bb, md, &z) ? 1 : 0;
            c[1] += pt_front(Ra, nu3, x, y, b, bb, md, &z) ? 1 : 0;
            c[2] += pt_front(Rb, u3, x, y, b, bb, md, &z) ? 1 : 0;
            c[3] += pt_front(Rb, nu3, x, y, b, bb, md, &z) ? 1 : 0;
            c[4]++;
        }
    pt_block_sum<5, PO_WAVES>(c, part);
    int best = 0, in_front = c[0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (c[k] > in_front) { in_front = c[k]; best = k; }             // ties to the smallest index
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = best < 2 ? Ra[k] : Rb[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (best & 1) ? nu3[k] : u3[k];

    // pass 2: the mask and the points under the winner
    if (masks || xyz) {
        const pt_out o(masks, xyz, pair, stride);
        for (int i = tid; i < n; i += PO_BLOCK) {
            bool front = false;
            double x = 0.0, y = 0.0, z = 0.0;
            if (model) {
                const float4 r = fd_load(m, i);
                if (fd_inlier(F, r, t2)) {
                    x = k1.x(r.x);
                    y = k1.y(r.y);
                    const double b[3] = {k2.x(r.z), k2.y(r.w), 1.0};
                    front = pt_front(R, t, x, y, b, pt_dot(b, b), md, &z);
                }
            }
            o.store(i, front, (float)(z * x), (float)(z * y), (float)z);
        }
    }
    if (tid == 0) {
        hak_pose o;
#pragma unroll
        for (int k = 0; k < 9; k++) o.R[k] = model ? (float)R[k] : (k % 4 == 0 ? 1.0f : 0.0f);
#pragma unroll
        for (int k = 0; k < 3; k++) o.t[k] = model ? (float)t[k] : 0.0f;
        o.inliers = model ? c[4] : 0; o.in_front = model ? in_front : 0; o.candidate = model ? best : -1; o.n = n;
        out[pair] = o;
    }
}

void hak_launch_pose(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                     const hak_fundamental* d_F, const float* h_F, const hak_intrinsics& K1, const hak_intrinsics& K2,
                     float threshold, float max_depth, hak_pose* out, unsigned char* masks, float* xyz)
{
    PoseCameras cam;
    cam.K1 = K1;
    cam.K2 = K2;
    cam.put(0, h_F, 9);
    k_pose<<<npairs, PO_BLOCK, 0, st>>>(matches, stride, counts, n_host, d_F, cam, threshold * threshold, max_depth, out, masks,
                                        xyz);
}

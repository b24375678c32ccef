// stub_hipakaze.cpp -- a HOST-MEMORY stand-in for the entry points of libhipakaze.so (and the two HIP runtime calls) that the
// C++ layer host/akaze.cpp uses, so that the layer's own logic -- pinned-buffer registry, context re-creation on a size change,
// per-call clamp, error style -- can run under AddressSanitizer / UBSan on the CPU (GPU sanitizers are not available on this
// pool).  Test scaffolding for `make -C cuda-akaze_amd/host asan` only: it computes nothing of AKAZE and is never shipped.
#include "hipakaze.h"
#include <hip/hip_runtime_api.h>
#include <cstdlib>
#include <cstring>
#include <string>

struct hak_ctx { hak_config cfg; int w, h; int retain_best; int retain_grid; };
static std::string g_err;
int g_live_ctx = 0, g_live_dev = 0, g_live_host = 0;          // leak accounting checked by the driver

extern "C" {
const char* hak_last_error(void) { return g_err.c_str(); }
void hak_default_config(hak_config* c)
{
    memset(c, 0, sizeof(*c));
    c->noctaves = 4; c->max_scale = 4; c->per = 0.7f; c->kcontrast = 0.03f; c->soffset = 1.6f; c->reordering = 1;
    c->derivative_factor = 1.5f; c->dthreshold = 0.001f; c->diffusivity = HAK_PM_G2; c->descriptor_pattern_size = 10;
    c->max_pts = 10000; c->batch = 1;
}
int hak_create(const hak_config* cfg, int w, int h, hak_ctx** out)
{
    if (w < 80 || h < 80) { g_err = "image smaller than 80 px"; return 1; }
    *out = new hak_ctx{*cfg, w, h, 0};
    g_live_ctx++;
    return 0;
}
void hak_destroy(hak_ctx* c) { if (c) { g_live_ctx--; delete c; } }
int hak_set_retain_best(hak_ctx* c, int on) { if (!c) { g_err = "null context"; return 1; } c->retain_best = on != 0; return 0; }
int hak_set_retain_grid(hak_ctx* c, int G)
{
    if (!c) { g_err = "null context"; return 1; }
    if (G != 0 && (G < 8 || G > 128)) { g_err = "cell size out of range"; return 1; }
    c->retain_grid = G;
    return 0;
}
int hak_host_alloc(void** p, long bytes) { *p = malloc((size_t)bytes); g_live_host += *p != nullptr; return *p ? 0 : 1; }
int hak_host_free(void* p) { g_live_host--; free(p); return 0; }
int hak_points_alloc(hak_point** d, int count) { *d = (hak_point*)malloc(sizeof(hak_point) * (size_t)count); g_live_dev++; return *d ? 0 : 1; }
int hak_points_free(hak_point* d) { g_live_dev--; free(d); return 0; }
// "detects" w*h/4096 points (a number that depends on the image size), clamped to the CALL's max_pts; writes every byte of
// every record it reports, so an undersized caller buffer is an ASan error
static int fake_detect(hak_ctx* c, int pitch, hak_point* d_points, int max_pts, int* num_pts, hak_point* h_points)
{
    if (!c || !d_points || !num_pts) { g_err = "null argument"; return 1; }
    if (pitch < c->w) { g_err = "pitch smaller than width"; return 1; }
    int n = c->w * c->h / 4096;
    if (n > max_pts) n = max_pts;
    for (int i = 0; i < n; i++) {
        memset(&d_points[i], 0, sizeof(hak_point));
        d_points[i].x = (float)(i % c->w); d_points[i].y = (float)(i / c->w); d_points[i].octave = i % 16;
        d_points[i].features[i % HAK_FLEN] = (unsigned char)i;
        d_points[i].match = -1;
    }
    *num_pts = n;
    if (h_points && n) memcpy(h_points, d_points, sizeof(hak_point) * (size_t)n);
    return 0;
}
int hak_detect_and_compute(hak_ctx* c, const float* img, int pitch, hak_point* d, int max_pts, int* n, hak_point* h, int)
{ return img ? fake_detect(c, pitch, d, max_pts, n, h) : (g_err = "null image", 1); }
int hak_fast_detect_and_compute(hak_ctx* c, const unsigned char* img, int pitch, hak_point* d, int max_pts, int* n, hak_point* h, int)
{ return img ? fake_detect(c, pitch, d, max_pts, n, h) : (g_err = "null image", 1); }
int hak_match(hak_ctx*, hak_point* p1, int n1, const hak_point* p2, int n2, hak_point* h1);
int hak_detect_and_compute_pair(hak_ctx* c, const float* i1, const float* i2, int pitch, hak_point* d1, hak_point* d2, int m1, int m2,
                                int* n1, int* n2, hak_point* h1, hak_point* h2, int, int match)
{
    if (!c || c->cfg.batch < 2) { g_err = "pair call needs batch >= 2"; return 1; }
    const int clamp = m1 < m2 ? m1 : m2;
    if (!i1 || !i2 || fake_detect(c, pitch, d1, clamp, n1, nullptr) || fake_detect(c, pitch, d2, clamp, n2, nullptr)) return 1;
    if (match) hak_match(nullptr, d1, *n1, d2, *n2, nullptr);
    if (h1 && *n1) memcpy(h1, d1, sizeof(hak_point) * (size_t)*n1);
    if (h2 && *n2) memcpy(h2, d2, sizeof(hak_point) * (size_t)*n2);
    return 0;
}
int hak_match(hak_ctx*, hak_point* p1, int n1, const hak_point* p2, int n2, hak_point* h1)
{
    for (int i = 0; i < n1; i++) {
        p1[i].match = n2 ? i % n2 : -1; p1[i].distance = n2 ? 7 : -1;
        p1[i].match_x = n2 ? p2[i % n2].x : -1; p1[i].match_y = n2 ? p2[i % n2].y : -1;
        if (h1) { h1[i].match = p1[i].match; h1[i].distance = p1[i].distance; h1[i].match_x = p1[i].match_x; h1[i].match_y = p1[i].match_y; }
    }
    return 0;
}
int hak_match_knn2(hak_ctx*, hak_point* p1, int n1, const hak_point* p2, int n2, int, int, int, int, hak_point* h1,
                   hak_match_pair* d_out, int* count, hak_match_pair* h_out)
{
    hak_match(nullptr, p1, n1, p2, n2, h1);
    int c = 0;
    for (int i = 0; i < n1 && n2; i += 2, c++)
        if (d_out) { d_out[c] = hak_match_pair{i, i % n2, 7, 9, p1[i].x, p1[i].y, p2[i % n2].x, p2[i % n2].y}; if (h_out) h_out[c] = d_out[c]; }
    *count = c;
    return 0;
}
int hak_match_guided(hak_ctx*, hak_point* p1, int n1, const hak_point* p2, int n2, const float* H, float radius, int rn, int rd, int cc,
                     int md, hak_point* h1, hak_match_pair* d_out, int* count, hak_match_pair* h_out)
{
    if (!H || !(radius > 0.f) || H[8] != H[8]) { g_err = "bad argument"; return 1; }
    return hak_match_knn2(nullptr, p1, n1, p2, n2, rn, rd, cc, md, h1, d_out, count, h_out);
}
int hak_match_epipolar(hak_ctx*, hak_point* p1, int n1, const hak_point* p2, int n2, const float* F, float radius, int rn, int rd, int cc,
                       int md, hak_point* h1, hak_match_pair* d_out, int* count, hak_match_pair* h_out)
{
    if (!F || !(radius > 0.f) || F[8] != F[8]) { g_err = "bad argument"; return 1; }
    return hak_match_knn2(nullptr, p1, n1, p2, n2, rn, rd, cc, md, h1, d_out, count, h_out);
}
int hak_memcpy_h2d(void* dst, const void* src, long bytes) { memcpy(dst, src, (size_t)bytes); return 0; }
int hak_memcpy_d2h(void* dst, const void* src, long bytes) { memcpy(dst, src, (size_t)bytes); return 0; }
// reads every record and writes every mask byte (an undersized caller buffer is an ASan error); "inliers" are the even indices
int hak_find_homography(hak_ctx*, const hak_match_pair* d, int n, int iterations, float threshold, unsigned, int refine,
                        unsigned char* mask, hak_homography* out)
{
    if (!out || (n > 0 && !d) || iterations < 1 || !(threshold > 0.f) || (refine != 0 && refine != 1)) { g_err = "bad argument"; return 1; }
    *out = hak_homography{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, 0, n >= 4 ? 0 : -1, 0, n};
    for (int i = 0; i < n; i++) {
        const bool in = n >= 4 && d[i].x1 == d[i].x1 && i % 2 == 0;
        out->inliers += in;
        if (mask) mask[i] = in;
    }
    return 0;
}
// as hak_find_homography's stub: every record read, every mask byte written; "inliers" are the indices that are multiples of 3
int hak_find_fundamental(hak_ctx*, const hak_match_pair* d, int n, int iterations, float threshold, unsigned, unsigned char* mask,
                         hak_fundamental* out)
{
    if (!out || (n > 0 && !d) || iterations < 1 || !(threshold > 0.f)) { g_err = "bad argument"; return 1; }
    *out = hak_fundamental{{0.f, 0.f, 0.f, 0.f, 0.f, n >= 7 ? -1.f : 0.f, 0.f, n >= 7 ? 1.f : 0.f, 0.f}, 0, n >= 7 ? 0 : -1, 0, n};
    for (int i = 0; i < n; i++) {
        const bool in = n >= 7 && d[i].x1 == d[i].x1 && i % 3 == 0;
        out->inliers += in;
        if (mask) mask[i] = in;
    }
    return 0;
}
// as hak_find_fundamental's stub from five records on, the intrinsics read: root = 16
int hak_find_essential(hak_ctx*, const hak_match_pair* d, int n, const hak_intrinsics* K1, const hak_intrinsics* K2, int iterations,
                       float threshold, unsigned, unsigned char* mask, hak_fundamental* out)
{
    if (!out || !K1 || !K2 || (n > 0 && !d) || iterations < 1 || !(threshold > 0.f) || K1->fx == 0.f || K2->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    *out = hak_fundamental{{0.f, 0.f, 0.f, 0.f, 0.f, n >= 5 ? -1.f : 0.f, 0.f, n >= 5 ? 1.f : 0.f, 0.f}, 0, n >= 5 ? 0 : -1, n >= 5 ? 16 : 0, n};
    for (int i = 0; i < n; i++) {
        const bool in = n >= 5 && d[i].x1 == d[i].x1 && i % 3 == 0;
        out->inliers += in;
        if (mask) mask[i] = in;
    }
    return 0;
}
// as hak_find_fundamental's stub: every record read, every mask byte written, the record rewritten in place with root = 3
int hak_refine_fundamental(hak_ctx*, const hak_match_pair* d, int n, float threshold, int rounds, unsigned char* mask,
                           hak_fundamental* inout)
{
    if (!inout || (n > 0 && !d) || rounds < 1 || rounds > 8 || !(threshold > 0.f)) { g_err = "bad argument"; return 1; }
    const bool model = inout->hypothesis >= 0 && n >= 8;
    inout->inliers = 0;
    inout->root = model ? 3 : inout->root;
    inout->n = n;
    for (int i = 0; i < n; i++) {
        const bool in = model && d[i].x1 == d[i].x1 && i % 3 == 0;
        inout->inliers += in;
        if (mask) mask[i] = in;
    }
    return 0;
}
// as hak_find_fundamental's stub: every record read, every mask byte and xyz float written; F[7] == 0 stands for "no pose";
// "in front" are the indices that are multiples of 3
int hak_recover_pose(hak_ctx*, const hak_match_pair* d, int n, const float* F, const hak_intrinsics* K1, const hak_intrinsics* K2,
                     float threshold, float max_depth, unsigned char* mask, float* xyz, hak_pose* out)
{
    if (!out || !F || !K1 || !K2 || (n > 0 && !d) || !(threshold > 0.f) || !(max_depth > 0.f) || K1->fx == 0.f || K2->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    const bool model = F[7] != 0.f && F[8] == F[8];
    *out = hak_pose{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {model ? 1.f : 0.f, 0.f, 0.f}, 0, 0, model ? 0 : -1, n};
    for (int i = 0; i < n; i++) {
        const bool in = model && d[i].x1 == d[i].x1 && i % 3 == 0;
        out->inliers += in;
        out->in_front += in;
        if (mask) mask[i] = in;
        if (xyz) xyz[3 * i] = xyz[3 * i + 1] = xyz[3 * i + 2] = in ? 1.f : 0.f;
    }
    return 0;
}
// as hak_recover_pose's stub on the record handed in: a pose with t = 0 has no model; five matches or more are "refitted"
int hak_refine_pose(hak_ctx*, const hak_match_pair* d, int n, const hak_intrinsics* K1, const hak_intrinsics* K2, float threshold,
                    float max_depth, int rounds, unsigned char* mask, float* xyz, hak_pose* inout)
{
    if (!inout || !K1 || !K2 || (n > 0 && !d) || rounds < 1 || rounds > 8 || !(threshold > 0.f) || !(max_depth > 0.f) ||
        K1->fx == 0.f || K2->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    const bool model = inout->candidate >= 0 && (inout->t[0] != 0.f || inout->t[1] != 0.f || inout->t[2] != 0.f);
    inout->inliers = inout->in_front = 0;
    inout->candidate = model ? (n >= 5 ? 4 : inout->candidate) : -1;
    inout->n = n;
    for (int i = 0; i < n; i++) {
        const bool in = model && d[i].x1 == d[i].x1 && i % 3 == 0;
        inout->inliers += in;
        inout->in_front += in;
        if (mask) mask[i] = in;
        if (xyz) xyz[3 * i] = xyz[3 * i + 1] = xyz[3 * i + 2] = in ? 1.f : 0.f;
    }
    return 0;
}
// as hak_recover_pose's stub: every record and every entry of a host view read, every mask byte and xyz float written; "kept" are
// the indices that are multiples of 3, their point is (tA0 + tB0, 0, 1)
int hak_triangulate(hak_ctx*, const hak_match_pair* d, int n, const float* RtA, const float* RtB, const hak_intrinsics* KA,
                    const hak_intrinsics* KB, float threshold, float max_depth, float min_sin, unsigned char* mask, float* xyz,
                    hak_triangulation* out)
{
    if (!out || !KA || !KB || n < 0 || (n > 0 && !d) || !(threshold > 0.f) || !(max_depth > 0.f) || !(min_sin >= 0.f && min_sin < 1.f) ||
        KA->fx == 0.f || KB->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    float sum = 0.f;
    for (int k = 0; k < 12; k++) sum += (RtA ? RtA[k] : 0.f) + (RtB ? RtB[k] : 0.f);
    if (sum != sum) {
        g_err = "a host view has a non-finite entry";
        return 1;
    }
    *out = hak_triangulation{n, 0, {0, 0, 0}, 1, {0, 0}};
    for (int i = 0; i < n; i++) {
        const bool in = d[i].x1 == d[i].x1 && i % 3 == 0;
        out->kept += in;
        out->rejected[2] += !in;
        if (mask) mask[i] = in;
        if (xyz) {
            xyz[3 * i] = in ? (RtA ? RtA[9] : 0.f) + (RtB ? RtB[9] : 0.f) : 0.f;
            xyz[3 * i + 1] = 0.f;
            xyz[3 * i + 2] = in ? 1.f : 0.f;
        }
    }
    return 0;
}
// the link rule itself, on the host: every record of both lists, every used mask byte and point read, `count` records written
int hak_link_tracks(hak_ctx*, const hak_match_pair* A, int nA, const unsigned char* maskA, const float* xyzA, const hak_match_pair* B,
                    int nB, int max_index, hak_corr3d* d_out, int* count, hak_corr3d* h_out)
{
    if (!count || nA < 0 || nB < 0 || max_index < 1 || (nA > 0 && (!A || !xyzA)) || (nB > 0 && (!B || !d_out))) {
        g_err = "bad argument";
        return 1;
    }
    *count = 0;
    for (int m = 0; m < nB; m++)
        for (int a = 0; a < nA; a++)
            if (A[a].train == B[m].query && A[a].train >= 0 && A[a].train < max_index && (!maskA || maskA[a])) {
                d_out[*count] = hak_corr3d{xyzA[3 * a], xyzA[3 * a + 1], xyzA[3 * a + 2], B[m].x2, B[m].y2, a, m, 0};
                if (h_out) h_out[*count] = d_out[*count];
                ++*count;
                break;
            }
    return 0;
}
// every record of A, every used mask byte and point, the landmark's descriptor and every entry of a host view read, `count` records
// written; "accepted" are the eligible landmarks whose index is a multiple of 3, matched to keypoint m % n2 of the new image
int hak_match_projected(hak_ctx*, const hak_match_pair* A, int nA, const unsigned char* maskA, const float* xyzA, const hak_point* D,
                        int nD, const hak_point* T, int n2, const float* Rt, const hak_intrinsics* K, float radius, int ratio_num,
                        int ratio_den, int, int, hak_corr3d* d_out, int* count, hak_corr3d* h_out)
{
    if (!count || !K || nA < 0 || nD < 0 || n2 < 0 || (nA > 0 && (!A || !xyzA)) || (nD > 0 && !D) || (n2 > 0 && !T) || (h_out && !d_out) ||
        !(radius > 0.f) || ratio_num <= 0 || ratio_den <= 0 || K->fx == 0.f || K->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    float sum = 0.f;
    for (int k = 0; k < 12; k++) sum += Rt ? Rt[k] : 0.f;
    if (sum != sum) {
        g_err = "a host view has a non-finite entry";
        return 1;
    }
    *count = 0;
    for (int m = 0; m < nA; m++) {
        const int e = A[m].train;
        if (e < 0 || e >= nD || (maskA && !maskA[m]) || n2 == 0 || m % 3 != 0) continue;
        static volatile int sink;
        sink = D[e].features[60];                                           // (the descriptor's last byte is read)
        const int j = m % n2;
        const hak_corr3d r{xyzA[3 * m], xyzA[3 * m + 1], xyzA[3 * m + 2], T[j].x, T[j].y, m, j, 0};
        if (d_out) d_out[*count] = r;
        if (h_out) h_out[*count] = r;
        ++*count;
    }
    return 0;
}
// as hak_find_fundamental's stub: every record read, every mask byte written; "inliers" are the indices that are multiples of 3
int hak_solve_pnp(hak_ctx*, const hak_corr3d* d, int n, const hak_intrinsics* K, int iterations, float threshold, unsigned,
                  unsigned char* mask, hak_abs_pose* out)
{
    if (!out || !K || (n > 0 && !d) || iterations < 1 || !(threshold > 0.f) || K->fx == 0.f || K->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    *out = hak_abs_pose{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, n >= 3 ? 1.f : 0.f}, 0, n >= 3 ? 0 : -1, 0, n};
    for (int i = 0; i < n; i++) {
        const bool in = n >= 3 && d[i].X == d[i].X && i % 3 == 0;
        out->inliers += in;
        if (mask) mask[i] = in;
    }
    return 0;
}
// as hak_solve_pnp's stub: every record read, every mask byte written, the record rewritten in place with solution = 4
int hak_refine_pnp(hak_ctx*, const hak_corr3d* d, int n, const hak_intrinsics* K, float threshold, int rounds, unsigned char* mask,
                   hak_abs_pose* inout)
{
    if (!inout || !K || (n > 0 && !d) || rounds < 1 || rounds > 8 || !(threshold > 0.f) || K->fx == 0.f || K->fy == 0.f) {
        g_err = "bad argument";
        return 1;
    }
    const bool model = inout->hypothesis >= 0 && n >= 4;
    inout->inliers = 0;
    inout->solution = model ? 4 : inout->solution;
    inout->n = n;
    for (int i = 0; i < n; i++) {
        const bool in = model && d[i].X == d[i].X && i % 3 == 0;
        inout->inliers += in;
        if (mask) mask[i] = in;
    }
    return 0;
}
// the HIP runtime calls of cuMatchKnn, cuFindHomography, cuFindFundamental, cuRefineFundamental, cuRecoverPose, cuTriangulate, cuLinkTracks,
// cuMatchProjected, cuSolvePnP and cuRefinePnP
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
}

// akaze.cpp -- akaze::Akazer / initAkazeData / freeAkazeData / cuMatch over the C ABI.
// Behavioural mirror of the reference's akaze.cpp:24-150 (same call contract and error style);
// all device work happens behind hipakaze.h.
#include "akaze.h"
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>

namespace
{
    void die(const char* what)
    {
        fprintf(stderr, "hip-akaze: %s failed: %s\n", what, hak_last_error());
        exit(-1);                                                     // cuda_utils.h:23
    }
    // host buffers handed out pinned (device-visible), so that freeAkazeData knows how to release them
    std::mutex g_pinned_mu;
    std::set<void*> g_pinned;

    // The device side of a wrapper over one host list: the list's device copy, uploaded here, and the device buffers of the mask
    // and the points the caller asked for.  `name` is the wrapper's, for the messages; others_ok: its further pointers are there.
    // An empty list allocates nothing, and every pointer stays NULL.
    template <class Rec>
    struct DeviceList {
        const char* name;
        int n;
        Rec* d = nullptr;
        unsigned char* d_mask = nullptr;
        float* d_xyz = nullptr;

        DeviceList(const char* name, const Rec* h, int n, bool others_ok, bool mask, bool xyz = false) : name(name), n(n)
        {
            if (n < 0 || (n > 0 && !h) || !others_ok) { fprintf(stderr, "hip-akaze: %s: bad argument\n", name); exit(-1); }
            if (n == 0) return;
            if (hipMalloc((void**)&d, sizeof(Rec) * (size_t)n) != hipSuccess) fail("alloc");
            if (mask && hipMalloc((void**)&d_mask, (size_t)n) != hipSuccess) fail("alloc");
            if (xyz && hipMalloc((void**)&d_xyz, sizeof(float) * 3 * (size_t)n) != hipSuccess) fail("alloc");
            if (hak_memcpy_h2d(d, h, (long)(sizeof(Rec) * (size_t)n))) fail("upload");
        }
        DeviceList(const DeviceList&) = delete;
        DeviceList& operator=(const DeviceList&) = delete;
        ~DeviceList()
        {
            if (d_xyz) (void)hipFree(d_xyz);
            if (d_mask) (void)hipFree(d_mask);
            if (d) (void)hipFree(d);
        }
        void mask_to(unsigned char* h) const { if (d_mask && hak_memcpy_d2h(h, d_mask, n)) fail("download"); }
        void xyz_to(float* h) const { if (d_xyz && hak_memcpy_d2h(h, d_xyz, (long)(sizeof(float) * 3 * (size_t)n))) fail("download"); }
        void fail(const char* step) const { die((std::string(name) + " " + step).c_str()); }
    };

    // the call behind cuMatchGuided and cuMatchEpipolar: `entry` re-matches result1 against result2 under the nine floats of `model`;
    // `name` is the wrapper's, for the messages
    int match_gated(const char* name, decltype(&hak_match_guided) entry, akaze::AkazeData& result1, akaze::AkazeData& result2,
                    const float model[9], hak_match_pair* matches, float radius, int ratio_num, int ratio_den, bool cross_check)
    {
        int count = 0;
        hak_match_pair* d_out = nullptr;
        const int cap = result1.num_pts > 0 ? result1.num_pts : 1;
        if (matches && hipMalloc((void**)&d_out, sizeof(hak_match_pair) * (size_t)cap) != hipSuccess)
            die((std::string(name) + " alloc").c_str());
        if (entry(NULL, result1.d_data, result1.num_pts, result2.d_data, result2.num_pts, model, radius, ratio_num, ratio_den,
                  cross_check ? 1 : 0, 0, result1.h_data, d_out, &count, matches))
            die(name);
        if (d_out) (void)hipFree(d_out);
        return count;
    }
}

namespace akaze
{
    void initAkazeData(AkazeData& data, const int max_pts, const bool host, const bool dev)       // akaze.cpp:26-40
    {
        data.num_pts = 0;
        data.max_pts = max_pts;
        data.h_data = NULL;
        if (host) {
            // pinned host memory: detectAndCompute's launch sequence writes the records (and the count) straight into it, so a
            // call ends with ONE synchronisation instead of a count copy, a sync and a record copy (akaze.cpp:134-139 does the
            // latter on pageable memory).  Without a usable device the plain allocation of the reference remains.
            void* p = NULL;
            if (hak_host_alloc(&p, (long)(sizeof(AkazePoint) * (size_t)max_pts)) == 0 && p) {
                std::lock_guard<std::mutex> lock(g_pinned_mu);
                g_pinned.insert(p);
            } else p = malloc(sizeof(AkazePoint) * (size_t)max_pts);
            data.h_data = (AkazePoint*)p;
        }
        data.d_data = NULL;
        if (dev && hak_points_alloc(&data.d_data, max_pts)) die("initAkazeData");
    }

    void freeAkazeData(AkazeData& data)                                                          // akaze.cpp:43-52
    {
        if (data.d_data != NULL && hak_points_free(data.d_data)) die("freeAkazeData");
        if (data.h_data != NULL) {
            bool pinned;
            { std::lock_guard<std::mutex> lock(g_pinned_mu); pinned = g_pinned.erase(data.h_data) > 0; }
            if (pinned) { if (hak_host_free(data.h_data)) die("freeAkazeData"); }
            else free(data.h_data);
        }
        data.d_data = NULL;
        data.h_data = NULL;
        data.num_pts = 0;
        data.max_pts = 0;
    }

    void cuMatch(AkazeData& result1, AkazeData& result2)                                         // akaze.cpp:55-64
    {
        if (hak_match(NULL, result1.d_data, result1.num_pts, result2.d_data, result2.num_pts, result1.h_data))
            die("cuMatch");
    }

    int cuMatchKnn(AkazeData& result1, AkazeData& result2, hak_match_pair* matches, int ratio_num, int ratio_den, bool cross_check)
    {
        int count = 0;
        hak_match_pair* d_out = nullptr;
        const int cap = result1.num_pts > 0 ? result1.num_pts : 1;
        if (matches && hipMalloc((void**)&d_out, sizeof(hak_match_pair) * (size_t)cap) != hipSuccess) die("cuMatchKnn alloc");
        if (hak_match_knn2(NULL, result1.d_data, result1.num_pts, result2.d_data, result2.num_pts, ratio_num, ratio_den,
                           cross_check ? 1 : 0, 0, result1.h_data, d_out, &count, matches))
            die("cuMatchKnn");
        if (d_out) (void)hipFree(d_out);
        return count;
    }

    int cuMatchGuided(AkazeData& result1, AkazeData& result2, const float H[9], hak_match_pair* matches, float radius, int ratio_num,
                      int ratio_den, bool cross_check)
    {
        return match_gated("cuMatchGuided", hak_match_guided, result1, result2, H, matches, radius, ratio_num, ratio_den, cross_check);
    }

    int cuMatchEpipolar(AkazeData& result1, AkazeData& result2, const float F[9], hak_match_pair* matches, float radius, int ratio_num,
                        int ratio_den, bool cross_check)
    {
        return match_gated("cuMatchEpipolar", hak_match_epipolar, result1, result2, F, matches, radius, ratio_num, ratio_den, cross_check);
    }

    int cuFindHomography(const hak_match_pair* matches, int n, float H[9], unsigned char* inlier_mask, int iterations, float threshold,
                         unsigned seed, bool refine)
    {
        DeviceList<hak_match_pair> l("cuFindHomography", matches, n, H != nullptr, inlier_mask != nullptr);
        hak_homography r;
        if (hak_find_homography(NULL, l.d, n, iterations, threshold, seed, refine ? 1 : 0, l.d_mask, &r)) die(l.name);
        l.mask_to(inlier_mask);
        for (int k = 0; k < 9; k++) H[k] = r.H[k];
        return r.inliers;
    }

    int cuFindFundamental(const hak_match_pair* matches, int n, float F[9], unsigned char* inlier_mask, int iterations, float threshold,
                          unsigned seed)
    {
        DeviceList<hak_match_pair> l("cuFindFundamental", matches, n, F != nullptr, inlier_mask != nullptr);
        hak_fundamental r;
        if (hak_find_fundamental(NULL, l.d, n, iterations, threshold, seed, l.d_mask, &r)) die(l.name);
        l.mask_to(inlier_mask);
        for (int k = 0; k < 9; k++) F[k] = r.F[k];
        return r.inliers;
    }

    int cuFindEssential(const hak_match_pair* matches, int n, const hak_intrinsics& K1, const hak_intrinsics& K2, float F[9],
                        unsigned char* inlier_mask, int iterations, float threshold, unsigned seed)
    {
        DeviceList<hak_match_pair> l("cuFindEssential", matches, n, F != nullptr, inlier_mask != nullptr);
        hak_fundamental r;
        if (hak_find_essential(NULL, l.d, n, &K1, &K2, iterations, threshold, seed, l.d_mask, &r)) die(l.name);
        l.mask_to(inlier_mask);
        for (int k = 0; k < 9; k++) F[k] = r.F[k];
        return r.inliers;
    }

    int cuRefineFundamental(const hak_match_pair* matches, int n, float F[9], unsigned char* inlier_mask, float threshold, int rounds)
    {
        DeviceList<hak_match_pair> l("cuRefineFundamental", matches, n, F != nullptr, inlier_mask != nullptr);
        hak_fundamental r{};
        for (int k = 0; k < 9; k++) r.F[k] = F[k];
        r.n = n;
        if (hak_refine_fundamental(NULL, l.d, n, threshold, rounds, l.d_mask, &r)) die(l.name);
        l.mask_to(inlier_mask);
        for (int k = 0; k < 9; k++) F[k] = r.F[k];
        return r.inliers;
    }

    int cuRecoverPose(const hak_match_pair* matches, int n, const float F[9], const hak_intrinsics& K1, const hak_intrinsics& K2,
                      float R[9], float t[3], unsigned char* front_mask, float threshold, float max_depth)
    {
        DeviceList<hak_match_pair> l("cuRecoverPose", matches, n, F && R && t, front_mask != nullptr);
        hak_pose r;
        if (hak_recover_pose(NULL, l.d, n, F, &K1, &K2, threshold, max_depth, l.d_mask, NULL, &r)) die(l.name);
        l.mask_to(front_mask);
        for (int k = 0; k < 9; k++) R[k] = r.R[k];
        for (int k = 0; k < 3; k++) t[k] = r.t[k];
        return r.candidate < 0 ? -1 : r.in_front;
    }

    int cuRefinePose(const hak_match_pair* matches, int n, const hak_intrinsics& K1, const hak_intrinsics& K2, float R[9], float t[3],
                     unsigned char* front_mask, float threshold, float max_depth, int rounds)
    {
        DeviceList<hak_match_pair> l("cuRefinePose", matches, n, R && t, front_mask != nullptr);
        hak_pose r{};
        for (int k = 0; k < 9; k++) r.R[k] = R[k];
        for (int k = 0; k < 3; k++) r.t[k] = t[k];
        r.n = n;
        if (hak_refine_pose(NULL, l.d, n, &K1, &K2, threshold, max_depth, rounds, l.d_mask, NULL, &r)) die(l.name);
        l.mask_to(front_mask);
        for (int k = 0; k < 9; k++) R[k] = r.R[k];
        for (int k = 0; k < 3; k++) t[k] = r.t[k];
        return r.candidate < 0 ? -1 : r.in_front;
    }

    int cuTriangulate(const hak_match_pair* matches, int n, const float* RtA, const float* RtB, const hak_intrinsics& KA,
                      const hak_intrinsics& KB, float* xyz, unsigned char* mask, float threshold, float max_depth, float min_sin)
    {
        DeviceList<hak_match_pair> l("cuTriangulate", matches, n, true, mask != nullptr, xyz != nullptr);
        hak_triangulation r;
        if (hak_triangulate(NULL, l.d, n, RtA, RtB, &KA, &KB, threshold, max_depth, min_sin, l.d_mask, l.d_xyz, &r)) die(l.name);
        l.mask_to(mask);
        l.xyz_to(xyz);
        return r.kept;
    }

    int cuLinkTracks(const hak_match_pair* A, int nA, const float* xyzA, const unsigned char* maskA, const hak_match_pair* B, int nB,
                     int max_index, hak_corr3d* out)
    {
        if (nA < 0 || nB < 0 || (nA > 0 && (!A || !xyzA)) || (nB > 0 && (!B || !out))) {
            fprintf(stderr, "hip-akaze: cuLinkTracks: bad argument\n");
            exit(-1);
        }
        if (nA == 0 || nB == 0) return 0;
        // one device block: A | B | out | xyzA | maskA (the 32-byte records first: every part stays 16-byte aligned)
        const size_t rec = sizeof(hak_match_pair), bytesA = rec * (size_t)nA, bytesB = rec * (size_t)nB;
        const size_t bytesX = sizeof(float) * 3 * (size_t)nA;
        char* d = nullptr;
        if (hipMalloc((void**)&d, bytesA + 2 * bytesB + bytesX + (maskA ? (size_t)nA : 0)) != hipSuccess) die("cuLinkTracks alloc");
        hak_match_pair* d_A = reinterpret_cast<hak_match_pair*>(d);
        hak_match_pair* d_B = reinterpret_cast<hak_match_pair*>(d + bytesA);
        hak_corr3d* d_out = reinterpret_cast<hak_corr3d*>(d + bytesA + bytesB);
        float* d_xyz = reinterpret_cast<float*>(d + bytesA + 2 * bytesB);
        unsigned char* d_mask = maskA ? reinterpret_cast<unsigned char*>(d + bytesA + 2 * bytesB + bytesX) : nullptr;
        if (hak_memcpy_h2d(d_A, A, (long)bytesA) || hak_memcpy_h2d(d_B, B, (long)bytesB) || hak_memcpy_h2d(d_xyz, xyzA, (long)bytesX) ||
            (maskA && hak_memcpy_h2d(d_mask, maskA, nA)))
            die("cuLinkTracks upload");
        int count = 0;
        if (hak_link_tracks(NULL, d_A, nA, d_mask, d_xyz, d_B, nB, max_index, d_out, &count, out)) die("cuLinkTracks");
        (void)hipFree(d);
        return count;
    }

    int cuMatchProjected(const hak_match_pair* A, int nA, const float* xyzA, const unsigned char* maskA, AkazeData& result_desc,
                         AkazeData& result2, const float* Rt, const hak_intrinsics& K, hak_corr3d* out, float radius, int ratio_num,
                         int ratio_den, bool cross_check)
    {
        if (nA < 0 || (nA > 0 && (!A || !xyzA))) {
            fprintf(stderr, "hip-akaze: cuMatchProjected: bad argument\n");
            exit(-1);
        }
        if (nA == 0) return 0;
        // one device block: A | out | xyzA | maskA (the 32-byte records first: every part stays 16-byte aligned)
        const size_t bytesA = sizeof(hak_match_pair) * (size_t)nA, bytesO = out ? sizeof(hak_corr3d) * (size_t)nA : 0;
        const size_t bytesX = sizeof(float) * 3 * (size_t)nA;
        char* d = nullptr;
        if (hipMalloc((void**)&d, bytesA + bytesO + bytesX + (maskA ? (size_t)nA : 0)) != hipSuccess) die("cuMatchProjected alloc");
        hak_match_pair* d_A = reinterpret_cast<hak_match_pair*>(d);
        hak_corr3d* d_out = out ? reinterpret_cast<hak_corr3d*>(d + bytesA) : nullptr;
        float* d_xyz = reinterpret_cast<float*>(d + bytesA + bytesO);
        unsigned char* d_mask = maskA ? reinterpret_cast<unsigned char*>(d + bytesA + bytesO + bytesX) : nullptr;
        if (hak_memcpy_h2d(d_A, A, (long)bytesA) || hak_memcpy_h2d(d_xyz, xyzA, (long)bytesX) || (maskA && hak_memcpy_h2d(d_mask, maskA, nA)))
            die("cuMatchProjected upload");
        int count = 0;
        if (hak_match_projected(NULL, d_A, nA, d_mask, d_xyz, result_desc.d_data, result_desc.num_pts, result2.d_data, result2.num_pts, Rt,
                                &K, radius, ratio_num, ratio_den, cross_check ? 1 : 0, 0, d_out, &count, out))
            die("cuMatchProjected");
        (void)hipFree(d);
        return count;
    }

    int cuSolvePnP(const hak_corr3d* corr, int n, const hak_intrinsics& K, float R[9], float t[3], unsigned char* inlier_mask,
                   int iterations, float threshold, unsigned seed)
    {
        DeviceList<hak_corr3d> l("cuSolvePnP", corr, n, R && t, inlier_mask != nullptr);
        hak_abs_pose r;
        if (hak_solve_pnp(NULL, l.d, n, &K, iterations, threshold, seed, l.d_mask, &r)) die(l.name);
        l.mask_to(inlier_mask);
        for (int k = 0; k < 9; k++) R[k] = r.R[k];
        for (int k = 0; k < 3; k++) t[k] = r.t[k];
        return r.hypothesis < 0 ? -1 : r.inliers;
    }

    int cuRefinePnP(const hak_corr3d* corr, int n, const hak_intrinsics& K, float R[9], float t[3], unsigned char* inlier_mask,
                    float threshold, int rounds)
    {
        DeviceList<hak_corr3d> l("cuRefinePnP", corr, n, R && t, inlier_mask != nullptr);
        hak_abs_pose r{};
        for (int k = 0; k < 9; k++) r.R[k] = R[k];
        for (int k = 0; k < 3; k++) r.t[k] = t[k];
        r.n = n;
        if (hak_refine_pnp(NULL, l.d, n, &K, threshold, rounds, l.d_mask, &r)) die(l.name);
        l.mask_to(inlier_mask);
        for (int k = 0; k < 9; k++) R[k] = r.R[k];
        for (int k = 0; k < 3; k++) t[k] = r.t[k];
        return r.inliers;
    }

    Akazer::Akazer() { hak_default_config(&cfg); }

    Akazer::~Akazer() { hak_destroy(ctx); }                              // akaze.cpp:74-77

    void Akazer::setMaxPoints(int max_pts) { cfg.max_pts = max_pts; hak_destroy(ctx); ctx = nullptr; }
    void Akazer::setUpright(bool upright) { cfg.upright = upright ? 1 : 0; hak_destroy(ctx); ctx = nullptr; }
    void Akazer::setRetainBest(bool on)
    {
        retain_best = on;
        if (ctx && hak_set_retain_best(ctx, on ? 1 : 0)) die("setRetainBest");
    }

    void Akazer::setRetainGrid(int G)
    {
        if (G != 0 && (G < 8 || G > 128)) die("setRetainGrid: the cell size must be 0 or between 8 and 128");
        retain_grid = G;
        if (ctx && hak_set_retain_grid(ctx, G)) die("setRetainGrid");
    }

    void Akazer::ensureContext(int w, int h)
    {
        if (ctx && ctx_w == w && ctx_h == h) return;
        hak_destroy(ctx);
        ctx = nullptr;
        if (hak_create(&cfg, w, h, &ctx)) die("Akazer: hak_create");
        if (retain_best && hak_set_retain_best(ctx, 1)) die("Akazer: hak_set_retain_best");
        if (retain_grid && hak_set_retain_grid(ctx, retain_grid)) die("Akazer: hak_set_retain_grid");
        ctx_w = w;
        ctx_h = h;
    }

    void Akazer::init(int3 whp0, int _noctaves, int _max_scale, float _per, float _kcontrast, float _soffset, bool _reordering,
                      float _derivative_factor, float _dthreshold, int _diffusivity, int _descriptor_pattern_size)
    {
        whp = whp0;                                                                             // akaze.cpp:83-95
        cfg.noctaves = _noctaves;
        cfg.max_scale = _max_scale;
        cfg.per = _per;
        cfg.kcontrast = _kcontrast;
        cfg.soffset = _soffset;
        cfg.reordering = _reordering ? 1 : 0;
        cfg.derivative_factor = _derivative_factor;
        cfg.dthreshold = _dthreshold;
        cfg.diffusivity = _diffusivity;
        cfg.descriptor_pattern_size = _descriptor_pattern_size;
        // ONE context serves detectAndCompute (one image of it) and detectAndComputePair (both): a second context would double the
        // streams of the process, and launch chains that share a hardware queue run one after the other
        cfg.batch = 2;
        hak_destroy(ctx);
        ctx = nullptr;
        ensureContext(whp.x, whp.y);                  // arena allocated once for the init size ("reused", akaze.cpp:109-113)
    }

    void Akazer::detectAndCompute(float* image, AkazeData& result, int3 whp0, const bool desc)   // akaze.cpp:101-150
    {
        ensureContext(whp0.x, whp0.y);                // other size than init(): new arena (akaze.cpp:114-117)
        // the clamp of THIS call is result.max_pts, as the reference's setMaxNumPoints(result.max_pts) (akaze.cpp:246, 451);
        // nothing in the context is sized by it, so neither a smaller nor a larger AkazeData rebuilds anything
        if (hak_detect_and_compute(ctx, image, whp0.z, result.d_data, result.max_pts, &result.num_pts, result.h_data, desc ? 1 : 0))
            die("detectAndCompute");
    }

    void Akazer::detectAndComputePair(float* image1, float* image2, AkazeData& result1, AkazeData& result2, int3 whp0, const bool desc,
                                      const bool match)
    {
        ensureContext(whp0.x, whp0.y);
        if (hak_detect_and_compute_pair(ctx, image1, image2, whp0.z, result1.d_data, result2.d_data, result1.max_pts, result2.max_pts,
                                        &result1.num_pts, &result2.num_pts, result1.h_data, result2.h_data, desc ? 1 : 0, match ? 1 : 0))
            die("detectAndComputePair");
    }

    void Akazer::fastDetectAndCompute(unsigned char* image, AkazeData& result, int3 whp0, const bool desc)   // akaze.cpp:153-201
    {
        ensureContext(whp0.x, whp0.y);
        if (hak_fast_detect_and_compute(ctx, image, whp0.z, result.d_data, result.max_pts, &result.num_pts, result.h_data, desc ? 1 : 0))
            die("fastDetectAndCompute");
    }
}

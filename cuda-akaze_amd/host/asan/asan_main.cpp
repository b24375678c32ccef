// asan_main.cpp -- drives host/akaze.cpp (the C++ drop-in layer) against stub_hipakaze.cpp under ASan + UBSan:
// the call patterns of the reference demo (main.cpp:190-232) plus the layer's own edge cases.
#include "akaze.h"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

extern int g_live_ctx, g_live_dev, g_live_host;
#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "asan_main: %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main()
{
    using namespace akaze;
    std::vector<float> img(1920 * 1080, 0.5f);
    std::vector<unsigned char> img8(1920 * 1080, 128);
    {
        AkazeData d1, d2, small, hostless, devless;
        initAkazeData(d1, 10000, true, true);                       // main.cpp:193-194
        initAkazeData(d2, 10000, true, true);
        initAkazeData(small, 7, true, true);                        // a clamp far below what the image holds
        initAkazeData(hostless, 10000, false, true);
        initAkazeData(devless, 100, true, false);
        REQUIRE(hostless.h_data == NULL && devless.d_data == NULL && g_live_host == 4 && g_live_dev == 4);
        std::unique_ptr<Akazer> det(new Akazer);
        int3 whp{1920, 1080, 1920};
        det->init(whp, 4, 4, 0.7f, 0.03f, 1.6f, true, 1.5f, 0.001f, 1, 10);
        REQUIRE(g_live_ctx == 1);
        for (int i = 0; i < 3; i++) {                               // main.cpp:199-205
            det->detectAndCompute(img.data(), d1, whp, true);
            det->detectAndCompute(img.data(), d2, whp, true);
        }
        REQUIRE(d1.num_pts == 1920 * 1080 / 4096 && d1.h_data[d1.num_pts - 1].match == -1);
        cuMatch(d1, d2);                                            // main.cpp:209
        REQUIRE(d1.h_data[5].match == 5 && d1.h_data[5].distance == 7);
        det->detectAndCompute(img.data(), small, whp, true);        // per-call clamp = the caller's max_pts (akaze.cpp:246, 451)
        REQUIRE(small.num_pts == 7);
        det->detectAndCompute(img.data(), hostless, whp, false);    // no host copy requested
        REQUIRE(hostless.num_pts == d1.num_pts);
        int3 whp2{1280, 720, 1280};                                 // another size than init(): a new arena (akaze.cpp:114-117)
        det->detectAndCompute(img.data(), d2, whp2, true);
        REQUIRE(d2.num_pts == 1280 * 720 / 4096 && g_live_ctx == 1);
        det->fastDetectAndCompute(img8.data(), d2, whp, true);
        REQUIRE(d2.num_pts == d1.num_pts && g_live_ctx == 1);
        std::vector<hak_match_pair> pairs(d1.num_pts);
        REQUIRE(cuMatchKnn(d1, d2, pairs.data()) == (d1.num_pts + 1) / 2 && pairs[1].query == 2);
        REQUIRE(cuMatchKnn(d1, d2, NULL) == (d1.num_pts + 1) / 2);
        {                                                           // RANSAC over the host list: exact-size buffers
            const int np = (d1.num_pts + 1) / 2;
            std::vector<unsigned char> mask(np);
            float H[9], F[9];
            REQUIRE(cuFindHomography(pairs.data(), np, H, mask.data()) == (np + 1) / 2 && mask[2] == 1 && mask[1] == 0);
            REQUIRE(cuFindFundamental(pairs.data(), np, F, mask.data()) == (np + 2) / 3 && mask[3] == 1 && mask[1] == 0 && F[7] == 1.f);
            REQUIRE(cuFindFundamental(pairs.data(), np, F) == (np + 2) / 3);
            REQUIRE(cuFindFundamental(pairs.data(), 6, F, mask.data()) == 0 && F[7] == 0.f && mask[0] == 0);
            REQUIRE(cuFindFundamental(NULL, 0, F) == 0);
            REQUIRE(cuFindFundamental(pairs.data(), np, F) == (np + 2) / 3);
            REQUIRE(cuRefineFundamental(pairs.data(), np, F, mask.data()) == (np + 2) / 3 && mask[3] == 1 && mask[1] == 0 && F[7] == 1.f);
            const hak_intrinsics K{1500.f, 1500.f, 960.f, 540.f};      // pose over the host list: exact-size mask
            float R[9], t[3];
            {                                                       // the calibrated estimator: exact-size list and mask
                float E[9];
                REQUIRE(cuFindEssential(pairs.data(), np, K, K, E, mask.data()) == (np + 2) / 3 && mask[3] == 1 && mask[1] == 0 && E[7] == 1.f);
                REQUIRE(cuFindEssential(pairs.data(), 4, K, K, E, mask.data()) == 0 && E[7] == 0.f && mask[0] == 0);
                REQUIRE(cuFindEssential(pairs.data(), np, K, K, E) == (np + 2) / 3 && cuFindEssential(NULL, 0, K, K, E) == 0);
            }
            REQUIRE(cuRecoverPose(pairs.data(), np, F, K, K, R, t, mask.data()) == (np + 2) / 3 && mask[3] == 1 && mask[1] == 0 &&
                    R[4] == 1.f && t[0] == 1.f);
            REQUIRE(cuRecoverPose(pairs.data(), np, F, K, K, R, t) == (np + 2) / 3);
            REQUIRE(cuRecoverPose(NULL, 0, F, K, K, R, t) == 0);
            F[7] = 0.f;                                                 // the stub's "no pose"
            REQUIRE(cuRecoverPose(pairs.data(), np, F, K, K, R, t, mask.data()) == -1 && t[0] == 0.f && mask[3] == 0);
            {                                                           // triangulation: exact-size mask and points, host views
                std::vector<float> xyz(3 * (size_t)np);
                const float RtB[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, -1.f, 0.f, 0.f};
                REQUIRE(cuTriangulate(pairs.data(), np, NULL, RtB, K, K, xyz.data(), mask.data()) == (np + 2) / 3 && mask[3] == 1 &&
                        mask[1] == 0 && xyz[9] == -1.f && xyz[11] == 1.f && xyz[3] == 0.f && xyz[3 * (size_t)np - 1] == ((np - 1) % 3 ? 0.f : 1.f));
                REQUIRE(cuTriangulate(pairs.data(), np, RtB, RtB, K, K, xyz.data()) == (np + 2) / 3 && xyz[9] == -2.f);
                REQUIRE(cuTriangulate(pairs.data(), np, RtB, NULL, K, K, NULL, mask.data()) == (np + 2) / 3 && mask[3] == 1);
                REQUIRE(cuTriangulate(NULL, 0, NULL, RtB, K, K, NULL) == 0);
            }
            std::vector<hak_corr3d> corr(np);                           // absolute pose and its refit: exact-size list and mask
            for (int i = 0; i < np; i++) corr[i] = hak_corr3d{(float)i, 1.f, 5.f, pairs[i].x2, pairs[i].y2, i, i, 0};
            REQUIRE(cuSolvePnP(corr.data(), np, K, R, t, mask.data()) == (np + 2) / 3 && mask[3] == 1 && mask[1] == 0 && t[2] == 1.f);
            mask[3] = 0;
            REQUIRE(cuRefinePnP(corr.data(), np, K, R, t, mask.data()) == (np + 2) / 3 && mask[3] == 1 && mask[1] == 0 && t[2] == 1.f);
            REQUIRE(cuRefinePnP(corr.data(), np, K, R, t) == (np + 2) / 3);
            REQUIRE(cuRefinePnP(corr.data(), 3, K, R, t, mask.data()) == 0 && mask[0] == 0);
            REQUIRE(cuRefinePnP(NULL, 0, K, R, t) == 0);
            {                                                           // projection-guided matching: exact-size list, points, mask and output
                std::vector<float> xyz(3 * (size_t)np, 2.f);
                std::vector<unsigned char> use(np, 1);
                use[3] = 0;
                const float Rt[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 1.f};
                REQUIRE(cuMatchProjected(pairs.data(), np, xyz.data(), NULL, d2, d1, Rt, K, corr.data()) == (np + 2) / 3 &&
                        corr[1].src3d == 3 && corr[1].src2d == 3 % d1.num_pts && corr[1].Z == 2.f && corr[1].u == d1.h_data[3 % d1.num_pts].x);
                REQUIRE(cuMatchProjected(pairs.data(), np, xyz.data(), use.data(), d2, d1, NULL, K, corr.data()) == (np + 2) / 3 - 1 &&
                        corr[1].src3d == 6);
                REQUIRE(cuMatchProjected(pairs.data(), np, xyz.data(), use.data(), d2, d1, Rt, K, NULL) == (np + 2) / 3 - 1);
                REQUIRE(cuMatchProjected(NULL, 0, NULL, NULL, d2, d1, Rt, K, NULL) == 0);
            }
        }
        cuMatch(d1, hostless);                                      // train side without a host buffer
        d2.num_pts = 0;
        cuMatch(d1, d2);                                            // empty train set (D10)
        REQUIRE(d1.h_data[0].match == -1);
        // the pair call on the same (two-image) context; results as the three calls give them; the smaller capacity is the clamp
        det->detectAndComputePair(img.data(), img.data(), d1, d2, whp, true, true);
        REQUIRE(d1.num_pts == 1920 * 1080 / 4096 && d2.num_pts == d1.num_pts && d1.h_data[7].match == 7 && g_live_ctx == 1);
        det->detectAndComputePair(img.data(), img.data(), d1, small, whp, true, false);
        REQUIRE(d1.num_pts == 7 && small.num_pts == 7);
        det->detectAndComputePair(img.data(), img.data(), d1, d2, whp2, false, true);   // another size: the context is rebuilt
        REQUIRE(d1.num_pts == 1280 * 720 / 4096 && g_live_ctx == 1);
        det->setMaxPoints(500);                                     // drops the context; the next call rebuilds it
        det->setUpright(true);
        REQUIRE(g_live_ctx == 0);
        det->detectAndCompute(img.data(), d1, whp, true);
        det->init(whp2, 3, 3, 0.7f, 0.03f, 1.2f, false, 1.5f, 0.001f, 3, 8);    // re-init replaces the context
        REQUIRE(g_live_ctx == 1);
        freeAkazeData(d1); freeAkazeData(d2); freeAkazeData(small); freeAkazeData(hostless); freeAkazeData(devless);
        freeAkazeData(d1);                                          // freeing twice is harmless (pointers are reset)
        REQUIRE(d1.h_data == NULL && d1.max_pts == 0);
    }
    REQUIRE(g_live_ctx == 0 && g_live_dev == 0 && g_live_host == 0);
    printf("asan_main: host layer clean\n");
    return 0;
}

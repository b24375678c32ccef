// main.cpp -- counterpart of the reference demo cudaAkazeDemo2 (main.cpp:128-233) without OpenCV:
// reads two binary PGMs (or synthesises a pair), uploads them, runs detectAndCompute on both images
// `nrepeats` times and cuMatch once, and prints the same five result lines.
//
//   hipakaze_demo [device] [left.pgm right.pgm] [nrepeats] [--dump file] [--api-checks] [--pair] [--homography] [--retain-best N]
//                 [--retain-grid G] [--guided R] [--fundamental] [--refine N] [--epipolar R] [--pose FX FY CX CY] [--pose-refine N]
//                 [--essential FX FY CX CY]
//
// --dump file   writes the host-side results as raw 104-byte AkazePoint records:
//               int32 n1, n2, then n1 + n2 records of the float path (image 1 after cuMatch),
//               then int32 f1, f2 and f1 + f2 records of the FAST path (image 1 after cuMatch).
// --pair        the loop calls Akazer::detectAndComputePair (both images + cuMatch in ONE launch sequence, akaze.h) instead of
//               detectAndCompute x 2 (+ cuMatch after the loop); the printed counts and the dumped records are the same
// --api-checks  additionally drives Akazer through the call patterns of akaze.cpp:101-150 that the demo loop does not:
//               an AkazeData smaller and larger than the default capacity, and an image size other than init()'s.
// --homography  after the 2-NN match, estimates the homography between the two images from its matches (cuFindHomography: RANSAC,
//               1024 hypotheses, 3 px, seed 0, least-squares refit) and prints it; with --dump, appends at the very end of the file
//               int32 n, int32 inliers, float32 H[9], the n 32-byte hak_match_pair records and the n inlier-mask bytes.
// --guided R   implies --homography; after RANSAC re-matches the pair under that homography (cuMatchGuided: every keypoint of image 1
//               is searched only within R pixels of where H sends it; ratio 4/5 + cross-check inside that neighbourhood), runs
//               cuFindHomography again on the guided list and prints both match and inlier counts
// --fundamental  after the 2-NN match, estimates the fundamental matrix between the two images from its matches (cuFindFundamental:
//               RANSAC, 1024 seven-point hypotheses, Sampson distance < 1 px, seed 0, no refit) and prints it; with --dump, appends
//               after everything else int32 n, int32 inliers, float32 F[9], the n hak_match_pair records and the n inlier-mask bytes
// --refine N    implies --fundamental; behind RANSAC refits F over its inliers, up to N rounds of 1..8 (cuRefineFundamental: rank-2
//               least squares, kept when it scores at least as well), prints the inlier count before and after, and F, the count
//               and the mask of the dump and of --epipolar are the refitted ones
// --epipolar R  implies --fundamental; after RANSAC re-matches the pair under that fundamental matrix (cuMatchEpipolar: every keypoint
//               of image 1 is searched only within R pixels of its epipolar line; ratio 4/5 + cross-check inside that band), runs
//               cuFindFundamental again on the new list and prints both match and inlier counts
// --pose FX FY CX CY  implies --fundamental; behind RANSAC (and --refine) recovers the relative pose of the two images from F and the
//               pinhole intrinsics, the same for both cameras (hak_recover_pose: 1 px, no depth limit), and prints R, the unit
//               baseline direction t and the counts; with --dump, appends after the fundamental section the 64-byte hak_pose record,
//               the n front-mask bytes and the 3 n float32 of the points
// --pose-refine N  behind --pose (ignored without it) refits that pose with the calibration over the matches that count under it, up
//               to N rounds of 1..8 (cuRefinePose: 1 px, no depth limit), and prints the refitted R, t and the count; with --dump,
//               appends after the pose section the refitted R (9 float32), t (3 float32), the count (int32, -1 = no pose) and the n
//               bytes of its front mask
// --essential FX FY CX CY  takes the place of --fundamental in front of --pose / --pose-refine / --epipolar (and of the dump's
//               fundamental section): estimates the essential matrix under these pinhole intrinsics, the same for both cameras
//               (cuFindEssential: RANSAC, 1024 five-point hypotheses, Sampson distance < 1 px, seed 0) and prints F = K^-T E K^-1;
//               --refine still refits it as a fundamental matrix, which gives up the essential constraints
// --retain-best N  both AkazeData get capacity N (instead of 10000) and Akazer::setRetainBest(true): an image with more keypoints
//               keeps its N strongest (hak_set_retain_best), in raster order, on the float and the FAST path alike
// --retain-grid G  Akazer::setRetainGrid(G), G in 8..128: an image with more keypoints than the capacity (N of --retain-best, else
//               10000) keeps the best of every G x G pixel cell (hak_set_retain_grid); with both options G decides the policy
#include "akaze.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

static bool readPgm(const std::string& path, std::vector<unsigned char>& px, int& w, int& h)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::string magic;
    f >> magic;
    if (magic != "P5") return false;
    auto next = [&]() {
        std::string t;
        while (f >> t) {
            if (t[0] == '#') { std::getline(f, t); continue; }
            return std::stoi(t);
        }
        return -1;
    };
    w = next(); h = next();
    int maxv = next();
    if (w <= 0 || h <= 0 || maxv != 255) return false;
    f.get();
    px.resize((size_t)w * h);
    f.read((char*)px.data(), px.size());
    return (bool)f;
}

static void synthPair(std::vector<unsigned char>& a, std::vector<unsigned char>& b, int w, int h)
{
    a.resize((size_t)w * h); b.resize((size_t)w * h);
    unsigned s = 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };      // xorshift32, seed 1
    std::vector<float> img((size_t)w * h);
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) img[(size_t)y * w + x] = 0.35f + 0.25f * x / w + 0.15f * y / h;
    for (int n = 0; n < 180; n++) {
        int cx = rnd() % w, cy = rnd() % h, rw = 8 + rnd() % (w / 10), rh = 8 + rnd() % (h / 10);
        float amp = (0.08f + (rnd() % 1000) * 0.00037f) * ((rnd() & 1) ? 1.f : -1.f);
        for (int y = std::max(0, cy - rh / 2); y < std::min(h, cy + rh / 2); y++)
            for (int x = std::max(0, cx - rw / 2); x < std::min(w, cx + rw / 2); x++) img[(size_t)y * w + x] += amp;
    }
    for (size_t i = 0; i < img.size(); i++) a[i] = (unsigned char)std::min(255.f, std::max(0.f, std::round(img[i] * 255.f)));
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++)          // second view: 20 px shift
        b[(size_t)y * w + x] = a[(size_t)std::min(h - 1, y + 20) * w + std::min(w - 1, x + 20)];
}

static void dumpPoints(std::ofstream& f, const akaze::AkazeData& a, const akaze::AkazeData& b)
{
    const int n[2] = {a.num_pts, b.num_pts};
    f.write((const char*)n, sizeof(n));
    f.write((const char*)a.h_data, sizeof(akaze::AkazePoint) * (size_t)a.num_pts);
    f.write((const char*)b.h_data, sizeof(akaze::AkazePoint) * (size_t)b.num_pts);
}

int main(int argc, char** argv)
{
    // One image per call keeps four launch chains in flight: ask the HIP runtime for more than its default of four
    // hardware queues -- before its first call, and only if the user has not chosen a value ("Hardware queues")
    // (--pair: one launch sequence per call, replayed as a graph -- the runtime's default of four queues is the better one there)
    {
        bool pair = false;
        for (int i = 1; i < argc; i++) pair |= !strcmp(argv[i], "--pair");
        if (!pair) setenv("GPU_MAX_HW_QUEUES", "8", 0);
    }
    std::cout << "===== Registration by HIP-AKAZE (MI355X) =====" << std::endl;
    std::string dumpPath;
    bool apiChecks = false, pairCalls = false, homography = false, fundamental = false;
    int retainBest = 0, retainGrid = 0, refine = 0;
    bool pose = false;
    int poseRefine = 0;
    hak_intrinsics poseK{0.f, 0.f, 0.f, 0.f};
    bool essential = false;
    hak_intrinsics essK{0.f, 0.f, 0.f, 0.f};
    float guided = 0.f, epipolar = 0.f;
    {   // strip the options; what is left are the reference demo's positional arguments (main.cpp:131-135)
        int n = 1;
        for (int i = 1; i < argc; i++) {
            if (!strcmp(argv[i], "--dump") && i + 1 < argc) dumpPath = argv[++i];
            else if (!strcmp(argv[i], "--api-checks")) apiChecks = true;
            else if (!strcmp(argv[i], "--pair")) pairCalls = true;
            else if (!strcmp(argv[i], "--homography")) homography = true;
            else if (!strcmp(argv[i], "--fundamental")) fundamental = true;
            else if (!strcmp(argv[i], "--guided") && i + 1 < argc) { guided = (float)std::atof(argv[++i]); homography = true; }
            else if (!strcmp(argv[i], "--refine") && i + 1 < argc) { refine = std::atoi(argv[++i]); fundamental = true; }
            else if (!strcmp(argv[i], "--pose-refine") && i + 1 < argc) poseRefine = std::atoi(argv[++i]);
            else if (!strcmp(argv[i], "--pose") && i + 4 < argc) {
                poseK.fx = (float)std::atof(argv[i + 1]); poseK.fy = (float)std::atof(argv[i + 2]);
                poseK.cx = (float)std::atof(argv[i + 3]); poseK.cy = (float)std::atof(argv[i + 4]);
                i += 4;
                pose = fundamental = true;
            }
            else if (!strcmp(argv[i], "--essential") && i + 4 < argc) {
                essK.fx = (float)std::atof(argv[i + 1]); essK.fy = (float)std::atof(argv[i + 2]);
                essK.cx = (float)std::atof(argv[i + 3]); essK.cy = (float)std::atof(argv[i + 4]);
                i += 4;
                essential = fundamental = true;
            }
            else if (!strcmp(argv[i], "--epipolar") && i + 1 < argc) { epipolar = (float)std::atof(argv[++i]); fundamental = true; }
            else if (!strcmp(argv[i], "--retain-best") && i + 1 < argc) retainBest = std::atoi(argv[++i]);
            else if (!strcmp(argv[i], "--retain-grid") && i + 1 < argc) retainGrid = std::atoi(argv[++i]);
            else argv[n++] = argv[i];
        }
        argc = n;
    }
    int devNum = argc > 1 ? std::atoi(argv[1]) : 0;
    int nrepeats = argc > 4 ? std::atoi(argv[4]) : 100;
    std::ofstream dump;
    if (!dumpPath.empty()) {
        dump.open(dumpPath, std::ios::binary);
        if (!dump) { std::cerr << "cannot open " << dumpPath << std::endl; return 1; }
    }
    std::vector<unsigned char> l8, r8;
    int w = 1920, h = 1080, w2 = 0, h2 = 0;
    if (argc > 3) {
        if (!readPgm(argv[2], l8, w, h) || !readPgm(argv[3], r8, w2, h2) || w != w2 || h != h2) {
            std::cerr << "cannot read the PGM pair" << std::endl;
            return 1;
        }
    } else synthPair(l8, r8, w, h);
    std::vector<float> limg(l8.size()), rimg(r8.size());
    for (size_t i = 0; i < l8.size(); i++) { limg[i] = (float)(l8[i] * (1.0 / 255.0)); rimg[i] = (float)(r8[i] * (1.0 / 255.0)); }   // main.cpp:149
    std::cout << "Image size = (" << w << "," << h << ")" << std::endl;

    // configuration: main.cpp:155-166
    int max_npts = retainBest > 0 ? retainBest : 10000, noctaves = 4, max_scale = 4;
    float per = 0.7f, kcontrast = 0.03f, soffset = 1.6f, derivative_factor = 1.5f, dthreshold = 0.001f;
    bool reordering = true;
    int diffusivity = 1, descriptor_pattern_size = 10;

    std::cout << "Initializing data..." << std::endl;
    initDevice(devNum);
    GpuTimer timer(0);
    int3 whp1, whp2;
    whp1.x = w; whp1.y = h; whp1.z = iAlignUp(w, 128);
    whp2 = whp1;
    float *img1 = NULL, *img2 = NULL;
    CHECK(hipMalloc((void**)&img1, sizeof(float) * (size_t)whp1.y * whp1.z));
    CHECK(hipMalloc((void**)&img2, sizeof(float) * (size_t)whp2.y * whp2.z));
    CHECK(hipMemcpy2D(img1, sizeof(float) * whp1.z, limg.data(), sizeof(float) * w, sizeof(float) * w, h, hipMemcpyHostToDevice));
    CHECK(hipMemcpy2D(img2, sizeof(float) * whp2.z, rimg.data(), sizeof(float) * w, sizeof(float) * w, h, hipMemcpyHostToDevice));
    float t0 = timer.read();

    akaze::AkazeData akaze_data1, akaze_data2;
    akaze::initAkazeData(akaze_data1, max_npts, true, true);
    akaze::initAkazeData(akaze_data2, max_npts, true, true);
    std::unique_ptr<akaze::Akazer> detector(new akaze::Akazer);
    detector->init(whp1, noctaves, max_scale, per, kcontrast, soffset, reordering, derivative_factor, dthreshold, diffusivity,
                   descriptor_pattern_size);
    if (retainBest > 0) detector->setRetainBest(true);
    if (retainGrid > 0) detector->setRetainGrid(retainGrid);

    float t1 = timer.read();
    for (int i = 0; i < nrepeats; i++) {
        if (pairCalls) detector->detectAndComputePair(img1, img2, akaze_data1, akaze_data2, whp1, true, true);
        else {
            detector->detectAndCompute(img1, akaze_data1, whp1, true);
            detector->detectAndCompute(img2, akaze_data2, whp2, true);
        }
    }
    float t2 = timer.read();
    if (!pairCalls) akaze::cuMatch(akaze_data1, akaze_data2);
    float t3 = timer.read();

    int nmatch = 0;
    for (int i = 0; i < akaze_data1.num_pts; i++) nmatch += akaze_data1.h_data[i].match >= 0;
    std::cout << "Number of features1: " << akaze_data1.num_pts << std::endl
              << "Number of features2: " << akaze_data2.num_pts << std::endl
              << "Number of accepted matches: " << nmatch << std::endl;
    std::cout << "Time for allocating image memory:  " << t0 << std::endl
              << "Time for allocating point memory:  " << t1 - t0 << std::endl
              << "Time of detection and computation: " << (t2 - t1) / nrepeats << std::endl
              << "Time of matching AKAZE keypoints:   " << (t3 - t2) << std::endl;

    if (dump.is_open()) dumpPoints(dump, akaze_data1, akaze_data2);

    // match post-processing (build-side addition): ratio 4/5 + cross-check, compacted on the device
    std::vector<hak_match_pair> good(akaze_data1.num_pts > 0 ? akaze_data1.num_pts : 1);
    float t4 = timer.read();
    int ngood = akaze::cuMatchKnn(akaze_data1, akaze_data2, good.data(), 4, 5, true);
    float t5 = timer.read();
    std::cout << "2-NN ratio 0.8 + cross-check matches: " << ngood << "  (" << t5 - t4 << " ms)" << std::endl;
    float hom[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    std::vector<unsigned char> inlier(good.size(), 0);
    int ninlier = 0;
    if (homography) {
        float t6 = timer.read();
        ninlier = akaze::cuFindHomography(good.data(), ngood, hom, inlier.data());
        float t7 = timer.read();
        std::cout << "Homography (RANSAC 1024 x 3 px, refit): " << ninlier << " inliers of " << ngood << "  (" << t7 - t6 << " ms)"
                  << std::endl;
        for (int r = 0; r < 3; r++)
            std::cout << "  [" << hom[3 * r] << ", " << hom[3 * r + 1] << ", " << hom[3 * r + 2] << "]" << std::endl;
    }
    float fund[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    std::vector<unsigned char> finlier(good.size(), 0);
    int nfinlier = 0;
    if (fundamental) {
        float t6 = timer.read();
        nfinlier = essential ? akaze::cuFindEssential(good.data(), ngood, essK, essK, fund, finlier.data())
                             : akaze::cuFindFundamental(good.data(), ngood, fund, finlier.data());
        float t7 = timer.read();
        std::cout << (essential ? "Essential matrix as F (RANSAC 1024 five-point x 1 px Sampson): "
                                : "Fundamental matrix (RANSAC 1024 x 1 px Sampson, no refit): ")
                  << nfinlier << " inliers of " << ngood << "  (" << t7 - t6 << " ms)" << std::endl;
        for (int r = 0; r < 3; r++)
            std::cout << "  [" << fund[3 * r] << ", " << fund[3 * r + 1] << ", " << fund[3 * r + 2] << "]" << std::endl;
        if (refine > 0) {
            const int before = nfinlier;
            nfinlier = akaze::cuRefineFundamental(good.data(), ngood, fund, finlier.data(), 1.f, refine);
            std::cout << "Refit of the fundamental matrix (rank-2 least squares, up to " << refine << " rounds): " << nfinlier
                      << " inliers against " << before << "  (" << timer.read() - t7 << " ms)" << std::endl;
        }
    }
    hak_pose poseRec{};
    std::vector<unsigned char> front(good.size(), 0);
    std::vector<float> xyz(3 * good.size(), 0.f);
    if (pose) {
        hak_match_pair* dGood = NULL;
        unsigned char* dFront = NULL;
        float* dXyz = NULL;
        const size_t cap = ngood > 0 ? (size_t)ngood : 1;
        CHECK(hipMalloc((void**)&dGood, sizeof(hak_match_pair) * cap));
        CHECK(hipMalloc((void**)&dFront, cap));
        CHECK(hipMalloc((void**)&dXyz, sizeof(float) * 3 * cap));
        CHECK(hipMemcpy(dGood, good.data(), sizeof(hak_match_pair) * (size_t)ngood, hipMemcpyHostToDevice));
        float t8 = timer.read();
        if (hak_recover_pose(NULL, dGood, ngood, fund, &poseK, &poseK, 1.f, INFINITY, dFront, dXyz, &poseRec)) {
            std::cerr << "hak_recover_pose: " << hak_last_error() << std::endl;
            return -1;
        }
        float t9 = timer.read();
        CHECK(hipMemcpy(front.data(), dFront, (size_t)ngood, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(xyz.data(), dXyz, sizeof(float) * 3 * (size_t)ngood, hipMemcpyDeviceToHost));
        CHECK(hipFree(dGood));
        CHECK(hipFree(dFront));
        CHECK(hipFree(dXyz));
        std::cout << "Relative pose from the fundamental matrix (candidate " << poseRec.candidate << "): " << poseRec.in_front
                  << " in front of both cameras of " << poseRec.inliers << " inliers of " << poseRec.n << "  (" << t9 - t8 << " ms)"
                  << std::endl;
        for (int r = 0; r < 3; r++)
            std::cout << "  R [" << poseRec.R[3 * r] << ", " << poseRec.R[3 * r + 1] << ", " << poseRec.R[3 * r + 2] << "]" << std::endl;
        std::cout << "  t [" << poseRec.t[0] << ", " << poseRec.t[1] << ", " << poseRec.t[2] << "]" << std::endl;
    }
    float refR[9], refT[3];
    int refFront = -1;
    std::vector<unsigned char> refMask(good.size(), 0);
    if (pose && poseRefine > 0) {
        for (int k = 0; k < 9; k++) refR[k] = poseRec.R[k];
        for (int k = 0; k < 3; k++) refT[k] = poseRec.t[k];
        float t8 = timer.read();
        refFront = akaze::cuRefinePose(good.data(), ngood, poseK, poseK, refR, refT, refMask.data(), 1.f, INFINITY, poseRefine);
        float t9 = timer.read();
        std::cout << "Refit of the relative pose (calibrated Gauss-Newton, up to " << poseRefine << " rounds): " << refFront
                  << " matches count under it  (" << t9 - t8 << " ms)" << std::endl;
        for (int r = 0; r < 3; r++)
            std::cout << "  R [" << refR[3 * r] << ", " << refR[3 * r + 1] << ", " << refR[3 * r + 2] << "]" << std::endl;
        std::cout << "  t [" << refT[0] << ", " << refT[1] << ", " << refT[2] << "]" << std::endl;
    }
    if (guided > 0.f) {
        std::vector<hak_match_pair> gm(good.size());
        float t8 = timer.read();
        const int nguided = akaze::cuMatchGuided(akaze_data1, akaze_data2, hom, gm.data(), guided, 4, 5, true);
        float t9 = timer.read();
        std::cout << "Guided matches (radius " << guided << " px, ratio 0.8 + cross-check): " << nguided << " against " << ngood
                  << " of the 2-NN match  (" << t9 - t8 << " ms)" << std::endl;
        float hom2[9];
        const int ninlier2 = akaze::cuFindHomography(gm.data(), nguided, hom2);
        std::cout << "Homography of the guided matches: " << ninlier2 << " inliers of " << nguided << " against " << ninlier << " of "
                  << ngood << std::endl;
    }
    if (epipolar > 0.f) {
        std::vector<hak_match_pair> em(good.size());
        float t8 = timer.read();
        const int nepi = akaze::cuMatchEpipolar(akaze_data1, akaze_data2, fund, em.data(), epipolar, 4, 5, true);
        float t9 = timer.read();
        std::cout << "Epipolar matches (radius " << epipolar << " px, ratio 0.8 + cross-check): " << nepi << " against " << ngood
                  << " of the 2-NN match  (" << t9 - t8 << " ms)" << std::endl;
        float fund2[9];
        const int nfinlier2 = essential ? akaze::cuFindEssential(em.data(), nepi, essK, essK, fund2)
                                        : akaze::cuFindFundamental(em.data(), nepi, fund2);
        std::cout << (essential ? "Essential matrix of the epipolar matches: " : "Fundamental matrix of the epipolar matches: ") << nfinlier2 << " inliers of " << nepi << " against " << nfinlier
                  << " of " << ngood << std::endl;
    }

    // ---- the reference's second demo (main.cpp:227-300): the integer FAST path on the uint8 images
    std::cout << "===== FAST (16.16 fixed-point) path =====" << std::endl;
    unsigned char *fimg1 = NULL, *fimg2 = NULL;
    CHECK(hipMalloc((void**)&fimg1, (size_t)whp1.y * whp1.z));
    CHECK(hipMalloc((void**)&fimg2, (size_t)whp2.y * whp2.z));
    CHECK(hipMemcpy2D(fimg1, whp1.z, l8.data(), w, w, h, hipMemcpyHostToDevice));
    CHECK(hipMemcpy2D(fimg2, whp2.z, r8.data(), w, w, h, hipMemcpyHostToDevice));
    float f1 = timer.read();
    for (int i = 0; i < nrepeats; i++) {
        detector->fastDetectAndCompute(fimg1, akaze_data1, whp1, true);
        detector->fastDetectAndCompute(fimg2, akaze_data2, whp2, true);
    }
    float f2 = timer.read();
    akaze::cuMatch(akaze_data1, akaze_data2);
    float f3 = timer.read();
    nmatch = 0;
    for (int i = 0; i < akaze_data1.num_pts; i++) nmatch += akaze_data1.h_data[i].match >= 0;
    std::cout << "Number of features1: " << akaze_data1.num_pts << std::endl
              << "Number of features2: " << akaze_data2.num_pts << std::endl
              << "Number of accepted matches: " << nmatch << std::endl
              << "Time of detection and computation: " << (f2 - f1) / nrepeats << std::endl
              << "Time of matching AKAZE keypoints:   " << (f3 - f2) << std::endl;
    if (dump.is_open()) dumpPoints(dump, akaze_data1, akaze_data2);
    CHECK(hipFree(fimg1));
    CHECK(hipFree(fimg2));

    if (apiChecks) {
        // (a) an AkazeData smaller than the default capacity clamps THIS call (akaze.cpp:246 setMaxNumPoints(result.max_pts)) ...
        std::cout << "===== API checks =====" << std::endl;
        akaze::AkazeData small, large;
        akaze::initAkazeData(small, 500, true, true);
        akaze::initAkazeData(large, 20000, true, true);
        detector->detectAndCompute(img1, small, whp1, true);
        std::cout << "small AkazeData (500): " << small.num_pts << std::endl;
        // ... and does not shrink later calls; a larger one is not clamped to the default 10000 either
        detector->detectAndCompute(img1, large, whp1, true);
        std::cout << "large AkazeData (20000): " << large.num_pts << std::endl;
        detector->detectAndCompute(img1, akaze_data1, whp1, true);
        std::cout << "default AkazeData again: " << akaze_data1.num_pts << std::endl;
        int same = small.num_pts <= large.num_pts;
        for (int i = 0; i < small.num_pts && same; i++)                       // the clamp keeps the raster-order prefix
            same = memcmp(&small.h_data[i], &large.h_data[i], 85) == 0;
        std::cout << "small is a prefix of large: " << (same ? "yes" : "NO") << std::endl;
        // (b) a size other than init()'s: new arena (akaze.cpp:109-117), then back
        int3 whpc; whpc.x = w / 2 / 4 * 4; whpc.y = h / 2; whpc.z = iAlignUp(whpc.x, 128);
        float* crop = NULL;
        CHECK(hipMalloc((void**)&crop, sizeof(float) * (size_t)whpc.y * whpc.z));
        CHECK(hipMemcpy2D(crop, sizeof(float) * whpc.z, limg.data(), sizeof(float) * w, sizeof(float) * whpc.x, whpc.y, hipMemcpyHostToDevice));
        detector->detectAndCompute(crop, large, whpc, true);
        std::cout << "top-left quarter (" << whpc.x << "x" << whpc.y << "): " << large.num_pts << std::endl;
        if (dump.is_open()) dumpPoints(dump, small, large);
        detector->detectAndCompute(img1, large, whp1, true);
        std::cout << "full size again: " << large.num_pts << std::endl;
        CHECK(hipFree(crop));
        akaze::freeAkazeData(small);
        akaze::freeAkazeData(large);
    }

    if (homography && dump.is_open()) {
        const int hdr[2] = {ngood, ninlier};
        dump.write((const char*)hdr, sizeof(hdr));
        dump.write((const char*)hom, sizeof(hom));
        dump.write((const char*)good.data(), sizeof(hak_match_pair) * (size_t)ngood);
        dump.write((const char*)inlier.data(), (size_t)ngood);
    }

    if (fundamental && dump.is_open()) {
        const int hdr[2] = {ngood, nfinlier};
        dump.write((const char*)hdr, sizeof(hdr));
        dump.write((const char*)fund, sizeof(fund));
        dump.write((const char*)good.data(), sizeof(hak_match_pair) * (size_t)ngood);
        dump.write((const char*)finlier.data(), (size_t)ngood);
        if (pose) {
            dump.write((const char*)&poseRec, sizeof(poseRec));
            dump.write((const char*)front.data(), (size_t)ngood);
            dump.write((const char*)xyz.data(), sizeof(float) * 3 * (size_t)ngood);
            if (poseRefine > 0) {
                dump.write((const char*)refR, sizeof(refR));
                dump.write((const char*)refT, sizeof(refT));
                dump.write((const char*)&refFront, sizeof(refFront));
                dump.write((const char*)refMask.data(), (size_t)ngood);
            }
        }
    }

    akaze::freeAkazeData(akaze_data1);
    akaze::freeAkazeData(akaze_data2);
    CHECK(hipFree(img1));
    CHECK(hipFree(img2));
    return 0;
}

// akaze.h -- the CUDA-AKAZE public API (akaze.h:10-30 of the reference) on top of libhipakaze's C ABI.
//
// Drop-in for main.cpp-style callers: same namespace, names, argument order and types.  `int3` is
// HIP's vector type (layout-identical to CUDA's).  Images are DEVICE pointers to float32 in [0,1]
// with pitch whp0.z elements (main.cpp:174); AkazeData is caller-owned and filled in place.  Errors
// print to stderr and exit(-1) like the reference's CHECK (cuda_utils.h:18-37).
#pragma once
#include "akaze_structures.h"
#include "hip_utils.h"

namespace akaze
{
    void initAkazeData(AkazeData& data, const int max_pts, const bool host, const bool dev);     // akaze.h:10
    void freeAkazeData(AkazeData& data);                                                        // akaze.h:12
    void cuMatch(AkazeData& result1, AkazeData& result2);                                       // akaze.h:14

    // build-side addition: 2-NN ratio test (the reference's unused gMatch, akazed.cu:2028-2122) +
    // symmetric cross-check; fills result1 like cuMatch and returns the accepted matches in query order
    // (host array `matches`, capacity >= result1.num_pts; may be NULL to only count).
    int cuMatchKnn(AkazeData& result1, AkazeData& result2, hak_match_pair* matches, int ratio_num = 1, int ratio_den = 1,
                   bool cross_check = true);

    // build-side addition: RANSAC homography over a host match list (e.g. cuMatchKnn's), on the device (hak_find_homography):
    // writes H (row-major, H[8] = 1; identity when there is no model) and, when inlier_mask is not NULL, n bytes (1 = inlier of H);
    // returns the inlier count
    int cuFindHomography(const hak_match_pair* matches, int n, float H[9], unsigned char* inlier_mask = nullptr, int iterations = 1024,
                         float threshold = 3.f, unsigned seed = 0, bool refine = true);

    // build-side addition: RANSAC fundamental matrix over a host match list, on the device (hak_find_fundamental): writes F (row-major,
    // (x2 y2 1) F (x1 y1 1)^T = 0, largest |entry| 1; all zero when there is no model) and, when inlier_mask is not NULL, n bytes
    // (1 = inlier of F: Sampson distance below `threshold` px); returns the inlier count.  The winning seven-point model, no refit.
    int cuFindFundamental(const hak_match_pair* matches, int n, float F[9], unsigned char* inlier_mask = nullptr, int iterations = 1024,
                          float threshold = 1.f, unsigned seed = 0);

    // build-side addition: five-point RANSAC essential matrix over a host match list under the two cameras' pinhole intrinsics, on the
    // device (hak_find_essential): writes F = K2^-T E K1^-1 as cuFindFundamental writes its F (all zero when there is no model) and,
    // when inlier_mask is not NULL, n bytes (1 = Sampson distance below `threshold` px); returns the inlier count.  It takes
    // cuFindFundamental's place in front of cuRecoverPose and cuRefinePose when the calibration is known.
    int cuFindEssential(const hak_match_pair* matches, int n, const hak_intrinsics& K1, const hak_intrinsics& K2, float F[9],
                        unsigned char* inlier_mask = nullptr, int iterations = 1024, float threshold = 1.f, unsigned seed = 0);

    // build-side addition: rank-2 least-squares refit of a fundamental matrix over its inliers among a host match list, iterated up to
    // `rounds` (1..8) times, on the device (hak_refine_fundamental): F (e.g. cuFindFundamental's; an all-zero F stays as it is) is
    // replaced by the refitted matrix when that scores at least as well at `threshold`, the optional inlier_mask (n bytes) gets the
    // inliers of the returned F, and the return value is their count -- never fewer than F had at that threshold.
    int cuRefineFundamental(const hak_match_pair* matches, int n, float F[9], unsigned char* inlier_mask = nullptr, float threshold = 1.f,
                            int rounds = 3);

    // build-side addition: relative pose from a fundamental matrix F (e.g. cuRefineFundamental's) and the two cameras' pinhole
    // intrinsics over a host match list, on the device (hak_recover_pose): writes R (row-major) and the unit baseline direction t with
    // X2 = R X1 + t (identity and 0 when there is no pose) and, when front_mask is not NULL, n bytes (1 = an inlier of F at
    // `threshold` px that lies in front of both cameras, nearer than max_depth baselines); returns the number of such matches, or
    // -1 when F gives no pose.
    int cuRecoverPose(const hak_match_pair* matches, int n, const float F[9], const hak_intrinsics& K1, const hak_intrinsics& K2,
                      float R[9], float t[3], unsigned char* front_mask = nullptr, float threshold = 1.f,
                      float max_depth = __builtin_inff());

    // cuRefinePose (hak_refine_pose): calibrated Gauss-Newton refit of a relative pose over the matches that count under it (inliers
    // of the pose's own F at `threshold` px, in front of both cameras), iterated up to `rounds` (1..8) times, on the device: R and t
    // (cuRecoverPose's, when that found a pose) are replaced by the refitted pose when as many matches count under it, the optional
    // front_mask (n bytes) gets those matches, and the return value is their count -- never fewer than the count under the given
    // pose at that threshold -- or -1 when the given pose is none (non-finite, or t = 0 as cuRecoverPose leaves it without a pose).
    int cuRefinePose(const hak_match_pair* matches, int n, const hak_intrinsics& K1, const hak_intrinsics& K2, float R[9], float t[3],
                     unsigned char* front_mask = nullptr, float threshold = 1.f, float max_depth = __builtin_inff(), int rounds = 3);

    // build-side addition: a fourth view.  cuTriangulate (hak_triangulate) triangulates a host match list under two known views,
    // on the device: RtA, RtB are 12 floats {R row-major, t} with Xc = R X + t (cuRecoverPose's, cuSolvePnP's or cuRefinePnP's R
    // and t side by side), NULL = the identity.  xyz, when not NULL, gets 3 n floats (the midpoint of the two rays' common
    // perpendicular in the frame the views map from; zeros for a rejected match) and mask, when not NULL, n bytes (1 = the rays'
    // angle has a sine >= min_sin, the point lies in front of both cameras nearer than max_depth, and it reprojects within
    // `threshold` px in both images).  Returns the number of such matches.  With (RtA, RtB) = (pose of I1, pose of I2) over the
    // matches of (I1, I2), mask and xyz are what cuLinkTracks takes as maskA and xyzA to reach I3.
    int cuTriangulate(const hak_match_pair* matches, int n, const float* RtA, const float* RtB, const hak_intrinsics& KA,
                      const hak_intrinsics& KB, float* xyz, unsigned char* mask = nullptr, float threshold = 2.f,
                      float max_depth = __builtin_inff(), float min_sin = 0.f);

    // build-side addition: a third view.  cuLinkTracks (hak_link_tracks) joins the host match list A of images (I0, I1), with a point
    // per match (xyzA, 3 n floats, as hak_recover_pose writes them; maskA NULL or nA bytes, 0 = leave the match out), and the host
    // match list B of images (I1, I2) on the keypoints of I1 (indices below max_index): `out` (room for nB records) receives one
    // 3-D to 2-D correspondence per linked match of B in ascending order; returns their number.
    int cuLinkTracks(const hak_match_pair* A, int nA, const float* xyzA, const unsigned char* maskA, const hak_match_pair* B, int nB,
                     int max_index, hak_corr3d* out);
    // cuSolvePnP (hak_solve_pnp): RANSAC absolute pose of the new image from such correspondences by the three-point solve: writes R
    // (row-major) and t with Xc = R X + t in the units of the points (identity and 0 when there is no model) and, when inlier_mask
    // is not NULL, n bytes (1 = reprojected closer than `threshold` px, in front of the camera); returns the number of inliers, or -1
    // when there is no model.
    int cuSolvePnP(const hak_corr3d* corr, int n, const hak_intrinsics& K, float R[9], float t[3], unsigned char* inlier_mask = nullptr,
                   int iterations = 1024, float threshold = 2.f, unsigned seed = 0);
    // cuRefinePnP (hak_refine_pnp): Gauss-Newton refit of an absolute pose over its inliers among the host correspondences, iterated
    // up to `rounds` (1..8) times, on the device: R and t (e.g. cuSolvePnP's, when that found a model) are replaced by the refitted
    // pose when that scores at least as well at `threshold`, the optional inlier_mask (n bytes) gets the inliers of the returned
    // pose, and the return value is their count -- never fewer than the given pose had at that threshold.
    int cuRefinePnP(const hak_corr3d* corr, int n, const hak_intrinsics& K, float R[9], float t[3], unsigned char* inlier_mask = nullptr,
                    float threshold = 2.f, int rounds = 3);

    // build-side addition: projection-guided matching (hak_match_projected) -- re-matches 3-D points against the keypoints of a new
    // image under its known pose: landmark m is the point xyzA[3m ..] (cuRecoverPose's or cuTriangulate's) of the host match list A
    // (maskA NULL or nA bytes, 0 = leave the landmark out) with the descriptor of keypoint A[m].train of result_desc; Rt is 12 floats
    // {R row-major, t} with Xc = R X + t (cuSolvePnP's or cuRefinePnP's R and t side by side), NULL = the identity.  Every landmark
    // is searched only among the keypoints of result2 within `radius` pixels of its projection, ratio test and cross-check inside
    // that neighbourhood.  `out` (room for nA records; may be NULL to only count) receives one 3-D to 2-D correspondence per accepted
    // landmark in ascending order -- src3d = m, src2d = the keypoint index in result2 -- the list cuRefinePnP takes; returns their number.
    int cuMatchProjected(const hak_match_pair* A, int nA, const float* xyzA, const unsigned char* maskA, AkazeData& result_desc,
                         AkazeData& result2, const float* Rt, const hak_intrinsics& K, hak_corr3d* out, float radius = 8.f,
                         int ratio_num = 4, int ratio_den = 5, bool cross_check = true);

    // build-side addition: guided matching (hak_match_guided) -- re-matches result1 against result2 under a homography H (row-major,
    // (x1, y1, 1) -> image 2, e.g. cuFindHomography's): every keypoint of result1 is searched only among the keypoints of result2
    // within `radius` pixels of where H sends it, ratio test and cross-check inside that neighbourhood.  Fills result1 like cuMatch
    // and returns the accepted matches in query order (host array `matches`, capacity >= result1.num_pts; may be NULL to only count).
    int cuMatchGuided(AkazeData& result1, AkazeData& result2, const float H[9], hak_match_pair* matches, float radius = 8.f,
                      int ratio_num = 4, int ratio_den = 5, bool cross_check = true);

    // build-side addition: epipolar guided matching (hak_match_epipolar) -- re-matches result1 against result2 under a fundamental
    // matrix F (row-major, (x2 y2 1) F (x1 y1 1)^T = 0, e.g. cuFindFundamental's): every keypoint of result1 is searched only among
    // the keypoints of result2 closer than `radius` pixels to its epipolar line, ratio test and cross-check inside that band.  Fills
    // result1 like cuMatch and returns the accepted matches in query order (host array `matches`, capacity >= result1.num_pts; may
    // be NULL to only count).
    int cuMatchEpipolar(AkazeData& result1, AkazeData& result2, const float F[9], hak_match_pair* matches, float radius = 2.f,
                        int ratio_num = 4, int ratio_den = 5, bool cross_check = true);

    class Akazer
    {
    public:
        Akazer();
        ~Akazer();

        // akaze.h:25-26
        void init(int3 whp0, int _noctaves, int _max_scale, float _per, float _kcontrast, float _soffset, bool _reordering,
                  float _derivative_factor, float _dthreshold, int _diffusivity, int _descriptor_pattern_size);

        // akaze.h:29-30
        void detectAndCompute(float* image, AkazeData& result, int3 whp0, const bool desc = true);
        void fastDetectAndCompute(unsigned char* image, AkazeData& result, int3 whp0, const bool desc = true);

        // build-side additions (no reference counterpart)
        // both images of a pair + cuMatch(result1, result2) as ONE launch sequence and one synchronisation (hak_detect_and_compute_pair):
        // same results in result1 / result2 as the two detectAndCompute calls followed by cuMatch of main.cpp:201-209
        void detectAndComputePair(float* image1, float* image2, AkazeData& result1, AkazeData& result2, int3 whp0,
                                  const bool desc = true, const bool match = true);
        void setMaxPoints(int max_pts);      // capacity the context is built for (default 10000, main.cpp:155)
        void setUpright(bool upright);       // MLDB-upright extension
        // an AkazeData that overflows keeps its result.max_pts STRONGEST keypoints (in raster order) instead of the first ones in
        // raster order (hak_set_retain_best); remembered across context re-creation.  Default off.
        void setRetainBest(bool on);
        // G in 8..128: an AkazeData that overflows keeps the best keypoints of every G x G pixel cell instead (hak_set_retain_grid;
        // it then decides the policy whatever setRetainBest says); 0 (default): off.  Remembered across context re-creation.
        void setRetainGrid(int G);
        hak_ctx* context() { return ctx; }

    private:
        hak_config cfg;
        int3 whp{0, 0, 0};
        hak_ctx* ctx = nullptr;      // owns the arena (the reference's omem; room for the two images of a pair call), freed in the destructor
        int ctx_w = 0, ctx_h = 0;
        bool retain_best = false;
        int retain_grid = 0;
        void ensureContext(int w, int h);
    };
}

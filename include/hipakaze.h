/*
 * hipakaze.h -- C ABI of libhipakaze.so, the MI355X-native AKAZE hot path
 * (detect + describe + match) behind the CUDA-AKAZE interface.
 *
 * The reference has no C layer: its boundary is the C++ class in akaze.h.  The
 * entry points below are what a binding for that class needs; each one cites
 * the reference interface it replaces (file:line in the reference checkout).
 * include/akaze.h re-creates akaze::Akazer / akaze::cuMatch on top of this
 * ABI, so main.cpp-style callers drop in.
 *
 * Conventions (as the reference): images are DEVICE pointers to
 * float32 in [0,1], row pitch in elements; point arrays are caller-owned
 * device arrays of 104-byte hak_point; every function returns 0 on success and
 * a non-zero status otherwise, with the message in hak_last_error().  There is
 * no CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef HIPAKAZE_H
#define HIPAKAZE_H

#ifdef __cplusplus
extern "C" {
#endif

#define HAK_FLEN 61          /* akaze_structures.h:29  (FEATURE_TYPE 5, MLDB) */
#define HAK_MAX_OCTAVES 8    /* akazed.cu:10 MAX_OCTAVE */
#define HAK_MAX_SCALES 5     /* akazed.cu:9  MAX_SCALE  */
#define HAK_MAX_DIST 96      /* akazed.cu:11 MAX_DIST   */

/* akaze_structures.h:19-40 AkazePoint: 104 bytes, align 4.
 * offsets: x 0, y 4, octave 8 (= octave*max_scale + sublevel), response 12,
 * size 16, angle 20, features 24..84, pad 85..87, match 88, distance 92,
 * match_x 96, match_y 100. */
typedef struct hak_point {
    float x;
    float y;
    int octave;
    float response;
    float size;
    float angle;
    unsigned char features[HAK_FLEN];
    int match;
    int distance;
    float match_x;
    float match_y;
} hak_point;

/* akaze_structures.h:53-59 DiffusivityType */
enum { HAK_PM_G1 = 0, HAK_PM_G2 = 1, HAK_WEICKERT = 2, HAK_CHARBONNIER = 3 };

/* The 11 arguments of Akazer::init (akaze.h:25-26, defaults akaze.h:35-54,
 * demo values main.cpp:156-166) plus what the reference keeps as macros or
 * call arguments. */
typedef struct hak_config {
    int noctaves;                 /* 4 */
    int max_scale;                /* 4  sublevels per octave */
    float per;                    /* 0.7  contrast percentile */
    float kcontrast;              /* 0.03 (overwritten per image, akazed.cu:2481) */
    float soffset;                /* 1.6 */
    int reordering;               /* 1 */
    float derivative_factor;      /* 1.5 */
    float dthreshold;             /* 0.001; >= 0 (see hak_create) */
    int diffusivity;              /* HAK_PM_G2 */
    int descriptor_pattern_size;  /* 10 */
    int max_pts;                  /* capacity of every per-image point array (main.cpp:155: 10000) */
    int upright;                  /* 0; 1 = MLDB-upright extension: angle = 0 (no reference behaviour) */
    int batch;                    /* images one launch sequence processes (>= 1) */
} hak_config;

typedef struct hak_ctx hak_ctx;

/* ---- device / errors: cuda_utils.h:41-67 initDevice, :18-37 CHECK/CheckMsg */
int hak_device_count(void);
int hak_set_device(int dev);
const char* hak_last_error(void);
void hak_default_config(hak_config* cfg);

/* ---- detector object: Akazer::Akazer/init/allocMemory/~Akazer (akaze.cpp:67-98, 204-237).
 * Geometry is fixed at creation (w x h pixels); the arena for `batch` images,
 * the FED schedule and all tables live in the context.
 * dthreshold must be >= 0 (0 is allowed; a negative value or a NaN is refused).  The cross-scale key map orders responses by their
 * bit patterns, which is the order of the values for positive floats only: a negative maximum would rank above every positive one,
 * in the map and in the NMS, where the reference compares floats against maps that start at -0.0926 (so one below that never enters,
 * and one above it loses to any positive response).  Measured on noise at dthreshold = -1: 23 of 81344 map pixels and 3 of 3088
 * keypoints differ from the reference; at 0 none.  An order-preserving key for negative floats would put two more operations into
 * every key write and every NMS compare of the positive path, for thresholds nothing uses. */
int hak_create(const hak_config* cfg, int w, int h, hak_ctx** out);
/* Waits for the context's last launch sequence (an event recorded behind it, so a caller-provided stream that has been destroyed
 * meanwhile is never touched), then releases everything.  Kernel-selection knobs are read from the environment by
 * hak_create INTO the context: two contexts of one process may differ. */
void hak_destroy(hak_ctx* ctx);
/* Run on a caller-provided hipStream_t (e.g. torch's current stream); NULL = the context's own.  The stream must stay valid while
 * calls are made with it; switching streams does not synchronise -- order work across the two yourself (hak_sync before switching
 * is enough).  Launch-bound single-image sequences and batched ones both start and end on this stream. */
int hak_set_stream(hak_ctx* ctx, void* hip_stream);
int hak_sync(hak_ctx* ctx);
/* make the context's stream wait for a hipEvent_t recorded elsewhere (e.g. the end of an upload on a copy stream) without
 * blocking the host: everything enqueued on the context afterwards runs behind the event */
int hak_wait_event(hak_ctx* ctx, void* hip_event);
/* the context's phase event (a hipEvent_t owned by the context): every float detect sequence records it where its scale space
 * (FED / Hessian kernels: bound by HBM stores) ends and its keypoint stages (NMS, orientation, MLDB, then the caller's match:
 * bound by gathers and integer work) begin.  A caller that keeps two contexts busy makes each one's next sequence wait for the
 * OTHER one's phase event (hak_wait_event): the two kinds of work then run beside each other instead of in lockstep. */
int hak_phase_event(hak_ctx* ctx, void** hip_event);
/* 1 (default): octaves run on their own HIP streams (octave o+1 depends only on Lt(o,0), akaze.cpp:371-375);
 * 0: one stream, strictly serial launches (used for per-kernel timing). Env HAK_SERIAL=1 presets 0. */
int hak_set_concurrency(hak_ctx* ctx, int on);
/* 1 (default): every call that enqueues work on the context first makes the context's stream wait for what the caller has enqueued on
 * the NULL stream so far (an event recorded there; no host wait).  The reference runs on the default stream, so its callers' own
 * hipMemset / hipMemcpyAsync / kernels on that stream are ordered in front of detectAndCompute and cuMatch by themselves
 * (akaze.cpp:101-150 issues everything on stream 0); a context's streams are non-blocking and would not wait (hipMemset returns
 * before its fill has run: tools/probes/memset_order_probe.hip).  0: no such dependency (a caller that drives the context from its
 * own stream, hak_set_stream, or captures graphs while calling).  Env HAK_NULL_ORDER=0 presets 0. */
int hak_set_null_order(hak_ctx* ctx, int on);
/* 0 (default): an image with more NMS survivors than its clamp keeps the raster-order prefix of them (the reference's behaviour
 * up to its arbitrary arrival order).  1: it keeps its N strongest, N = the clamp (a call's max_pts, a pair call's per-image cap,
 * cfg.max_pts in a batch), selected on the device before emission; refinement, orientation, MLDB and the pair call's match then
 * run on the kept set only.  The rule, per image with S survivors in raster order and clamp C:
 *   S <= C: the output does not change, byte for byte.
 *   S >  C: the C survivors ranking highest by (K(response word), then the smaller raster index y * w + x of the integer
 *           full-resolution position before refinement) are kept and emitted in raster order -- a subsequence of the
 *           unclamped output, every record byte-identical to the unclamped call's; num_pts = C.
 *   K maps the 32-bit response word order-preservingly to unsigned: float path (bits u) u >> 31 ? ~u : u | 0x80000000;
 *   FAST path (int32 response) u ^ 0x80000000.
 * Covers every detect entry point of the context (hak_detect_and_compute, _batch, _pair, hak_fast_detect_and_compute, _batch)
 * and the test ABI's hak_op_tail_finish; takes effect with the next call, allocates nothing and does not synchronise. */
int hak_set_retain_best(hak_ctx* ctx, int on);
/* G == 0 (default): off, the context behaves as above, hak_set_retain_best included.  8 <= G <= 128: an image with more NMS
 * survivors than its clamp spreads the clamp over a grid of square cells of G pixels, so that every region keeps its best points;
 * while it is on, this replaces both other policies, whatever hak_set_retain_best says.  Any other G: non-zero status and a
 * message; a null context is refused without touching a device.  The rule, per image with S survivors and clamp C (as above):
 *   S <= C: the output does not change, byte for byte.
 *   S >  C: a survivor at the integer full-resolution position (x, y) before refinement lies in cell c = (y / G) * ncx + x / G,
 *           ncx = ceil(w / G); n_c = survivors of cell c.  Inside a cell and between cells alike survivors rank by K(response
 *           word) descending, then by the smaller raster index y * w + x (K: the map of hak_set_retain_best).
 *           1. the quota q is the largest integer >= 0 with sum_c min(n_c, q) <= C;
 *           2. every cell keeps its min(n_c, q) highest-ranked survivors;
 *           3. R = C - sum_c min(n_c, q) places remain (R < number of cells with n_c > q);
 *           4. the candidates for them are the rank-q survivors (0-based) of the cells with n_c > q, one per cell;
 *           5. the R highest-ranked candidates are kept as well.
 *           Every cell ends with min(n_c, q) or q + 1 keypoints, exactly C are kept and emitted in raster order -- a subsequence
 *           of the unclamped output, every record byte-identical to the unclamped call's; num_pts = C.
 * Refinement, orientation, MLDB and the pair call's match run on the kept set only.  Covers the entry points hak_set_retain_best
 * covers; takes effect with the next call and does not synchronise; its scratch is allocated by the first call with G > 0 (never
 * inside a call's launch sequence).  Statement: tests/retain_grid_ref.py; device code: csrc/kernels_grid_select.hip. */
int hak_set_retain_grid(hak_ctx* ctx, int G);

/* ---- Akazer::detectAndCompute (akaze.h:29, akaze.cpp:101-150), one image,
 * synchronous.  d_image: device float32, pitch elements per row.  d_points:
 * device array of max_pts points; max_pts is also this call's clamp, as the
 * reference's setMaxNumPoints(result.max_pts) (akaze.cpp:246, 451) -- it may be
 * smaller or larger than cfg.max_pts (which sizes the batch entry points).
 * *num_pts (host) receives the count; when h_points != NULL the points are
 * copied to it (whole 104-byte records). */
int hak_detect_and_compute(hak_ctx* ctx, const float* d_image, int pitch,
                           hak_point* d_points, int max_pts, int* num_pts,
                           hak_point* h_points, int desc);

/* ---- batched, asynchronous form used by the frame-sharded driver.
 * nimg <= cfg.batch images at d_images + i*image_stride (elements); points of
 * image i at d_points + i*max_pts; counts written to d_num_pts[i] (device).
 * Returns after enqueueing; hak_sync() or stream sync to wait. */
int hak_detect_and_compute_batch(hak_ctx* ctx, const float* d_images, long image_stride, int pitch,
                                 int nimg, hak_point* d_points, int* d_num_pts, int desc);

/* ---- Akazer::fastDetectAndCompute (akaze.h:30, akaze.cpp:153-201, 506-743): the integer "FAST" path --
 * uint8 image in [0,255] (pitch in bytes), the whole pipeline in int32 with 16.16 fixed-point weights
 * (namespace fastakaze, akazed.cu:2781-4367), detector threshold fixed at 65 (akaze.cpp:559).  Same
 * output contract as hak_detect_and_compute; `response` holds the integer determinant as a float. */
int hak_fast_detect_and_compute(hak_ctx* ctx, const unsigned char* d_image, int pitch,
                                hak_point* d_points, int max_pts, int* num_pts,
                                hak_point* h_points, int desc);
int hak_fast_detect_and_compute_batch(hak_ctx* ctx, const unsigned char* d_images, long image_stride, int pitch,
                                      int nimg, hak_point* d_points, int* d_num_pts, int desc);

/* ---- one PAIR per call: detectAndCompute on both images + cuMatch of the pair (main.cpp:201-209's three synchronous calls) as ONE
 * launch sequence and ONE synchronisation.  Build-side addition for callers that are bound by launches, not by bytes (a single
 * 1080p pair: 0.94 ms through the three calls).  The context must have been created with batch >= 2.  d_points1 / d_points2
 * (device, max_pts1 / max_pts2 records), h_points1 / h_points2 (host or NULL; pinned host arrays are written by the launch
 * sequence itself) and the counts are filled exactly as two hak_detect_and_compute calls followed by hak_match(ctx, 1, 2) would;
 * each image keeps its own clamp min(max_pts_i, the context's max_pts) (setMaxNumPoints(result.max_pts), akaze.cpp:246, 451), and
 * the matcher sees the clamped sets.  match = 0 skips the matcher. */
int hak_detect_and_compute_pair(hak_ctx* ctx, const float* d_image1, const float* d_image2, int pitch,
                                hak_point* d_points1, hak_point* d_points2, int max_pts1, int max_pts2,
                                int* num_pts1, int* num_pts2, hak_point* h_points1, hak_point* h_points2, int desc, int match);

/* ---- cuMatch (akaze.h:14; ctx may be NULL = default stream, akaze.cpp:55-64, akazed.cu:2144-2241): 1-NN
 * Hamming, accepted iff dist < 96 and the minimum is attained in exactly one
 * of the 16 residue classes j mod 16.  Fills match/distance/match_x/match_y
 * of d_pts1; copies those 16 bytes per point into h_pts1 when not NULL. */
int hak_match(hak_ctx* ctx, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2,
              hak_point* h_pts1);
/* batched: pair k matches (d_pts + (2k)*max_pts) against (d_pts + (2k+1)*max_pts),
 * counts read from d_num_pts[2k], d_num_pts[2k+1] on the device. Asynchronous. */
int hak_match_batch(hak_ctx* ctx, hak_point* d_points, const int* d_num_pts, int npairs);

/* ---- match post-processing.  The reference ships an unused 2-NN matcher (gMatch,
 * akazed.cu:2028-2122: best and second-best score, accept iff best < second && best < MAX_DIST); this is
 * that rule made well-defined, plus the usual symmetric cross-check and a device-side compaction:
 *   j1(i) = nearest train point of query i (smallest index among ties), d1 its distance,
 *   d2    = distance to the nearest OTHER train point (512 when n2 < 2, gMatch's initial score);
 *   accept iff d1 < max_dist  and  d1 * ratio_den < d2 * ratio_num  (1/1 = gMatch's rule)
 *          and (cross_check == 0 or the nearest query of train point j1(i) is i, ties to the smallest index).
 * Writes match/distance/match_x/match_y of pts1 like cuMatch (rejected: -1; copied to h_pts1 when given) and appends the accepted
 * matches, in ascending query order, to d_out (capacity >= n1; may be NULL); *count receives their number.
 * ctx may be NULL (scratch is then allocated per call).  max_dist <= 0 selects 96 (akazed.cu:6).  Fewer than 2^20 points per
 * side (the batch form: a context whose max_pts is below 2^20); more is refused before a buffer is touched. */
typedef struct hak_match_pair {
    int   query, train;      /* indices into pts1 / pts2 */
    int   distance, second;  /* d1, d2 */
    float x1, y1, x2, y2;    /* refined coordinates of both ends */
} hak_match_pair;
int hak_match_knn2(hak_ctx* ctx, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2,
                   int ratio_num, int ratio_den, int cross_check, int max_dist, hak_point* h_pts1,
                   hak_match_pair* d_out, int* count, hak_match_pair* h_out);
/* batched over the pairs of a detect batch (layout as hak_match_batch): pair k's accepted matches go to
 * d_out + k*max_pts, their number to d_counts[k].  Asynchronous on the context's stream. */
int hak_match_knn2_batch(hak_ctx* ctx, hak_point* d_points, const int* d_num_pts, int npairs,
                         int ratio_num, int ratio_den, int cross_check, int max_dist,
                         hak_match_pair* d_out, int* d_counts);

/* ---- geometric verification of a match list: RANSAC homography (build-side addition, "registration" of main.cpp:130).
 * A pure function of (matches, iterations, threshold, seed, refine); tests/homography_ref.py is its bit-exact numpy statement.
 * Input: n hak_match_pair records, the device list of hak_match_knn2 (only x1, y1, x2, y2 are read; 16-byte aligned).
 *   1. Hypothesis h (0 <= h < iterations, 1 <= iterations <= 65536) draws r_d = mix64(seed + (16 h + d + 1) * 0x9E3779B97F4A7C15)
 *      (splitmix64, mod 2^64) for d = 0..15 and takes index ((r_d >> 32) * n) >> 32 unless already chosen, until it has four.
 *      It is degenerate without four distinct indices (and always when n < 4).
 *   2. float64, no FMA: for the triples 012, 013, 023, 123 of the four points in each image c = (b - a) x (c - a); the sample is
 *      degenerate unless |c| > 1 px^2 everywhere and sign(c) agrees between the images (NaN fails).  H = S2 * adj(S1) with S the
 *      square-to-quad maps of the two quads (Heckbert), divided by H[2][2]; degenerate if that is 0 or anything is non-finite
 *      after rounding to float32; H[8] = 1.
 *   3. float32, no FMA: wz = (h6 x1 + h7 y1) + 1, u = (h0 x1 + h1 y1) + h2, v = (h3 x1 + h4 y1) + h5, ex = u - x2 wz, ey = v - y2 wz;
 *      inlier iff wz > 0 and ex ex + ey ey < t2 (wz wz), t2 = threshold * threshold (threshold finite, > 0).  A record with a
 *      non-finite coordinate is never an inlier (nor part of a usable sample).
 *   4. The non-degenerate hypothesis with the most inliers wins, ties to the smallest h.
 *   5. refine = 1 and >= 4 inliers: float64 least squares over the winner's inliers (Hartley normalisation per image: centroid,
 *      s = sqrt(2 m / sum r^2); 8x8 normal equations with h22 = 1 by Gaussian elimination with partial pivoting; sums in a fixed
 *      order: lane l of a wave takes matches i = l mod 64 ascending, then an xor butterfly over 32, 16, .., 1), denormalised,
 *      divided by [2][2], rounded to float32 and re-scored.  It replaces the sample's H iff it is finite, the system was
 *      non-singular and its inlier count is >= the sample's.
 * Output: hypothesis = -1 means no model (H = identity, inliers = 0).  The optional mask gets 1 for every inlier of the returned H,
 * 0 otherwise (n bytes). */
typedef struct hak_homography {
    float H[9];              /* row-major, x2 ~ (H[0] x1 + H[1] y1 + H[2]) / (H[6] x1 + H[7] y1 + 1); H[8] = 1 */
    int   inliers;           /* inliers of H */
    int   hypothesis;        /* winning hypothesis, -1 = no model */
    int   refined;           /* 1 when H is the least-squares refit */
    int   n;                 /* matches considered */
} hak_homography;
/* one list, synchronous: d_matches (device, n records), d_mask (device, n bytes) or NULL, result to *h_out.  ctx may be NULL
 * (default stream; the call allocates its own scratch). */
int hak_find_homography(hak_ctx* ctx, const hak_match_pair* d_matches, int n, int iterations, float threshold, unsigned seed,
                        int refine, unsigned char* d_mask, hak_homography* h_out);
/* batched, asynchronous on the context's stream, in the layout of hak_match_knn2_batch's output: pair k's list at
 * d_matches + k*stride, its count d_counts[k] read on the device and clamped to [0, stride]; record k to d_out[k] (device), mask
 * of pair k to d_masks + k*stride (device) unless d_masks is NULL. */
int hak_find_homography_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                              int iterations, float threshold, unsigned seed, int refine, hak_homography* d_out,
                              unsigned char* d_masks);

/* ---- geometric verification of a match list: RANSAC fundamental matrix (build-side addition).  The epipolar model of two
 * views of a 3-D scene, x2^T F x1 = 0, next to the homography of a plane or a rotating camera; its inlier mask is the outlier
 * filter of stereo, SfM and SLAM front ends.  A pure function of (matches, iterations, threshold, seed);
 * tests/fundamental_ref.py is its bit-exact numpy statement.  Input as hak_find_homography; a record with a non-finite
 * coordinate is never an inlier and makes any sample it is in degenerate.
 *   1. Hypothesis h (0 <= h < iterations, 1 <= iterations <= 65536) draws r_d = mix64(seed + (32 h + d + 1) * 0x9E3779B97F4A7C15)
 *      for d = 0..31 and takes index ((r_d >> 32) * n) >> 32 unless already chosen, until it has seven.  It is degenerate with
 *      fewer than seven distinct indices (always when n < 7).
 *   2. float64, no FMA, sums over the sample in draw order starting from 0: per image the centroid c = sum / 7, d_k = p_k - c,
 *      q = sum (dx dx + dy dy), s = sqrt(14 / q), normalised point s d_k.  Degenerate if q is 0 or s is non-finite.
 *   3. The 7 x 9 system has the row [u x, u y, u, v x, v y, v, x, y, 1] per point, (x, y) the normalised point of image 1 and
 *      (u, v) that of image 2.  Gaussian elimination with partial pivoting over rows only, pivot columns 0..6 in order: the pivot
 *      of column c is the largest |entry| of rows c..6, ties to the smallest row; degenerate if it is 0 or non-finite;
 *      f = M[r][c] / M[c][c], M[r][q] = M[r][q] - f M[c][q].  Two null vectors by back substitution, i = 6..0:
 *      f_i = ((-M[i][free]) - M[i][i+1] f_(i+1) - .. - M[i][6] f_6) / M[i][i] (subtractions in ascending j): A with
 *      (f7, f8) = (1, 0), free = 7, and B with (f7, f8) = (0, 1), free = 8.  This is an F8-normalised parametrisation inside the
 *      sample: a sample whose leading 7 x 7 block is ill-conditioned is not re-pivoted over columns, it simply scores badly.
 *   4. det(a A + B) = c3 a^3 + c2 a^2 + c1 a + c0: c3 = det A, c0 = det B, c2 = (d0 + d1) + d2 with d_i = det(A with row i taken
 *      from B), c1 likewise with A and B exchanged; det m = (m0 (m4 m8 - m5 m7) - m1 (m3 m8 - m5 m6)) + m2 (m3 m7 - m4 m6).
 *      Degenerate if c3 is 0 or a coefficient is non-finite.
 *   5. Real roots with + - * / sqrt only: b_k = c_k / c3, q(a) = ((a + b2) a + b1) a + b0, B = 1 + max |b_k| (degenerate if a b_k
 *      or B is non-finite), D = b2 b2 - 3 b1.  D > 0: s = sqrt(D), t1 = (-b2 - s) / 3, t2 = (-b2 + s) / 3, brackets [-B, t1],
 *      [t1, t2], [t2, B]; otherwise the one bracket [-B, B].  A bracket holds a root iff (q(lo) < 0) != (q(hi) < 0); there, 64
 *      bisections: mid = 0.5 (lo + hi) replaces lo when (q(mid) < 0) == (q(lo_0) < 0), lo_0 the bracket's original lower end,
 *      and hi otherwise; the root is 0.5 (lo + hi).  Roots are numbered 0.. in bracket order (one or three; a double root
 *      comes out as two nearly equal ones).
 *   6. Per root: Fn[k] = a A[k] + B[k], F = T2^T (Fn T1) with T = [s 0 -(s cx); 0 s -(s cy); 0 0 1], each product
 *      C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]; divided by its entry of largest |value| (ties to the
 *      smallest index) and rounded to float32.  The model is dropped if that entry is 0 or anything is non-finite.
 *   7. float32, no FMA, Sampson distance: a = (F0 x1 + F1 y1) + F2, b = (F3 x1 + F4 y1) + F5, c = (F6 x1 + F7 y1) + F8,
 *      e = (a x2 + b y2) + c, p = (F0 x2 + F3 y2) + F6, q = (F1 x2 + F4 y2) + F7, den = (a a + b b) + (p p + q q);
 *      inlier iff e e < t2 den, t2 = threshold * threshold (threshold finite, > 0; NaN fails).
 *   8. The model with the most inliers wins, ties to the smallest h, then the smallest root.
 * Output: hypothesis = -1 means no model (F all zero, inliers = 0, mask all zero).  The optional mask gets 1 for every inlier of
 * the returned F, 0 otherwise (n bytes).  F is the winning seven-point model, exactly rank 2 up to rounding; the rank-2
 * least-squares refit over its inliers is the next stage, hak_refine_fundamental below.  Refused with a non-zero
 * status and a message before any device is touched: iterations outside 1..65536, a threshold that is not finite or not > 0,
 * n < 0, a NULL list with n > 0, NULL h_out / d_out / d_counts, npairs < 1, stride < 1, a NULL context for the batch form.
 * Device code: csrc/kernels_fundamental.hip (RANSAC scaffold: csrc/ransac_common.h). */
typedef struct hak_fundamental {
    float F[9];              /* row-major, (x2 y2 1) F (x1 y1 1)^T = 0; the entry of largest |value| is 1 */
    int   inliers;           /* inliers of F */
    int   hypothesis;        /* winning hypothesis, -1 = no model (F = 0, inliers = 0) */
    int   root;              /* which real root of the winner's cubic (0..2); 3 = refitted by hak_refine_fundamental;
                              * 16 + r = root r (0..9) of the degree-10 polynomial of hak_find_essential */
    int   n;                 /* matches considered */
} hak_fundamental;           /* 52 bytes, as hak_homography */
/* one list, synchronous; ctx may be NULL (default stream; the call allocates its own scratch); result to *h_out (host) */
int hak_find_fundamental(hak_ctx* ctx, const hak_match_pair* d_matches, int n, int iterations, float threshold, unsigned seed,
                         unsigned char* d_mask, hak_fundamental* h_out);
/* batched, asynchronous on the context's stream, layouts as hak_find_homography_batch: the output of hak_match_knn2_batch or
 * hak_match_guided_batch goes in without a host synchronisation */
int hak_find_fundamental_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                               int iterations, float threshold, unsigned seed, hak_fundamental* d_out,
                               unsigned char* d_masks);

/* ---- rank-2 least-squares refit of a fundamental matrix over its inliers, iterated (build-side addition; the stage behind
 * hak_find_fundamental, and the local-optimisation step of LO-RANSAC).  The seven-point winner is fitted to seven noisy points;
 * the refit fits all of its inliers, re-scores, and repeats from the larger inlier set.  A pure function of (matches, input
 * record, threshold, rounds); tests/fundamental_refit_ref.py is its bit-exact numpy statement.  float64, no FMA, + - * / sqrt
 * only; records are read as by hak_find_fundamental (a non-finite coordinate is never an inlier and enters no sum).
 *   0. 1 <= rounds <= 8, threshold finite and > 0, t2 = threshold * threshold in float32.  A record with hypothesis < 0 or a
 *      non-finite entry of F has no model: the output is the no-model record (F = 0, inliers 0, hypothesis -1, root 0, n) and an
 *      all-zero mask.  Otherwise cur = F and cnt = the inliers of cur by step 7 of hak_find_fundamental at THIS call's t2.
 *      Steps 1-7 repeat up to `rounds` times and stop at the first round that fails or is not accepted.
 *   1. I = the inliers of cur, m = |I|.  The round fails if m < 8.
 *   2. Every sum over I is taken in the order of hak_find_homography's refit: lane l of one wave takes the matches i = l (mod 64)
 *      in ascending i, non-inliers skipped, every partial sum starting from 0.0; then an xor butterfly over 32, 16, .., 1.
 *   3. Hartley normalisation per image: c = sum / m, d = p - c, q = sum (dx dx + dy dy), s = sqrt((2 m) / q).  The round fails
 *      unless q > 0 and s is finite.  Normalised points (x, y) = s1 d1, (u, v) = s2 d2.
 *   4. w = [u x, u y, u, v x, v y, v, x, y, 1]; the 45 sums N[p][q] += w[p] * w[q], p <= q, mirrored afterwards.
 *   5. jacobi(A, n, S), cyclic Jacobi: V = I; for sweep = 0..S-1, p = 0..n-2, q = p+1..n-1: apq = A[p][q]; nothing if apq == 0;
 *      th = (A[q][q] - A[p][p]) / (2 apq), sg = +1 if th >= 0 else -1, t = sg / (|th| + sqrt(th th + 1)),
 *      c = 1 / sqrt(t t + 1), sn = t c; for k not in {p, q}, x = A[k][p], y = A[k][q]: A[k][p] = A[p][k] = c x - sn y,
 *      A[k][q] = A[q][k] = sn x + c y; A[p][p] = A[p][p] - t apq, A[q][q] = A[q][q] + t apq, A[p][q] = A[q][p] = 0; for all k,
 *      x = V[k][p], y = V[k][q]: V[k][p] = c x - sn y, V[k][q] = sn x + c y.  The answer is the column j of V with the smallest
 *      A[j][j] (found with <, from j = 0: ties to the smallest j).  f = jacobi(N, 9, 8); the round fails if an entry of f is
 *      non-finite.
 *   6. Rank 2: Fn = f as 3 x 3, row-major; G[i][j] = (Fn[0][i] Fn[0][j] + Fn[1][i] Fn[1][j]) + Fn[2][i] Fn[2][j];
 *      v = jacobi(G, 3, 6); g_i = (Fn[i][0] v0 + Fn[i][1] v1) + Fn[i][2] v2; Fn'[i][j] = Fn[i][j] - g_i v_j -- Fn without its
 *      smallest singular triplet, the closest rank-2 matrix in the Frobenius norm.
 *   7. F = T2^T (Fn' T1), divided by its entry of largest |value| (ties to the smallest index) and rounded to float32, exactly
 *      as step 6 of hak_find_fundamental; the round fails if that entry is 0 or anything is non-finite.  cnt' = the inliers of
 *      that F.  The round is accepted iff cnt' >= cnt; then cur = F, cnt = cnt'.
 *   8. Output: F = cur, inliers = cnt, hypothesis unchanged, n = the matches considered, root = 3 if a round was accepted and
 *      the input's root otherwise; the optional mask gets the inliers of cur at this call's threshold.  So inliers never falls
 *      below the input F's count at the same threshold, and a refitted record may be passed in again.
 * Limits: an unweighted algebraic (eight-point) fit -- no Sampson weighting, no re-weighting; nothing is estimated beyond F (the pose is the
 * next stage, hak_recover_pose below).
 * Refused with a non-zero status and a message before any device is touched: rounds outside 1..8, a threshold that is not finite
 * or not > 0, n < 0, a NULL list with n > 0, a list that is not 16-byte aligned, NULL h_inout / d_inout / d_counts, npairs < 1,
 * stride < 1, a NULL context for the batch form.  Device code: csrc/kernels_fundrefit.hip. */
/* one list, synchronous; ctx may be NULL (default stream; the call needs no scratch and allocates nothing: calls without a
 * context share one device-resident record and take it in turn).  *h_inout (host): in = a record of hak_find_fundamental,
 * out = the result */
int hak_refine_fundamental(hak_ctx* ctx, const hak_match_pair* d_matches, int n, float threshold, int rounds,
                           unsigned char* d_mask, hak_fundamental* h_inout);
/* batched, asynchronous on the context's stream, layouts as hak_find_fundamental_batch; d_inout[k] (device) is read and rewritten
 * in place, so detect batch -> hak_match_knn2_batch -> hak_find_fundamental_batch -> hak_refine_fundamental_batch ->
 * hak_match_epipolar_batch needs no host synchronisation */
int hak_refine_fundamental_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                                 float threshold, int rounds, hak_fundamental* d_inout, unsigned char* d_masks);

/* ---- relative pose from a fundamental matrix (build-side addition; the stage behind hak_find_fundamental and
 * hak_refine_fundamental, and what a stereo, SfM or SLAM front end consumes).  From F and the two cameras' pinhole intrinsics:
 * the rotation and the baseline's direction between the cameras, which matches lie in front of both, and a first 3-D point per
 * such match.  Conventions: X2 = R X1 + t with X1, X2 the same point in the first and the second camera's frame; |t| = 1 (the
 * baseline's length is not observable); points are in the FIRST camera's frame in units of the baseline.  A pure function of
 * (matches, F, K1, K2, threshold, max_depth); tests/pose_ref.py is its bit-exact numpy statement.  float64, no FMA, + - * / sqrt
 * only; records are read as by hak_find_fundamental (a non-finite coordinate is never an inlier).  dot(a, b) below is
 * (a0 b0 + a1 b1) + a2 b2, cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), M v has the entries dot(row i of M, v).
 *   1. No model: a record with hypothesis < 0 (batch form), or an F with a non-finite entry, gives the no-pose record
 *      (R = identity, t = 0, inliers = 0, in_front = 0, candidate = -1, n) and an all-zero mask and xyz.
 *   2. Essential matrix: E = K2^T (F K1), K = [fx 0 cx; 0 fy cy; 0 0 1] widened to float64, both products as in step 6 of
 *      hak_find_fundamental; every entry of E is divided by E's entry of largest |value| (ties to the smallest index; E stays
 *      float64).  No pose (the record of step 1) if that entry is 0 or non-finite.
 *   3. Decomposition: G[i][j] = (E[0][i] E[0][j] + E[1][i] E[1][j]) + E[2][i] E[2][j]; the sweeps of jacobi(G, 3, 6) of
 *      hak_refine_fundamental leave the eigenvalues on G's diagonal and the eigenvectors in V's columns.  j3 = the column with the
 *      smallest G[j][j] (<, ties to the smallest j); v1, v2 = the other two columns in ascending order; v3 = cross(v1, v2).
 *      x = E v1, l1 = sqrt(dot(x, x)), u1 = x / l1; y = E v2, d = dot(u1, y), w = y - d u1, l2 = sqrt(dot(w, w)), u2 = w / l2;
 *      u3 = cross(u1, u2).  No pose unless l1 and l2 are finite and > 0.  [u1 u2 u3] and [v1 v2 v3] have determinant +1 by
 *      construction, so both rotations below are proper.
 *   4. Candidates: Ra[i][j] = (u2_i v1_j - u1_i v2_j) + u3_i v3_j (= U W V^T, W = [0 -1 0; 1 0 0; 0 0 1]),
 *      Rb[i][j] = (u1_i v2_j - u2_i v1_j) + u3_i v3_j (= U W^T V^T); candidates 0..3 = (Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3),
 *      all float64 (nothing is rounded before step 6).
 *   5. Depths, for every inlier of F by step 7 of hak_find_fundamental at t2 = threshold * threshold in float32, under a
 *      candidate (R, t): x = (x1 - cx1) / fx1, y = (y1 - cy1) / fy1, a_i = (R[i][0] x + R[i][1] y) + R[i][2],
 *      b = ((x2 - cx2) / fx2, (y2 - cy2) / fy2, 1); aa = dot(a, a), bb = dot(b, b), ab = dot(a, b), at = dot(a, t),
 *      bt = dot(b, t); det = aa bb - ab ab, z1 = (ab bt - bb at) / det, z2 = (aa bt - ab at) / det -- the least-squares solution
 *      of z1 a + t = z2 b.  In front iff det > 0 and 0 < z1 < max_depth and 0 < z2 < max_depth (max_depth widened to float64;
 *      NaN fails).
 *   6. The candidate with the most inliers in front wins, ties to the smallest index.  R and t are the winner's, rounded to
 *      float32; inliers = the inliers of F, in_front = the winner's count, candidate = its index.  The optional mask gets 1 for
 *      an inlier in front under the winner, 0 otherwise (n bytes); the optional xyz gets (float32(z1 x), float32(z1 y),
 *      float32(z1)) for such a match and (0, 0, 0) otherwise (3 n floats).  in_front = 0 is still a pose: candidate = -1 only
 *      comes from steps 1-3.
 * Every value reduced across lanes is an integer count, so the result does not depend on the launch shape.
 * Limits: the pose comes from whatever F it is handed (hak_find_essential below is the calibrated estimator, hak_refine_pose the
 * calibrated refit); no lens distortion, no skew;
 * no bundle adjustment; depths are a linear two-ray solve, not a reprojection-error minimum.  A planar scene or a pure rotation
 * gives an F that does not determine the pose: the call returns whatever wins, and in_front / inliers is the caller's signal.
 * Refused with a non-zero status and a message before any device is touched: a threshold that is not finite or not > 0, a
 * max_depth that is NaN or not > 0 (+inf is allowed), fx or fy not finite or 0, a non-finite cx or cy, NULL F / K1 / K2 / h_out /
 * d_out / d_F / d_counts, n < 0, a NULL list with n > 0, a list that is not 16-byte aligned, npairs < 1, stride < 1, a NULL context
 * for the batch form.  Device code: csrc/kernels_pose.hip. */
typedef struct hak_intrinsics { float fx, fy, cx, cy; } hak_intrinsics;   /* pinhole, zero skew */
typedef struct hak_pose {
    float R[9];              /* row-major, X2 = R X1 + t */
    float t[3];              /* unit length: the baseline's direction, its scale is not observable */
    int   inliers;           /* Sampson inliers of F at this call's threshold */
    int   in_front;          /* of those, the matches in front of both cameras under (R, t) */
    int   candidate;         /* 0..3: which of the four decompositions won; 4 = refitted by hak_refine_pose; -1 = no pose
                              * (R = identity, t = 0) */
    int   n;                 /* matches considered */
} hak_pose;                  /* 64 bytes */
/* one list, synchronous; ctx may be NULL (default stream); F: 9 floats on the HOST, row-major as hak_fundamental.F; d_mask (device,
 * n bytes) and d_xyz (device, 3 n floats) may each be NULL; result to *h_out (host).  The call needs no scratch and allocates
 * nothing: calls share one device-resident record and take it in turn. */
int hak_recover_pose(hak_ctx* ctx, const hak_match_pair* d_matches, int n, const float F[9] /* host */,
                     const hak_intrinsics* K1, const hak_intrinsics* K2, float threshold, float max_depth,
                     unsigned char* d_mask, float* d_xyz, hak_pose* h_out);
/* batched, asynchronous on the context's stream, layouts as hak_refine_fundamental_batch; K1 and K2 are host arguments, the same
 * for every pair of the call.  F of pair k is read ON THE DEVICE from d_F[k]; record k to d_out[k], mask of pair k to
 * d_masks + k*stride, its points to d_xyz + 3*k*stride (each unless NULL).  The chain detect batch -> hak_match_knn2_batch ->
 * hak_find_fundamental_batch (-> hak_refine_fundamental_batch) -> hak_recover_pose_batch needs no host synchronisation. */
int hak_recover_pose_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                           const hak_fundamental* d_F, const hak_intrinsics* K1, const hak_intrinsics* K2,
                           float threshold, float max_depth, hak_pose* d_out, unsigned char* d_masks, float* d_xyz);

/* ---- calibrated Gauss-Newton refit of the relative pose, iterated (build-side addition; the stage behind hak_recover_pose).
 * hak_recover_pose decomposes an F that was fitted with seven degrees of freedom and without the calibration; the refit fits the
 * five that remain once K1 and K2 are known -- rotation and baseline direction -- to the Sampson error in pixels of the matches
 * that count under the pose, re-scores, and repeats from the larger set.  A pure function of (matches, input record, K1, K2,
 * threshold, max_depth, rounds); tests/pose_refit_ref.py is its bit-exact numpy statement.  float64, no FMA, + - * / sqrt only,
 * except where float32 is named; records are read as by hak_find_fundamental; dot, cross and M v as hak_recover_pose defines them.
 *   1. No model: 1 <= rounds <= 8, t2 = threshold * threshold in float32.  A record with candidate < 0 or a non-finite entry of R
 *      or t, or whose pose has no F by step 2, gives the no-pose record of step 1 of hak_recover_pose and an all-zero mask and xyz.
 *   2. The F of a pose (R, t as float32, widened): column j of E = [t]x R is (t1 R[2][j] - t2 R[1][j], t2 R[0][j] - t0 R[2][j],
 *      t0 R[1][j] - t1 R[0][j]).  G = E K1^-1 row by row: G[i][0] = E[i][0] / fx1, G[i][1] = E[i][1] / fy1,
 *      G[i][2] = (E[i][2] - G[i][0] cx1) - G[i][1] cy1.  F = K2^-T G column by column: F[0][j] = G[0][j] / fx2,
 *      F[1][j] = G[1][j] / fy2, F[2][j] = (G[2][j] - F[0][j] cx2) - F[1][j] cy2.  Every entry is divided by F's entry of largest
 *      |value| (ties to the smallest index) and rounded to float32, as in step 6 of hak_find_fundamental; no model if that entry is
 *      0 or non-finite.  A match COUNTS under a pose when it is an inlier of this F by step 7 of hak_find_fundamental at t2 and lies
 *      in front by step 5 of hak_recover_pose under (R, t) widened from float32, with the same max_depth gates: the mask
 *      hak_recover_pose writes, taken under the pose's own F.  cur = the input pose, cnt = the matches that count under it.
 *   3. One round, over the matches that count under cur = (R, t): a = (x, y, 1) and b the normalised points of step 5 of
 *      hak_recover_pose, q = R a, c = cross(t, q), e = dot(b, c), v = cross(b, t), u_j = (R[0][j] v0 + R[1][j] v1) + R[2][j] v2
 *      (j = 0, 1); the Sampson denominator in pixels p0 = c0 / fx2, p1 = c1 / fy2, p2 = u0 / fx1, p3 = u1 / fy1,
 *      s = sqrt((p0 p0 + p1 p1) + (p2 p2 + p3 p3)); the residual res = e / s.  The tangent basis of t: k = the index of the
 *      smallest |t_k| (ties to the smallest index), nv = cross(t, e_k) written out as (0, t2, -t1), (-t2, 0, t0) or (t1, -t0, 0),
 *      b1 = nv / sqrt(dot(nv, nv)), b2 = cross(t, b1).  Five unknowns (w0, w1, w2, d3, d4) under the left perturbation
 *      R' = (I + [w]x) R and the tangent step t' = t + d3 b1 + d4 b2, with s held fixed: the Jacobian row is
 *      w = [ jw0 / s, jw1 / s, jw2 / s, dot(h, b1) / s, dot(h, b2) / s ], jw = cross(q, v), h = cross(q, b).
 *      The 15 sums N[p][q] += w[p] w[q], p <= q, mirrored afterwards, and the 5 sums g[p] += -(w[p] res), in the order of
 *      hak_find_homography's refit (lane l of one wave takes the matches i = l (mod 64) in ascending i, the others skipped, every
 *      partial sum from 0.0; then an xor butterfly over 32, 16, .., 1).  [N | g] (5 x 6) is solved as step 4 of hak_refine_pnp
 *      solves its 6 x 7; the solution is d.  Update: R' = C R with C the Cayley map of 0.5 (d0, d1, d2) exactly as step 5 of
 *      hak_refine_pnp; tn_i = (t_i + d3 b1_i) + d4 b2_i, len = sqrt(dot(tn, tn)), t' = tn / len; both rounded to float32; then
 *      the F of (R', t') by step 2.  The round fails if fewer than 5 matches count, a pivot is 0 or non-finite, an entry of d,
 *      len, R' or t' is non-finite, or (R', t') has no F.
 *   4. Acceptance: cnt' = the matches that count under (R', t').  The round is accepted iff cnt' >= cnt; then cur = (R', t'),
 *      cnt = cnt'.  At most `rounds` rounds are run; the first that fails or is not accepted ends the loop.
 *   5. Output: R, t = cur; in_front = cnt; inliers = the inliers of cur's F alone at this call's threshold; n = the matches
 *      considered; candidate = 4 if a round was accepted and the input's otherwise (4 is >= 0: every reader of a hak_pose view
 *      takes a refitted record as a model).  The optional mask gets the matches that count under cur, the optional xyz
 *      (float32(z1 x), float32(z1 y), float32(z1)) for them and zeros elsewhere, as step 6 of hak_recover_pose.
 * in_front never falls below the input pose's count RECOMPUTED BY STEP 2 AT THIS CALL'S THRESHOLD.  That need not be the input
 * record's in_front field, which hak_recover_pose counted under the F it was handed, not under the pose's own F; a refitted
 * record's `inliers` changes its meaning in the same way (inliers of the pose's F, not of the F that was decomposed).  A
 * refitted record may be passed in again, and at another threshold.
 * Every value reduced across lanes outside the fixed-order float64 sums is an integer count.
 * Limits: the Sampson denominator is frozen within a round; plain Gauss-Newton, one step per round, no damping and no robust
 * kernel; R is re-rounded to float32 every round and not re-orthonormalised; the
 * input pose must already be near (hak_find_essential or hak_find_fundamental + hak_recover_pose give the start).  A pure rotation or a planar scene makes the t-columns vanish or the system ill-conditioned,
 * and nothing rescues it: the round fails or is rejected and the record comes back unchanged.
 * Refused with a non-zero status and a message before any device is touched: what hak_recover_pose(_batch) refuses (with
 * h_inout / d_inout in place of F / h_out / d_out / d_F), and rounds outside 1..8.  Device code: csrc/kernels_poserefit.hip. */
/* one list, synchronous; ctx may be NULL (default stream; the call needs no scratch and allocates nothing: calls without a
 * context share one device-resident record and take it in turn).  K1, K2 are host arguments.  *h_inout (host): in = a record of
 * hak_recover_pose or of an earlier refit, out = the result; d_mask (device, n bytes) and d_xyz (device, 3 n floats) may each be
 * NULL */
int hak_refine_pose(hak_ctx* ctx, const hak_match_pair* d_matches, int n, const hak_intrinsics* K1, const hak_intrinsics* K2,
                    float threshold, float max_depth, int rounds, unsigned char* d_mask, float* d_xyz, hak_pose* h_inout);
/* batched, asynchronous on the context's stream, layouts exactly as hak_recover_pose_batch; d_inout[k] (device) is read and
 * rewritten in place, d_masks / d_xyz (each unless NULL) are overwritten with the refitted pose's -- in a chain the buffers
 * hak_recover_pose_batch wrote -- so .. -> hak_recover_pose_batch -> hak_refine_pose_batch -> hak_link_tracks_batch ->
 * hak_solve_pnp_batch -> .. needs no host synchronisation and no allocation */
int hak_refine_pose_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                          const hak_intrinsics* K1, const hak_intrinsics* K2, float threshold, float max_depth, int rounds,
                          hak_pose* d_inout, unsigned char* d_masks, float* d_xyz);

/* ---- five-point RANSAC essential matrix (build-side addition; the calibrated estimator next to hak_find_fundamental, for the
 * caller who knows K1 and K2 before the first match).  It samples five points, not seven, enforces the two essential constraints
 * and stays determined on a scene with a dominant plane (not on an exactly planar one: see the limits).  It writes a hak_fundamental record -- F = K2^-T E K1^-1 scaled so that its entry of largest
 * |value| is 1 -- scored by the float32 Sampson test in pixels of hak_find_fundamental, so inlier counts and masks compare directly
 * with the seven-point call at the same threshold, and hak_recover_pose(_batch), hak_refine_pose(_batch), hak_match_epipolar(_batch)
 * and hak_refine_fundamental(_batch) take the record as it is.  hak_refine_fundamental is legal on it but gives up the essential
 * constraints; the calibrated refit is hak_refine_pose.  A pure function of (matches, K1, K2, iterations, threshold, seed),
 * whatever the launch shape; tests/essential_ref.py is its bit-exact numpy statement.  float64, no FMA, + - * / only; records are
 * read as by hak_find_fundamental.  The rule is Nister's five-point solver:
 *   1. Hypothesis h (0 <= h < iterations, 1 <= iterations <= 65536) draws as step 1 of hak_find_fundamental (32 draws) until it has
 *      five distinct indices; it is degenerate with fewer (always when n < 5).
 *   2. Bearings: x = (x1 - cx1) / fx1, y = (y1 - cy1) / fy1, u = (x2 - cx2) / fx2, v = (y2 - cy2) / fy2, everything widened to
 *      float64 first.  Degenerate if one of them is non-finite.  No Hartley normalisation.
 *   3. The 5 x 9 system has the row [u x, u y, u, v x, v y, v, x, y, 1] per point, in draw order.  Gaussian elimination with COMPLETE
 *      pivoting, c = 0..4: the pivot is the largest |entry| of rows c..4 and columns c..8, scanned row by row with >, so ties go to
 *      the smallest row, then the smallest column; degenerate if it is 0 or non-finite; rows c and the pivot's are exchanged, then
 *      columns c and the pivot's (in all five rows; the column permutation is remembered); f = M[r][c] / M[c][c],
 *      M[r][q] = M[r][q] - f M[c][q] for r > c, q > c.  Four null vectors X, Y, Z, W by back substitution with the identity on the
 *      free positions 5..8: for vector k, f_(5+j) = (j == k), and for i = 4..0
 *      f_i = ((-M[i][5+k]) - M[i][i+1] f_(i+1) - .. - M[i][4] f_4) / M[i][i]; position p belongs to entry perm[p] of E.  Then the
 *      last free coordinate is mixed in: X' = X - 1.125 W, Y' = Y + 0.625 W, Z' = Z - 0.875 W (each entry v - a w with
 *      a = 1.125, -0.625, 0.875), W' = W, and E = x X' + y Y' + z Z' + W'.  Without the mix, w = 1 normalises a coordinate that is
 *      exactly zero on the true solution when R = I (E = [t]x has a zero diagonal): a stereo rig, a forward-moving camera.
 *   4. The ten cubic constraints.  Polynomials over v = (x, y, z, 1): a linear one has 4 coefficients, a quadratic one 10 (the pairs
 *      i <= j of variables in lexicographic order), a cubic one 20 (the triples likewise).  Products accumulate from 0.0:
 *      linear * linear adds a_i b_j to the coefficient of v_i v_j for i = 0..3, j = 0..3 in that order; quadratic * linear adds A_a b_k
 *      for a = 0..9, k = 0..3 in that order; a sum of products keeps accumulating into the same coefficients, a difference is taken
 *      between two finished products.  Row 0 is det E = E00 c0 + E01 c1 + E02 c2 with c0 = E11 E22 - E12 E21,
 *      c1 = E12 E20 - E10 E22, c2 = E10 E21 - E11 E20 (c_k * E0k, accumulated in k).  Row 1 + 3 i + j is entry (i, j) of
 *      2 E E^T E - tr(E E^T) E as sum over k of A_ik * E_kj with L_ik = sum over l of E_il * E_kl, t = (L00 + L11) + L22,
 *      A_ik = 2 L_ik - t for i = k and 2 L_ik otherwise.  The columns are then put in Nister's order
 *      x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.  Gauss-Jordan on the left 10 x 10 block with fixed
 *      pivot columns 0..9 and partial pivoting over rows, without moving a row: the pivot of column c is the largest |entry| among
 *      the rows that hold no pivot yet (>, ties to the smallest row); degenerate if it is 0 or non-finite; v_q = M[p][q] / M[p][c]
 *      for q > c replaces the pivot row p, every other row gets M[r][q] = M[r][q] - M[r][c] v_q.
 *   5. With e, f, g, h, i, j the right halves of the rows that hold the pivots of x^2z, x^2, y^2z, y^2, xyz, xy: k = e - z f,
 *      l = g - z h, m = i - z j, e.g. k_x(z) = e_x + (e_xz - f_x) z + (e_xz2 - f_xz) z^2 + (-f_xz2) z^3; B(z) has the rows k, l, m and
 *      the columns (x, y, 1), of degree 3, 3 and 4.  Polynomial products out[i + j] += a[i] b[j] in ascending (i, j) from 0.0;
 *      c0 = l_y m_1 - l_1 m_y, c1 = l_1 m_x - l_x m_1, c2 = l_x m_y - l_y m_x, det B = (k_x c0 + k_y c1) + k_1 c2: eleven
 *      coefficients.  Degenerate if the leading one is 0 or any is non-finite.
 *   6. Real roots by a derivative chain.  b_k = c_k / c_10, bound = 1 + max |b_k| (degenerate if a b_k or the bound is non-finite).
 *      Level d = 1..10 is the (10 - d)-th derivative over (10 - d)!: a_j = C(j + 10 - d, 10 - d) b_(j + 10 - d), j = 0..d (b_10 = 1),
 *      evaluated by Horner as ((a_d z + a_(d-1)) z + ..) + a_0.  It has d brackets between -bound, the d - 1 points of level d - 1
 *      and bound.  A bracket holds a root iff (p(lo) < 0) != (p(hi) < 0); there, 64 bisections with the replacement rule of step 5 of
 *      hak_find_fundamental, and the bracket's point is 0.5 (lo + hi); a bracket without a root passes its upper end on as its
 *      point (a split of an interval on which the next level is monotonic, so no root of that level is lost or found twice).  The
 *      roots of level 10 are numbered r = 0..9 in ascending bracket order, brackets without a root not counted.  A root of even
 *      multiplicity is missed.
 *   7. Per root z: (x, y, 1) is the cross product of two rows of B(z) divided by its third component, of the pair (0, 1), (0, 2) or
 *      (1, 2) whose third component is largest in magnitude (>, ties to the first); the model is dropped if that component is 0 or
 *      non-finite.  Then three Newton steps on B(z) (x, y, 1)^T = 0 in (x, y, z): residuals r_i = (a_i x + b_i y) + c_i, Jacobian rows
 *      [a_i, b_i, (a_i' x + b_i' y) + c_i'] (the derivatives' coefficients are k a_k), the step by Cramer's rule with the determinant
 *      of step 4 of hak_find_fundamental, columns replaced by r, subtracted.  (The expanded degree-10 polynomial loses digits on planar
 *      scenes; B(z) itself does not.)  E_k = ((x X'_k + y Y'_k) + z Z'_k) + W_k; F = K2^-T (E K1^-1) with
 *      K^-1 = [1/fx 0 -(cx/fx); 0 1/fy -(cy/fy); 0 0 1] and the products of step 6 of hak_find_fundamental; divided by its entry of
 *      largest |value| (ties to the smallest index) and rounded to float32.  The model is dropped if that entry is 0 or anything
 *      is non-finite.
 *   8. Scored as step 7 of hak_find_fundamental.  The model with the most inliers wins, ties to the smallest h, then the smallest
 *      root.
 * Output: a hak_fundamental record with root = 16 + r; hypothesis = -1 means no model (F all zero, inliers = 0, root = 0, mask all
 * zero).  Limits: roots of even multiplicity are missed; no lens distortion or skew; a pure rotation still leaves t undetermined;
 * on an EXACTLY planar scene two essential matrices fit every point and tie on inliers, the smallest (h, root) of them wins, and
 * in_front / inliers of the pose behind it is the caller's signal; no local optimisation inside the RANSAC loop (hak_refine_pose is the refit).
 * Refused with a non-zero status and a message before any device is touched: what hak_find_fundamental(_batch) refuses, NULL K1 /
 * K2, fx or fy not finite or 0, a non-finite cx or cy.  Device code: csrc/kernels_essential.hip (ten lanes per hypothesis; the
 * scaffold of csrc/ransac_common.h over three virtual hypotheses of four models per hypothesis). */
/* one list, synchronous; ctx may be NULL (default stream; the call allocates its own scratch); K1, K2 are host arguments; result to
 * *h_out (host); d_mask (device, n bytes) may be NULL */
int hak_find_essential(hak_ctx* ctx, const hak_match_pair* d_matches, int n, const hak_intrinsics* K1, const hak_intrinsics* K2,
                       int iterations, float threshold, unsigned seed, unsigned char* d_mask, hak_fundamental* h_out);
/* batched, asynchronous on the context's stream, layouts as hak_find_fundamental_batch; counts are read on the device; K1 and K2
 * are host arguments, the same for every pair of the call, as in hak_recover_pose_batch.  detect batch -> hak_match_knn2_batch ->
 * hak_find_essential_batch -> hak_recover_pose_batch -> hak_refine_pose_batch needs no host synchronisation */
int hak_find_essential_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                             const hak_intrinsics* K1, const hak_intrinsics* K2, int iterations, float threshold, unsigned seed,
                             hak_fundamental* d_out, unsigned char* d_masks);

/* ---- a third view: track linking and RANSAC absolute pose (build-side addition; the stages behind hak_recover_pose).  A second
 * hak_recover_pose for the next image pair has a unit baseline of its own, unrelated to the first pair's, so two relative poses do
 * not chain into a trajectory.  What keeps the scale is the absolute pose of the new image from 3-D to 2-D correspondences: the
 * points hak_recover_pose triangulated from images (I0, I1), as seen in I2.
 *
 * Link rule (hak_link_tracks; tests/link_ref.py is its byte-exact numpy statement).  List A (nA records, its optional mask and its
 * points xyzA, 3 floats per record, as hak_recover_pose writes them) comes from images (I0, I1), list B (nB records) from images
 * (I1, I2), I1 the same detection in both (detection is deterministic: the same image detected twice in one batch gives identical
 * records), so A[a].train and B[m].query index the same keypoints.  For each match m of B in ascending m, a is the smallest index
 * of A with A[a].train == B[m].query, that index in [0, max_index), and maskA NULL or maskA[a] != 0.  If there is such an a, the
 * record {X, Y, Z = xyzA[3a .. 3a+2], u = B[m].x2, v = B[m].y2, src3d = a, src2d = m, pad = 0} is appended to the output; count is
 * the number appended.  A record with a non-finite coordinate is still linked: the estimator is what rejects it.  Fewer than 2^30
 * records per list.  Scratch is a table train -> a of max_index ints per pair, cleared and filled with atomicMin inside the call;
 * it belongs to the context, is grown by the call that first needs it before anything is enqueued (as hak_set_retain_grid
 * allocates) and never inside a launch sequence.
 *
 * PnP rule (hak_solve_pnp; tests/pnp_ref.py is its bit-exact numpy statement).  A pure function of (corr, K, iterations,
 * threshold, seed).  float64, no FMA, + - * / sqrt only, except where float32 is named; dot and cross as in hak_recover_pose.  A
 * record with a non-finite X, Y, Z, u or v is never an inlier and makes any sample it is in degenerate (it is read with X = NaN).
 *   1. Sampling: hypothesis h (0 <= h < iterations, 1 <= iterations <= 65536) draws r_d = mix64(seed + (16 h + d + 1) *
 *      0x9E3779B97F4A7C15) for d = 0..15, as step 1 of hak_find_homography, and takes index ((r_d >> 32) * n) >> 32 unless already
 *      chosen, until it has three: points 1, 2, 3 in draw order.  Degenerate with fewer than three distinct indices (always when n < 3).
 *   2. Bearings, K widened to float64: x = (u - cx) / fx, y = (v - cy) / fy, r = sqrt((x x + y y) + 1), b_i = (x / r, y / r, 1 / r).
 *      Squared sides a2 = |X2 - X3|^2, b2 = |X1 - X3|^2, c2 = |X1 - X2|^2, each dot(d, d) of the difference in that order; cosines
 *      ca = dot(b_2, b_3), cb = dot(b_1, b_3), cg = dot(b_1, b_2).  Degenerate if b2 is 0 or any of the six is non-finite.
 *   3. Grunert's quartic in v = s3 / s1 (s_i the distance of point i from the camera): p = (a2 - c2) / b2, q = (a2 + c2) / b2,
 *      rab = a2 / b2, rcb = c2 / b2, rbc = (b2 - c2) / b2, rba = (b2 - a2) / b2, ca2 = ca ca, cb2 = cb cb, cg2 = cg cg, pm = p - 1,
 *      pp = p p, pq = 1 + p;
 *        A4 = pm pm - 4 (rcb ca2)
 *        A3 = 4 (((p (1 - p)) cb - ((1 - q) ca) cg) + 2 ((rcb ca2) cb))
 *        A2 = 2 (((((pp - 1) + 2 (pp cb2)) + 2 (rbc ca2)) - 4 (((q ca) cb) cg)) + 2 (rba cg2))
 *        A1 = 4 (((-(p pq)) cb + 2 ((rab cg2) cb)) - ((1 - q) ca) cg)
 *        A0 = pq pq - 4 (rab cg2)
 *      Degenerate if A4 is 0 or a coefficient is non-finite.
 *   4. Positive real roots: b_k = A_k / A4 (k = 3..0), q(v) = (((v + b3) v + b2) v + b1) v + b0, B = 1 + max |b_k| (taken over
 *      k = 3, 2, 1, 0 with >); degenerate if a b_k or B is non-finite.  The critical points are the real roots of the monic cubic
 *      with the coefficients (0.75 b3, 0.5 b2, 0.25 b1), found by step 5 of hak_find_fundamental verbatim (its b2, b1, b0, its own
 *      bound, brackets and bisections; degenerate if it reports a non-finite value).  Of those, the r with 0 < r < B are kept in
 *      that step's order: r_0, ..; the brackets are [0, r_0], [r_0, r_1], .., [r_last, B] ([0, B] when none is kept).  A bracket
 *      holds a root iff (q(lo) < 0) != (q(hi) < 0); there, 64 bisections exactly as in that step, the root is 0.5 (lo + hi).  Up
 *      to four roots, numbered 0.. in bracket order: the solution index.
 *   5. Per root v: vv = v v, den = 2 (cg - v ca), w = (1 + vv) - (2 v) cb, u = ((pm vv - ((2 p) cb) v) + pq) / den,
 *      s1 = sqrt(b2 / w), s2 = u s1, s3 = v s1.  The root gives no model unless den != 0, w > 0 and s1, s2, s3 are finite and > 0.
 *      P_i = s_i b_i.  triad(P1, P2, P3): d1 = P2 - P1, d2 = P3 - P1, l1 = sqrt(dot(d1, d1)), e1 = d1 / l1, n = cross(d1, d2),
 *      ln = sqrt(dot(n, n)), e3 = n / ln, e2 = cross(e3, e1); no model if l1 or ln is 0 or non-finite.  (e1, e2, e3) =
 *      triad(P1, P2, P3), (f1, f2, f3) = triad(X1, X2, X3).  R[i][j] = (e1_i f1_j + e2_i f2_j) + e3_i f3_j,
 *      t_i = P1_i - dot(row i of R, X1), so that Xc = R X + t.  R and t are rounded to float32; no model if anything is non-finite.
 *   6. Score, float32, no FMA, K as given: xc = ((R0 X + R1 Y) + R2 Z) + t0, yc = ((R3 X + R4 Y) + R5 Z) + t1,
 *      zc = ((R6 X + R7 Y) + R8 Z) + t2; ex = (fx xc + cx zc) - u zc, ey = (fy yc + cy zc) - v zc; inlier iff zc > 0 and
 *      ex ex + ey ey < t2 (zc zc), t2 = threshold * threshold (threshold finite, > 0; NaN fails): the reprojection error in
 *      pixels is below the threshold and the point is in front of the camera.
 *   7. The model with the most inliers wins, ties to the smallest h, then the smallest solution index.  The optional mask gets 1
 *      for every inlier of the winner, 0 otherwise (n bytes).  No model at all: the no-model record (R = identity, t = 0,
 *      inliers = 0, hypothesis = -1, solution = 0, n) and an all-zero mask.
 * Every value reduced across lanes is an integer count, so the result does not depend on the launch shape.
 * Limits: the result is the three-point winner, fitted to three noisy points; the least-squares (Gauss-Newton) refit over its
 * inliers is the next stage, hak_refine_pnp below.  A root at which q touches zero without changing sign (a tangent double
 * root) is missed by design.  No lens distortion, no skew.
 * Refused with a non-zero status and a message before any device is touched: iterations outside 1..65536, a threshold that is not
 * finite or not > 0, fx or fy not finite or 0, a non-finite cx or cy, a count < 0 (or >= 2^30 for the link), a NULL list with a
 * positive count, a list or output list that is not 16-byte aligned, NULL outputs, counts, xyz or K, npairs < 1, a stride < 1, a
 * count step < 1, max_index < 1, a NULL context for the batch forms.  Device code: csrc/kernels_pnp.hip
 * (RANSAC scaffold: csrc/ransac_common.h). */
typedef struct hak_corr3d {  /* 32 bytes, 16-byte aligned loads */
    float X, Y, Z;           /* point, frame and units of the xyz it came from */
    float u, v;              /* its observation in the new image, pixels */
    int   src3d, src2d;      /* hak_link_tracks: index of the match in list A / list B it came from.  hak_match_projected: src3d =
                                the landmark's index in list A, src2d = the KEYPOINT index in the new image, not a match index */
    int   pad;               /* 0 */
} hak_corr3d;
typedef struct hak_abs_pose {
    float R[9];              /* row-major, Xc = R X + t */
    float t[3];              /* in the units of X */
    int   inliers;           /* inliers of (R, t) */
    int   hypothesis;        /* winning hypothesis, -1 = no model (R = identity, t = 0, inliers = 0) */
    int   solution;          /* which positive root of the winner's quartic, 0..3; 4 = refitted by hak_refine_pnp */
    int   n;                 /* correspondences considered */
} hak_abs_pose;              /* 64 bytes */
/* one pair of lists, synchronous; ctx may be NULL (default stream; the call allocates its own table).  d_maskA may be NULL; d_out
 * (device) has room for nB records; *count (host) their number; h_out (host, nB records) or NULL receives the list as well. */
int hak_link_tracks(hak_ctx* ctx, const hak_match_pair* d_A, int nA, const unsigned char* d_maskA, const float* d_xyzA,
                    const hak_match_pair* d_B, int nB, int max_index, hak_corr3d* d_out, int* count, hak_corr3d* h_out);
/* batched, asynchronous on the context's stream.  List k of A is at d_A + k*strideA, its count d_countsA[k*count_stepA] (read on the
 * device, clamped to [0, strideA]), its mask at d_masksA + k*strideA (unless NULL), its points at d_xyzA + 3*k*strideA; list k of B
 * at d_B + k*strideB with the count d_countsB[k*count_stepB], clamped to [0, min(strideB, out_stride)]; correspondences of k to
 * d_out + k*out_stride, their number to d_counts[k]; max_index is the context's cfg.max_pts.  With the outputs of one
 * hak_match_knn2_batch / hak_recover_pose_batch over a detect batch of image pairs (I0, I1), (I1, I2), .. -- d_A = d_matches,
 * d_B = d_matches + max_pts, d_countsA = d_counts, d_countsB = d_counts + 1, strides 2*max_pts, count steps 2 -- pair 2j links to
 * pair 2j+1, and detect batch -> hak_match_knn2_batch -> hak_find_fundamental_batch -> hak_refine_fundamental_batch ->
 * hak_recover_pose_batch -> hak_link_tracks_batch -> hak_solve_pnp_batch -> hak_refine_pnp_batch needs no host synchronisation. */
int hak_link_tracks_batch(hak_ctx* ctx, const hak_match_pair* d_A, long strideA, const int* d_countsA, int count_stepA,
                          const unsigned char* d_masksA, const float* d_xyzA, const hak_match_pair* d_B, long strideB,
                          const int* d_countsB, int count_stepB, int npairs, hak_corr3d* d_out, long out_stride, int* d_counts);
/* one list, synchronous; ctx may be NULL (default stream; the call allocates its own scratch); d_mask (device, n bytes) may be
 * NULL; result to *h_out (host) */
int hak_solve_pnp(hak_ctx* ctx, const hak_corr3d* d_corr, int n, const hak_intrinsics* K, int iterations, float threshold,
                  unsigned seed, unsigned char* d_mask, hak_abs_pose* h_out);
/* batched, asynchronous on the context's stream: list k at d_corr + k*stride, its count d_counts[k] read on the device and clamped
 * to [0, stride] (the layout hak_link_tracks_batch writes); record k to d_out[k], mask of k to d_masks + k*stride unless NULL */
int hak_solve_pnp_batch(hak_ctx* ctx, const hak_corr3d* d_corr, long stride, const int* d_counts, int npairs,
                        const hak_intrinsics* K, int iterations, float threshold, unsigned seed, hak_abs_pose* d_out,
                        unsigned char* d_masks);

/* ---- Gauss-Newton refit of the absolute pose over its inliers, iterated (build-side addition; the stage behind hak_solve_pnp).
 * The three-point winner is fitted to three noisy correspondences; the refit minimises the reprojection error over all of its
 * inliers, re-scores, and repeats from the larger inlier set.  A pure function of (corr, input record, K, threshold, rounds);
 * tests/pnp_refit_ref.py is its bit-exact numpy statement.  float64, no FMA, + - * / only, except where float32 is named; records
 * are read as by hak_solve_pnp (a record with a non-finite field is never an inlier and enters no sum).
 *   0. 1 <= rounds <= 8, threshold finite and > 0, t2 = threshold * threshold in float32.  A record with hypothesis < 0 or a
 *      non-finite entry of R or t has no model: the output is hak_solve_pnp's no-model record (R = identity, t = 0, inliers 0,
 *      hypothesis -1, solution 0, n) and an all-zero mask.  Otherwise cur = (R, t) as float32 and cnt = the inliers of cur by step 6
 *      of hak_solve_pnp at THIS call's t2.  Steps 1-5 repeat up to `rounds` times and stop at the first round that fails or is not
 *      accepted.
 *   1. I = the inliers of cur, m = |I|.  The round fails if m < 4.
 *   2. Per inlier, M = cur and K widened to float64: xc = ((M0 X + M1 Y) + M2 Z) + t0, yc = ((M3 X + M4 Y) + M5 Z) + t1,
 *      zc = ((M6 X + M7 Y) + M8 Z) + t2; iz = 1 / zc, a = xc iz, b = yc iz; residuals rx = (fx a + cx) - u, ry = (fy b + cy) - v;
 *      px = fx iz, py = fy iz.  The Jacobian rows with respect to the left perturbation Xc' = Xc + w x Xc + dt, unknowns
 *      (w0, w1, w2, dt0, dt1, dt2):
 *        jx = [ -((px a) yc), px zc + (px a) xc, -(px yc), px, 0, -(px a) ]
 *        jy = [ (-(py zc)) - (py b) yc, (py b) xc, py xc, 0, py, -(py b) ]
 *   3. The 21 sums N[p][q] += jx[p] jx[q] + jy[p] jy[q], p <= q, mirrored afterwards, and the 6 sums g[p] += -(jx[p] rx + jy[p] ry),
 *      over I in the order of hak_find_homography's refit: lane l of one wave takes the correspondences i = l (mod 64) in ascending
 *      i, non-inliers skipped, every partial sum starting from 0.0; then an xor butterfly over 32, 16, .., 1.
 *   4. [N | g] (6 x 7) is solved by Gaussian elimination with partial pivoting exactly as step 5 of hak_find_homography solves its
 *      8 x 9 system: the pivot of column c is the largest |entry| of rows c..5, ties to the smallest row; the round fails if it is
 *      0 or non-finite; f = M[r][c] / M[c][c], M[r][q] = M[r][q] - f M[c][q]; back substitution i = 5..0 with the subtractions in
 *      ascending j.  The solution is d; the round fails if an entry of d is non-finite.
 *   5. Update by the Cayley map (rational: no sin / cos, an exact rotation up to rounding): w = 0.5 (d0, d1, d2),
 *      ww = (w0 w0 + w1 w1) + w2 w2, k = 1 - ww, den = 1 + ww,
 *        C = [ k + 2 (w0 w0), 2 (w0 w1 - w2), 2 (w0 w2 + w1);  2 (w0 w1 + w2), k + 2 (w1 w1), 2 (w1 w2 - w0);
 *              2 (w0 w2 - w1), 2 (w1 w2 + w0), k + 2 (w2 w2) ], every entry divided by den;
 *      R' = C R and t' = C t + (d3, d4, d5), every entry (c0 r0 + c1 r1) + c2 r2 (then + d for t'), rounded to float32; the round
 *      fails if anything is non-finite.  cnt' = the inliers of (R', t').  The round is accepted iff cnt' >= cnt; then
 *      cur = (R', t'), cnt = cnt'.
 *   6. Output: R, t = cur, inliers = cnt, hypothesis unchanged, n = the correspondences considered, solution = 4 if a round was
 *      accepted and the input's otherwise; the optional mask gets the inliers of cur at this call's threshold.  So inliers never
 *      falls below the input pose's count at the same threshold, and a refitted record may be passed in again.
 * Limits: an unweighted reprojection-error minimum over a hard inlier set -- no robust kernel, no damping (plain Gauss-Newton, one
 * step per round), no refinement of the 3-D points or of K.  R is re-rounded to float32 every round and is not re-orthonormalised
 * (the drift after 8 rounds is of the order of 1e-7 in |R R^T - I|).  Coplanar or near-collinear inlier sets give an
 * ill-conditioned N; nothing rescues the round: it scores badly and is rejected.
 * Refused with a non-zero status and a message before any device is touched: rounds outside 1..8, a threshold that is not finite
 * or not > 0, fx or fy not finite or 0, a non-finite cx or cy, NULL K, n < 0, a NULL list with n > 0, a list that is not 16-byte
 * aligned, NULL h_inout / d_inout / d_counts, npairs < 1, stride < 1, a NULL context for the batch form.
 * Device code: csrc/kernels_pnprefit.hip. */
/* one list, synchronous; ctx may be NULL (default stream; the call needs no scratch and allocates nothing: calls without a
 * context share one device-resident record and take it in turn).  K is a host argument.  *h_inout (host): in = a record of
 * hak_solve_pnp or of an earlier refit, out = the result; d_mask (device, n bytes) may be NULL */
int hak_refine_pnp(hak_ctx* ctx, const hak_corr3d* d_corr, int n, const hak_intrinsics* K, float threshold, int rounds,
                   unsigned char* d_mask, hak_abs_pose* h_inout);
/* batched, asynchronous on the context's stream, layouts as hak_solve_pnp_batch; K is a host argument, the same for every list;
 * d_inout[k] (device) is read and rewritten in place, so .. -> hak_link_tracks_batch -> hak_solve_pnp_batch ->
 * hak_refine_pnp_batch needs no host synchronisation */
int hak_refine_pnp_batch(hak_ctx* ctx, const hak_corr3d* d_corr, long stride, const int* d_counts, int npairs,
                         const hak_intrinsics* K, float threshold, int rounds, hak_abs_pose* d_inout, unsigned char* d_masks);

/* ---- a fourth view: triangulation under two known views (build-side addition; the stage behind hak_refine_pnp).  The only 3-D
 * points the stages above produce are those hak_recover_pose computes from images (I0, I1).  With the pose of I1 (hak_recover_pose)
 * and the absolute pose of I2 (hak_solve_pnp, hak_refine_pnp) both known in the first camera's frame, the matches of (I1, I2) are
 * triangulated under those two views, in the same frame and scale and in the layout hak_link_tracks reads, so that linking them to
 * the matches of (I2, I3) and another hak_solve_pnp give the pose of I3 -- and so on.  A view is Xc = R X + t; the points are in
 * the frame the two views map FROM, in the units of their t.
 * A pure function of (matches, view A, view B, KA, KB, threshold, max_depth, min_sin); tests/triangulate_ref.py is its bit-exact
 * numpy statement.  float64, no FMA, + - * / only, except where float32 is named; records are read as by hak_find_fundamental
 * (x1, y1 is seen by view A, x2, y2 by view B); dot as in hak_recover_pose.
 *   1. No model: a view of kind HAK_VIEW_RELATIVE with candidate < 0, of kind HAK_VIEW_ABSOLUTE with hypothesis < 0, or with a
 *      non-finite entry of R or t, gives the no-model record {n, 0, {0, 0, 0}, 0, 0, 0}, an all-zero mask and all-zero points.  An
 *      identity view (kind HAK_VIEW_IDENTITY, or a NULL host view) is R = I, t = 0, always has a model and goes through every
 *      expression below like any other.
 *   2. Centres: R and t widened to float64; cA_j = -((RA[0][j] tA0 + RA[1][j] tA1) + RA[2][j] tA2) for j = 0..2, cB likewise;
 *      w = cA - cB.
 *   3. Rays, per match: xa = (x1 - cxA) / fxA, ya = (y1 - cyA) / fyA, a_j = (RA[0][j] xa + RA[1][j] ya) + RA[2][j] -- the bearing
 *      turned into the common frame; b likewise from (x2, y2), KB and RB.  aa = dot(a, a), bb = dot(b, b), ab = dot(a, b),
 *      aw = dot(a, w), bw = dot(b, w); det = aa bb - ab ab, z1 = (ab bw - bb aw) / det, z2 = (aa bw - ab aw) / det -- the
 *      least-squares solution of cA + z1 a = cB + z2 b, in the form of step 5 of hak_recover_pose.  The bearings have third camera
 *      coordinate 1, so z1 and z2 are depths along the optical axes, in the units of the views' t.
 *   4. Gate 0, parallax: det > 0 and det >= s2 (aa bb), s2 = min_sin min_sin with min_sin widened to float64 first (det / (aa bb)
 *      is the squared sine of the angle between the rays).  NaN fails, so a record with a non-finite coordinate is rejected here.
 *   5. Gate 1, depth: 0 < z1 < max_depth and 0 < z2 < max_depth (max_depth widened to float64; both bounds strict).
 *   6. Point: P_j = 0.5 ((cA_j + z1 a_j) + (cB_j + z2 b_j)), rounded to float32: the midpoint of the common perpendicular.
 *   7. Gate 2, reprojection: the float32 test of step 6 of hak_solve_pnp, unchanged, of the float32 P under view A's float32
 *      (R, t), KA and the observation (x1, y1), and again under view B with KB and (x2, y2); both must pass at
 *      t2 = threshold * threshold in float32.
 *   8. Outputs: mask 1 and xyz = P for a match that passes every gate, mask 0 and xyz (0, 0, 0) otherwise; kept = the matches
 *      that passed, rejected[g] = the matches whose FIRST failed gate is g, so kept + rejected[0] + rejected[1] + rejected[2] = n
 *      when there is a model.
 * Every value reduced across lanes is an integer count, so the result does not depend on the launch shape.
 * Limits: a midpoint solve under a reprojection gate, not a reprojection-error minimum, and there is no per-point refit -- three
 * Gauss-Newton rounds per point moved no figure of the four-view accuracy table (README.md) by more than its last digit, except one
 * translation direction on the 1 px leg, for the worse.  Two views only: no multi-view tracks, no bundle adjustment.  No lens
 * distortion, no skew.  With A the identity and B a pair's own hak_pose the point set is close to hak_recover_pose's but not
 * bit-identical: a different frame for the solve, a midpoint instead of a point on the first ray, a reprojection gate instead of
 * a Sampson gate.
 * Refused with a non-zero status and a message before any device is touched: a threshold that is not finite or not > 0, a
 * max_depth that is NaN or not > 0 (+inf is allowed), a min_sin outside [0, 1) or NaN, a kind outside 0..2, a NULL view array for
 * kind 1 or 2, a view step < 0, a count step < 1, fx or fy not finite or 0, a non-finite cx or cy, NULL KA / KB / h_out / d_out /
 * d_counts, n < 0, a NULL list with n > 0, a list that is not 16-byte aligned, npairs < 1, stride < 1, a NULL context for the batch
 * form, a non-finite entry of a host RtA or RtB.  Device code: csrc/kernels_triangulate.hip. */
enum { HAK_VIEW_IDENTITY = 0, HAK_VIEW_RELATIVE = 1, HAK_VIEW_ABSOLUTE = 2 };
typedef struct hak_triangulation {   /* 32 bytes */
    int n;                   /* matches considered */
    int kept;                /* matches that passed every gate: mask = 1, a point written */
    int rejected[3];         /* by the FIRST gate a match fails: 0 parallax, 1 depth, 2 reprojection; kept + sum = n when model */
    int model;               /* 1, or 0 = a view without a model: kept = 0, rejected = 0, all-zero mask and points */
    int pad[2];              /* 0 */
} hak_triangulation;
/* one list, synchronous; ctx may be NULL (default stream); RtA / RtB: 12 floats on the HOST {R row-major, t}, Xc = R X + t,
 * NULL = identity; d_mask (device, n bytes) and d_xyz (device, 3 n floats) may each be NULL; result to *h_out (host).  The call
 * needs no scratch and allocates nothing: calls share one device-resident record and take it in turn. */
int hak_triangulate(hak_ctx* ctx, const hak_match_pair* d_matches, int n, const float* RtA, const float* RtB,
                    const hak_intrinsics* KA, const hak_intrinsics* KB, float threshold, float max_depth, float min_sin,
                    unsigned char* d_mask, float* d_xyz, hak_triangulation* h_out);
/* batched, asynchronous on the context's stream.  List k is at d_matches + k*stride, its count d_counts[k*count_step] (read on the
 * device, clamped to [0, stride]); view A of list k is record k*view_stepA of d_viewsA, read ON THE DEVICE: an array of hak_pose
 * for kindA = HAK_VIEW_RELATIVE, of hak_abs_pose for HAK_VIEW_ABSOLUTE (both are 64 bytes and begin with R[9], t[3]; no record is
 * copied or converted), ignored (may be NULL) for HAK_VIEW_IDENTITY; view B likewise.  A step of 0 gives every list the same view.
 * KA and KB are host arguments, the same for every list.  Record k to d_out[k], the mask of list k to d_masks + k*stride, its
 * points to d_xyz + 3*k*stride (each unless NULL).  The call needs no scratch and allocates nothing.
 * After a detect batch of six images per chain (I0, I1, I1, I2, I2, I3) and hak_match_knn2_batch, pairs 3j, 3j+1, 3j+2 are
 * (I0, I1), (I1, I2), (I2, I3).  With d_pose from hak_recover_pose_batch (one record per pair) and d_abs from hak_refine_pnp_batch
 * (one per chain), the call on (I1, I2) is d_matches + max_pts, stride 3*max_pts, d_counts + 1, count step 3, npairs = the
 * chains, view A = d_pose, RELATIVE, step 3, view B = d_abs, ABSOLUTE, step 1, d_masks + max_pts and d_xyz + 3*max_pts of the
 * buffers hak_recover_pose_batch wrote: mask and points of (I1, I2) then have that call's layout, a following
 * hak_link_tracks_batch takes d_A = d_matches + max_pts, d_masksA = d_masks + max_pts, d_xyzA = d_xyz + 3*max_pts,
 * d_B = d_matches + 2*max_pts with strides 3*max_pts and count steps 3, and .. -> hak_refine_pnp_batch -> hak_triangulate_batch ->
 * hak_link_tracks_batch -> hak_solve_pnp_batch -> hak_refine_pnp_batch gives the pose of I3 with no host synchronisation.  With
 * A = HAK_VIEW_IDENTITY and B = the pair's own hak_pose the call re-triangulates the first pair under a reprojection gate. */
int hak_triangulate_batch(hak_ctx* ctx, const hak_match_pair* d_matches, long stride, const int* d_counts, int count_step,
                          int npairs, const void* d_viewsA, int kindA, int view_stepA, const void* d_viewsB, int kindB,
                          int view_stepB, const hak_intrinsics* KA, const hak_intrinsics* KB, float threshold,
                          float max_depth, float min_sin, hak_triangulation* d_out, unsigned char* d_masks, float* d_xyz);

/* ---- guided matching: re-match a pair under its estimated homography (build-side addition; the stage behind
 * hak_find_homography).  The 2-NN search of hak_match_knn2 looks at the whole other image, so on repetitive texture its ratio
 * test rejects correct matches that lose to a look-alike elsewhere; once H is known, each query is searched only among the train
 * points near where H sends it.  A pure function of its arguments -- in particular it does not depend on how the implementation
 * bins the points; tests/guided_match_ref.py is its bit-exact numpy statement.
 *   Projection of query i, float32, no FMA, (x, y) = pts1[i].x, .y:
 *      wz = (h6 x + h7 y) + h8, u = (h0 x + h1 y) + h2, v = (h3 x + h4 y) + h5, px = u / wz, py = v / wz (correctly rounded).
 *   Gate G(i, j): wz > 0 and, with dx = x2_j - px, dy = y2_j - py, (dx dx) + (dy dy) < r2, r2 = radius * radius in float32.
 *      Any NaN makes the comparison false: a record with a non-finite coordinate, or a non-finite projection, is in no gate.
 *   Distance d(i, j): the Hamming distance of hak_match_knn2 (the 61 descriptor bytes).
 *   Forward: J_i = { j : G(i, j) }; j1 = the member of J_i with the smallest d, ties to the smallest j; d1 = d(i, j1);
 *      d2 = the smallest d over J_i \ {j1}, 512 when there is none.
 *   Reverse: I_j = { i : G(i, j) } -- the same gate, no inverse projection; rev(j) = the member of I_j with the smallest d, ties to
 *      the smallest i.
 *   Accept query i iff J_i is not empty and d1 < max_dist and d1 * ratio_den < d2 * ratio_num (64-bit products)
 *      and (cross_check == 0 or rev(j1) == i).
 *   Outputs as hak_match_knn2: match / distance / match_x / match_y of an accepted query, -1 / -1 / -1.f / -1.f of a rejected one
 *      (copied to h_pts1 when given); the accepted matches in ascending query order to d_out (capacity >= n1; may be NULL) with
 *      second = d2; *count their number; h_out (needs d_out) receives the list as well.
 * Synchronous; ctx may be NULL (default stream, scratch allocated for the call).  H: 9 floats on the HOST, row-major.
 * max_dist <= 0 selects 96.  Refused with a non-zero status and a message before any device is touched: radius not finite or
 * not > 0, radius * radius not finite in float32, H NULL or with a non-finite entry, a negative count, a ratio term <= 0, a NULL
 * point array with a positive count.  Fewer than 2^20 points per side.  Device code: csrc/kernels_guided.hip. */
int hak_match_guided(hak_ctx* ctx, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2,
                     const float H[9] /* host */, float radius, int ratio_num, int ratio_den, int cross_check,
                     int max_dist, hak_point* h_pts1, hak_match_pair* d_out, int* count, hak_match_pair* h_out);
/* batched over the pairs of a detect batch, layouts and outputs as hak_match_knn2_batch; asynchronous on the context's stream.
 * H of pair k is read ON THE DEVICE from d_H[k], the record hak_find_homography_batch wrote: the chain detect batch ->
 * hak_match_knn2_batch -> hak_find_homography_batch -> hak_match_guided_batch needs no host synchronisation.  A pair whose
 * record has hypothesis < 0 or a non-finite entry of H has no model: count 0, every query rejected.  A NULL context is refused. */
int hak_match_guided_batch(hak_ctx* ctx, hak_point* d_points, const int* d_num_pts, int npairs,
                           const hak_homography* d_H /* device, one per pair */, float radius,
                           int ratio_num, int ratio_den, int cross_check, int max_dist,
                           hak_match_pair* d_out, int* d_counts);

/* ---- epipolar guided matching: re-match a pair under its estimated fundamental matrix (build-side addition; the stage behind
 * hak_find_fundamental, as hak_match_guided is the stage behind hak_find_homography).  For two views of a 3-D scene there is no
 * point-to-point map, but F sends query i to a LINE in image 2; each query is searched only among the train points closer than
 * `radius` to its line.  A pure function of its arguments -- in particular it does not depend on how the implementation bins the
 * points; tests/epipolar_match_ref.py is its bit-exact numpy statement.
 *   Line of query i, float32, no FMA, (x, y) = pts1[i].x, .y, F row-major with (x2 y2 1) F (x1 y1 1)^T = 0 as hak_fundamental:
 *      a = (F0 x + F1 y) + F2, b = (F3 x + F4 y) + F5, c = (F6 x + F7 y) + F8, den = a a + b b -- the a, b, c of step 7 of
 *      hak_find_fundamental.
 *   Domain, L = 16384, DEN_MIN = 2^-100: query i has no gate unless |x| <= L and |y| <= L and den is finite and >= DEN_MIN; train
 *      point j is in no gate unless |x2_j| <= L and |y2_j| <= L.  NaN fails every comparison.  These bounds belong to the rule, not
 *      to an implementation: they are what makes a conservative search window provable.  The floor on den keeps e e from
 *      underflowing into a pass far from the line; a query at the epipole has a = b = 0 and, correctly, no band.
 *   Gate G(i, j): the domain holds and, with e = (a x2_j + b y2_j) + c, e e < r2 den, r2 = radius * radius, all in float32: the
 *      distance of train point j from the line of query i in image 2 is below radius.  The Sampson distance of hak_find_fundamental
 *      divides the same e e by a LARGER denominator (den + p p + q q), so it is never larger than this distance: up to rounding,
 *      every accepted match is an inlier of F at threshold = radius.
 *   Distance d(i, j): the Hamming distance of hak_match_knn2 (the 61 descriptor bytes).
 *   Forward: J_i = { j : G(i, j) }; j1 = the member of J_i with the smallest d, ties to the smallest j; d1 = d(i, j1);
 *      d2 = the smallest d over J_i \ {j1}, 512 when there is none.
 *   Reverse: I_j = { i : G(i, j) } -- the same gate, no transposed F; rev(j) = the member of I_j with the smallest d, ties to the
 *      smallest i.
 *   Accept query i iff J_i is not empty and d1 < max_dist and d1 * ratio_den < d2 * ratio_num (64-bit products)
 *      and (cross_check == 0 or rev(j1) == i).
 *   Outputs as hak_match_knn2: match / distance / match_x / match_y of an accepted query, -1 / -1 / -1.f / -1.f of a rejected one
 *      (copied to h_pts1 when given); the accepted matches in ascending query order to d_out (capacity >= n1; may be NULL) with
 *      second = d2; *count their number; h_out (needs d_out) receives the list as well.
 * Known limit: the band runs across the whole image, so a look-alike that happens to lie on the line is NOT excluded -- the ratio
 * test inside the band is what guards against it.  The gate is one-dimensional where the homography's is two-dimensional.
 * Synchronous; ctx may be NULL (default stream, scratch allocated for the call).  F: 9 floats on the HOST, row-major.
 * max_dist <= 0 selects 96.  Refused with a non-zero status and a message before any device is touched: radius not finite or
 * not > 0, radius * radius not finite in float32, F NULL or with a non-finite entry, a negative count, a ratio term <= 0, a NULL
 * point array with a positive count.  Fewer than 2^20 points per side.  Device code: csrc/kernels_epipolar.hip. */
int hak_match_epipolar(hak_ctx* ctx, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2,
                       const float F[9] /* host */, float radius, int ratio_num, int ratio_den, int cross_check,
                       int max_dist, hak_point* h_pts1, hak_match_pair* d_out, int* count, hak_match_pair* h_out);
/* batched over the pairs of a detect batch, layouts and outputs as hak_match_knn2_batch; asynchronous on the context's stream.
 * F of pair k is read ON THE DEVICE from d_F[k], the record hak_find_fundamental_batch wrote: the chain detect batch ->
 * hak_match_knn2_batch -> hak_find_fundamental_batch -> hak_match_epipolar_batch needs no host synchronisation.  A pair whose
 * record has hypothesis < 0 or a non-finite entry of F has no model: count 0, every query rejected (an all-zero F has no gate
 * anyway).  A NULL d_F and a NULL context are refused. */
int hak_match_epipolar_batch(hak_ctx* ctx, hak_point* d_points, const int* d_num_pts, int npairs,
                             const hak_fundamental* d_F /* device, one per pair */, float radius,
                             int ratio_num, int ratio_den, int cross_check, int max_dist,
                             hak_match_pair* d_out, int* d_counts);

/* ---- projection-guided matching: re-match 3-D points under a known pose (build-side addition; the stage behind hak_solve_pnp /
 * hak_refine_pnp, as hak_match_guided is the stage behind hak_find_homography and hak_match_epipolar the one behind
 * hak_find_fundamental).  The 3-D to 2-D correspondences PnP sees come from hak_link_tracks, which joins two whole-image 2-NN lists:
 * a landmark whose keypoint has a look-alike elsewhere in the new image is lost to the ratio test, or arrives as a wrong
 * correspondence.  Once the pose of the new image is known the landmark projects to one pixel, and only the keypoints within a few
 * pixels of it are candidates -- the "search by projection" of SLAM / SfM trackers.  A pure function of (list A, mask, xyz,
 * descriptor set D, train set T, view, K, radius, ratio, cross_check, max_dist) -- in particular it does not depend on how the
 * implementation bins the points; tests/projected_match_ref.py is its bit-exact numpy statement.
 *   Inputs: list A, nA hak_match_pair records of which only `train` is read; an optional mask of nA bytes; xyz, 3 nA floats in the
 *      layout hak_recover_pose(_batch) and hak_triangulate(_batch) write; descriptor set D, n_desc hak_point records of the image
 *      that A's `train` indexes, of which only `features` is read; train set T, n2 hak_point records of the new image, of which x,
 *      y and features are read; a view Xc = R X + t in float32; the intrinsics K.
 *   1. Landmark m is eligible iff (mask is NULL or mask[m] != 0) and 0 <= A[m].train < n_desc; e(m) = A[m].train.
 *   2. Projection, float32, no FMA, every operation correctly rounded, (X, Y, Z) = xyz[3m .. 3m+2]: xc, yc, zc are exactly the
 *      expressions of step 6 of hak_solve_pnp; px = (fx * (xc / zc)) + cx, py = (fy * (yc / zc)) + cy.
 *   3. Gate G(m, j): m is eligible, zc > 0 and, with dx = x2_j - px, dy = y2_j - py, (dx dx) + (dy dy) < r2, r2 = radius * radius
 *      in float32.  Any NaN makes it false: a non-finite point, projection or train coordinate is in no gate.
 *   4. Distance d(m, j): the Hamming distance of hak_match_knn2 between D[e(m)].features and T[j].features.
 *   5. Forward, reverse and accept are those of hak_match_guided with the landmark index m in the query's place:
 *      J_m = { j : G(m, j) }; j1 = the member of J_m with the smallest d, ties to the smallest j; d1 = d(m, j1); d2 = the smallest
 *      d over J_m \ {j1}, 512 when there is none; rev(j) = the landmark with the smallest d among those that gate j, ties to the
 *      smallest m; accept m iff J_m is not empty and d1 < max_dist and d1 * ratio_den < d2 * ratio_num (64-bit products) and
 *      (cross_check == 0 or rev(j1) == m).  max_dist <= 0 selects 96.
 *   6. Output: the accepted landmarks in ascending m as hak_corr3d {X, Y, Z = the three words of xyz, copied; u = T[j1].x,
 *      v = T[j1].y; src3d = m; src2d = j1 -- here the keypoint index in the new image, not a match index; pad = 0}, then their
 *      number.  No point record is written: D and T are const.
 *   7. No model gives count 0: a view of kind HAK_VIEW_RELATIVE with candidate < 0, of kind HAK_VIEW_ABSOLUTE with hypothesis < 0,
 *      or with a non-finite entry of R or t.  The identity view is R = I, t = 0 and goes through every expression.
 * Limits: nA, n_desc and n2 below 2^20; no scale or octave prediction and no orientation check; the only bound in front of the
 * camera is zc > 0; one descriptor per landmark (that of the keypoint it was triangulated from), no fusion over a track.  Points
 * rejected by hak_triangulate have xyz = 0 and mask 0; with a NULL mask they project to t -- that is the caller's business.
 * Refused with a non-zero status and a message before any device is touched: a radius that is not finite or not > 0,
 * radius * radius not finite in float32, a ratio term <= 0, fx or fy not finite or 0, a non-finite cx or cy, NULL K, count or
 * d_counts, a negative count or a count of 2^20 or more, a NULL array with a positive count, h_out without d_out, a list A or an
 * output list that is not 16-byte aligned, a non-finite entry of a host view, a kind outside 0..2, a NULL view array for kind 1 or
 * 2, a view step < 0, a stride or count step < 1, npairs < 1 or above the context's pair capacity ((batch + 1) / 2), a NULL
 * context for the batch form.  Device code: csrc/kernels_projected.hip (bin and reverse steps: csrc/kernels_guided.hip). */
/* one list, synchronous; ctx may be NULL (default stream, scratch allocated for the call).  Rt: 12 host floats {R row-major, t},
 * NULL = identity.  d_out: room for nA records (may be NULL: count only); h_out (needs d_out) receives the list as well */
int hak_match_projected(hak_ctx* ctx, const hak_match_pair* d_A, int nA, const unsigned char* d_maskA, const float* d_xyzA,
                        const hak_point* d_desc, int n_desc, const hak_point* d_pts2, int n2, const float* Rt,
                        const hak_intrinsics* K, float radius, int ratio_num, int ratio_den, int cross_check, int max_dist,
                        hak_corr3d* d_out, int* count, hak_corr3d* h_out);
/* batched, asynchronous on the context's stream; every count is read on the device.  List k of A is at d_A + k*strideA, its count
 * d_countsA[k*count_stepA], clamped to [0, min(strideA, out_stride, max_pts)], its mask at d_masksA + k*strideA (unless NULL), its
 * points at d_xyzA + 3*k*strideA -- as hak_link_tracks_batch addresses A; descriptor set k at d_desc + k*desc_stride with the
 * count d_desc_counts[k*desc_count_step], clamped to [0, min(desc_stride, max_pts)]; train set k at d_pts2 + k*stride2 with the
 * count d_counts2[k*count_step2], clamped to [0, min(stride2, max_pts)]; the view of list k is record k*view_step of d_views, read
 * ON THE DEVICE by kind as hak_triangulate_batch reads it (a step of 0 gives every list the same view; HAK_VIEW_IDENTITY ignores
 * d_views); K is a host argument, the same for every list.  Correspondences of k to d_out + k*out_stride, their number to
 * d_counts[k], nothing past it: the layout hak_solve_pnp_batch / hak_refine_pnp_batch read.
 * After a detect batch of four images per chain (I0, I1, I1, I2) and .. -> hak_refine_pnp_batch (d_abs, one record per chain): A is
 * the list of pair 2j (d_matches, stride 2*max_pts, d_counts, count step 2, with d_masks and d_xyz of hak_recover_pose_batch), D is
 * image 4j+1 (d_points + max_pts, stride 4*max_pts, d_num_pts + 1, count step 4), T is image 4j+3 (d_points + 3*max_pts, stride
 * 4*max_pts, d_num_pts + 3, count step 4), the view is d_abs[j] of kind HAK_VIEW_ABSOLUTE with step 1.  So .. ->
 * hak_refine_pnp_batch -> hak_match_projected_batch -> hak_refine_pnp_batch runs the refit on the larger list with no host
 * synchronisation and no allocation in the launch sequence (scratch grows before anything is enqueued, as the gated matchers do
 * it).  In the six-image chain (I0, I1, I1, I2, I2, I3) the landmarks for I3 are the triangulated matches of (I1, I2): A is the
 * list of pair 3j+1 with the mask and points hak_triangulate_batch wrote, D is image 6j+3, T is image 6j+5, the view the refitted
 * pose of I3. */
int hak_match_projected_batch(hak_ctx* ctx, const hak_match_pair* d_A, long strideA, const int* d_countsA, int count_stepA,
                              const unsigned char* d_masksA, const float* d_xyzA,
                              const hak_point* d_desc, long desc_stride, const int* d_desc_counts, int desc_count_step,
                              const hak_point* d_pts2, long stride2, const int* d_counts2, int count_step2, int npairs,
                              const void* d_views, int kind, int view_step, const hak_intrinsics* K,
                              float radius, int ratio_num, int ratio_den, int cross_check, int max_dist,
                              hak_corr3d* d_out, long out_stride, int* d_counts);

/* ---- memory helpers: initAkazeData/freeAkazeData (akaze.cpp:26-52) and the
 * image upload of main.cpp:172-188 */
int hak_points_alloc(hak_point** d_points, int count);
int hak_points_free(hak_point* d_points);
int hak_image_alloc(float** d_image, int w, int h, int* pitch);   /* pitch = iAlignUp(w,128), cuda_utils.h:160 */
int hak_image_upload(float* d_image, int pitch, const float* h_image, int w, int h);
int hak_image_free(float* d_image);
/* uint8 -> float32 in [0,1] on the device, exactly main.cpp:149 (convertTo(CV_32FC1, 1.0/255.0)):
 * dst = (float)(src * (1.0 / 255.0)).  nimg images, strides in elements; runs on the context's stream
 * (ctx may be NULL = default stream).  Quarters the H2D traffic of the float upload at main.cpp:187-188. */
int hak_ingest_u8(hak_ctx* ctx, const unsigned char* d_src, long src_stride, int src_pitch,
                  float* d_dst, long dst_stride, int dst_pitch, int w, int h, int nimg);
/* pinned host memory + the batched counterpart of the D2H copies at akaze.cpp:134-139 / 60-62:
 * counts first (one sync), then the first h_num_pts[i] records of every image, asynchronously,
 * then a final sync.  h_points is [nimg][max_pts]. */
int hak_host_alloc(void** p, long bytes);
int hak_host_free(void* p);
int hak_download_batch(hak_ctx* ctx, const hak_point* d_points, const int* d_num_pts, int nimg,
                       hak_point* h_points, int* h_num_pts);
int hak_memcpy_d2h(void* dst, const void* src, long bytes);
int hak_memcpy_h2d(void* dst, const void* src, long bytes);

/* ---- host-side schedule (pure CPU, usable without a GPU).
 * fed.cpp:41-119 fed_tau_by_process_time; returns n, writes tau[0..n). */
int hak_fed_tau(float T, int M, float tau_max, int reordering, float* tau, int cap);
/* akazed.cu:2298-2333 createGaussKernel */
void hak_gauss_taps(float var, int radius, float* taps);
/* akazed.cu:65-159 setCompareIndices (486 pairs, arrays of >= 488 ints) */
void hak_compare_indices(int* idx1, int* idx2);
/* The MLDB kernel's per-lane sample plan for one descriptor_pattern_size (akazed.cu:1905-1955 restated per (lane, turn): sample
 * i = lane + 64 * turn of the (winsize x winsize) window, its offset from the window centre and its accumulator row in the 2x2 /
 * 3x3 / 4x4 grid).  pos / cell: 7 * 64 words each, [turn * 64 + lane], or NULL.  pos: bits 0..7 x - size2 (signed), 8..15
 * y - size2 (signed), bit 16 the sample exists.  cell: byte g = row of grid g (0x7F none) | 0x80 when the lane's previous sample
 * went to the same row; bit 24 + g: the lane's last sample in that row.  Returns 1 when the planned kernel serves this size (at
 * most 7 samples per lane and no lane returning to a row it has left), 0 when the generic kernel does. */
int hak_describe_plan_query(int pattern_size, unsigned int* pos, unsigned int* cell);
/* The planned MLDB kernel's gather order: which samples share a gather instruction.  Row `row` < NB lists the window's samples
 * sorted by image row, then column, under a rotation by the bin's centre angle row * 2 pi / NB; row NB is the window order.
 * slots: 7 * 64 words, [turn * 64 + lane], or NULL: bits 0..7 x - size2 (signed), 8..15 y - size2 (signed), bit 16 the slot holds a
 * sample, bits 17..25 the sample's window index i (a slot without a sample: an index of its own >= the sample count, so that a
 * row is a permutation of 0 .. 7 * 64 - 1).  Returns NB, or 0 for a size the generic kernel serves or a row outside 0 .. NB.
 * hak_describe_order_bin: the row (0 .. NB - 1) the kernel takes for a keypoint angle -- any float, NaN and infinities included.
 * The order groups memory accesses only; no result depends on it. */
int hak_describe_order_query(int pattern_size, int row, unsigned int* slots);
int hak_describe_order_bin(float angle);
/* schedule the context was built with: per (octave, sublevel) the number of FED
 * steps, sigma_size, size, border; returns effective number of octaves. */
int hak_query_schedule(const hak_ctx* ctx, int* nsteps, int* sigma_size, float* sizes, float* borders);
int hak_query_geometry(const hak_ctx* ctx, int* whp /* 3 ints per octave */);

/* ---- instrumentation (not on the hot path): byte accounting and per-class timing of the launch sequence.
 * The stage operators, plane introspection and bandwidth probes the tests use are a separate ABI:
 * include/hipakaze_test.h -> libhipakaze_test.so. */
/* algorithmic-byte accounting of the last detect call on this context */
typedef struct hak_traffic {
    double fed_px_steps;     /* sum over FED steps of pixels updated, per image */
    double fed_bytes;        /* 12 B x fed_px_steps, + 16 B/px (low-pass 8 + conductivity 8) for every
                                sublevel whose low-pass and conductivity run inside its first FED launch (k_fed_sf), + the decimation /
                                low-pass / conductivity bytes of every octave head that does the same */
    double all_stage_bytes;  /* all-stage compulsory bytes per image, keypoint part for npts_hint points */
    int fed_launches;        /* FED kernel launches per batch */
    /* compulsory HBM bytes per image of each kernel class AS BUILT (after fusion): what its launches must move even with
       perfect reuse inside a launch -- the numerator of the per-class roofline fractions in bench.py */
    double fed_fused_bytes;  /* FED launches as enqueued by the last detect call: read L (+ g), write L' (+ smooth, + g) */
    double hessian_bytes;    /* 12 B/px per level: read smooth, write the interleaved {Lx, Ly} plane (the determinant is not stored) */
    double prologue_bytes;   /* 16 B/px of octave 0: read image, write Lt(0,0) + gradient plane, re-read it for the histogram */
    double describe_bytes;   /* (872 + 5292) B sampled per keypoint (orientation + MLDB) x npts_hint */
    double nms_bytes;        /* 104 B record per keypoint x npts_hint */
} hak_traffic;
int hak_query_traffic(const hak_ctx* ctx, int npts_hint, hak_traffic* out);

/* ---- per-kernel-class timing with HIP events on the context's stream.
 * When enabled, every launch of the class is bracketed by an event pair; read
 * back accumulated milliseconds and launch count after hak_sync(). */
enum { HAK_PROF_FED = 0, HAK_PROF_LOWPASS, HAK_PROF_FLOW, HAK_PROF_HESSIAN, HAK_PROF_CONTRAST,
       HAK_PROF_DOWN, HAK_PROF_EXTREMA, HAK_PROF_NMS, HAK_PROF_DESCRIBE, HAK_PROF_MATCH, HAK_PROF_COUNT };
int hak_prof_enable(hak_ctx* ctx, int on);
int hak_prof_read(hak_ctx* ctx, int klass, double* total_ms, int* launches);
int hak_prof_reset(hak_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HIPAKAZE_H */

/*
 * hipakaze_test.h -- the TEST ABI of the HIP AKAZE path: libhipakaze_test.so.
 *
 * NOT part of the product: a maintainer who binds the reference's interface needs include/hipakaze.h (libhipakaze.so) or
 * include/akaze.h only.  This library links against libhipakaze.so and drives the SAME launchers and kernels the launch
 * sequence uses, one stage at a time, so that tests/ can compare every stage with the oracle and with hand-derived fixtures:
 *   hak_debug_*   planes / contrast factor / RANSAC scratch of the last call on a context, writing a plane
 *   hak_op_*      single-stage operators (one h*() wrapper of akazed.cu each), the detector tail and the descriptor stages on
 *                 hand-made inputs, the conductivity's reciprocal self-check, bandwidth probes of the box
 *   hak_op_fast_* the stage operators once more on the integer FAST path: int32 planes (any value: products wrap, conversions
 *                 saturate), uint8 images, integer contrast factors; the `int` overloads of the same launchers
 */
#ifndef HIPAKAZE_TEST_H
#define HIPAKAZE_TEST_H
#include "hipakaze.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- introspection of the last call on a context */
enum { HAK_PLANE_LT = 0, HAK_PLANE_DET = 1, HAK_PLANE_LX = 2, HAK_PLANE_LY = 3 };
/* copy plane (kind, octave, sublevel) of batch image `img`, densely packed w x h, to host */
int hak_debug_plane(hak_ctx* ctx, int img, int kind, int octave, int sublevel, float* h_dst);
int hak_debug_kcontrast(hak_ctx* ctx, int img, float* kcontrast);
/* the context's arena, for the write-contract test of the whole launch sequence (tests/test_gpu_plane_guard.py), which poisons the
 * pad columns of every plane and looks at them afterwards.  hak_debug_arena_layout reports the layout as the library holds it, so
 * that no test restates the pitch rule: 4 + noct * (6 + 2 ms) words
 *   {noct, ms, elements per image, batch}, then per octave {w, h, p, smooth, flow, tmp, Lt(o, 0 .. ms-1), dxy(o, 0 .. ms-1)}
 * with every plane as its offset in elements from the image's first; Lt, smooth, flow and tmp are h rows of p elements, dxy is the
 * interleaved {Lx, Ly} plane, h rows of 2 p.  Returns the number of words, also when out is NULL or n is too small (ask first);
 * -1 for a NULL context.  hak_debug_arena_read / _write copy the whole arena of batch image `img` (elements-per-image 32-bit words,
 * float or int32 as the last call left them) after synchronising the context. */
int hak_debug_arena_layout(hak_ctx* ctx, long* out, int n);
int hak_debug_arena_read(hak_ctx* ctx, int img, float* h_dst);
int hak_debug_arena_write(hak_ctx* ctx, int img, const float* h_src);

/* ---- single-stage operators on caller-provided device planes (pitch p
 * elements, dense row-major), used by the per-kernel parity tests.  Each is
 * the HIP counterpart of one h*() wrapper of akazed.cu. Synchronous. */
int hak_op_lowpass(const float* d_src, float* d_dst, int w, int h, int p, float var, int radius);         /* hLowPass 2336 */
int hak_op_down_smooth(const float* d_src, float* d_dst, float* d_smooth, int sw, int sh, int sp,
                       int dw, int dh, int dp);                                                          /* hDownWithSmooth 2389 */
int hak_op_kcontrast(const float* d_smooth, int w, int h, int p, float per, float* kcontrast,
                     float* hmax, int* hist300);                                                         /* hScharrContrast 2410 */
int hak_op_flow(const float* d_src, float* d_dst, int w, int h, int p, int diffusivity, float kcontrast); /* hFlow 2487 */
int hak_op_nld_steps(const float* d_src, const float* d_flow, float* d_dst, float* d_tmp,
                     int w, int h, int p, const float* tau, int nsteps);                                  /* hNldStep 2509, n steps */
/* hak_op_nld_steps on a batch: image i's planes lie `stride` elements behind image i-1's */
int hak_op_nld_steps_batch(const float* d_src, const float* d_flow, float* d_dst, float* d_tmp, long stride,
                           int w, int h, int p, int nimg, const float* tau, int nsteps);
/* one whole FED cycle as the launch sequence runs it on large batches: hLowPass(var 1) + hFlow(PM_G2) + the first group of steps
 * in one launch (head != 0: hDownWithSmooth of the sw x sh source plane first, akaze.cpp:369-392), then the remaining groups.
 * d_smooth and d_dst receive the low-pass and L after nsteps steps; kcontrast: one factor per image (host).  Fails when the
 * fused kernel does not cover the case. */
int hak_op_fed_cycle(const float* d_src, int head, int sw, int sh, int sp, float* d_smooth, float* d_flow, float* d_dst, float* d_tmp,
                     long stride, int w, int h, int p, int nimg, const float* kcontrast, const float* tau, int nsteps);
/* self-check of the conductivity's fast reciprocal (csrc/fed_common.h hak_rcp_newton): counts the floats with bit patterns
 * in [lo_bits, hi_bits) whose 3-instruction reciprocal differs from the IEEE quotient 1.0f / d.  Must be 0 on [1, 2^64). */
int hak_op_rcp_check(unsigned lo_bits, unsigned hi_bits, unsigned long long* mismatches);
int hak_op_smooth_flow(const float* d_src, float* d_smooth, float* d_flow, int w, int h, int p,
                       int diffusivity, float kcontrast);                                               /* hLowPass(var 1) + hFlow, akaze.cpp:403-404 */
int hak_op_hessian(const float* d_src, float* d_lx, float* d_ly, float* d_det, int w, int h, int p, int step); /* hHessianDeterminant 2531 */
/* the Hessian of one level on the CALLER's planes, as the kernels write them: d_dxy the interleaved {Lx, Ly} plane (h rows of 2 p
 * elements, element (y, x) = {Lx, Ly} at 2 (y p + x)), d_det the determinant; the three planes of image i lie `stride` elements
 * behind image i-1's and all of them in ONE allocation (the streaming kernel addresses d_det as a 32-bit offset from d_dxy).  Every
 * dilation >= 1; *route (may be NULL): 1 streaming, 2 tile kernel, 3 the unfused pair above dilation 4.  hak_op_hessian and the batch
 * forms below run this on an allocation of their own and copy the w columns of every row out (the caller's pad columns are left
 * alone), so that nothing beside the kernels' planes can be seen; here the
 * write-contract test sees every word around them (tests/test_gpu_plane_guard.py). */
int hak_op_hessian_planes(const float* d_src, float* d_dxy, float* d_det, long stride, int w, int h, int p, int nimg, int step, int* route);

/* ---- the same stage operators on the integer FAST path (namespace fastakaze, akazed.cu:2781-4367): int32 planes in 16.16 fixed
 * point, uint8 images for the two operators that read one.  Each drives the `int` overload of the launcher its float twin drives
 * (csrc/hak_internal.h), reads the knobs per call and synchronises before it returns.  Any int32 value is a valid plane element:
 * products wrap, float -> int conversions saturate with NaN -> 0 (tests/fast_domain.py).  Contrast factors are the reference's
 * integers, 0 .. 46340 (above that kcontrast * kcontrast is a signed overflow in the reference itself: rejected).
 * The launchers do not report which kernel they took: route 3 is observed (the launcher's return value), routes 1 and 2 are INFERRED
 * from a restatement of the streaming launchers' cover rules in hak_test_api.hip (launch_base_stream, hak_hessian_stream_covers +
 * hak_stream_pays) -- keep the two in step when a launcher's guard changes.
 *   route (hak_op_fast_base):    1 streaming prologue (k_base_stream), 2 tile prologue (kf_base), 3 unfused (the three launches
 *                                of the launch sequence where hak_launch_base_level does not cover the radius)
 *   route (hak_op_fast_hessian): 1 streaming (k_hessian_stream), 2 tile (k_hessian_fused), 3 dilation > 4 (k_derivate + k_hessian) */
int hak_op_fast_conv_u8(const unsigned char* d_u8, int sp, int* d_dst, int w, int h, int p, float var, int radius);   /* gConv2d<R> 2990, gConv2dR2 2786 */
int hak_op_fast_lowpass(const int* d_src, int* d_dst, int w, int h, int p, float var, int radius);                    /* gConv2dR2 (int) 2922 */
/* the octave-0 prologue (akaze.cpp:589-623): Lt(0,0) = the base Gaussian (var_base, radius) of the image, and the contrast factor,
 * lattice maximum and histogram of its sigma = 1 low-pass, through the fused prologue the context would pick under the knobs */
int hak_op_fast_base(const unsigned char* d_u8, int sp, int* d_lt, int w, int h, int p, float var_base, int radius, float per,
                     int* kcontrast, int* hmax, int* hist300, int* route);
/* hak_op_fast_base on the CALLER's planes, all three in one allocation: routes 1 and 2 write d_lt and d_grad (the gradient magnitude of
 * the sigma = 1 image, read back by the histogram pass), route 3 writes d_lt and d_smooth (the sigma = 1 image); the third is not touched */
int hak_op_fast_base_planes(const unsigned char* d_u8, int sp, int* d_lt, int* d_grad, int* d_smooth, int w, int h, int p, float var_base,
                            int radius, float per, int* kcontrast, int* hmax, int* hist300, int* route);
int hak_op_fast_down_smooth(const int* d_src, int* d_dst, int* d_smooth, int sw, int sh, int sp, int dw, int dh, int dp);
int hak_op_fast_kcontrast(const int* d_smooth, int w, int h, int p, float per, int* kcontrast, int* hmax, int* hist300);
int hak_op_fast_flow(const int* d_src, int* d_dst, int w, int h, int p, int diffusivity, int kcontrast);
int hak_op_fast_smooth_flow(const int* d_src, int* d_smooth, int* d_flow, int w, int h, int p, int diffusivity, int kcontrast);
/* n steps in the groups of the FAST launch sequence (at most 4 steps per launch whatever HAK_FED_MAX_FUSE allows the float path) */
int hak_op_fast_nld_steps(const int* d_src, const int* d_flow, int* d_dst, int* d_tmp, int w, int h, int p, const float* tau, int nsteps);
int hak_op_fast_nld_steps_batch(const int* d_src, const int* d_flow, int* d_dst, int* d_tmp, long stride, int w, int h, int p,
                                int nimg, const float* tau, int nsteps);
/* hak_op_fed_cycle on int32 planes (PM_G2 only; fails when the fused kernel does not cover the case); kcontrast: one per image */
int hak_op_fast_fed_cycle(const int* d_src, int head, int sw, int sh, int sp, int* d_smooth, int* d_flow, int* d_dst, int* d_tmp,
                          long stride, int w, int h, int p, int nimg, const int* kcontrast, const float* tau, int nsteps);
/* one whole sublevel per launch out of LDS tiles (k_level_tile, without the level's Hessian): head != 0 decimates the sw x sh
 * source plane first.  d_smooth and d_dst receive the low-pass and L after nsteps steps (d_tmp: cycles of more than 36 steps) */
int hak_op_fast_level_tile(const int* d_src, int head, int sw, int sh, int sp, int* d_smooth, int* d_dst, int* d_tmp, long stride,
                           int w, int h, int p, int nimg, int diffusivity, const int* kcontrast, const float* tau, int nsteps,
                           int* launches);   /* *launches (may be NULL): what hak_launch_level_tile returns, the kernel launches of the cycle */
int hak_op_fast_hessian(const int* d_src, int* d_lx, int* d_ly, int* d_det, int w, int h, int p, int step, int* route);
/* hak_op_hessian / hak_op_fast_hessian on a batch of `nimg` dense planes (image i lies h * p elements behind image i-1, inputs and
 * outputs alike), through the fused kernel the knobs pick; *route as above (1 streaming, 2 tile).  Fails above dilation 4. */
int hak_op_hessian_batch(const float* d_src, float* d_lx, float* d_ly, float* d_det, int w, int h, int p, int nimg, int step, int* route);
int hak_op_fast_hessian_batch(const int* d_src, int* d_lx, int* d_ly, int* d_det, int w, int h, int p, int nimg, int step, int* route);
/* hak_op_hessian_planes on int32 planes */
int hak_op_fast_hessian_planes(const int* d_src, int* d_dxy, int* d_det, long stride, int w, int h, int p, int nimg, int step, int* route);

/* ---- detector-tail and descriptor stages on hand-made inputs (tests/test_gpu_literal.py: micro-fixtures whose expected
 * output is derived by hand from the cited reference statements).  They drive the SAME launchers as the launch sequence, on
 * image 0 of the context, and synchronise before returning.  A sequence is begin -> {level | det_level | seed}* -> finish.
 *   hak_debug_set_plane   write plane (HAK_PLANE_LT / LX / LY) of (octave, sublevel) from a dense w x h host array
 *   hak_op_tail_begin     reset the per-image state (candidate list, counters); the key map is already clear
 *   hak_op_tail_level     hHessianDeterminant 2531 + gCalcExtremaMap 1334 of one level from a dense host L-plane, through the
 *                         fused kernel the context would pick (knobs as in hak_create), threshold = cfg.dthreshold
 *   hak_op_tail_det_level gCalcExtremaMap 1334 alone (the stand-alone kernel of the dilation > 4 fallback) on a dense host
 *                         determinant plane
 *   hak_op_fast_tail_level / hak_op_fast_tail_det_level  the `int` twins of the two above (fastakaze::gCalcExtremaMap 3476) on dense
 *                         int32 planes, through the `int` overloads of the same launchers; `threshold` is the integer response
 *                         threshold (the FAST launch sequence uses 65); >= 0, a negative one is refused (hak_create, hipakaze.h, has the reason)
 *   hak_debug_tail_maps   between begin and finish: image 0's key map as dense w x h response words and layers (empty pixel: word 0,
 *                         layer -1), the first min(ncand, capacity) words of its candidate list in arrival order
 *                         (layer << 32 | y << 16 | x, full resolution), the list's capacity and the candidate count.  Any output
 *                         pointer may be NULL; h_cand holds `capacity` words (ask with h_cand == NULL first).
 *                         The extrema stage by itself: after the NMS a missed or extra candidate is mostly masked
 *   hak_op_tail_seed      hand-made full-resolution maps: response words (float or int bits) and layer ids (< 0: empty)
 *   hak_op_tail_finish    gNmsRNaive 1554 (+ gRefine 1615 when `refine`) -> d_points in raster order; *num_pts = survivors
 *   hak_debug_tail_total  after finish: the survivors of the NMS before the clamp to max_pts (*num_pts above is the clamped count)
 *   hak_op_orient_describe gCalcOrient 1665 + gDescribe2 1869 on the first n records of d_points, reading the planes the
 *                         arena holds now (desc: 0 none, 1 both, 2 descriptor only with the records' own angles)
 *   hak_op_fast_orient_describe  the same on the integer FAST path: gRefine 3600 + gCalcOrient 3649 + gDescribe2 3723 through
 *                         hakf_launch_describe, on int32 planes (written with hak_debug_set_plane, which copies bits: pass the int32
 *                         array as it lies in memory).  desc: 0 refinement only, otherwise refinement + orientation (unless the
 *                         context is upright) + MLDB; there is no descriptor-only mode, the FAST sequence has none */
int hak_debug_set_plane(hak_ctx* ctx, int img, int kind, int octave, int sublevel, const float* h_src);
int hak_op_tail_begin(hak_ctx* ctx);
int hak_op_tail_level(hak_ctx* ctx, int octave, int sublevel, const float* h_src);
int hak_op_tail_det_level(hak_ctx* ctx, int octave, int sublevel, const float* h_det);
int hak_op_fast_tail_level(hak_ctx* ctx, int octave, int sublevel, const int* h_src, int threshold);
int hak_op_fast_tail_det_level(hak_ctx* ctx, int octave, int sublevel, const int* h_det, int threshold);
int hak_debug_tail_maps(hak_ctx* ctx, unsigned int* h_response_bits, int* h_layer, unsigned long long* h_cand, long* cand_cap_out,
                        int* ncand_out);
int hak_op_tail_seed(hak_ctx* ctx, const unsigned int* h_response_bits, const int* h_layer);
int hak_op_tail_finish(hak_ctx* ctx, hak_point* d_points, int max_pts, int refine, int fast, int* num_pts);
int hak_debug_tail_total(hak_ctx* ctx, int* total);
int hak_op_orient_describe(hak_ctx* ctx, hak_point* d_points, int n, int desc);
int hak_op_fast_orient_describe(hak_ctx* ctx, hak_point* d_points, int n, int desc);

/* ---- bandwidth ceilings of the box (SURVEY 8d "copy-kernel ceiling"; not on the hot path).
 * hak_op_copy_probe: float4 copy of `bytes` with the streaming kernels' access shape (16 B/lane), `iters` times per launch
 * shape (24 shapes: loads in flight, nt / plain stores, grid size); *gbytes_per_s = (read + write bytes) / average kernel
 * time of the best shape.
 * hak_op_gather_probe: `blocks` x 256 lanes each gather `per_lane` dwords from pseudo-random 128-byte lines of a
 * `bytes`-sized buffer (the descriptor's access shape), `iters` times; *ms_per_launch = average kernel time.  Used to
 * calibrate the FETCH_SIZE counter for 4-byte gathers. */
int hak_op_copy_probe(long bytes, int iters, double* gbytes_per_s);
/* every launch shape of the probe: entry (g * 6 + s * 3 + l) = grid g {8, 16, 32 blocks per CU, one pass} x stores s {nt, plain} x
 * loads in flight per lane l {2, 4, 8}; then the read-only and the write-only stream.  Returns the number of entries (26). */
int hak_op_copy_probe_shapes(long bytes, int iters, double* gbytes_per_s, int n);
int hak_op_gather_probe(long bytes, int blocks, int per_lane, int iters, double* ms_per_launch);
/* hak_op_stream_probe: the FED family's access shape with the arithmetic taken out -- `nimg` planes of w x h read once (16 B per lane
 * and row, 256-lane strips with 8-column halos, row segments as the streaming kernels cut them, `warm_rows` warm-up rows per
 * segment) and `nwrite` (1..3) planes written with nt buffer stores; *gbytes_per_s = compulsory bytes (1 + nwrite) x 4 x w x h x nimg /
 * average kernel time: the data-movement floor of k_fed_sf / k_fed_multi at that launch geometry. */
int hak_op_stream_probe(int w, int h, int nimg, int nwrite, int warm_rows, int iters, double* ms_per_launch, double* gbytes_per_s);

/* hak_op_hess_probe: the streaming Hessian's access shape with the arithmetic taken out (k_hessian_stream, dilation `step` 1..4): its strips,
 * row segments and warm-up rows, 4 B/px read, the interleaved {Lx, Ly} plane written through the same per-wave LDS turn and the same
 * two dense 16-byte nt buffer stores per lane and row, at the kernel's LDS footprint and occupancy target; *gbytes_per_s = 12 B/px
 * compulsory / average kernel time: the data-movement floor of the Hessian class at that launch geometry. */
int hak_op_hess_probe(int w, int h, int nimg, int step, int iters, double* ms_per_launch, double* gbytes_per_s);
/* hak_debug_fill_match_scratch: fills the context's per-slice match summaries (kernels_match.hip: `part`) with `byte`, on the context's
 * stream -- the hand-off stress run makes a stale summary visible with it (tests/stress_handoff.py) */
int hak_debug_fill_match_scratch(hak_ctx* ctx, int byte);
/* hak_op_ransac_shape: the launch shape the homography and the fundamental-matrix RANSAC calls (single and batch) take for `npairs`
 * lists and `iterations` hypotheses -- *hp hypotheses per score block (16 .. 256) and *hblocks score blocks per pair.  It asks the
 * launchers' own rule and touches no device: the shape tests (tests/ransac_shapes.py) read the rule here and do not restate it. */
int hak_op_ransac_shape(int npairs, int iterations, int* hp, int* hblocks);
/* hak_op_match_shape: the launch plan the matcher takes for a call, from the launchers' own rule (one host function, which reads
 * the HAK_MATCH_* variables as every call does) and without touching a device.  The limit tests (tests/match_limits.py) assert with
 * it that a case reached the path it was made for and choose where to plant rows; they never form an expected match from it.
 *   search          0: the 1-NN search of hak_match / hak_match_batch; 1: one 2-NN search of hak_match_knn2 / hak_match_knn2_batch
 *                   (n1 queries against n2 train rows; the reverse search is the same call with the counts exchanged)
 *   device_counts   != 0: a batch call (counts on the device); the launchers then see `capacity` (the context's max_pts) in the place
 *                   of both counts, and n1 / n2 are ignored
 *   scratch         != 0: a match scratch is at hand (a context's, or the per-device pool's for ctx == NULL: always, for the public
 *                   entry points)
 *   plan            7 int32: {kernel (0 = matrix-core k_match_mfma, 1 = vector-pipe k_match / k_knn2), query tiles per wave (k_match:
 *                   queries per thread), gx = query blocks, train slices (1 = not sliced), rows per slice (0 = not sliced or cut inside
 *                   the kernel), LDS chunks per block pass (192 rows, a tail counts; k_match: tiles of 128; k_knn2: 0), blocks of the
 *                   2-NN finish for n1 queries (1 = one block per pair, else two passes of that many)} */
int hak_op_match_shape(int search, int n1, int n2, int npairs, int device_counts, int capacity, int scratch, int* plan);
/* hak_debug_ransac_scratch: what the last hak_find_homography / hak_find_fundamental / hak_find_essential / hak_solve_pnp call (single or batch) on `ctx`
 * left in the context's RANSAC scratch, so that the tests (tests/ransac_trace.py) see every hypothesis and every score block and not
 * only the winner.  Synchronises the context's stream and launches nothing.
 *   h_models  npairs * words_per_hypothesis * iterations 32-bit words, as they lie: [pair][word][iterations], word NW r + q = word q of
 *             model r, the last word the mask of the models that exist (bit r = model r).  28 words per hypothesis for the fundamental
 *             matrix (3 models of 9), 49 for P3P (4 models of 12); 0 for the homography, which keeps no models: nothing is copied and
 *             h_models may be NULL.  hak_find_essential keeps hypothesis h as the three virtual hypotheses 3 h + g of four models each
 *             (root r = model r mod 4 of virtual hypothesis 3 h + r / 4): 37 words per hypothesis, and `iterations` (here, in h_slots
 *             and in hak_op_ransac_shape) is 3 x the call's, which both take up to 65536: calls of up to 21845 hypotheses.
 *   h_slots   npairs * hblocks triples of int32 {inliers, hypothesis, model}: the best of each score block, [pair][block], decoded
 *             from the block's key on the host; a block without a model gives {0, -1, 0}.
 * npairs, iterations and hblocks (hak_op_ransac_shape) are those of that call.  Refused with a message: a NULL context, a NULL
 * h_slots, a NULL h_models with words to copy, sizes out of range or beyond what the context's scratch holds. */
int hak_debug_ransac_scratch(hak_ctx* ctx, int npairs, int words_per_hypothesis, int iterations, int hblocks, unsigned* h_models,
                             int* h_slots);

#ifdef __cplusplus
}
#endif
#endif /* HIPAKAZE_TEST_H */

// hak_internal.h -- shared declarations of libhipakaze (gfx950 only).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hipakaze.h"
#include "hak_knobs.h"

#define HAK_NBINS 300        // akazed.cu:8
#define HAK_WAVE 64
#define HAK_DSC_NB 32        // angle bins of the MLDB gather-order table (a power of two; HakTables::dsc_ord)

// ---------------------------------------------------------------- geometry
struct HakOct {
    int w, h, p;             // width, height, pitch (elements) of one octave plane
    long plane;              // h * p
};

// Per-image arena (floats). Planes persist until the descriptors are done.
//   per (octave o, sublevel s): Lt (1 plane) and Dxy (2 planes' worth: the first derivatives INTERLEAVED, element
//                               (y, x) = {Lx, Ly} at dxy + 2 * (y * p + x))                      persistent
//   per octave: smooth, flow, tmp                                                                  scratch
// The determinant is never stored: its only consumers are the extrema test (fused into the Hessian kernels) and the
// sub-pixel refinement of the ~2 k keypoints, which re-evaluates the nine values it needs from Dxy (hak_det_at).
struct HakLayout {
    int noct, ms;
    HakOct oct[HAK_MAX_OCTAVES];
    long lvl_off[HAK_MAX_OCTAVES];              // start of the 3*ms persistent planes of octave o
    long smooth_off[HAK_MAX_OCTAVES], flow_off[HAK_MAX_OCTAVES], tmp_off[HAK_MAX_OCTAVES];
    long arena;                                 // floats per image

    __host__ __device__ long lt(int o, int s) const { return lvl_off[o] + (long)s * oct[o].plane; }
    __host__ __device__ long dxy(int o, int s) const { return lvl_off[o] + (long)(ms + 2 * s) * oct[o].plane; }
};

// Per-image device scalars.
struct HakImgState {
    unsigned int hmax_bits;                     // max Scharr gradient magnitude over the 16-px lattice (float bits), floored at 0.03f
    int hist[HAK_NBINS];
    float kcontrast[HAK_MAX_OCTAVES];           // per octave: k0, k0*0.75, ...
    float ikc[HAK_MAX_OCTAVES];                 // 1/(k*k)
    int ihmax;                                  // FAST path: max integer gradient magnitude over the 16-px lattice (floored at 1)
    int ikcontrast[HAK_MAX_OCTAVES];            // FAST path: integer contrast factor per octave
    int ncand;                                  // entries in the image's extrema candidate list
    int total_pts;                              // NMS survivors before clamping to max_pts
    int num_pts;                                // min(total, max_pts)
};

// Read-only tables shared by all images of a context.
struct HakTables {
    float sizes[HAK_MAX_OCTAVES * HAK_MAX_SCALES];     // d_extrema_param sizes, per layer
    float borders[HAK_MAX_OCTAVES * HAK_MAX_SCALES];
    int sigma_size[HAK_MAX_OCTAVES * HAK_MAX_SCALES];
    float orient_w[36];                                // exp(-r2*0.08f)
    int orient_ij[128];                                // k_orient's 109 disc samples in the reference's thread order: i | j << 8 (bytes)
    float orient_gw[128];                              // ... and their weight orient_w[i*i + j*j]; slots 109.. unused (0)
    float fac1, fac2;                                  // dilated-Scharr factors (akazed.cu:2537-2539); FAST: ifac = (int)(fac * 65536 + 0.5f)
    int ifac1, ifac2;
    int comp1[488], comp2[488];                        // MLDB pair table (akazed.cu:65-159)
    unsigned char comp_packed[64 * 16];                // per descriptor byte: 8 x (idx1, idx2) as bytes
    // MLDB sample plan of the configured descriptor_pattern_size (hak_describe_plan, kernels_describe.hip): which sample a
    // lane SUMS in its n-th turn (sample n * 64 + lane of the window) and where it goes depends on (lane, n) only, never on the
    // keypoint.  [n * 64 + lane]:
    //   dsc_cell: byte g (2x2, 3x3, 4x4 grid) = accumulator row (0x7F none) | 0x80 when the lane's previous sample went to the
    //             same row; bit 24 + g: last sample of this lane in that row
    unsigned int dsc_cell[7 * 64];
    int dsc_plan_ok;                                   // 0: pattern too large or a lane revisits a row -> generic k_describe
    // Gather order of k_describe_runs: WHICH samples share a gather instruction.  Row b < HAK_DSC_NB lists the window's samples
    // sorted by their image row, then column, under a rotation by the centre angle of bin b (v = k sin a + l cos a, then
    // u = k cos a - l sin a; a = b * 2 pi / HAK_DSC_NB, hak_dsc_bin), so the 64 lanes of turn n gather neighbours along image rows,
    // which share 128-byte lines; row HAK_DSC_NB is the window order (slot = sample).  [row][n * 64 + lane]: bits 0..7
    // l = x - size2 (signed), 8..15 k = y - size2 (signed), bit 16 sample exists, bits 17..25 the window index i, where
    // the kernel stages the values for the lane (i % 64, turn i / 64) that sums them.  A slot without a sample (the window's
    // 7 * 64 - nsmp pads) has l = k = 0 and an index of its own >= nsmp: every row is a permutation of 0 .. 7 * 64 - 1.
    unsigned int dsc_ord[(HAK_DSC_NB + 1) * 7 * 64];
};
void hak_describe_plan(HakTables* t, int patsize);

// the order-table row of a keypoint angle: nearest bin centre, every float (NaN, +-inf, negative, huge) in 0 .. HAK_DSC_NB - 1.
// The row only groups the gathers; results do not depend on it.
__host__ __device__ inline int hak_dsc_bin(float angle)
{
    float t = angle * (float)(HAK_DSC_NB / (2.0 * 3.14159265358979323846));
    t = fminf(fmaxf(t, -1.0e6f), 1.0e6f);              // (fmaxf drops a NaN; the cast below is then defined for every input)
    return (int)floorf(t + 0.5f) & (HAK_DSC_NB - 1);
}

// ---------------------------------------------------------------- device helpers
// hScharrContrast as the reference's kernels actually compute it (akazed.cu:827-877, 901-938 / 3245-3336; derivation:
// DESIGN.md 2, D2 / D3):
//   the maximum -- gFindMaxContrastU4's "reduction" compares with absolute pixels of the image's top-left tile, not with the
//   block's other threads, and only thread 0 of each 32 x 32 block feeds atomicMax: what arrives deterministically is the maximum
//   over the pixels x % 16 == 0 && y % 16 == 0 that grid1 = ceil((n / 2) / 16) blocks of 32 cover (an odd n with
//   (n - 1) % 32 == 0 leaves its last column / row out);
//   the histogram -- the guard `ix >= width && iy >= height` returns only when BOTH are outside, so the 32 x 16 blocks' threads
//   right of and below the image count as well, zeros of the reused arena (akaze.cpp:142-149): hak_hist_extra0 entries in bin 0.
__host__ __device__ inline int hak_lattice_cov(int n) { const int c = 32 * ((n / 2 + 15) / 16); return c < n ? c : n; }
__host__ __device__ inline bool hak_on_lattice(int x, int y, int w, int h)
{
    return ((x | y) & 15) == 0 && x < hak_lattice_cov(w) && y < hak_lattice_cov(h);
}
__host__ __device__ inline int hak_hist_extra0(int w, int h) { return ((w + 31) / 32 * 32 - w) * h + ((h + 15) / 16 * 16 - h) * w; }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() lowers to
// `s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier`, i.e. it also drains every outstanding global load and
// store of the wave -- which serialises a register prefetch and exposes the store latency at each
// phase boundary of the persistent tile kernels.  Use this between phases that only exchange data
// through LDS; global results are complete at kernel end as usual.
// XCD-aware block order.  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs (each has its own
// L2).  A 1-D grid of hak_xcd_grid() = nbx * nby * nimg blocks is decoded so that, within every full group of 8
// images, all blocks of one image carry ids congruent mod 8: an image's tiles (which share halos) then run on one
// XCD.  The nimg % 8 images left over are laid out plainly (no padding blocks: a single-image call launches exactly
// its own tiles).  Always returns true (kept as a predicate so callers read `if (!decode) return`).
__device__ __forceinline__ bool hak_xcd_decode(int nbx, int nby, int nimg, int& bx, int& by, int& img)
{
    const int nb = nbx * nby;
    const int full = nimg & ~7;                             // images covered by complete groups of 8
    const int bid = blockIdx.x;
    int t;
    if (bid < full * nb) {
        const int xcd = bid & 7, j = bid >> 3;
        const int g = j / nb;
        t = j - g * nb;
        img = g * 8 + xcd;
    } else {
        const int r = bid - full * nb;
        const int k = r / nb;
        t = r - k * nb;
        img = full + k;
    }
    by = t / nbx;
    bx = t - by * nbx;
    return img < nimg;
}
static inline unsigned hak_xcd_grid(int nbx, int nby, int nimg) { return (unsigned)nimg * (unsigned)nbx * (unsigned)nby; }

__device__ __forceinline__ void hak_lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- key helpers of the Hessian kernels (the dilated Scharr and the determinant: pixel_rules.h)
__device__ __forceinline__ unsigned hs_key_bits(float v) { return __float_as_uint(v); }     // positive floats order like their bits
__device__ __forceinline__ unsigned hs_key_bits(int v) { return (unsigned)v; }              // positive ints
__device__ __forceinline__ unsigned hs_key_bits(unsigned v) { return v; }                   // a response word as it is (k_seed_maps)

// ---- the per-level extrema rule (gCalcExtremaMap akazed.cu:1334-1393, FAST 3476-3515), stated once for the five kernels that
// apply it: k_hessian_stream, k_hessian_fused, k_level_tile and the two k_extrema<V>.  The border filter, the strict maximum,
// the tie order of the key and the coordinate packing of the candidate word are defined here and nowhere else.
// What a kernel needs to apply the rule to one level; filled on the host by hak_extrema_args (below HakBatch).
template <typename V>
struct HakExtremaArgs {
    unsigned long long* maps;       // [nimg][map_stride]; nullptr: determinant only, no extrema
    long map_stride;
    unsigned long long* cand;       // [nimg][cand_cap]
    long cand_cap;
    HakImgState* state;
    int p0;                         // pitch of the full-resolution map
    int octave, layer;
    int psz;                        // (int)borders[octave*ms]     akazed.cu:2572
    float border;
    V threshold;
};
// border filter of one axis (akazed.cu:1346-1353): coordinate i of an axis of n pixels
__device__ __forceinline__ bool hak_ext_inside(int i, int n, int psz, float border)
{
    return i >= psz && i < n && (int)(i - border + 0.5f) - 1 >= 0 && (int)(i + border + 0.5f) + 1 < n;
}
// strict 3 x 3 maximum (akazed.cu:1361): eight ORDERED compares.  A maximum over the neighbours must never stand in for them: it
// drops a NaN operand, while a NaN neighbour makes its compare -- and so the test -- false (NaN determinants, inf - inf, come
// from finite images: tests/test_gpu_value_domain.py).  A maximum may pre-select (k_hessian_stream); these compares decide.
template <typename V>
__device__ __forceinline__ bool hak_ext_strict_max(V v, V up, V dn, V lf, V rt, V ul, V ur, V dl, V dr)
{
    return v > up && v > dn && v > lf && v > rt && v > ul && v > ur && v > dl && v > dr;
}
template <typename V>
__device__ __forceinline__ bool hak_ext_strict_max(V v, const V* vp, int pitch)
{
    return hak_ext_strict_max(v, vp[-pitch], vp[pitch], vp[-1], vp[1], vp[-pitch - 1], vp[-pitch + 1], vp[pitch - 1], vp[pitch + 1]);
}
// key-map word: response bits << 32 | (0xFFFFFFFF - layer).  One atomicMax keeps the larger response and, on a tie, the lower
// layer (the reference's sequential `response_map[oidx] < *vp`, akazed.cu:1368).
template <typename V>
__device__ __forceinline__ unsigned long long hak_ext_key(V v, int layer)
{
    return ((unsigned long long)hs_key_bits(v) << 32) | (0xFFFFFFFFu - (unsigned)layer);
}
__device__ __forceinline__ unsigned hak_key_word(unsigned long long k) { return (unsigned)(k >> 32); }       // response bits
__device__ __forceinline__ float hak_key_resp(unsigned long long k) { return __uint_as_float(hak_key_word(k)); }
__device__ __forceinline__ int hak_key_layer(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)k); }
// candidate-list word: layer << 32 | y << 16 | x at full resolution -- 16 bits per coordinate (build_plan refuses larger images)
__device__ __forceinline__ unsigned long long hak_cand_word(int layer, int fx, int fy)
{
    return ((unsigned long long)layer << 32) | ((unsigned)fy << 16) | (unsigned)fx;
}
__device__ __forceinline__ int hak_cand_layer(unsigned long long e) { return (int)(e >> 32); }
__device__ __forceinline__ int hak_cand_x(unsigned long long e) { return (int)(e & 0xFFFFu); }
__device__ __forceinline__ int hak_cand_y(unsigned long long e) { return (int)((e >> 16) & 0xFFFFu); }
// one wave's hits of level pixels (x, y) -> the image's candidate list (one slot reservation per wave) and its key map.  Called
// by all 64 lanes.  (k_hessian_stream and k_hessian_fused stage their candidates in LDS first, for the reasons given there.)
template <typename V>
__device__ __forceinline__ void hak_ext_append_wave(bool hit, V v, int x, int y, int img, int lane, const HakExtremaArgs<V>& ex)
{
    const unsigned long long m = __ballot(hit);
    if (!m) return;
    int cbase = 0;
    if (lane == 0) cbase = atomicAdd(&ex.state[img].ncand, __popcll(m));
    cbase = __builtin_amdgcn_readfirstlane(cbase);
    if (hit) {
        const int fx = x << ex.octave, fy = y << ex.octave;
        atomicMax(&ex.maps[(long)img * ex.map_stride + (long)fy * ex.p0 + fx], hak_ext_key(v, ex.layer));
        const long slot = cbase + __popcll(m & ((1ull << lane) - 1ull));
        if (slot < ex.cand_cap) ex.cand[(long)img * ex.cand_cap + slot] = hak_cand_word(ex.layer, fx, fy);
    }
}

// ------------------------------------------------- deterministic float32 math
// Same operation sequence as the parity oracle's (oracle/okz_math.h): one IEEE
// binary32 op per step, explicit fmaf only.  The reference's libdevice /
// fast-math calls (akazed.cu:1697,1701,1887-1888) are not reproducible.
#define HAK_PI_F  3.14159274101257324f
#define HAK_HPI_F 1.57079637050628662f
#define HAK_PI_D  3.14159265358979323846

__host__ __device__ __forceinline__ void hak_sincosf(float a, float* s_out, float* c_out)
{
    float q = floorf(a * 0.636619747f + 0.5f);
    float r = fmaf(q, -1.57079601287841796875f, a);
    r = fmaf(q, -3.139164786504813217e-7f, r);
    r = fmaf(q, -5.390302529957764765e-15f, r);
    int n = ((int)q) & 3;
    float r2 = r * r;
    float sp = fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
    sp = fmaf(sp, r2, -1.6666654611e-1f);
    float sr = fmaf(r * r2, sp, r);
    float cp = fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
    cp = fmaf(cp, r2, 4.166664568298827e-2f);
    float cr = fmaf(r2 * r2, cp, fmaf(r2, -0.5f, 1.0f));
    float s, c;
    if (n == 0)      { s = sr;  c = cr;  }
    else if (n == 1) { s = cr;  c = -sr; }
    else if (n == 2) { s = -sr; c = -cr; }
    else             { s = -cr; c = sr;  }
    *s_out = s;
    *c_out = c;
}

__host__ __device__ __forceinline__ float hak_atan2f(float y, float x)
{
    float ax = fabsf(x), ay = fabsf(y);
    float mx = ax > ay ? ax : ay;
    float mn = ax > ay ? ay : ax;
    if (mx == 0.0f) return 0.0f;
    float a = mn / mx;
    float t, base;
    if (a > 0.4142135679721832275f) {
        t = (a - 1.0f) / (a + 1.0f);
        base = 0.785398185253143310546875f;
    } else {
        t = a;
        base = 0.0f;
    }
    float z = t * t;
    float p = fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
    p = fmaf(p, z, 1.99777106478e-1f);
    p = fmaf(p, z, -3.33329491539e-1f);
    float r = base + fmaf(p * z, t, t);
    if (ay > ax) r = HAK_HPI_F - r;
    if (x < 0.0f) r = HAK_PI_F - r;
    if (y < 0.0f) r = -r;
    return r;
}

__host__ __device__ __forceinline__ float hak_expf(float x)
{
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) x = 88.0f;
    float k = floorf(x * 1.44269502162933349609375f + 0.5f);
    float r = fmaf(k, -0.693359375f, x);
    r = fmaf(k, 2.12194440e-4f, r);
    float p = fmaf(1.9875691500e-4f, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    float e = fmaf(p, r * r, r) + 1.0f;
    return ldexpf(e, (int)k);
}

// the per-pixel rules of both pipelines (element arithmetic, reflect-101, Gaussian, Scharr, histogram, conductivity, determinant)
#include "pixel_rules.h"

// ---------------------------------------------------------------- launchers
// (defined in the kernel files; all asynchronous on `st`; nimg = batch images,
//  base = arena of image 0, stride = floats between image arenas)
// The HAK_* tuning variables (struct HakKnobs, per context; HakMatchKnobs, per call): hak_knobs.h

// Per-image state and scratch of the strongest-N selection (kernels_select.hip), allocated by hak_create for cfg.batch images.
// Every word a call reads is written earlier in the same call (k_sel_init, k_sel_rows): nothing is cleared outside the sequence.
struct HakSelState {
    int active;                                 // survivors > clamp: this image selects (else every select kernel leaves at once)
    int need;                                   // keys still to keep among those whose leading digits equal `prefix`
    unsigned prefix;                            // the digits of the C-th largest key picked so far; after the last pass: the key T
    int pad;
};
#define HAK_SEL_BINS 2048                       // radix digits of 11, 11 and 10 bits: three passes over the 32-bit key
#define HAK_SEL_PASSES 3
struct HakSelScratch {
    HakSelState* st = nullptr;                  // [nimg]
    unsigned* bins = nullptr;                   // [nimg][HAK_SEL_PASSES][HAK_SEL_BINS] global digit histograms
    int* tie = nullptr;                         // [nimg][h0] keys equal to T per row
};

// the order-preserving map of the 32-bit response word: float bits (negative values reversed below the positive ones) or int32
__device__ __forceinline__ unsigned sel_key(unsigned u, int fast)
{
    return fast ? (u ^ 0x80000000u) : ((u >> 31) ? ~u : (u | 0x80000000u));
}
// the clamp of image img, exactly as k_row_scan computes it
__device__ __forceinline__ int sel_cap(int img, int max_pts, int cap0, int cap1)
{
    return cap0 > 0 ? (img == 0 ? cap0 : cap1) : max_pts;
}

// Per-image state and scratch of the grid selection (kernels_grid_select.hip, hak_set_retain_grid), allocated at the first use of
// the mode for cfg.batch images and the smallest cell size (HAK_GRID_MIN).  Every word a call reads is written earlier in the same call.
#define HAK_GRID_MIN 8
#define HAK_GRID_MAX 128
struct HakGridState {
    int active;                                 // survivors > clamp: this image selects (else every grid kernel leaves at once)
    int cap;                                    // the image's clamp C
    int q;                                      // the quota: every cell keeps its min(n_c, q) highest-ranked survivors
    int rem;                                    // R = C - sum min(n_c, q): places for the rank-q candidates
};
struct HakGridScratch {
    HakGridState* st = nullptr;                 // [nimg]
    int* count = nullptr;                       // [nimg][cell_cap] n_c
    unsigned long long* comp = nullptr;         // [nimg][cell_cap] the rank-q candidate of a cell with n_c > q: K << 32 | ~raster index
    long cell_cap = 0;                          // cells per image at HAK_GRID_MIN
    int G = 0;                                  // the cell size of this call; 0: the mode is off
};

struct HakBatch {
    float* base;                  // arena of image 0
    long stride;                  // floats between consecutive image arenas
    int nimg;
    HakImgState* state;           // [nimg]
    unsigned long long* maps;     // [nimg][map_stride] packed response/layer keys, full resolution
    long map_stride;              // h0 * p0
    unsigned long long* bitmap;   // [nimg][h0][ceil(w0/64)] NMS survivor bits
    int* rowcount;                // [nimg][h0]
    unsigned long long* cand;     // [nimg][cand_cap] extrema candidates: layer<<32 | y<<16 | x (full-res)
    long cand_cap;
    const HakKnobs* knobs = nullptr;   // the owning context's; nullptr (stage operators): read per call, hak_knobs_of()
    int* perm = nullptr;          // [nimg][perm_cap] visiting order of the keypoint kernels (k_desc_perm), or nullptr: output order
    int perm_cap = 0;
    // per-image clamps of a PAIR call (hak_detect_and_compute_pair: the two AkazeData capacities, akaze.cpp:246, 451); 0: every
    // image is clamped at the launch's max_pts, which is always the record stride between images
    int cap0 = 0, cap1 = 0;
    // scratch of the strongest-N selection (kernels_select.hip, hak_set_retain_best); sel.st == nullptr: the raster-order clamp
    HakSelScratch sel{};
    // scratch of the grid selection (kernels_grid_select.hip, hak_set_retain_grid); grid.G > 0: it replaces both other policies
    HakGridScratch grid{};
};
// the knobs a launcher works with: the owning context's, or (no context: b == nullptr or a stage operator's batch) the environment's now
static inline HakKnobs hak_knobs_of(const HakBatch* b) { return (b && b->knobs) ? *b->knobs : hak_knobs_from_env(); }
// the extrema parameters of level (octave, sub) for every kernel that applies the rule; htab: the HOST copy of the tables.
// b == nullptr: maps == nullptr, i.e. determinant only
template <typename V>
static inline HakExtremaArgs<V> hak_extrema_args(const HakBatch* b, const HakLayout* L, const HakTables* htab, int octave, int sub, V threshold)
{
    HakExtremaArgs<V> ex{};
    if (b) {
        const int layer = octave * L->ms + sub;
        ex.maps = b->maps; ex.map_stride = b->map_stride; ex.cand = b->cand; ex.cand_cap = b->cand_cap;
        ex.state = b->state; ex.p0 = L->oct[0].p; ex.octave = octave; ex.layer = layer;
        ex.psz = (int)htab->borders[octave * L->ms]; ex.border = htab->borders[layer]; ex.threshold = threshold;
    }
    return ex;
}

// scale space (kernels_scalespace.hip): one template per kernel, launchers overloaded on the element type.  taps: float, or
// 16.16 as hak_fix16(tap) for int planes; the int low-pass also reads the uint8 image
void hak_launch_lowpass(hipStream_t st, const float* src, long src_stride, int src_pitch, float* dst, long dst_stride,
                        int w, int h, int p, int nimg, const float* taps, int R);
void hak_launch_lowpass(hipStream_t st, const unsigned char* src, long src_stride, int src_pitch, int* dst, long dst_stride,
                        int w, int h, int p, int nimg, const int* taps, int R);
void hak_launch_lowpass(hipStream_t st, const int* src, long src_stride, int src_pitch, int* dst, long dst_stride,
                        int w, int h, int p, int nimg, const int* taps, int R);
void hak_launch_down_smooth(hipStream_t st, const float* src, float* dst, float* smooth, long stride,
                            HakOct so, HakOct dd, int nimg, const float* taps);
void hak_launch_down_smooth(hipStream_t st, const int* src, int* dst, int* smooth, long stride,
                            HakOct so, HakOct dd, int nimg, const int* taps);
void hak_launch_contrast(hipStream_t st, const float* smooth, long stride, int w, int h, int p, int nimg,
                         HakImgState* state, float per, int noct);
void hak_launch_contrast(hipStream_t st, const int* smooth, long stride, int w, int h, int p, int nimg,
                         HakImgState* state, float per, int noct);
void hak_launch_reset_state(hipStream_t st, HakImgState* state, int nimg);      // every field either pipeline uses
void hak_launch_flow(hipStream_t st, const float* src, float* dst, long stride, int w, int h, int p, int nimg,
                     int diffusivity, const HakImgState* state, int octave, float fixed_ikc = 0.f);
void hak_launch_flow(hipStream_t st, const int* src, int* dst, long stride, int w, int h, int p, int nimg,
                     int diffusivity, const HakImgState* state, int octave);
// derivate + determinant of one level, with the level's extrema search fused in when b != nullptr
// (kernels_hessian.hip); returns false when the caller still has to run hak_launch_extrema_level
// The register-streaming kernels (k_hessian_stream, k_fed_sf) need a few thousand waves of >= 32 rows to fill the chip;
// below that (small octaves, single-image calls) the LDS tile kernels are faster.  mode: 0 = never, 1 = by this size
// rule (default), 2 = always where the kernel applies (tests).  Measured on MI355X: 1080p octave 3 at 128 images and
// octave 0 at 1 image favour the tile kernels by 20-40 %, everything above ~2000 waves favours streaming by 6-35 %.
static inline bool hak_stream_pays(int mode, int w, int h, int nimg)
{
    if (mode != 1) return mode != 0;
    const long strips = (w + 239) / 240;
    return strips * ((h + 31) / 32) * nimg >= 2048;
}
// Rows per wave of the register-streaming kernels.  A block's four waves take four consecutive row segments of a strip, so the
// number of segments is a multiple of four (no block with idle waves) and the segments are equally tall (no short last one);
// about 256 rows each amortise the warm-up rows (NS + 4 .. 4S + 2 per segment); more, shorter segments while the grid cannot
// fill the chip.  1080 rows: 4 x 270, 2160: 8 x 270, 540: 4 x 135, 720: 4 x 180.  Measured on 256 x 1080p (FED / Hessian class,
// ms): 9 segments of 128 rows, the ninth 56 rows tall in a block of its own (the rule this replaces): 9.70 / 9.14; 8 x 135:
// 9.16 / 8.32; 4 x 270: 9.08 / 8.31; 12 x 90: 9.43 / 8.49; 16 x 68: 9.63 / 8.84.
// Segments are halved only while the launch has fewer than 2048 waves (round 3; 4096 before; HAK_STREAM_MIN_WAVES, once per process): at 384
// images octave 2 then keeps 4 x 68 rows and octave 3 gets 8 x 17 instead of 16 x 9 -- a 9-row segment spends half its rows
// on warm-up.  FED class per 384 x 1080p images, A/B on one box: 8192: 13.68 ms, 4096: 13.18, 2048: 12.75-12.92, 1536: 12.78-12.85.
static inline int hak_stream_rows(int h, long strips_times_images, int min_rows)
{
    const long want = hak_process_knobs().stream_min_waves;
    int nseg = 4 * ((h + 512) / 1024 > 1 ? (h + 512) / 1024 : 1);
    while (strips_times_images * nseg < want && (h + 2 * nseg - 1) / (2 * nseg) >= min_rows) nseg *= 2;
    const int ry = (h + nseg - 1) / nseg;
    return ry > min_rows ? ry : min_rows;                    // (small images: fewer, not shorter, segments)
}
// dxy: interleaved {Lx, Ly} plane (2 * h * p elements).  det: where the determinant goes -- the fused kernels write it only
// when store_det is set (stage tests); the launch sequence passes a scratch plane that only the dilation > 4 fallback fills.
// lp_taps != nullptr: `src` is Lt(o,s-1) and the kernel applies the sigma=1 low-pass (taps k0, k1, k2) on the way in.
// hak_hessian_stream_covers: the cases the streaming kernel takes (the launch sequence asks before it lets k_fed_sf drop `smooth`)
static inline bool hak_hessian_stream_covers(int w, int h, int step, bool lp)
{
    return step >= 1 && step <= 4 && (w & 3) == 0 && w >= 16 && h >= 2 * step + 2 && (!lp || h >= 8);
}
// Launchers of both pipelines are overloaded on the element type: float (AKAZE) or int planes (FAST, 16.16 fixed point; taps as
// (int)(tap * 65536 + 0.5f), integer thresholds), one template body next to the kernel.  fixed_ikc, lp_taps, store_smooth: float only.
bool hak_launch_hessian_stream(hipStream_t st, const float* src, float* dxy, float* det, bool store_det, long stride,
                               int w, int h, int p, int nimg, int step, float fac1, float fac2,
                               const HakBatch* b, const HakLayout* L, const HakTables* htab, int octave, int sub, float dthreshold,
                               const float* lp_taps = nullptr);
bool hak_launch_hessian_stream(hipStream_t st, const int* src, int* dxy, int* det, bool store_det, long stride,
                               int w, int h, int p, int nimg, int step, int fac1, int fac2,
                               const HakBatch* b, const HakLayout* L, const HakTables* htab, int octave, int sub, int idthreshold);
// (dilation > 4: hak_launch_derivate + hak_launch_hessian fill `det`; the caller adds hak_launch_extrema_level)
bool hak_launch_hessian_level(hipStream_t st, const float* src, float* dxy, float* det, bool store_det, long stride,
                              int w, int h, int p, int nimg, int step,
                              const HakBatch* b, const HakLayout* L, const HakTables* htab, int octave, int sub, float dthreshold,
                              const float* lp_taps = nullptr);
bool hak_launch_hessian_level(hipStream_t st, const int* src, int* dxy, int* det, bool store_det, long stride,
                              int w, int h, int p, int nimg, int step,
                              const HakBatch* b, const HakLayout* L, const HakTables* htab, int octave, int sub, int idthreshold);
// octave-0 prologue fused (kernels_base.hip): Lt(0,0) + contrast factors, sigma=1 plane never written
// register-streaming pass A of the octave-0 prologue (kernels_base_stream.hip); false: not covered / does not pay
bool hak_launch_base_stream(hipStream_t st, const float* img, long img_stride, int sp, float* lt, float* grad, long stride, int w, int h,
                            int p, int nimg, const float* taps1, const float* taps_base, int R, HakImgState* state, int mode);
bool hak_launch_base_stream(hipStream_t st, const unsigned char* img, long img_stride, int sp, int* lt, int* grad, long stride, int w,
                            int h, int p, int nimg, const int* taps1, const int* taps_base, int R, HakImgState* state, int mode);
bool hak_launch_base_level(hipStream_t st, const float* img, long img_stride, int sp, float* lt, float* grad_scratch, long stride,
                           int w, int h, int p, int nimg, const float* taps1, const float* taps_base, int R,
                           HakImgState* state, float per, int noct, const HakKnobs& knobs);
// FAST (kf_base<R>): img is uint8; false: R not covered (caller: hak_launch_lowpass x2 + hak_launch_contrast)
bool hak_launch_base_level(hipStream_t st, const unsigned char* img, long img_stride, int sp, int* lt, int* grad_scratch, long stride,
                           int w, int h, int p, int nimg, const int* taps1, const int* taps_base, int R, HakImgState* state,
                           float per, int noct, const HakKnobs& knobs);
// sigma=1 low-pass + conductivity fused (kernels_smoothflow.hip)
void hak_launch_smooth_flow(hipStream_t st, const float* src, float* smooth, float* flow, long stride,
                            int w, int h, int p, int nimg, const float* taps, int diffusivity,
                            const HakImgState* state, int octave, float fixed_ikc = 0.f);
void hak_launch_smooth_flow(hipStream_t st, const int* src, int* smooth, int* flow, long stride,
                            int w, int h, int p, int nimg, const int* taps, int diffusivity,
                            const HakImgState* state, int octave);
// one whole sublevel (low-pass | decimation, conductivity, every FED step) per launch out of LDS tiles, for launches too small
// to fill the chip (kernels_level.hip).  Returns the number of launches (1 up to 36 steps).
#define HAK_LEVEL_TILE_MAX_PX (1920L * 1088L)      // by-size rule: at most one 1080p plane's worth of pixels per launch
// dxy / step / b / L / htab / sub / threshold: the level's Hessian inside the same launch where the cycle is long enough
// (first launch has >= 2 * step steps); *hess_done tells the caller whether it still has to launch the Hessian kernel
int hak_launch_level_tile(hipStream_t st, const float* src, HakOct so, bool head, float* smooth, float* dst, float* tmp, long stride,
                          HakOct dd, int nimg, const float* taps, int diffusivity, const float* tau, int n,
                          const HakImgState* state, int octave, float* dxy = nullptr, int step = 0, const HakBatch* b = nullptr,
                          const HakLayout* L = nullptr, const HakTables* htab = nullptr, int sub = 0, float dthreshold = 0.f,
                          bool* hess_done = nullptr, float fixed_ikc = 0.f);
int hak_launch_level_tile(hipStream_t st, const int* src, HakOct so, bool head, int* smooth, int* dst, int* tmp, long stride,
                          HakOct dd, int nimg, const int* taps, int diffusivity, const float* tau, int n,
                          const HakImgState* state, int octave, int* dxy = nullptr, int step = 0, const HakBatch* b = nullptr,
                          const HakLayout* L = nullptr, const HakTables* htab = nullptr, int sub = 0, int idthreshold = 0, bool* hess_done = nullptr);
int hak_launch_rcp_check(unsigned lo, unsigned hi, unsigned long long* d_bad);
// the levels whose first FED launch is k_fed_sf: low-pass + conductivity + first FED group in one streaming pass (PM_G2, 16-byte rows);
// so = geometry of Lt(o-1,0): an octave head, decimation included (even source extents).  The launchers keep their own guards.
static inline bool hak_fed_sf_covers(const HakKnobs& kn, int diffusivity, const HakOct& dd, int nimg, const HakOct* so = nullptr)
{
    if (!hak_stream_pays(kn.fuse_sf, dd.w, dd.h, nimg) || diffusivity != HAK_PM_G2 || (dd.w & 3) != 0 || dd.w < 16 || dd.h < 8) return false;
    return !so || (kn.fuse_head && !(so->w & 1) && !(so->h & 1));
}
bool hak_launch_fed_sf_head(hipStream_t st, const float* src, HakOct so, float* smooth, float* flow, float* dst, long stride,
                            HakOct dd, int nimg, const float* taps, int diffusivity, const float* tau, int ns,
                            const HakImgState* state, int octave, bool write_g);
bool hak_launch_fed_sf_head(hipStream_t st, const int* src, HakOct so, int* smooth, int* flow, int* dst, long stride,
                            HakOct dd, int nimg, const int* taps, int diffusivity, const float* tau, int ns,
                            const HakImgState* state, int octave, bool write_g);
// store_smooth = false: the low-pass is not written (its only reader, the level's Hessian, runs in the LP variant)
bool hak_launch_fed_sf(hipStream_t st, const float* src, float* smooth, float* flow, float* dst, long stride,
                       int w, int h, int p, int nimg, const float* taps, int diffusivity, const float* tau, int ns,
                       const HakImgState* state, int octave, bool write_g, bool store_smooth = true, float fixed_ikc = 0.f);
bool hak_launch_fed_sf(hipStream_t st, const int* src, int* smooth, int* flow, int* dst, long stride,
                       int w, int h, int p, int nimg, const int* taps, int diffusivity, const float* tau, int ns,
                       const HakImgState* state, int octave, bool write_g);
// fused FED groups (kernels_fed.hip); w % 4 != 0: one step (tau[0]) per launch, k_fed_generic (float) / kf_nld_step (int)
int hak_fed_groups(int n, int max_fuse, int w, bool wide_only);
bool hak_fed_wide_only(int octave, int w);
int hak_fed_group_size(int n, int G, int g);
void hak_launch_fed_group(hipStream_t st, const float* src, const float* flow, float* dst, long stride,
                          int w, int h, int p, int nimg, const float* tau, int ns);
void hak_launch_fed_group(hipStream_t st, const int* src, const int* flow, int* dst, long stride,
                          int w, int h, int p, int nimg, const float* tau, int ns);
// the unfused pair (dilations > 4, debug / test planes): src -> interleaved {Lx, Ly}, and {Lx, Ly} -> determinant
void hak_launch_derivate(hipStream_t st, const float* src, float* dxy, long stride, int w, int h, int p, int nimg, int step);
void hak_launch_derivate(hipStream_t st, const int* src, int* dxy, long stride, int w, int h, int p, int nimg, int step);
void hak_launch_hessian(hipStream_t st, const float* dxy, float* det, long stride, int w, int h, int p, int nimg, int step);
void hak_launch_hessian(hipStream_t st, const int* dxy, int* det, long stride, int w, int h, int p, int nimg, int step);
void hak_deriv_factors(float* fac1, float* fac2);            // akazed.cu:2537-2539
template <typename V> static inline void hak_deriv_factors_as(V& f1, V& f2)     // ... as the element type (int: 16.16, akazed.cu:4183-4184)
{
    float a, b;
    hak_deriv_factors(&a, &b);
    f1 = hak_fac_as(a, V());
    f2 = hak_fac_as(b, V());
}
// interleaved {a, b} plane (pitch 2p) -> two dense planes (pitch p); bytes are copied, so it serves both element types
void hak_launch_deinterleave(hipStream_t st, const float* ab, float* a, float* b, int w, int h, int p);

void hak_launch_ingest_u8(hipStream_t st, const unsigned char* src, long src_stride, int sp, float* dst, long dst_stride,
                          int dp, int w, int h, int nimg);

// detector tail (kernels_detect.hip)
// stand-alone extrema of one level on the determinant plane at arena offset det_off (dilation > 4); htab: the host tables.
// No plane pointer ties the call to a pipeline: the TYPE of the threshold alone selects k_extrema<float> or, on int32 planes,
// k_extrema<int> -- pass a typed variable, never a literal
void hak_launch_extrema_level(hipStream_t st, const HakBatch& b, const HakLayout& L, const HakTables* htab, int octave,
                              int s, float dthreshold, long det_off);
void hak_launch_extrema_level(hipStream_t st, const HakBatch& b, const HakLayout& L, const HakTables* htab, int octave, int s, int threshold,
                              long det_off);
void hak_launch_download(hipStream_t st, const hak_point* d_points, const int* d_num, long max_pts, int nimg, hak_point* h_points,
                         int* h_num);
// destinations of a pair call's records: device arrays, pinned host arrays (or NULL), capacity of each in records
struct HakPairDst { hak_point* d[2]; hak_point* h[2]; int cap[2]; };
void hak_launch_download_pair(hipStream_t st, const hak_point* src, const int* d_num, long max_pts, const HakPairDst& dst, int* h_num);
void hak_launch_nms_emit(hipStream_t st, const HakBatch& b, const HakLayout& L, const HakTables* tab, int psz,
                         hak_point* points, int max_pts, int* num_out, int fast = 0, int refine = 1);
void hak_launch_clear_maps(hipStream_t st, const HakBatch& b, const HakLayout& L);
// strongest-N selection (kernels_select.hip): prunes the survivor bitmap and rewrites the row counts between k_nms_cand and k_row_scan
void hak_launch_select(hipStream_t st, const HakBatch& b, const HakLayout& L, int max_pts, int cap0, int cap1, int fast);
// grid selection (kernels_grid_select.hip): the same place and the same effect on bitmap and row counts, by the cell rule of hak_set_retain_grid
void hak_launch_grid_select(hipStream_t st, const HakBatch& b, const HakLayout& L, int max_pts, int cap0, int cap1, int fast);
void hak_launch_seed_maps(hipStream_t st, const HakBatch& b, const HakLayout& L, const unsigned* d_resp_bits, const int* d_layer);

// integer FAST path: what has a float counterpart with the same parameter types
void hakf_launch_describe(hipStream_t st, const HakBatch& b, const HakLayout& L, const HakTables* tab, hak_point* points, int max_pts,
                          int patsize, int upright, int desc, int planned);

// descriptors (kernels_describe.hip)
// orient = 0 (stage tests): skip k_orient and describe with the angles the records hold
void hak_launch_describe(hipStream_t st, const HakBatch& b, const HakLayout& L, const HakTables* tab,
                         hak_point* points, int max_pts, int patsize, int upright, int desc, int planned, int orient = 1);

// bandwidth probes (kernels_probe.hip)
#define HAK_COPY_SHAPES 26                  // 3 x 2 x 4 copy shapes + read-only + write-only (kernels_probe.hip)
int hak_launch_copy_probe(long bytes, int iters, double* ms_per_copy, double* shapes_ms = nullptr);
int hak_launch_gather_probe(long bytes, int blocks, int per_lane, int iters, double* ms_per_launch);
int hak_launch_stream_probe(int w, int h, int nimg, int nwrite, int warm, int iters, double* ms, double* bytes);
int hak_launch_hess_probe(int w, int h, int nimg, int step, int iters, double* ms, double* bytes);

// 1-D grids of looping blocks: at least one block, at most 4096
static inline int hak_grid_x(int blocks) { return blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks; }

// ---- the matcher's rules (cuMatch / gHammingMatch akazed.cu:2144-2223 and the 2-NN post-processing), stated once for
// every kernel of kernels_match.hip and of the gated matchers (kernels_guided.hip, kernels_epipolar.hip, kernels_projected.hip): the
// packed key, the descriptor words, the record a search leaves and the two accept rules with the fields they write are defined
// here and nowhere else.
// packed key: Hamming distance << 20 | point index.  An unsigned minimum keeps the smallest distance and, among equal distances,
// the smallest index -- the reference's "first strict minimum in ascending order" (akazed.cu:2176-2187).
#define HAK_MKEY_BITS 20                        // index bits: a set holds fewer than 2^20 points
#define HAK_MKEY_EMPTY 0xFFFFFFFFu              // no candidate
static inline bool hak_mkey_fits(long n) { return n < (1L << HAK_MKEY_BITS); }      // the bound the entry points check
__device__ __forceinline__ unsigned hak_mkey(unsigned dist, unsigned index) { return (dist << HAK_MKEY_BITS) | index; }
__device__ __forceinline__ unsigned hak_mkey_dist(unsigned k) { return k >> HAK_MKEY_BITS; }
__device__ __forceinline__ int hak_mkey_index(unsigned k) { return (int)(k & ((1u << HAK_MKEY_BITS) - 1u)); }
// the two smallest keys of a stream: best <= sec after every update
__device__ __forceinline__ void hak_mkey_two_smallest(unsigned& best, unsigned& sec, unsigned key)
{
    sec = min(sec, max(best, key));
    best = min(best, key);
}
// descriptor as 16 dwords: exactly the 61 feature bytes (D9: the reference reads 3 bytes past them).  Features start at byte 24 of
// the 104-byte record: 4-byte aligned; of the last dword byte 60 only -- bytes 61..63 are struct padding
__device__ __forceinline__ void hak_desc_load(const hak_point* p, unsigned int d[16])
{
    const unsigned int* f = reinterpret_cast<const unsigned int*>(p->features);
#pragma unroll
    for (int i = 0; i < 15; i++) d[i] = f[i];
    d[15] = f[15] & 0xFFu;
}
// v_bcnt_u32_b32 computes popcount(x) + acc in ONE instruction; left to itself the compiler takes sixteen plain popcounts
// and rebuilds the sum as a tree of v_add3 (7 extra instructions per distance)
__device__ __forceinline__ unsigned hak_bcnt_acc(unsigned x, unsigned acc)
{
    unsigned r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
// 2-NN result record of one query from its two smallest keys: {j1, d1, d2, 0}; 512 stands for a missing second neighbour (the
// initial score of the reference's gMatch, akazed.cu:2028-2122), {-1, 512, 512, 0} for a query without a candidate
#define HAK_KNN_NO_DIST 512
__device__ __forceinline__ int4 hak_knn_none() { return make_int4(-1, HAK_KNN_NO_DIST, HAK_KNN_NO_DIST, 0); }
__device__ __forceinline__ int4 hak_knn_record(unsigned k1, unsigned k2)
{
    if (k1 == HAK_MKEY_EMPTY) return hak_knn_none();
    return make_int4(hak_mkey_index(k1), (int)hak_mkey_dist(k1), k2 == HAK_MKEY_EMPTY ? HAK_KNN_NO_DIST : (int)hak_mkey_dist(k2), 0);
}
// match fields of a query record (akaze.cpp:58-63 downloads these 16 bytes): accepted -> the train point, rejected -> -1
__device__ __forceinline__ void hak_match_store(hak_point* p1, const hak_point* __restrict__ pts2, bool ok, int bi, int dist)
{
    if (ok) {
        p1->match = bi;
        p1->distance = dist;
        p1->match_x = pts2[bi].x;
        p1->match_y = pts2[bi].y;
    } else {
        p1->match = -1;
        p1->distance = -1;
        p1->match_x = -1.f;
        p1->match_y = -1.f;
    }
}
// accept rule of gHammingMatch (akazed.cu:2190-2223): the train set is split into 16 residue classes j mod 16, each keeps its
// first strict minimum, and the match is accepted iff exactly ONE class attains the global minimum distance (akazed.cu:2206)
// and that distance is < HAK_MAX_DIST (akazed.cu:2223).  kmin: the smallest key; attain: the classes that attain its distance.
// (the clamp of the index never changes it: belt and braces for the gather)
__device__ __forceinline__ void hak_match_decide(hak_point* p1, const hak_point* __restrict__ pts2, int n2, unsigned kmin, int attain)
{
    const int dmin = (int)hak_mkey_dist(kmin);
    const bool ok = kmin != HAK_MKEY_EMPTY && attain == 1 && dmin < HAK_MAX_DIST;
    hak_match_store(p1, pts2, ok, min(hak_mkey_index(kmin), max(n2 - 1, 0)), dmin);
}
// ... from a query's 16 class minima: distances only decide -- the rule compares class minima, not indices, and ties between
// classes never matter for the result (they reject).  cls(t): the key of class t
template <typename F>
__device__ __forceinline__ void hak_match_decide_classes(hak_point* p1, const hak_point* __restrict__ pts2, int n2, F cls)
{
    unsigned kmin = cls(0);
#pragma unroll
    for (int t = 1; t < 16; t++)
        if (hak_mkey_dist(cls(t)) < hak_mkey_dist(kmin)) kmin = cls(t);
    int attain = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) attain += hak_mkey_dist(cls(t)) == hak_mkey_dist(kmin) ? 1 : 0;
    hak_match_decide(p1, pts2, n2, kmin, attain);
}
// ... from the slices' summaries {smallest key, mask of the classes that attain its distance}: one more summary into (K, M)
__device__ __forceinline__ void hak_match_merge_slice(unsigned& K, unsigned& M, unsigned k2, unsigned m2)
{
    if (hak_mkey_dist(k2) < hak_mkey_dist(K)) M = m2;          // a smaller distance: its classes alone attain it
    else if (hak_mkey_dist(k2) == hak_mkey_dist(K)) M |= m2;
    K = min(K, k2);
}
// 2-NN accept rule of query i: a candidate, d1 < max_dist, the ratio test d1 / d2 < ratio_num / ratio_den and,
// cross != 0, rev(j1) == i.  f: the query's search record ({-1, 512, 512, 0} past n1)
__device__ __forceinline__ bool hak_knn2_rule(const int i, const int n1, const int4* __restrict__ fwd, const int4* __restrict__ rev,
                                              const int ratio_num, const int ratio_den, const int cross, const int max_dist, int4& f)
{
    f = hak_knn_none();
    if (i >= n1) return false;
    f = fwd[i];
    bool ok = f.x >= 0 && f.y < max_dist && (long)f.y * ratio_den < (long)f.z * ratio_num;
    if (ok && cross) ok = rev[f.x].x == i;
    return ok;
}
// the list entry of an accepted query
__device__ __forceinline__ hak_match_pair hak_knn2_pair(int i, const int4 f, const hak_point* pts1, const hak_point* __restrict__ pts2)
{
    hak_match_pair r;
    r.query = i; r.train = f.x; r.distance = f.y; r.second = f.z;
    r.x1 = pts1[i].x; r.y1 = pts1[i].y; r.x2 = pts2[f.x].x; r.y2 = pts2[f.x].y;
    return r;
}

// matcher (kernels_match.hip)
// Scratch of the SLICED searches (one big pair through hak_match / hak_match_knn2, e.g. 10k x 10k: the train set is cut into
// slices so that the query blocks x slices fill the chip).  Owned by a context or handed out by the per-device pool of
// hak_api.hip (ctx == NULL: cuMatch is a free function in the reference); lives on one device, used by one call at a time.
// Invariant between calls: every key is HAK_MKEY_EMPTY and every ticket 0 -- the kernels restore that themselves (k_match_finish
// writes the empty key back over every key it reads; the block that draws a query block's last ticket resets the ticket; the
// slices' summaries in `part` are plain stores with no initial state), so no call starts with a memset.
struct HakMatchScratch {
    unsigned* keys = nullptr; long keys_cap = 0;        // [queries][16] class minima, merged with atomicMin          (1-NN)
    int* ticket = nullptr; long ticket_cap = 0;         // [query blocks of 128]
    uint2* part = nullptr; long part_cap = 0;           // [slices][queries padded to 128] two smallest keys per slice (2-NN)
    int4* knn = nullptr; long knn_cap = 0;              // forward | reverse 2-NN results of hak_match_knn2
    int* blk = nullptr; long blk_cap = 0;               // accepted matches per 1024-query block (compaction of hak_match_knn2)
    int* d_cnt = nullptr; int* h_cnt = nullptr;         // accepted-match count: device word and its pinned host mirror
    int device = -1;
};
// grow-only; returns false (and leaves a usable smaller state) when the device is out of memory.  `st`: the stream earlier
// users of the buffers ran on (synchronised before a buffer is replaced).
bool hak_match_scratch_reserve(HakMatchScratch* sc, hipStream_t st, long keys, long tickets, long parts, long knn, long blks);
void hak_match_scratch_free(HakMatchScratch* sc);
// What a search or the 2-NN finish launches for a call -- decided in ONE host function (hak_match_plan) that touches no device;
// hak_launch_match, hak_launch_knn2 and hak_launch_knn2_finish launch what it says (their one decision left: a sliced plan whose
// scratch cannot be reserved runs unsliced), and the test ABI
// (hak_op_match_shape) hands the same plan to the tests, which assert with it that a case reached the path it was made for.
struct HakMatchPlan {
    int kernel = 0;             // 0: k_match_mfma (matrix cores); 1: the vector-pipe kernels k_match / k_knn2
    int qt = 1;                 // k_match_mfma: query tiles per wave; k_match: queries per thread
    int gx = 1;                 // grid.x: query blocks
    int slices = 1;             // train-set slices; 1: not sliced
    int rows_per_slice = 0;     // rows of a slice cut on the host; 0: not sliced, or cut inside the kernel (device-side counts)
    int chunks_per_slice = 0;   // LDS chunks one block pass stages (k_match_mfma: 192 rows, a tail counts; k_match: tiles of 128) --
                                // of the whole set when not sliced, of the capacity with device-side counts
    int finish_blocks = 1;      // 2-NN accept rule + compaction: 1 = one block per pair, > 1 = two passes of that many blocks
};
// search: 0 = hak_launch_match, 1 = hak_launch_knn2 (queries n1_host, train set n2_host; with device-side counts both carry the
// CAPACITY of a set); finish_blocks is hak_launch_knn2_finish's for n1_host queries.  scratch: a HakMatchScratch is at hand.
HakMatchPlan hak_match_plan(const HakMatchKnobs& mk, int search, bool device_counts, int n1_host, int n2_host, int npairs, bool scratch);
void hak_launch_match(hipStream_t st, hak_point* pts1, const hak_point* pts2, const int* n1_dev, const int* n2_dev,
                      int n1_host, int n2_host, long pair_stride1, long pair_stride2, int npairs,
                      HakMatchScratch* scratch = nullptr);
void hak_launch_knn2(hipStream_t st, const hak_point* ptsA, const hak_point* ptsB, const int* nA_dev, const int* nB_dev,
                     int nA_host, int nB_host, long strideA, long strideB, int npairs, int4* out, long out_stride,
                     HakMatchScratch* scratch = nullptr);
void hak_launch_knn2_finish(hipStream_t st, hak_point* pts1, const hak_point* pts2, const int* n1_dev, int n1_host, long stride1,
                            long stride2, int npairs, const int4* fwd, const int4* rev, long knn_stride, int ratio_num,
                            int ratio_den, int cross, int max_dist, hak_match_pair* out, long out_stride, int* out_count,
                            HakMatchScratch* scratch = nullptr);

// guided matching (kernels_guided.hip, hak_match_guided): the scratch of npairs pairs of at most pts_cap train points each.  Owned
// by a context (grown outside a launch sequence) or allocated for the duration of a call without one; every word a call reads is
// written earlier in the same call.
struct HakGuidedScratch {
    float2* xy = nullptr;                       // [npairs][pts_cap] train coordinates, sorted by cell
    int* idx = nullptr;                         // [npairs][pts_cap] ... and their indices
    int* off = nullptr;                         // [npairs][64 * 64 + 1] first list entry of every cell
    int* grid = nullptr;                        // [npairs][8] the pair's grid: origin, 1 / cell side, cells per axis
    long pts_cap = 0;
    int4* rev = nullptr;                        // [npairs][rev_stride] reverse keys, then {rev(j), d, 512, 0} (the 2-NN scratch's reverse half)
    long rev_stride = 0;
};
// (the grid GdGrid / gd_cell and the device code the three searches share: gated_common.h)
size_t hak_guided_scratch_bytes(long npairs, long pts_cap);
HakGuidedScratch hak_guided_scratch_carve(void* base, long npairs, long pts_cap, int4* rev, long rev_stride);
// the two steps the gated searches share: the bin step (train points of npairs pairs into sc's grid of cells of side >= rp; resets
// the reverse keys) and, after a search, the reverse step (reverse keys -> the records k_knn2_finish reads).  The count of pair k
// is n2_dev[k * count_step]: 2 in a detect batch of image pairs.  gd_launch (gated_common.h) runs them around a search kernel
void hak_launch_guided_bin(hipStream_t st, const hak_point* pts2, const int* n2_dev, int n2_host, long stride2, int npairs, float rp,
                           const HakGuidedScratch& sc, int count_step);
void hak_launch_guided_rev(hipStream_t st, const int* n2_dev, int n2_host, int npairs, const HakGuidedScratch& sc, int count_step);
void hak_launch_guided(hipStream_t st, const hak_point* pts1, const hak_point* pts2, const int* n1_dev, const int* n2_dev, int count_step,
                       int n1_host, int n2_host, long stride1, long stride2, int npairs, const hak_homography* d_H, const float* h_H,
                       float radius, int cross, const HakGuidedScratch& sc, int4* fwd, long fwd_stride);
// epipolar guided matching (kernels_epipolar.hip, hak_match_epipolar): as hak_launch_guided with a fundamental matrix per pair
// (d_F on the device, or NULL: h_F[9] on the host serves the only pair); the same scratch
void hak_launch_epipolar(hipStream_t st, const hak_point* pts1, const hak_point* pts2, const int* n1_dev, const int* n2_dev, int count_step,
                         int n1_host, int n2_host, long stride1, long stride2, int npairs, const hak_fundamental* d_F, const float* h_F,
                         float radius, int cross, const HakGuidedScratch& sc, int4* fwd, long fwd_stride);
// projection-guided matching (kernels_projected.hip, hak_match_projected): landmark m of list A (its point xyzA[3m ..], its descriptor
// desc[A[m].train]) is projected through a view and K and searched among the train points pts2 near the projection; the same
// scratch and the same bin and reverse steps as hak_launch_guided.  Counts on the device (countsA[k * stepA], desc_counts[k *
// desc_step], counts2[k * step2]) or, NULL, the host values for the only list (with device counts n2_host carries the capacity of
// a train set); capA / capD / sc.pts_cap: what the counts are clamped to.  The view of list k is record k * view_step of `views`
// (kind: HAK_VIEW_*), or h_view != NULL: these 12 host floats.  The accepted landmarks go to out + k * out_stride in ascending m
// (out may be NULL: count only), their number to out_counts[k].
void hak_launch_projected(hipStream_t st, const hak_match_pair* A, long strideA, const int* countsA, int stepA, int nA_host, long capA,
                          const unsigned char* masksA, const float* xyzA, const hak_point* desc, long desc_stride,
                          const int* desc_counts, int desc_step, int nD_host, long capD, const hak_point* pts2, long stride2,
                          const int* counts2, int step2, int n2_host, int npairs, const void* views, int kind, int view_step,
                          const float* h_view, const hak_intrinsics& K, float radius, int ratio_num, int ratio_den, int cross,
                          int max_dist, const HakGuidedScratch& sc, int4* fwd, long fwd_stride, hak_corr3d* out, long out_stride,
                          int* out_counts);

// The three RANSAC estimators share one scaffold (ransac_common.h) and one launch-shape rule, hak_homography_blocks: score blocks per
// pair (and hypotheses per block through hp_out).  A launcher writes one uint64 slot per (pair, block) to `slots` (npairs *
// hak_homography_blocks(...) of them); those with a models kernel keep `models`, hak_*_words(npairs, iterations) 32-bit words, in the
// scaffold's word-major layout.
// RANSAC homography (kernels_homography.hip): no models kernel
int hak_homography_blocks(int npairs, int iterations, int* hp_out);
void hak_launch_homography(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                           int iterations, float threshold, unsigned seed, int refine, unsigned long long* slots,
                           hak_homography* out, unsigned char* masks, long mask_stride);

// RANSAC fundamental matrix (kernels_fundamental.hip): 28 model words per hypothesis
long hak_fundamental_words(int npairs, int iterations);
void hak_launch_fundamental(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                            int iterations, float threshold, unsigned seed, unsigned* models, unsigned long long* slots,
                            hak_fundamental* out, unsigned char* masks, long mask_stride);
// five-point RANSAC essential matrix (kernels_essential.hip): each hypothesis is stored as three virtual hypotheses of four models,
// 37 model words each (hak_essential_words), and scored in hak_essential_blocks = hak_homography_blocks(npairs, 3 * iterations) blocks
long hak_essential_words(int npairs, int iterations);
int hak_essential_blocks(int npairs, int iterations);
void hak_launch_essential(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                          const hak_intrinsics& K1, const hak_intrinsics& K2, int iterations, float threshold, unsigned seed,
                          unsigned* models, unsigned long long* slots, hak_fundamental* out, unsigned char* masks, long mask_stride);
// hak_shared_record(): the current device's one record of HAK_REC_BYTES (kernels_fundrefit.hip; NULL on failure) for the synchronous
// one-list calls that own none: both refits without a context, hak_recover_pose and hak_triangulate always.  They take it in turn.
#define HAK_REC_BYTES 64         // room for the largest record of an estimator or refit (hak_abs_pose)
void* hak_shared_record();
// rank-2 refit of a fundamental matrix (kernels_fundrefit.hip): record k is read from and rewritten to inout[k]; no scratch.
void hak_launch_fundamental_refit(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host,
                                  int npairs, float threshold, int rounds, hak_fundamental* inout, unsigned char* masks,
                                  long mask_stride);
// relative pose from a fundamental matrix (kernels_pose.hip): F of pair k from d_F[k] on the device, or d_F = NULL: h_F[9] on the
// host serves the only pair; masks and xyz (3 floats per record) at the lists' stride, either may be NULL; no scratch.
void hak_launch_pose(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                     const hak_fundamental* d_F, const float* h_F, const hak_intrinsics& K1, const hak_intrinsics& K2,
                     float threshold, float max_depth, hak_pose* out, unsigned char* masks, float* xyz);
// Gauss-Newton refit of a relative pose (kernels_poserefit.hip): record k is read from and rewritten to inout[k]; masks and xyz as
// hak_launch_pose writes them, under the refitted pose; no scratch.
void hak_launch_pose_refit(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int n_host, int npairs,
                           const hak_intrinsics& K1, const hak_intrinsics& K2, float threshold, float max_depth, int rounds,
                           hak_pose* inout, unsigned char* masks, float* xyz);
// RANSAC absolute pose (kernels_pnp.hip): 49 model words per hypothesis
long hak_pnp_words(int npairs, int iterations);
void hak_launch_pnp(hipStream_t st, const hak_corr3d* corr, long stride, const int* counts, int n_host, int npairs,
                    const hak_intrinsics& K, int iterations, float threshold, unsigned seed, unsigned* models,
                    unsigned long long* slots, hak_abs_pose* out, unsigned char* masks, long mask_stride);
// Gauss-Newton refit of an absolute pose (kernels_pnprefit.hip): record k is read from and rewritten to inout[k]; no scratch.
void hak_launch_pnp_refit(hipStream_t st, const hak_corr3d* corr, long stride, const int* counts, int n_host, int npairs,
                          const hak_intrinsics& K, float threshold, int rounds, hak_abs_pose* inout, unsigned char* masks,
                          long mask_stride);
// triangulation under two known views (kernels_triangulate.hip): the count of list k is counts[k * count_step], or counts = NULL:
// n_host serves the only list; view A of list k is record k * stepA of viewsA (kindA: HAK_VIEW_*), or h_A != NULL: these 12 host
// floats serve every list; B likewise; masks and xyz (3 floats per record) at the lists' stride, either may be NULL; no scratch.
void hak_launch_triangulate(hipStream_t st, const hak_match_pair* matches, long stride, const int* counts, int count_step, int n_host,
                            int npairs, const void* viewsA, int kindA, int stepA, const float* h_A, const void* viewsB, int kindB,
                            int stepB, const float* h_B, const hak_intrinsics& KA, const hak_intrinsics& KB, float threshold,
                            float max_depth, float min_sin, hak_triangulation* out, unsigned char* masks, float* xyz);
// track linking (kernels_pnp.hip): countsA / countsB NULL: nA_host / nB_host serve the only pair; `table`: npairs * max_index ints
// of scratch, cleared by the launch; masksA may be NULL
void hak_launch_link(hipStream_t st, const hak_match_pair* A, long strideA, const int* countsA, int stepA, int nA_host,
                     const unsigned char* masksA, const float* xyzA, const hak_match_pair* B, long strideB, const int* countsB,
                     int stepB, int nB_host, int npairs, int max_index, int* table, hak_corr3d* out, long out_stride, int* out_counts);

// A launcher that cannot do what it was asked (a precondition its caller should have checked) records the reason here instead
// of aborting; enqueue_detect turns it into the call's error (hak_sequence.hip).  Thread-local, like hak_last_error().
void hak_note_launch_error(const char* msg);

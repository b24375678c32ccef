// hak_test_api.hip -- the TEST ABI (include/hipakaze_test.h, libhipakaze_test.so): plane / kcontrast introspection, single-stage
// operators, detector-tail and descriptor stages on hand-made inputs, bandwidth probes.  Everything here drives the launchers
// of libhipakaze.so (the kernels of the launch sequence); nothing of it is part of the product ABI.
#include "hak_ctx.h"
#include "../../include/hipakaze_test.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

extern "C" int hak_debug_plane(hak_ctx* c, int img, int kind, int o, int s, float* h_dst)
{
    if (!c || img < 0 || img >= c->cfg.batch || o < 0 || o >= c->L.noct || s < 0 || s >= c->L.ms) return fail("bad plane");
    const HakLayout& L = c->L;
    const HakOct oc = L.oct[o];
    HIP_TRY(hipStreamSynchronize(c->stream));
    const float* arena = c->arena + (long)img * L.arena;
    if (kind == HAK_PLANE_LT) {
        HIP_TRY(hipMemcpy2D(h_dst, sizeof(float) * oc.w, arena + L.lt(o, s), sizeof(float) * oc.p, sizeof(float) * oc.w, oc.h, hipMemcpyDeviceToHost));
        return 0;
    }
    // Lx / Ly live interleaved; the determinant is not stored at all (HakLayout): both are produced here, for the tests, by
    // the unfused kernels from the stored derivative plane
    float* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, sizeof(float) * 2 * (size_t)oc.plane));
    int rc = 0;
    const float* src = tmp;
    if (kind == HAK_PLANE_DET) {
        const int step = c->plan[(size_t)o * L.ms + s].sigma_size;
        if (c->last_fast) hak_launch_hessian(nullptr, reinterpret_cast<const int*>(arena + L.dxy(o, s)), reinterpret_cast<int*>(tmp), 0, oc.w, oc.h, oc.p, 1, step);
        else hak_launch_hessian(nullptr, arena + L.dxy(o, s), tmp, 0, oc.w, oc.h, oc.p, 1, step);
    } else {
        hak_launch_deinterleave(nullptr, arena + L.dxy(o, s), tmp, tmp + oc.plane, oc.w, oc.h, oc.p);
        if (kind == HAK_PLANE_LY) src = tmp + oc.plane;
    }
    if (hipDeviceSynchronize() != hipSuccess) rc = fail("debug plane kernel");
    if (!rc && hipMemcpy2D(h_dst, sizeof(float) * oc.w, src, sizeof(float) * oc.p, sizeof(float) * oc.w, oc.h, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail("debug plane copy");
    (void)hipFree(tmp);
    return rc;
}

// the context's arena as the library holds it (HakLayout): 4 + noct * (6 + 2 ms) words
//   {noct, ms, elements per image, batch} and per octave {w, h, p, smooth, flow, tmp, Lt(o, 0 .. ms-1), dxy(o, 0 .. ms-1)} -- offsets
// in elements from the image's first.  Returns the number of words (also when `out` is NULL or n too small: ask first), -1 on a bad call
extern "C" int hak_debug_arena_layout(hak_ctx* c, long* out, int n)
{
    if (!c) { fail("null context"); return -1; }
    const HakLayout& L = c->L;
    const int per = 6 + 2 * L.ms, need = 4 + L.noct * per;
    if (!out || n < need) return need;
    out[0] = L.noct; out[1] = L.ms; out[2] = L.arena; out[3] = c->cfg.batch;
    for (int o = 0; o < L.noct; o++) {
        long* q = out + 4 + o * per;
        q[0] = L.oct[o].w; q[1] = L.oct[o].h; q[2] = L.oct[o].p;
        q[3] = L.smooth_off[o]; q[4] = L.flow_off[o]; q[5] = L.tmp_off[o];
        for (int s = 0; s < L.ms; s++) { q[6 + s] = L.lt(o, s); q[6 + L.ms + s] = L.dxy(o, s); }
    }
    return need;
}
// the whole arena of batch image `img` to / from the host, as it lies (bits are copied: float and int32 planes alike)
extern "C" int hak_debug_arena_read(hak_ctx* c, int img, float* h_dst)
{
    if (!c || !h_dst || img < 0 || img >= c->cfg.batch) return fail("bad arena read");
    if (hak_sync(c)) return 1;
    HIP_TRY(hipMemcpy(h_dst, c->arena + (long)img * c->L.arena, sizeof(float) * (size_t)c->L.arena, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int hak_debug_arena_write(hak_ctx* c, int img, const float* h_src)
{
    if (!c || !h_src || img < 0 || img >= c->cfg.batch) return fail("bad arena write");
    if (hak_sync(c)) return 1;
    HIP_TRY(hipMemcpy(c->arena + (long)img * c->L.arena, h_src, sizeof(float) * (size_t)c->L.arena, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int hak_debug_kcontrast(hak_ctx* c, int img, float* kc)
{
    if (!c || img < 0 || img >= c->cfg.batch) return fail("bad image index");
    HakImgState s;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&s, c->state + img, sizeof(s), hipMemcpyDeviceToHost));
    *kc = s.kcontrast[0];
    return 0;
}

// ------------------------------------------------ single-stage test operators
// One template per operator serves the float operator and its integer FAST twin (tests/test_gpu_stages.py, tests/test_gpu_fast_stages.py):
// each drives the launcher overload the launch sequence (build_level<V> / hessian_level<V>, hak_sequence.hip) calls.  `who` is the
// text a failed device call is reported with: the operator's name, or for the float operators the call their HIP_TRY has always named.
#define HAK_FAST_KC_MAX 46340                                       // kcontrast * kcontrast stays inside int32 (akazed.cu:4215)
#define HAK_SYNC_TEXT "hipDeviceSynchronize()"
template <typename V> constexpr bool op_fast = std::is_same<V, int>::value;
// taps as V: the float taps, or 16.16 (akazed.cu:3896, as hak_create fills itaps1 / itaps_base)
template <typename V> static void op_taps(float var, int radius, V* out)
{
    float t[8];
    hak_gauss_taps(var, radius, t);
    for (int i = 0; i < 8; i++) {
        if constexpr (op_fast<V>) out[i] = i <= radius ? hak_fix16(t[i]) : 0;
        else out[i] = t[i];
    }
}
// a device HakImgState per image whose octave-0 contrast factor is set the way k_kcontrast<V> sets it; *out == nullptr on failure
template <typename V> static int op_state(HakImgState** out, const V* kcontrast, int nimg)
{
    *out = nullptr;
    std::vector<HakImgState> hs((size_t)nimg);
    for (int i = 0; i < nimg; i++) {
        hs[i] = HakImgState{};
        if constexpr (op_fast<V>) {
            if (kcontrast[i] < 0 || kcontrast[i] > HAK_FAST_KC_MAX) return fail("integer contrast factor must be in 0 .. 46340");
            hs[i].ikcontrast[0] = kcontrast[i];
            hs[i].ikc[0] = 1.f / (float)(kcontrast[i] * kcontrast[i]);            // akazed.cu:4215 (0 -> inf)
        } else {
            hs[i].kcontrast[0] = kcontrast[i];
            hs[i].ikc[0] = 1.f / (kcontrast[i] * kcontrast[i]);                   // akazed.cu:2493
        }
    }
    HakImgState* st = nullptr;
    HIP_TRY(hipMalloc((void**)&st, sizeof(HakImgState) * (size_t)nimg));
    if (hipMemcpy(st, hs.data(), sizeof(HakImgState) * (size_t)nimg, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(st);
        return fail("state upload");
    }
    *out = st;
    return 0;
}
static int op_sync(const char* who)
{
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(std::string(who) + ": " + hipGetErrorString(e));
    return 0;
}
// ... and frees a state on the way out
static int op_sync_free(const char* who, HakImgState* st)
{
    const int rc = op_sync(who);
    (void)hipFree(st);
    return rc;
}
// contrast factor, lattice maximum and the reference's h_hist of a one-image state; frees it.  h_hist: the w x h pixels plus what
// the threads beside / below the image add to bin 0 (hak_hist_extra0; the kernels carry that constant into `thresh` instead of
// adding it to the device histogram)
template <typename V> static int op_state_result(const char* who, HakImgState* st, int w, int h, V* kc, V* hmax, int* hist)
{
    HakImgState hs;
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t e2 = e == hipSuccess ? hipMemcpy(&hs, st, sizeof(hs), hipMemcpyDeviceToHost) : e;
    (void)hipFree(st);
    if (e2 != hipSuccess) return fail(std::string(who) + ": " + hipGetErrorString(e2));
    if constexpr (op_fast<V>) {
        if (kc) *kc = hs.ikcontrast[0];
        if (hmax) *hmax = hs.ihmax;
    } else {
        if (kc) *kc = hs.kcontrast[0];
        if (hmax) memcpy(hmax, &hs.hmax_bits, 4);
    }
    if (hist) { memcpy(hist, hs.hist, sizeof(hs.hist)); hist[0] += hak_hist_extra0(w, h); }
    return 0;
}
// max_fuse of the environment; FAST keeps the 4-px groups (hak_sequence.hip build_level: above 4 counts as 4; no deeper int kernel is built)
template <typename V> static int op_max_fuse()
{
    const int m = hak_knobs_from_env().max_fuse;
    return op_fast<V> && m > 4 ? 4 : m;
}
// the FED ping-pong of a cycle cut into G launches: groups g0 .. G-1 from `s` (`done` steps are behind it), alternating dst / tmp so
// that the last launch lands in dst
template <typename V>
static void op_fed_groups(const V* s, const V* flow, V* dst, V* tmp, long stride, int w, int h, int p, int nimg, const float* tau,
                          int nsteps, int G, int g0, int done)
{
    for (int g = g0; g < G; g++) {
        const int ns = hak_fed_group_size(nsteps, G, g);
        V* d = ((G - g) % 2 == 1) ? dst : tmp;
        hak_launch_fed_group(nullptr, s, flow, d, stride, w, h, p, nimg, tau + done, ns);
        done += ns;
        s = d;
    }
}

template <typename In, typename V>
static int lowpass_t(const char* who, const In* s, int sp, V* d, int w, int h, int p, float var, int radius)
{
    if (radius < 1 || radius > 5) return fail("radius must be 1..5");
    V taps[8];
    op_taps<V>(var, radius, taps);
    hak_launch_lowpass(nullptr, s, 0, sp, d, 0, w, h, p, 1, taps, radius);
    return op_sync(who);
}
extern "C" int hak_op_lowpass(const float* s, float* d, int w, int h, int p, float var, int radius)
{ return lowpass_t(HAK_SYNC_TEXT, s, p, d, w, h, p, var, radius); }
extern "C" int hak_op_fast_conv_u8(const unsigned char* s, int sp, int* d, int w, int h, int p, float var, int radius)
{ return lowpass_t("hak_op_fast_conv_u8", s, sp, d, w, h, p, var, radius); }
extern "C" int hak_op_fast_lowpass(const int* s, int* d, int w, int h, int p, float var, int radius)
{ return lowpass_t("hak_op_fast_lowpass", s, p, d, w, h, p, var, radius); }

template <typename V>
static int down_smooth_t(const char* who, const V* s, V* d, V* sm, int sw, int sh, int sp, int dw, int dh, int dp)
{
    V taps[8];
    op_taps<V>(1.f, 2, taps);
    HakOct so{sw, sh, sp, (long)sh * sp}, dd{dw, dh, dp, (long)dh * dp};
    hak_launch_down_smooth(nullptr, s, d, sm, 0, so, dd, 1, taps);
    return op_sync(who);
}
extern "C" int hak_op_down_smooth(const float* s, float* d, float* sm, int sw, int sh, int sp, int dw, int dh, int dp)
{ return down_smooth_t(HAK_SYNC_TEXT, s, d, sm, sw, sh, sp, dw, dh, dp); }
extern "C" int hak_op_fast_down_smooth(const int* s, int* d, int* sm, int sw, int sh, int sp, int dw, int dh, int dp)
{ return down_smooth_t("hak_op_fast_down_smooth", s, d, sm, sw, sh, sp, dw, dh, dp); }

template <typename V>
static int kcontrast_t(const char* who, const V* smooth, int w, int h, int p, float per, V* kc, V* hmax, int* hist)
{
    HakImgState* st = nullptr;
    HIP_TRY(hipMalloc((void**)&st, sizeof(HakImgState)));
    (void)hipMemset(st, 0, sizeof(HakImgState));
    hak_launch_reset_state(nullptr, st, 1);
    hak_launch_contrast(nullptr, smooth, 0, w, h, p, 1, st, per, 1);
    return op_state_result<V>(who, st, w, h, kc, hmax, hist);
}
extern "C" int hak_op_kcontrast(const float* smooth, int w, int h, int p, float per, float* kc, float* hmax, int* hist)
{ return kcontrast_t("hipMemcpy(&hs, st, sizeof(hs), hipMemcpyDeviceToHost)", smooth, w, h, p, per, kc, hmax, hist); }
extern "C" int hak_op_fast_kcontrast(const int* smooth, int w, int h, int p, float per, int* kc, int* hmax, int* hist)
{ return kcontrast_t("FAST contrast", smooth, w, h, p, per, kc, hmax, hist); }

template <typename V>
static int flow_t(const char* who, const V* s, V* d, int w, int h, int p, int diffusivity, V kcontrast)
{
    HakImgState* st = nullptr;
    if (op_state<V>(&st, &kcontrast, 1)) return 1;
    hak_launch_flow(nullptr, s, d, 0, w, h, p, 1, diffusivity, st, 0);
    return op_sync_free(who, st);
}
extern "C" int hak_op_flow(const float* s, float* d, int w, int h, int p, int diffusivity, float kcontrast)
{ return flow_t(HAK_SYNC_TEXT, s, d, w, h, p, diffusivity, kcontrast); }
extern "C" int hak_op_fast_flow(const int* s, int* d, int w, int h, int p, int diffusivity, int kcontrast)
{ return flow_t("hak_op_fast_flow", s, d, w, h, p, diffusivity, kcontrast); }

extern "C" int hak_op_rcp_check(unsigned lo_bits, unsigned hi_bits, unsigned long long* mismatches)
{
    if (!mismatches) return fail("null argument");
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d, 0, sizeof(unsigned long long)));
    int rc = hak_launch_rcp_check(lo_bits, hi_bits, d);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail("rcp check kernel");
    if (!rc && hipMemcpy(mismatches, d, sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) rc = fail("rcp check download");
    (void)hipFree(d);
    return rc;
}

template <typename V>
static int smooth_flow_t(const char* who, const V* s, V* sm, V* fl, int w, int h, int p, int diffusivity, V kcontrast)
{
    V taps[8];
    op_taps<V>(1.f, 2, taps);
    HakImgState* st = nullptr;
    if (op_state<V>(&st, &kcontrast, 1)) return 1;
    hak_launch_smooth_flow(nullptr, s, sm, fl, 0, w, h, p, 1, taps, diffusivity, st, 0);
    return op_sync_free(who, st);
}
extern "C" int hak_op_smooth_flow(const float* s, float* sm, float* fl, int w, int h, int p, int diffusivity, float kcontrast)
{ return smooth_flow_t(HAK_SYNC_TEXT, s, sm, fl, w, h, p, diffusivity, kcontrast); }
extern "C" int hak_op_fast_smooth_flow(const int* s, int* sm, int* fl, int w, int h, int p, int diffusivity, int kcontrast)
{ return smooth_flow_t("hak_op_fast_smooth_flow", s, sm, fl, w, h, p, diffusivity, kcontrast); }

// nsteps FED steps in the launches the sequence would cut them into; image i's planes lie `stride` elements behind image i-1's
template <typename V>
static int nld_steps_t(const char* who, const V* src, const V* flow, V* dst, V* tmp, long stride, int w, int h, int p, int nimg,
                       const float* tau, int nsteps)
{
    if (nsteps < 1 || nimg < 1) return fail("nsteps < 1 or nimg < 1");
    if (p % 4 || stride % 4) return fail("pitch and stride must be multiples of 4");
    const int G = hak_fed_groups(nsteps, op_max_fuse<V>(), w, false);
    op_fed_groups(src, flow, dst, tmp, stride, w, h, p, nimg, tau, nsteps, G, 0, 0);
    return op_sync(who);
}
extern "C" int hak_op_nld_steps(const float* src, const float* flow, float* dst, float* tmp, int w, int h, int p,
                                const float* tau, int nsteps)
{
    if (nsteps < 1) return fail("nsteps < 1");
    if (p % 4) return fail("pitch must be a multiple of 4");
    return nld_steps_t(HAK_SYNC_TEXT, src, flow, dst, tmp, 0, w, h, p, 1, tau, nsteps);
}
extern "C" int hak_op_nld_steps_batch(const float* src, const float* flow, float* dst, float* tmp, long stride, int w, int h, int p,
                                      int nimg, const float* tau, int nsteps)
{ return nld_steps_t(HAK_SYNC_TEXT, src, flow, dst, tmp, stride, w, h, p, nimg, tau, nsteps); }
extern "C" int hak_op_fast_nld_steps_batch(const int* src, const int* flow, int* dst, int* tmp, long stride, int w, int h, int p,
                                           int nimg, const float* tau, int nsteps)
{ return nld_steps_t("hak_op_fast_nld_steps", src, flow, dst, tmp, stride, w, h, p, nimg, tau, nsteps); }
extern "C" int hak_op_fast_nld_steps(const int* src, const int* flow, int* dst, int* tmp, int w, int h, int p, const float* tau, int nsteps)
{ return nld_steps_t("hak_op_fast_nld_steps", src, flow, dst, tmp, 0, w, h, p, 1, tau, nsteps); }

// One whole FED cycle of a sublevel the way the launch sequence runs it on large batches: k_fed_sf (sigma=1 low-pass + PM_G2
// conductivity + the first group of steps; head != 0: the decimating octave-head form, src = the sw x sh source plane of pitch sp)
// followed by the remaining groups through k_fed_multi.  All planes of image i lie `stride` elements behind image i-1's;
// kcontrast: one contrast factor per image.  Fails when k_fed_sf does not cover the case (no other kernel is substituted).
template <typename V>
static int fed_cycle_t(const char* who, const V* src, int head, int sw, int sh, int sp, V* smooth, V* flow, V* dst, V* tmp,
                       long stride, int w, int h, int p, int nimg, const V* kcontrast, const float* tau, int nsteps)
{
    if (nsteps < 1 || nimg < 1 || !kcontrast) return fail("nsteps < 1, nimg < 1 or no contrast factors");
    if (p % 4 || stride % 4 || (op_fast<V> && head && sp % 4)) return fail("pitch and stride must be multiples of 4");
    HakImgState* state = nullptr;
    if (op_state<V>(&state, kcontrast, nimg)) return 1;
    V taps[8];
    op_taps<V>(1.f, 2, taps);
    const int G = hak_fed_groups(nsteps, op_max_fuse<V>(), w, false);
    const int ns0 = hak_fed_group_size(nsteps, G, 0);
    V* dst0 = (G % 2 == 1) ? dst : tmp;
    int rc = 0;
    const bool ok = head ? hak_launch_fed_sf_head(nullptr, src, HakOct{sw, sh, sp, (long)sh * sp}, smooth, flow, dst0, stride,
                                                  HakOct{w, h, p, (long)h * p}, nimg, taps, HAK_PM_G2, tau, ns0, state, 0, G > 1)
                         : hak_launch_fed_sf(nullptr, src, smooth, flow, dst0, stride, w, h, p, nimg, taps, HAK_PM_G2, tau, ns0, state, 0, G > 1);
    if (!ok) rc = fail(std::string(who) + ": k_fed_sf does not cover this case");
    else op_fed_groups<V>(dst0, flow, dst, tmp, stride, w, h, p, nimg, tau, nsteps, G, 1, ns0);
    const hipError_t e = hipDeviceSynchronize();
    // (the float operator has always reported a failed kernel as "kernel", its twin by the error's name)
    if (e != hipSuccess && !rc) rc = fail(std::string(who) + ": " + (op_fast<V> ? hipGetErrorString(e) : "kernel"));
    (void)hipFree(state);
    return rc;
}
extern "C" int hak_op_fed_cycle(const float* src, int head, int sw, int sh, int sp, float* smooth, float* flow, float* dst, float* tmp,
                                long stride, int w, int h, int p, int nimg, const float* kcontrast, const float* tau, int nsteps)
{ return fed_cycle_t("hak_op_fed_cycle", src, head, sw, sh, sp, smooth, flow, dst, tmp, stride, w, h, p, nimg, kcontrast, tau, nsteps); }
extern "C" int hak_op_fast_fed_cycle(const int* src, int head, int sw, int sh, int sp, int* smooth, int* flow, int* dst, int* tmp,
                                     long stride, int w, int h, int p, int nimg, const int* kcontrast, const float* tau, int nsteps)
{ return fed_cycle_t("hak_op_fast_fed_cycle", src, head, sw, sh, sp, smooth, flow, dst, tmp, stride, w, h, p, nimg, kcontrast, tau, nsteps); }

// The octave-0 prologue on the caller's planes: Lt, the gradient scratch and the sigma = 1 plane lie in ONE allocation, as in the arena
// (the streaming kernels address their output planes as 32-bit offsets from the lower one and decline planes that lie too far apart).
// Routes 1 and 2 write d_lt and d_grad, route 3 d_lt and d_smooth; the third plane is not touched.
extern "C" int hak_op_fast_base_planes(const unsigned char* img, int sp, int* Lt, int* grad, int* smooth, int w, int h, int p, float var_base,
                                       int radius, float per, int* kc, int* hmax, int* hist, int* route)
{
    if (radius < 1 || radius > 5) return fail("radius must be 1..5");
    if (p % 4) return fail("pitch must be a multiple of 4");
    if (!Lt || !grad || !smooth) return fail("null plane");
    int taps1[8], tapsb[8];
    op_taps<int>(1.f, 2, taps1);
    op_taps<int>(var_base, radius, tapsb);
    const HakKnobs kn = hak_knobs_from_env();
    HakImgState* st = nullptr;
    HIP_TRY(hipMalloc((void**)&st, sizeof(HakImgState)));
    (void)hipMemset(st, 0, sizeof(HakImgState));
    hak_launch_reset_state(nullptr, st, 1);
    const bool based = hak_launch_base_level(nullptr, img, 0, sp, Lt, grad, 0, w, h, p, 1, taps1, tapsb, radius, st, per, 1, kn);
    if (!based) {                                                                 // hak_sequence.hip build_level, akaze.cpp:589-623
        hak_launch_lowpass(nullptr, img, 0, sp, smooth, 0, w, h, p, 1, taps1, 2);
        hak_launch_contrast(nullptr, smooth, 0, w, h, p, 1, st, per, 1);
        hak_launch_lowpass(nullptr, img, 0, sp, Lt, 0, w, h, p, 1, tapsb, radius);
    }
    // which kernel hak_launch_base_level took: the cover of launch_base_stream (kernels_base_stream.hip; its plane-distance clauses
    // do not trip on planes of one allocation)
    const bool streamed = radius >= 2 && radius <= 4 && (w & 3) == 0 && w >= 16 && h >= 16 && sp % 4 == 0 &&
                          reinterpret_cast<uintptr_t>(img) % 4 == 0 && hak_stream_pays(kn.base_stream, w, h, 1);
    if (route) *route = !based ? 3 : streamed ? 1 : 2;
    return op_state_result<int>("FAST contrast", st, w, h, kc, hmax, hist);
}
extern "C" int hak_op_fast_base(const unsigned char* img, int sp, int* lt, int w, int h, int p, float var_base, int radius, float per,
                                int* kc, int* hmax, int* hist, int* route)
{
    if (radius < 1 || radius > 5) return fail("radius must be 1..5");
    if (p % 4) return fail("pitch must be a multiple of 4");
    const size_t plane = (size_t)h * p;
    int* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, sizeof(int) * 3 * plane));
    int rc = hak_op_fast_base_planes(img, sp, buf, buf + plane, buf + 2 * plane, w, h, p, var_base, radius, per, kc, hmax, hist, route);
    // (the w columns of every row: the pad columns of the caller's plane are not the operator's to write)
    if (!rc && hipMemcpy2D(lt, sizeof(int) * p, buf, sizeof(int) * p, sizeof(int) * w, h, hipMemcpyDeviceToDevice) != hipSuccess)
        rc = fail("hak_op_fast_base: copy");
    (void)hipFree(buf);
    return rc;
}

extern "C" int hak_op_fast_level_tile(const int* src, int head, int sw, int sh, int sp, int* smooth, int* dst, int* tmp, long stride,
                                      int w, int h, int p, int nimg, int diffusivity, const int* kcontrast, const float* tau, int nsteps,
                                      int* launches)
{
    if (nsteps < 1 || nimg < 1 || !kcontrast) return fail("nsteps < 1, nimg < 1 or no contrast factors");
    if (p % 4 || stride % 4 || (head && sp % 4)) return fail("pitch and stride must be multiples of 4");      // (the kernel stores 16-byte groups)
    if (head && (w != sw / 2 || h != sh / 2)) return fail("an octave head halves the source extents");
    HakImgState* state = nullptr;
    if (op_state<int>(&state, kcontrast, nimg)) return 1;
    int taps[8];
    op_taps<int>(1.f, 2, taps);
    const HakOct dd{w, h, p, (long)h * p};
    const int nl = hak_launch_level_tile(nullptr, src, head ? HakOct{sw, sh, sp, (long)sh * sp} : dd, head != 0, smooth, dst, tmp, stride, dd,
                                         nimg, taps, diffusivity, tau, nsteps, state, 0);
    if (launches) *launches = nl;
    const int rc = op_sync("hak_op_fast_level_tile");
    (void)hipFree(state);
    return rc;
}

// Hessian of one level of `nimg` images on the caller's planes: the source, the interleaved {Lx, Ly} plane (2 h p elements) and the
// determinant of image i lie `stride` elements behind image i-1's, all in ONE allocation (see hak_op_fast_base_planes).
// route: 1 streaming, 2 tile kernel, 3 unfused pair
template <typename V>
static int hessian_planes_t(const char* who, const V* s, V* dxy, V* det, long stride, int w, int h, int p, int nimg, int step, int* route)
{
    if (nimg < 1 || step < 1 || p % 4 || p < w || stride % 4) return fail(std::string(who) + ": nimg < 1, step < 1 or a bad pitch or stride");
    if (!s || !dxy || !det) return fail(std::string(who) + ": null plane");
    const HakKnobs kn = hak_knobs_from_env();
    const V thr = 0;
    const bool fused = hak_launch_hessian_level(nullptr, s, dxy, det, true, stride, w, h, p, nimg, step, nullptr, nullptr, nullptr, 0, 0, thr);
    // launch_hessian_level_t (kernels_hessian.hip): streaming where it pays and covers, else the tile kernel up to dilation 4
    if (route) *route = !fused ? 3 : (hak_stream_pays(kn.hess_stream, w, h, nimg) && hak_hessian_stream_covers(w, h, step, false)) ? 1 : 2;
    int rc = op_sync(who);
    if (!rc && fused != (step <= 4)) rc = fail(std::string(who) + ": unexpected route");
    return rc;
}
extern "C" int hak_op_hessian_planes(const float* s, float* dxy, float* det, long stride, int w, int h, int p, int nimg, int step, int* route)
{ return hessian_planes_t("hak_op_hessian_planes", s, dxy, det, stride, w, h, p, nimg, step, route); }
extern "C" int hak_op_fast_hessian_planes(const int* s, int* dxy, int* det, long stride, int w, int h, int p, int nimg, int step, int* route)
{ return hessian_planes_t("hak_op_fast_hessian_planes", s, dxy, det, stride, w, h, p, nimg, step, route); }

// ... and into the reference's three dense planes (the kernels write the derivatives interleaved, HakLayout), on a batch of either
// element type.  Per image the slot of the operator's own allocation holds the interleaved derivatives, the determinant and then the
// source plane: the last image's last source row ends the allocation, as an image's last row ends the caller's buffer when its
// pitch is its width (tests/test_gpu_strip_seams.py).
template <typename V>
static int hessian_batch_t(const char* who, const V* s, V* lx, V* ly, V* det, int w, int h, int p, int nimg, int step, int* route, bool any_step)
{
    if (nimg < 1 || step < 1 || p % 4 || p < w) return fail(std::string(who) + ": nimg < 1, step < 1 or a bad pitch");
    const size_t plane = (size_t)h * p;
    const long stride = 4 * (long)plane;
    V* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, sizeof(V) * (size_t)stride * nimg));
    int rc = 0, rt = 0;
    if (hipMemcpy2D(buf + 3 * plane, sizeof(V) * stride, s, sizeof(V) * plane, sizeof(V) * plane, nimg, hipMemcpyDeviceToDevice) != hipSuccess)
        rc = fail(std::string(who) + ": copy in");
    if (!rc) rc = hessian_planes_t(who, buf + 3 * plane, buf, buf + 2 * plane, stride, w, h, p, nimg, step, &rt);
    if (!rc && rt == 3 && !any_step) rc = fail(std::string(who) + ": the fused kernels do not cover this dilation");
    if (route) *route = rt;
    for (int i = 0; i < nimg && !rc; i++)
        hak_launch_deinterleave(nullptr, reinterpret_cast<const float*>(buf + i * stride), reinterpret_cast<float*>(lx + i * plane),
                                reinterpret_cast<float*>(ly + i * plane), w, h, p);
    if (!rc) rc = op_sync(who);
    // (the w columns of every row: the pad columns of the caller's planes are not the operator's to write)
    for (int i = 0; i < nimg && !rc; i++)
        if (hipMemcpy2D(det + i * plane, sizeof(V) * p, buf + i * stride + 2 * plane, sizeof(V) * p, sizeof(V) * w, h, hipMemcpyDeviceToDevice) != hipSuccess)
            rc = fail(std::string(who) + ": copy out");
    (void)hipFree(buf);
    return rc;
}
extern "C" int hak_op_hessian(const float* s, float* lx, float* ly, float* det, int w, int h, int p, int step)
{ return hessian_batch_t<float>("hak_op_hessian", s, lx, ly, det, w, h, p, 1, step, nullptr, true); }
extern "C" int hak_op_fast_hessian(const int* s, int* lx, int* ly, int* det, int w, int h, int p, int step, int* route)
{ return hessian_batch_t<int>("hak_op_fast_hessian", s, lx, ly, det, w, h, p, 1, step, route, true); }
extern "C" int hak_op_hessian_batch(const float* s, float* lx, float* ly, float* det, int w, int h, int p, int nimg, int step, int* route)
{ return hessian_batch_t<float>("hak_op_hessian_batch", s, lx, ly, det, w, h, p, nimg, step, route, false); }
extern "C" int hak_op_fast_hessian_batch(const int* s, int* lx, int* ly, int* det, int w, int h, int p, int nimg, int step, int* route)
{ return hessian_batch_t<int>("hak_op_fast_hessian_batch", s, lx, ly, det, w, h, p, nimg, step, route, false); }

// ---- detector tail / descriptors on hand-made inputs (include/hipakaze.h; tests/test_gpu_literal.py)
static HakBatch tail_batch(hak_ctx* c)
{
    // (with the context's permutation buffer, as level_args of the launch sequence: HAK_DESC_SORT reaches the descriptor stages)
    HakBatch b{c->arena, c->L.arena, 1, c->state, c->maps, c->L.oct[0].plane, c->bitmap, c->rowcount, c->cand, c->cand_cap, &c->knobs,
               c->perm, c->cfg.max_pts};
    hak_batch_selection(c, b);                                      // (hak_op_tail_finish selects like the detect entry points)
    return b;
}
static int tail_level_ok(hak_ctx* c, int o, int s, const void* h)
{
    if (!c || !h) return fail("null argument");
    if (o < 0 || o >= c->L.noct || s < 0 || s >= c->L.ms) return fail("bad level");
    return 0;
}

extern "C" int hak_debug_set_plane(hak_ctx* c, int img, int kind, int o, int s, const float* h_src)
{
    if (tail_level_ok(c, o, s, h_src)) return 1;
    if (img < 0 || img >= c->cfg.batch) return fail("bad image index");
    const HakLayout& L = c->L;
    const HakOct oc = L.oct[o];
    HIP_TRY(hipStreamSynchronize(c->stream));
    float* arena = c->arena + (long)img * L.arena;
    if (kind == HAK_PLANE_LT) {
        HIP_TRY(hipMemcpy2D(arena + L.lt(o, s), sizeof(float) * oc.p, h_src, sizeof(float) * oc.w, sizeof(float) * oc.w, oc.h, hipMemcpyHostToDevice));
        return 0;
    }
    if (kind != HAK_PLANE_LX && kind != HAK_PLANE_LY) return fail("only the Lt, Lx and Ly planes can be set");
    // element (y, x) of the interleaved plane = {Lx, Ly} at 2 * (y * p + x): a strided 2-D copy of single floats
    float* dst = arena + L.dxy(o, s) + (kind == HAK_PLANE_LY ? 1 : 0);
    for (int y = 0; y < oc.h; y++)
        HIP_TRY(hipMemcpy2D(dst + 2L * y * oc.p, 2 * sizeof(float), h_src + (long)y * oc.w, sizeof(float), sizeof(float), oc.w, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int hak_op_tail_begin(hak_ctx* c)
{
    if (!c) return fail("null context");
    c->last_fast = false;
    c->sync_stream = c->stream;
    maps_guard_begin(c);                                            // (stays set until hak_op_tail_finish has cleaned the map)
    hak_launch_reset_state(c->stream, c->state, 1);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int hak_op_tail_level(hak_ctx* c, int o, int s, const float* h_src)
{
    if (tail_level_ok(c, o, s, h_src)) return 1;
    const HakLayout& L = c->L;
    const HakOct oc = L.oct[o];
    float* A = c->arena;
    float* smooth = A + L.smooth_off[o];
    HIP_TRY(hipMemcpy2D(smooth, sizeof(float) * oc.p, h_src, sizeof(float) * oc.w, sizeof(float) * oc.w, oc.h, hipMemcpyHostToDevice));
    HakBatch b = tail_batch(c);
    const int step = c->plan[(size_t)o * L.ms + s].sigma_size;
    if (!hak_launch_hessian_level(c->stream, smooth, A + L.dxy(o, s), A + L.flow_off[o], false, L.arena, oc.w, oc.h, oc.p, 1, step, &b, &L,
                                  &c->htab, o, s, c->cfg.dthreshold))
        hak_launch_extrema_level(c->stream, b, L, &c->htab, o, s, c->cfg.dthreshold, L.flow_off[o]);
    if (hipGetLastError() != hipSuccess) return fail("tail level launch failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int hak_op_tail_det_level(hak_ctx* c, int o, int s, const float* h_det)
{
    if (tail_level_ok(c, o, s, h_det)) return 1;
    const HakLayout& L = c->L;
    const HakOct oc = L.oct[o];
    HIP_TRY(hipMemcpy2D(c->arena + L.flow_off[o], sizeof(float) * oc.p, h_det, sizeof(float) * oc.w, sizeof(float) * oc.w, oc.h,
                        hipMemcpyHostToDevice));
    hak_launch_extrema_level(c->stream, tail_batch(c), L, &c->htab, o, s, c->cfg.dthreshold, L.flow_off[o]);
    if (hipGetLastError() != hipSuccess) return fail("extrema launch failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the `int` twins of the two operators above, for the FAST path's planes (fastakaze::gCalcExtremaMap akazed.cu:3476): the same two
// launchers through their `int` overloads, with the threshold as an argument (the launch sequence passes 65, dthreshold_of<int>)
// (a negative threshold would let negative responses into the key map, whose unsigned word order holds for positive ones only:
// refused, as hak_create refuses a negative dthreshold)
static int fast_threshold_ok(int threshold) { return threshold < 0 ? fail("the integer threshold must be >= 0: the key map orders positive responses only") : 0; }

extern "C" int hak_op_fast_tail_level(hak_ctx* c, int o, int s, const int* h_src, int threshold)
{
    if (tail_level_ok(c, o, s, h_src)) return 1;
    if (fast_threshold_ok(threshold)) return 1;
    const HakLayout& L = c->L;
    const HakOct oc = L.oct[o];
    int* A = reinterpret_cast<int*>(c->arena);
    int* smooth = A + L.smooth_off[o];
    HIP_TRY(hipMemcpy2D(smooth, sizeof(int) * oc.p, h_src, sizeof(int) * oc.w, sizeof(int) * oc.w, oc.h, hipMemcpyHostToDevice));
    HakBatch b = tail_batch(c);
    const int step = c->plan[(size_t)o * L.ms + s].sigma_size;
    if (!hak_launch_hessian_level(c->stream, smooth, A + L.dxy(o, s), A + L.flow_off[o], false, L.arena, oc.w, oc.h, oc.p, 1, step, &b, &L,
                                  &c->htab, o, s, threshold))
        hak_launch_extrema_level(c->stream, b, L, &c->htab, o, s, threshold, L.flow_off[o]);
    if (hipGetLastError() != hipSuccess) return fail("FAST tail level launch failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int hak_op_fast_tail_det_level(hak_ctx* c, int o, int s, const int* h_det, int threshold)
{
    if (tail_level_ok(c, o, s, h_det)) return 1;
    if (fast_threshold_ok(threshold)) return 1;
    const HakLayout& L = c->L;
    const HakOct oc = L.oct[o];
    HIP_TRY(hipMemcpy2D(reinterpret_cast<int*>(c->arena) + L.flow_off[o], sizeof(int) * oc.p, h_det, sizeof(int) * oc.w, sizeof(int) * oc.w, oc.h,
                        hipMemcpyHostToDevice));
    hak_launch_extrema_level(c->stream, tail_batch(c), L, &c->htab, o, s, threshold, L.flow_off[o]);
    if (hipGetLastError() != hipSuccess) return fail("FAST extrema launch failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// The extrema stage by itself, between hak_op_tail_begin and hak_op_tail_finish: image 0's key map as dense w x h response words
// and layers (an empty pixel: word 0, layer -1), the first min(ncand, cand_cap) words of its candidate list in the kernels'
// arrival order (layer << 32 | y << 16 | x), the list's capacity and the number of candidates the kernels counted.  Every output
// pointer may be NULL; h_cand holds cand_cap words (ask for the capacity first, with h_cand == NULL).
extern "C" int hak_debug_tail_maps(hak_ctx* c, unsigned int* h_resp_bits, int* h_layer, unsigned long long* h_cand, long* cand_cap_out,
                                   int* ncand_out)
{
    if (!c) return fail("null context");
    const HakOct oc = c->L.oct[0];
    HIP_TRY(hipStreamSynchronize(c->stream));
    HakImgState hs;
    HIP_TRY(hipMemcpy(&hs, c->state, sizeof(hs), hipMemcpyDeviceToHost));
    if (ncand_out) *ncand_out = hs.ncand;
    if (cand_cap_out) *cand_cap_out = c->cand_cap;
    if (h_resp_bits || h_layer) {
        std::vector<unsigned long long> keys((size_t)oc.w * oc.h);
        HIP_TRY(hipMemcpy2D(keys.data(), sizeof(unsigned long long) * oc.w, c->maps, sizeof(unsigned long long) * oc.p,
                            sizeof(unsigned long long) * oc.w, oc.h, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < keys.size(); i++) {                                // hak_ext_key (hak_internal.h)
            if (h_resp_bits) h_resp_bits[i] = (unsigned)(keys[i] >> 32);
            if (h_layer) h_layer[i] = keys[i] ? (int)(0xFFFFFFFFu - (unsigned)keys[i]) : -1;
        }
    }
    if (h_cand) {
        long n = hs.ncand < 0 ? 0 : hs.ncand;
        n = n < c->cand_cap ? n : c->cand_cap;
        if (n > 0) HIP_TRY(hipMemcpy(h_cand, c->cand, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return 0;
}

// survivors of image 0's last NMS before the clamp to max_pts (k_row_scan: total_pts); after hak_op_tail_finish
extern "C" int hak_debug_tail_total(hak_ctx* c, int* total)
{
    if (!c || !total) return fail("null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HakImgState hs;
    HIP_TRY(hipMemcpy(&hs, c->state, sizeof(hs), hipMemcpyDeviceToHost));
    *total = hs.total_pts;
    return 0;
}

extern "C" int hak_op_tail_seed(hak_ctx* c, const unsigned int* h_resp_bits, const int* h_layer)
{
    if (!c || !h_resp_bits || !h_layer) return fail("null argument");
    const size_t n = (size_t)c->L.oct[0].w * c->L.oct[0].h;
    unsigned* d_r = nullptr;
    int* d_l = nullptr;
    HIP_TRY(hipMalloc((void**)&d_r, sizeof(unsigned) * n));
    int rc = 0;
    if (hipMalloc((void**)&d_l, sizeof(int) * n) != hipSuccess) rc = fail("seed scratch");
    if (!rc && (hipMemcpy(d_r, h_resp_bits, sizeof(unsigned) * n, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_l, h_layer, sizeof(int) * n, hipMemcpyHostToDevice) != hipSuccess)) rc = fail("seed upload");
    if (!rc) {
        hak_launch_seed_maps(c->stream, tail_batch(c), c->L, d_r, d_l);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail("seed kernel");
    }
    (void)hipFree(d_r); (void)hipFree(d_l);
    return rc;
}

extern "C" int hak_op_tail_finish(hak_ctx* c, hak_point* d_points, int max_pts, int refine, int fast, int* num_pts)
{
    if (!c || !d_points || !num_pts || max_pts < 1) return fail("bad argument");
    hak_launch_nms_emit(c->stream, tail_batch(c), c->L, c->dtab, c->psz, d_points, max_pts, c->d_num, fast ? 1 : 0, refine ? 1 : 0);
    hak_launch_clear_maps(c->stream, tail_batch(c), c->L);
    int rc = hipGetLastError() != hipSuccess ? fail("tail finish launch failed") : 0;
    if (!rc && hipMemcpyAsync(c->h_num, c->d_num, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail("count download");
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail("sync");
    if (!rc) *num_pts = c->h_num[0];
    return maps_guard_end(c, rc);
}

extern "C" int hak_op_orient_describe(hak_ctx* c, hak_point* d_points, int n, int desc)
{
    if (!c || !d_points || n < 1) return fail("bad argument");
    HIP_TRY(hipMemcpy(&c->state[0].num_pts, &n, sizeof(int), hipMemcpyHostToDevice));
    // desc == 2: the MLDB kernel alone, rotated by the angles the records already hold
    hak_launch_describe(c->stream, tail_batch(c), c->L, c->dtab, d_points, n, c->cfg.descriptor_pattern_size, c->cfg.upright, desc ? 1 : 0,
                        c->htab.dsc_plan_ok, desc == 2 ? 0 : 1);
    if (hipGetLastError() != hipSuccess) return fail("describe launch failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the FAST twin: k_orient<int> (refinement akazed.cu:3600 + orientation 3649) and the MLDB kernel (3723) on int32 planes, which go in
// through hak_debug_set_plane as bit patterns.  Upright contexts still run k_orient<int>, for the refinement alone.
extern "C" int hak_op_fast_orient_describe(hak_ctx* c, hak_point* d_points, int n, int desc)
{
    if (!c || !d_points || n < 1) return fail("bad argument");
    HIP_TRY(hipMemcpy(&c->state[0].num_pts, &n, sizeof(int), hipMemcpyHostToDevice));
    hakf_launch_describe(c->stream, tail_batch(c), c->L, c->dtab, d_points, n, c->cfg.descriptor_pattern_size, c->cfg.upright, desc ? 1 : 0,
                         c->htab.dsc_plan_ok);
    if (hipGetLastError() != hipSuccess) return fail("FAST describe launch failed");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int hak_op_copy_probe(long bytes, int iters, double* gbytes_per_s)
{
    if (bytes < 16 || iters < 1 || !gbytes_per_s) return fail("bad probe argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    bytes &= ~15L;
    double ms = 0;
    if (hak_launch_copy_probe(bytes, iters, &ms) || ms <= 0) return fail("copy probe failed");
    *gbytes_per_s = 2.0 * (double)bytes / (ms * 1e-3) / 1e9;                      // read + write
    return 0;
}

extern "C" int hak_op_copy_probe_shapes(long bytes, int iters, double* gbytes_per_s, int n)
{
    if (bytes < 16 || iters < 1 || !gbytes_per_s || n < HAK_COPY_SHAPES) return fail("bad probe argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    bytes &= ~15L;
    double best = 0, ms[HAK_COPY_SHAPES] = {};
    if (hak_launch_copy_probe(bytes, iters, &best, ms)) return fail("copy probe failed");
    for (int i = 0; i < HAK_COPY_SHAPES; i++) {
        const double moved = i < HAK_COPY_SHAPES - 2 ? 2.0 * (double)bytes : (double)bytes;     // copy: read + write
        gbytes_per_s[i] = ms[i] > 0 ? moved / (ms[i] * 1e-3) / 1e9 : 0.0;
    }
    return HAK_COPY_SHAPES;
}

extern "C" int hak_op_stream_probe(int w, int h, int nimg, int nwrite, int warm_rows, int iters, double* ms_per_launch, double* gbytes_per_s)
{
    if (!ms_per_launch || !gbytes_per_s) return fail("null argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    double ms = 0, bytes = 0;
    if (hak_launch_stream_probe(w, h, nimg, nwrite, warm_rows, iters, &ms, &bytes) || ms <= 0) return fail("stream probe failed (w % 4, sizes, memory?)");
    *ms_per_launch = ms;
    *gbytes_per_s = bytes / (ms * 1e-3) / 1e9;
    return 0;
}

extern "C" int hak_op_hess_probe(int w, int h, int nimg, int step, int iters, double* ms_per_launch, double* gbytes_per_s)
{
    if (!ms_per_launch || !gbytes_per_s) return fail("null argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    double ms = 0, bytes = 0;
    if (hak_launch_hess_probe(w, h, nimg, step, iters, &ms, &bytes) || ms <= 0) return fail("hessian probe failed (w % 4, step 1..4, sizes, memory?)");
    *ms_per_launch = ms;
    *gbytes_per_s = bytes / (ms * 1e-3) / 1e9;
    return 0;
}

extern "C" int hak_op_gather_probe(long bytes, int blocks, int per_lane, int iters, double* ms_per_launch)
{
    if (bytes < 4096 || blocks < 1 || per_lane < 4 || iters < 1 || !ms_per_launch) return fail("bad probe argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    if (hak_launch_gather_probe(bytes & ~127L, blocks, per_lane & ~3, iters, ms_per_launch)) return fail("gather probe failed");
    return 0;
}

// the sliced matcher's per-slice summaries filled with `byte` on the context's stream (tests/stress_handoff.py: a stale read of a
// summary is only visible when the scratch does not already hold the same launch's values from the call before)
extern "C" int hak_debug_fill_match_scratch(hak_ctx* c, int byte)
{
    if (!c) return fail("null context");
    if (c->msc.part && c->msc.part_cap > 0) HIP_TRY(hipMemsetAsync(c->msc.part, byte, sizeof(uint2) * (size_t)c->msc.part_cap, c->stream));
    return 0;
}

// the launch shape both RANSAC estimators take for (npairs, iterations): hak_homography_blocks and nothing else, no device
extern "C" int hak_op_ransac_shape(int npairs, int iterations, int* hp, int* hblocks)
{
    if (!hp || !hblocks) return fail("null argument");
    if (npairs < 1 || iterations < 1 || iterations > 65536) return fail("npairs must be >= 1 and iterations in 1 .. 65536");
    *hblocks = hak_homography_blocks(npairs, iterations, hp);
    return 0;
}

// the launch plan of a matcher call: hak_match_plan with the environment's knobs and nothing else, no device
extern "C" int hak_op_match_shape(int search, int n1, int n2, int npairs, int device_counts, int capacity, int scratch, int* plan)
{
    if (!plan) return fail("null argument");
    if (search < 0 || search > 1 || n1 < 0 || n2 < 0 || npairs < 1 || capacity < 0) return fail("search must be 0 or 1, counts >= 0, npairs >= 1");
    // (with device-side counts the launchers see the capacity in the place of both counts)
    const HakMatchPlan p = hak_match_plan(hak_match_knobs_from_env(), search, device_counts != 0, device_counts ? capacity : n1,
                                          device_counts ? capacity : n2, npairs, scratch != 0);
    const int v[7] = {p.kernel, p.qt, p.gx, p.slices, p.rows_per_slice, p.chunks_per_slice, p.finish_blocks};
    memcpy(plan, v, sizeof(v));
    return 0;
}

// the RANSAC scratch of the last H, F or P3P call on the context, as that call left it: the models words [pair][word][iterations]
// (ransac_common.h) as they lie, and every score block's slot decoded here by rs_decode's rule, so that no test restates the key.
// Launches nothing.
extern "C" int hak_debug_ransac_scratch(hak_ctx* c, int npairs, int words_per_hypothesis, int iterations, int hblocks,
                                        unsigned* h_models, int* h_slots)
{
    if (!c) return fail("null context");
    if (npairs < 1 || words_per_hypothesis < 0 || iterations < 1 || iterations > 65536 || hblocks < 1)
        return fail("npairs, iterations and hblocks must be >= 1, words_per_hypothesis >= 0, iterations <= 65536");
    const long words = (long)npairs * words_per_hypothesis * iterations, slots = (long)npairs * hblocks;
    if (!h_slots || (words > 0 && !h_models)) return fail("null output");
    if (words > c->ransac_models_cap || slots > c->ransac_slots_cap) return fail("more than the context's RANSAC scratch holds");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (words > 0) HIP_TRY(hipMemcpy(h_models, c->ransac_models, sizeof(unsigned) * (size_t)words, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> keys((size_t)slots);
    HIP_TRY(hipMemcpy(keys.data(), c->ransac_slots, sizeof(unsigned long long) * (size_t)slots, hipMemcpyDeviceToHost));
    for (long k = 0; k < slots; k++) {
        const unsigned long long key = keys[(size_t)k];
        const unsigned id = ~(unsigned)key;                             // 4 h + r
        h_slots[3 * k] = (int)(key >> 32);
        h_slots[3 * k + 1] = key != 0 ? (int)(id >> 2) : -1;
        h_slots[3 * k + 2] = key != 0 ? (int)(id & 3u) : 0;
    }
    return 0;
}

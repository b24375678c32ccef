// pixel_rules.h -- the per-pixel rules of the scale space, stated once for both pipelines: V = float (akaze) and V = int
// (fastakaze, 16.16 fixed point on int32 planes).  Every kernel that filters, differentiates, bins or diffuses a pixel takes its
// arithmetic from here; each rule is bit-exact against the oracle and EVALUATION ORDER IS THE CONTRACT: the float forms keep the
// reference's source order (the library is built with -ffp-contract=off), the int forms wrap in two's complement exactly as the
// reference's int32 arithmetic does (F1 of the FAST parity oracle).  Included by hak_internal.h (needs HakImgState, hak_expf).
#pragma once
#include "hak_internal.h"

// ---- element arithmetic.  int: unsigned add / mul / sub, so every regrouping that is exact for wrapping integers stays exact
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float vsub(float a, float b) { return a - b; }
__device__ __forceinline__ float vmul(float a, float b) { return a * b; }
__device__ __forceinline__ float vneg(float a) { return -a; }
__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int vadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int vsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int vmul(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ __forceinline__ int vneg(int a) { return (int)(0u - (unsigned)a); }
__device__ __forceinline__ int vmax(int a, int b) { return max(a, b); }
// the end of a weighted sum: every 16.16 sum is followed by >> 16 (akazed.cu:2922-2985, 3339-3403)
__device__ __forceinline__ float vfix(float a) { return a; }
__device__ __forceinline__ int vfix(int a) { return a >> 16; }
// a float weight as 16.16 (taps akazed.cu:3896, derivative factors 4183-4184, conductivity 3444)
__host__ __device__ __forceinline__ int hak_fix16(float f) { return (int)(f * 65536 + 0.5f); }

// ---- reflect-101 as the reference: left/top abs(i), right/bottom borderAdd (akazed.cu:162-170).  A decimated coordinate d mirrors
// on the SOURCE extent as hak_refl(2 * d, source extent) (akazed.cu:466, 477-494)
__device__ __forceinline__ int hak_refl(int i, int m)
{
    i = i < 0 ? -i : i;
    i = i < m ? i : m + m - 2 - i;
    // tiles hanging over the image can index past one reflection; those values are never used
    i = i < 0 ? 0 : i;
    return i < m ? i : m - 1;
}

// ---- separable Gaussian, one pass (gConv2d<R> akazed.cu:227-239, 283-288; fastakaze 2922-2985; gDownWithSmooth 469-471, 507-509):
// k0 * c, then + k_i * (a_-i + a_+i) for i = 1..R in that order, then vfix.  k[i]: the taps, at(i): the sample at offset i
template <int R, typename K, typename F>
__device__ __forceinline__ auto hak_conv(const K& k, F at) -> decltype(at(0))
{
    auto ws = vmul(k[0], at(0));
#pragma unroll
    for (int i = 1; i <= R; i++) ws = vadd(ws, vmul(k[i], at(-i) + at(i)));
    return vfix(ws);
}
// the sigma=1 pass (R = 2) on five named samples: centre, the pair at distance 1, the pair at distance 2
template <typename V> struct SfTaps { V k0, k1, k2; };
template <typename V>
__device__ __forceinline__ V hak_conv5(V c, V a1, V b1, V a2, V b2, const SfTaps<V>& t)
{
    return vfix(vadd(vadd(vmul(c, t.k0), vmul(t.k1, a1 + b1)), vmul(t.k2, a2 + b2)));
}

// ---- un-normalised Scharr pair of a 3 x 3 neighbourhood (akazed.cu:664-665, 1088-1089; fastakaze 3208-3232, 3406-3428)
template <typename V>
__device__ __forceinline__ void hak_scharr(V ul, V uc, V ur, V cl, V cr, V ll, V lc, V lr, V& dx, V& dy)
{
    dx = 10 * (cr - cl) + 3 * (ur + lr - ul - ll);
    dy = 10 * (lc - uc) + 3 * (ll + lr - ul - ur);
}
// ... of plane pixel (x, y), neighbours at reflect-101 indices (abs / borderAdd, akazed.cu:1078-1081)
template <typename V>
__device__ __forceinline__ void hak_scharr_at(const V* __restrict__ s, int x, int y, int w, int h, int p, V& dx, V& dy)
{
    const int x0 = x - 1 < 0 ? 1 - x : x - 1, x2 = x + 1 < w ? x + 1 : w + w - 3 - x;
    const int y0 = y - 1 < 0 ? 1 - y : y - 1, y2 = y + 1 < h ? y + 1 : h + h - 3 - y;
    const V* r0 = s + (long)y0 * p;
    const V* r1 = s + (long)y * p;
    const V* r2 = s + (long)y2 * p;
    hak_scharr(r0[x0], r0[x], r0[x2], r1[x0], r1[x2], r2[x0], r2[x], r2[x2], dx, dy);
}
// gradient magnitude (akazed.cu:666; fastakaze 3232: wrapped sum of squares, rounded square root)
__device__ __forceinline__ float hak_grad_mag(float dx, float dy) { return sqrtf(dx * dx + dy * dy); }
__device__ __forceinline__ int hak_grad_mag(int dx, int dy) { return (int)(sqrtf((float)vadd(vmul(dx, dx), vmul(dy, dy))) + 0.5f); }

// ---- hScharrContrast's histogram (akazed.cu:901-938 / 3299-3336).  The lattice maximum of an image as V ...
template <typename V> __device__ __forceinline__ V hak_state_hmax(const HakImgState* st);
template <> __device__ __forceinline__ float hak_state_hmax<float>(const HakImgState* st) { return __uint_as_float(st->hmax_bits); }
template <> __device__ __forceinline__ int hak_state_hmax<int>(const HakImgState* st) { return st->ihmax; }
// ... the per-image factor NBINS / hmax (akazed.cu:2450; as a double: the bin takes the exact double product) or its 16.16 form
// (akazed.cu:4133) ...
__device__ __forceinline__ double hak_hist_factor(float hmax) { return (double)(HAK_NBINS / hmax); }
__device__ __forceinline__ int hak_hist_factor(int hmax) { return hak_fix16(HAK_NBINS / (float)hmax); }
// ... and the bin of one magnitude.  float: (int)__fmul_rz(g, factor) = the exact double product truncated, clamped high
// (akazed.cu:924-928); int: the wrapping product >> 16, clamped both ways (akazed.cu:3319-3326)
__device__ __forceinline__ int hak_hist_bin(float g, double factor)
{
    const int hi = (int)((double)g * factor);
    return hi >= HAK_NBINS ? HAK_NBINS - 1 : hi;
}
__device__ __forceinline__ int hak_hist_bin(int g, int factor)
{
    const int hi = vmul(g, factor) >> 16;
    return hi >= HAK_NBINS ? HAK_NBINS - 1 : (hi < 0 ? 0 : hi);
}
// host half of hScharrContrast (akazed.cu:2467-2481 / 4146-4162): the first bin at which the cumulated histogram reaches the
// percentile.  hist_words: the image's 300 bins; extra0: hak_hist_extra0
__device__ __forceinline__ int hak_contrast_bin(const int* hist_words, int npix, int extra0, float per)
{
    const int thresh = (int)((npix - (hist_words[0] + extra0)) * per);     // akazed.cu:2468, 3305
    int cumuv = 0, k = 1;
    while (k < HAK_NBINS) {
        if (cumuv >= thresh) break;
        cumuv += hist_words[k];
        k++;
    }
    return k;
}
// ... then the contrast factor of every octave, kept on the device: the 0.75 decay per octave (akaze.cpp:371 / 642) and
// ikc = 1 / (k * k) (akazed.cu:2493 / 4215)
template <typename V>
__device__ __forceinline__ void hak_finish_kcontrast(HakImgState* st, const int* hist_words, int npix, int extra0, float per, int noct);
template <>
__device__ __forceinline__ void hak_finish_kcontrast<float>(HakImgState* st, const int* hist_words, int npix, int extra0, float per, int noct)
{
    const float hfactor = HAK_NBINS / hak_state_hmax<float>(st);
    float kc = hak_contrast_bin(hist_words, npix, extra0, per) / hfactor;
    for (int o = 0; o < noct; o++) {
        if (o > 0) kc *= 0.75f;
        st->kcontrast[o] = kc;
        st->ikc[o] = 1.f / (kc * kc);
    }
}
template <>
__device__ __forceinline__ void hak_finish_kcontrast<int>(HakImgState* st, const int* hist_words, int npix, int extra0, float per, int noct)
{
    int kc = hak_contrast_bin(hist_words, npix, extra0, per) * hak_state_hmax<int>(st) / HAK_NBINS;     // akazed.cu:4162
    for (int o = 0; o < noct; o++) {
        if (o > 0) kc = (int)(kc * 0.75f + 0.5f);
        st->ikcontrast[o] = kc;
        st->ikc[o] = 1.f / (kc * kc);
    }
}

// ---- conductivity (gFlowNaive akazed.cu:1090-1106 / 3430-3445): the normalised gradient energy (int: formed in wrapping int32),
// the four diffusivities, and the value as the element type (int: 16.16)
__device__ __forceinline__ float hak_dif2(float dx, float dy, float ikc) { return ikc * (dx * dx + dy * dy); }
__device__ __forceinline__ float hak_dif2(int dx, int dy, float ikc) { return (float)vadd(vmul(dx, dx), vmul(dy, dy)) * ikc; }
__device__ __forceinline__ float hak_conductivity(float dif2, int type)
{
    if (type == HAK_PM_G2) return 1.f / (1.f + dif2);
    if (type == HAK_PM_G1) return hak_expf(-dif2);
    if (type == HAK_WEICKERT) {
        const float d2 = dif2 * dif2;
        return 1.f - hak_expf(-3.315f / (d2 * d2));
    }
    return 1.f / sqrtf(1.f + dif2);
}
template <typename V> __device__ __forceinline__ V hak_g_as(float g);
template <> __device__ __forceinline__ float hak_g_as<float>(float g) { return g; }
template <> __device__ __forceinline__ int hak_g_as<int>(float g) { return hak_fix16(g); }

// ---- dilated Scharr derivative and determinant of the Hessian kernels and of the keypoint refinement (gDerivate akazed.cu:1294-1295,
// gHessianDeterminant 1326-1330; fastakaze 3339-3403: every weighted sum is followed by >> 16, the determinant is not shifted)
template <typename V> __device__ __forceinline__ V hs_d(V f1, V f2, V a, V b) { return vfix(vadd(vmul(f1, a), vmul(f2, b))); }
template <typename V> __device__ __forceinline__ V hs_det(V dxx, V dyy, V dxy) { return vsub(vmul(dxx, dyy), vmul(dxy, dxy)); }
// the factors of hak_deriv_factors as the element type (akazed.cu:4183-4184)
__host__ __device__ __forceinline__ float hak_fac_as(float f, float) { return f; }
__host__ __device__ __forceinline__ int hak_fac_as(float f, int) { return hak_fix16(f); }

// Hessian determinant of one level at (x, y), re-evaluated from the interleaved derivative plane with the expressions and
// the reflect-101 index rule of the Hessian kernels (akazed.cu:1318-1330): bit-identical to the value those kernels
// compared in their extrema test.  The determinant plane itself is never written (hak_internal.h HakLayout).
template <typename V>
__device__ __forceinline__ V hak_det_at(const V* __restrict__ dxy, int x, int y, int S, int w, int h, int p, V f1, V f2)
{
    const long x0 = hak_refl(x - S, w), x1 = x, x2 = hak_refl(x + S, w);
    const long o0 = (long)hak_refl(y - S, h) * p, o1 = (long)y * p, o2 = (long)hak_refl(y + S, h) * p;
    const V xul = dxy[2 * (o0 + x0)], xuc = dxy[2 * (o0 + x1)], xur = dxy[2 * (o0 + x2)];
    const V xcl = dxy[2 * (o1 + x0)], xcr = dxy[2 * (o1 + x2)];
    const V xll = dxy[2 * (o2 + x0)], xlc = dxy[2 * (o2 + x1)], xlr = dxy[2 * (o2 + x2)];
    const V yul = dxy[2 * (o0 + x0) + 1], yuc = dxy[2 * (o0 + x1) + 1], yur = dxy[2 * (o0 + x2) + 1];
    const V yll = dxy[2 * (o2 + x0) + 1], ylc = dxy[2 * (o2 + x1) + 1], ylr = dxy[2 * (o2 + x2) + 1];
    const V dxx = hs_d(f1, f2, xur + xlr - xul - xll, xcr - xcl);
    const V dxy_ = hs_d(f1, f2, xlr + xll - xur - xul, xlc - xuc);
    const V dyy = hs_d(f1, f2, ylr + yll - yur - yul, ylc - yuc);
    return hs_det(dxx, dyy, dxy_);
}

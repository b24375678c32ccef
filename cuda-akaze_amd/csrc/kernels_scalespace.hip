// kernels_scalespace.hip -- nonlinear scale space for gfx950 (CDNA4, wave64), both pipelines: V = float (akaze) and V = int
// (fastakaze, akazed.cu:2781-4367: int32 planes, 16.16 fixed-point weights, uint8 input).
//
// Stages (reference wrapper -> kernel here; fastakaze lines after the slash):
//   hLowPass/gConv2d<R>            akazed.cu:2336, 204 / 2990, 2786, 2922  -> k_lowpass<In, V, R>
//   hDownWithSmooth                akazed.cu:2389, 449 / 3143              -> k_down_smooth<V>
//   hScharrContrast                akazed.cu:2410, 644, 827, 901 / 3208-3336, 4101-4162 -> k_grad_max<V>, k_grad_hist<V>, k_kcontrast<V>
//   hFlow/gFlowNaive               akazed.cu:2487, 1068 / 3406             -> k_flow<V>
//   hNldStep/gNldStepNaive         akazed.cu:2509, 1241 / 3448             -> kernels_fed.hip (the FED hot loop)
//   hHessianDeterminant            akazed.cu:2531, 1267, 1299 / 3339, 3371 -> k_derivate<V>, k_hessian<V>
//
// All kernels take the batch image in blockIdx.z.  The arithmetic of every pixel is pixel_rules.h: float evaluation order is
// the reference's source order (no contraction: built with -ffp-contract=off), int32 products wrap as in the oracle;
// the only fused op is the explicit fmaf of the FED step (akazed.cu:1263).
#include "hak_internal.h"

#define TILE_X 64
#define TILE_Y 16

// what differs between the pipelines and is not arithmetic: the taps as a kernel argument, and the state field that takes the
// lattice maximum with the smallest value that may raise it (the float field is floored at 0.03f, the int one at 1: k_reset_state)
template <typename V> struct SsT;
template <> struct SsT<float> {
    struct Taps { float k[8]; };
    static __device__ __forceinline__ void raise_max(HakImgState* st, float m) { if (m > 0.f) atomicMax(&st->hmax_bits, __float_as_uint(m)); }
};
template <> struct SsT<int> {
    struct Taps { int k[8]; };
    static __device__ __forceinline__ void raise_max(HakImgState* st, int m) { if (m > 1) atomicMax(&st->ihmax, m); }
};
template <typename V> static typename SsT<V>::Taps ss_taps(const V* taps, int R)
{
    typename SsT<V>::Taps t;
    for (int i = 0; i < 8; i++) t.k[i] = i <= R ? taps[i] : V(0);
    return t;
}
static dim3 ss_grid(int w, int h, int nimg) { return dim3((w + TILE_X - 1) / TILE_X, (h + TILE_Y - 1) / TILE_Y, nimg); }

// ------------------------------------------------------------------ lowpass
// Separable Gaussian, reflect-101.  One 64x16 output tile per 256-thread
// block: raw tile (+R halo) -> LDS, row pass -> LDS, column pass -> HBM.  In = float, or uint8 / int for int planes
template <typename In, typename V, int R>
__global__ __launch_bounds__(256) void k_lowpass(const In* __restrict__ src, long src_stride, int sp,
                                                 V* __restrict__ dst, long dst_stride,
                                                 int w, int h, int p, typename SsT<V>::Taps taps)
{
    constexpr int RW = TILE_X + 2 * R, RH = TILE_Y + 2 * R;
    __shared__ V raw[RH][RW + 1];
    __shared__ V rowp[RH][TILE_X];
    const In* s = src + (long)blockIdx.z * src_stride;
    V* d = dst + (long)blockIdx.z * dst_stride;
    const int x0 = blockIdx.x * TILE_X, y0 = blockIdx.y * TILE_Y, tid = threadIdx.x;

    for (int i = tid; i < RH * RW; i += 256) {
        int r = i / RW, c = i - r * RW;
        raw[r][c] = (V)s[(long)hak_refl(y0 - R + r, h) * sp + hak_refl(x0 - R + c, w)];
    }
    __syncthreads();
    for (int i = tid; i < RH * TILE_X; i += 256) {
        int r = i >> 6, c = i & 63;
        rowp[r][c] = hak_conv<R>(taps.k, [&](int k) { return raw[r][c + R + k]; });
    }
    __syncthreads();
    const int c = tid & 63, x = x0 + c;
    if (x >= w) return;
    for (int rr = tid >> 6; rr < TILE_Y; rr += 4) {
        int y = y0 + rr;
        if (y >= h) break;
        d[(long)y * p + x] = hak_conv<R>(taps.k, [&](int k) { return rowp[rr + R + k][c]; });
    }
}

template <typename In, typename V>
static void launch_lowpass_t(hipStream_t st, const In* src, long src_stride, int src_pitch, V* dst, long dst_stride,
                             int w, int h, int p, int nimg, const V* taps, int R)
{
    const typename SsT<V>::Taps t = ss_taps<V>(taps, R);
    const dim3 grid = ss_grid(w, h, nimg);
    switch (R) {
    case 2: k_lowpass<In, V, 2><<<grid, 256, 0, st>>>(src, src_stride, src_pitch, dst, dst_stride, w, h, p, t); break;
    case 3: k_lowpass<In, V, 3><<<grid, 256, 0, st>>>(src, src_stride, src_pitch, dst, dst_stride, w, h, p, t); break;
    case 4: k_lowpass<In, V, 4><<<grid, 256, 0, st>>>(src, src_stride, src_pitch, dst, dst_stride, w, h, p, t); break;
    default: k_lowpass<In, V, 5><<<grid, 256, 0, st>>>(src, src_stride, src_pitch, dst, dst_stride, w, h, p, t); break;
    }
}
void hak_launch_lowpass(hipStream_t st, const float* src, long src_stride, int src_pitch, float* dst, long dst_stride,
                        int w, int h, int p, int nimg, const float* taps, int R)
{ launch_lowpass_t(st, src, src_stride, src_pitch, dst, dst_stride, w, h, p, nimg, taps, R); }
void hak_launch_lowpass(hipStream_t st, const unsigned char* src, long src_stride, int src_pitch, int* dst, long dst_stride,
                        int w, int h, int p, int nimg, const int* taps, int R)
{ launch_lowpass_t(st, src, src_stride, src_pitch, dst, dst_stride, w, h, p, nimg, taps, R); }
void hak_launch_lowpass(hipStream_t st, const int* src, long src_stride, int src_pitch, int* dst, long dst_stride,
                        int w, int h, int p, int nimg, const int* taps, int R)
{ launch_lowpass_t(st, src, src_stride, src_pitch, dst, dst_stride, w, h, p, nimg, taps, R); }

// ------------------------------------------------------------ down + smooth
// dst = src[2y][2x]; smooth = G(sigma=1, R=2) on the decimated lattice with the
// mirror taken on the SOURCE extents (akazed.cu:466, 477-494).
template <typename V>
__global__ __launch_bounds__(256) void k_down_smooth(const V* __restrict__ src, V* __restrict__ dst,
                                                     V* __restrict__ smooth, long stride,
                                                     HakOct so, HakOct dd, typename SsT<V>::Taps taps)
{
    constexpr int RW = TILE_X + 4, RH = TILE_Y + 4;
    __shared__ V dec[RH][RW + 1];
    __shared__ V rowp[RH][TILE_X];
    const V* s = src + (long)blockIdx.z * stride;
    V* d = dst + (long)blockIdx.z * stride;
    V* sm = smooth + (long)blockIdx.z * stride;
    const int x0 = blockIdx.x * TILE_X, y0 = blockIdx.y * TILE_Y, tid = threadIdx.x;

    for (int i = tid; i < RH * RW; i += 256) {
        int r = i / RW, c = i - r * RW;
        int sy = hak_refl(2 * (y0 - 2 + r), so.h), sx = hak_refl(2 * (x0 - 2 + c), so.w);
        dec[r][c] = s[(long)sy * so.p + sx];
    }
    __syncthreads();
    for (int i = tid; i < RH * TILE_X; i += 256) {
        int r = i >> 6, c = i & 63;
        rowp[r][c] = hak_conv<2>(taps.k, [&](int k) { return dec[r][c + 2 + k]; });
    }
    __syncthreads();
    const int c = tid & 63, x = x0 + c;
    if (x >= dd.w) return;
    for (int rr = tid >> 6; rr < TILE_Y; rr += 4) {
        int y = y0 + rr;
        if (y >= dd.h) break;
        long o = (long)y * dd.p + x;
        d[o] = dec[rr + 2][c + 2];
        sm[o] = hak_conv<2>(taps.k, [&](int k) { return rowp[rr + 2 + k][c]; });
    }
}

template <typename V>
static void launch_down_smooth_t(hipStream_t st, const V* src, V* dst, V* smooth, long stride, HakOct so, HakOct dd, int nimg, const V* taps)
{
    k_down_smooth<V><<<ss_grid(dd.w, dd.h, nimg), 256, 0, st>>>(src, dst, smooth, stride, so, dd, ss_taps<V>(taps, 2));
}
void hak_launch_down_smooth(hipStream_t st, const float* src, float* dst, float* smooth, long stride,
                            HakOct so, HakOct dd, int nimg, const float* taps)
{ launch_down_smooth_t(st, src, dst, smooth, stride, so, dd, nimg, taps); }
void hak_launch_down_smooth(hipStream_t st, const int* src, int* dst, int* smooth, long stride,
                            HakOct so, HakOct dd, int nimg, const int* taps)
{ launch_down_smooth_t(st, src, dst, smooth, stride, so, dd, nimg, taps); }

// ------------------------------------------------------- Scharr + contrast
// every field of the image state either pipeline uses
__global__ __launch_bounds__(256) void k_reset_state(HakImgState* state)
{
    HakImgState* st = state + blockIdx.x;
    for (int i = threadIdx.x; i < HAK_NBINS; i += 256) st->hist[i] = 0;
    if (threadIdx.x == 0) {
        st->hmax_bits = __float_as_uint(0.03f);        // akazed.cu:2413
        st->ihmax = 1;                                 // akazed.cu:4101
        st->ncand = 0;
        st->total_pts = 0;
        st->num_pts = 0;
    }
}

void hak_launch_reset_state(hipStream_t st, HakImgState* state, int nimg)
{
    k_reset_state<<<nimg, 256, 0, st>>>(state);
}

// pass 1: maximum gradient magnitude over the 16-px lattice (what gFindMaxContrastU4 delivers, hak_internal.h; akazed.cu:3245-3296)
template <typename V>
__global__ __launch_bounds__(256) void k_grad_max(const V* __restrict__ smooth, long stride, int w, int h, int p,
                                                  HakImgState* state)
{
    const V* s = smooth + (long)blockIdx.z * stride;
    const int x = blockIdx.x * TILE_X + (threadIdx.x & 63);
    const int y0 = blockIdx.y * TILE_Y + (threadIdx.x >> 6);
    V m = 0;
    if (x < w)
        for (int y = y0; y < blockIdx.y * TILE_Y + TILE_Y && y < h; y += 4) {
            if (!hak_on_lattice(x, y, w, h)) continue;
            V dx, dy;
            hak_scharr_at(s, x, y, w, h, p, dx, dy);
            m = vmax(m, hak_grad_mag(dx, dy));
        }
    for (int o = 32; o > 0; o >>= 1) m = vmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) SsT<V>::raise_max(state + blockIdx.z, m);
}

// pass 2: 300-bin histogram, gradient recomputed (cheaper than storing it)
template <typename V>
__global__ __launch_bounds__(256) void k_grad_hist(const V* __restrict__ smooth, long stride, int w, int h, int p,
                                                   HakImgState* state)
{
    __shared__ int shist[HAK_NBINS];
    for (int i = threadIdx.x; i < HAK_NBINS; i += 256) shist[i] = 0;
    __syncthreads();
    const V* s = smooth + (long)blockIdx.z * stride;
    const auto hfactor = hak_hist_factor(hak_state_hmax<V>(state + blockIdx.z));
    const int x = blockIdx.x * TILE_X + (threadIdx.x & 63);
    const int y0 = blockIdx.y * TILE_Y + (threadIdx.x >> 6);
    if (x < w)
        for (int y = y0; y < blockIdx.y * TILE_Y + TILE_Y && y < h; y += 4) {
            V dx, dy;
            hak_scharr_at(s, x, y, w, h, p, dx, dy);
            atomicAdd(&shist[hak_hist_bin(hak_grad_mag(dx, dy), hfactor)], 1);
        }
    __syncthreads();
    for (int i = threadIdx.x; i < HAK_NBINS; i += 256)
        if (shist[i]) atomicAdd(&state[blockIdx.z].hist[i], shist[i]);
}

// host half of hScharrContrast, kept on the device (hak_finish_kcontrast, pixel_rules.h)
template <typename V>
__global__ void k_kcontrast(HakImgState* state, int npix, int extra0, float per, int noct)
{
    if (threadIdx.x != 0) return;
    hak_finish_kcontrast<V>(state + blockIdx.x, state[blockIdx.x].hist, npix, extra0, per, noct);
}

template <typename V>
static void launch_contrast_t(hipStream_t st, const V* smooth, long stride, int w, int h, int p, int nimg,
                              HakImgState* state, float per, int noct)
{
    const dim3 grid = ss_grid(w, h, nimg);
    k_grad_max<V><<<grid, 256, 0, st>>>(smooth, stride, w, h, p, state);
    k_grad_hist<V><<<grid, 256, 0, st>>>(smooth, stride, w, h, p, state);
    k_kcontrast<V><<<nimg, 64, 0, st>>>(state, w * h, hak_hist_extra0(w, h), per, noct);
}
void hak_launch_contrast(hipStream_t st, const float* smooth, long stride, int w, int h, int p, int nimg,
                         HakImgState* state, float per, int noct)
{ launch_contrast_t(st, smooth, stride, w, h, p, nimg, state, per, noct); }
void hak_launch_contrast(hipStream_t st, const int* smooth, long stride, int w, int h, int p, int nimg,
                         HakImgState* state, float per, int noct)
{ launch_contrast_t(st, smooth, stride, w, h, p, nimg, state, per, noct); }

// --------------------------------------------------------------------- flow
template <typename V>
__global__ __launch_bounds__(256) void k_flow(const V* __restrict__ src, V* __restrict__ dst, long stride,
                                              int w, int h, int p, int type, const HakImgState* state, int octave,
                                              float fixed_ikc)
{
    const V* s = src + (long)blockIdx.z * stride;
    V* d = dst + (long)blockIdx.z * stride;
    const float ikc = state ? state[blockIdx.z].ikc[octave] : fixed_ikc;
    const int x = blockIdx.x * TILE_X + (threadIdx.x & 63);
    const int y0 = blockIdx.y * TILE_Y + (threadIdx.x >> 6);
    if (x >= w) return;
    for (int y = y0; y < blockIdx.y * TILE_Y + TILE_Y && y < h; y += 4) {
        V dx, dy;
        hak_scharr_at(s, x, y, w, h, p, dx, dy);
        d[(long)y * p + x] = hak_g_as<V>(hak_conductivity(hak_dif2(dx, dy, ikc), type));
    }
}

void hak_launch_flow(hipStream_t st, const float* src, float* dst, long stride, int w, int h, int p, int nimg,
                     int diffusivity, const HakImgState* state, int octave, float fixed_ikc)
{ k_flow<float><<<ss_grid(w, h, nimg), 256, 0, st>>>(src, dst, stride, w, h, p, diffusivity, state, octave, fixed_ikc); }
void hak_launch_flow(hipStream_t st, const int* src, int* dst, long stride, int w, int h, int p, int nimg,
                     int diffusivity, const HakImgState* state, int octave)
{ k_flow<int><<<ss_grid(w, h, nimg), 256, 0, st>>>(src, dst, stride, w, h, p, diffusivity, state, octave, 0.f); }

// ------------------------------------------------- derivatives + determinant
// unfused fallback for dilations > 4 and the debug / test planes: dxy = interleaved {Lx, Ly} (HakLayout)
template <typename V>
__global__ __launch_bounds__(256) void k_derivate(const V* __restrict__ src, V* __restrict__ dxy, long stride, int w, int h, int p,
                                                  int step, V fac1, V fac2)
{
    const V* s = src + (long)blockIdx.z * stride;
    V* o = dxy + (long)blockIdx.z * stride;
    const int x = blockIdx.x * TILE_X + (threadIdx.x & 63);
    const int y0 = blockIdx.y * TILE_Y + (threadIdx.x >> 6);
    if (x >= w) return;
    const int x0 = hak_refl(x - step, w), x2 = hak_refl(x + step, w);
    for (int y = y0; y < blockIdx.y * TILE_Y + TILE_Y && y < h; y += 4) {
        const V* r0 = s + (long)hak_refl(y - step, h) * p;
        const V* r1 = s + (long)y * p;
        const V* r2 = s + (long)hak_refl(y + step, h) * p;
        V ul = r0[x0], uc = r0[x], ur = r0[x2];
        V cl = r1[x0], cr = r1[x2];
        V ll = r2[x0], lc = r2[x], lr = r2[x2];
        typedef V V2 __attribute__((ext_vector_type(2)));
        const V2 v = {hs_d(fac1, fac2, ur + lr - ul - ll, cr - cl),        // akazed.cu:1294
                      hs_d(fac1, fac2, lr + ll - ur - ul, lc - uc)};       // akazed.cu:1295
        *reinterpret_cast<V2*>(o + 2 * ((long)y * p + x)) = v;
    }
}

template <typename V>
__global__ __launch_bounds__(256) void k_hessian(const V* __restrict__ dxy, V* __restrict__ det, long stride, int w, int h, int p,
                                                 int step, V fac1, V fac2)
{
    const V* d = dxy + (long)blockIdx.z * stride;
    V* o = det + (long)blockIdx.z * stride;
    const int x = blockIdx.x * TILE_X + (threadIdx.x & 63);
    const int y0 = blockIdx.y * TILE_Y + (threadIdx.x >> 6);
    if (x >= w) return;
    for (int y = y0; y < blockIdx.y * TILE_Y + TILE_Y && y < h; y += 4)
        o[(long)y * p + x] = hak_det_at<V>(d, x, y, step, w, h, p, fac1, fac2);                 // akazed.cu:1318-1330
}

void hak_deriv_factors(float* fac1, float* fac2)
{
    float wv = 10.f / 3.f;                                   // akazed.cu:2537-2539
    *fac1 = 1.f / (2.f * (wv + 2.f));
    *fac2 = wv * *fac1;
}

template <typename V>
static void launch_derivate_t(hipStream_t st, const V* src, V* dxy, long stride, int w, int h, int p, int nimg, int step)
{
    V f1, f2;
    hak_deriv_factors_as(f1, f2);
    k_derivate<V><<<ss_grid(w, h, nimg), 256, 0, st>>>(src, dxy, stride, w, h, p, step, f1, f2);
}
template <typename V>
static void launch_hessian_t(hipStream_t st, const V* dxy, V* det, long stride, int w, int h, int p, int nimg, int step)
{
    V f1, f2;
    hak_deriv_factors_as(f1, f2);
    k_hessian<V><<<ss_grid(w, h, nimg), 256, 0, st>>>(dxy, det, stride, w, h, p, step, f1, f2);
}
void hak_launch_derivate(hipStream_t st, const float* src, float* dxy, long stride, int w, int h, int p, int nimg, int step)
{ launch_derivate_t(st, src, dxy, stride, w, h, p, nimg, step); }
void hak_launch_derivate(hipStream_t st, const int* src, int* dxy, long stride, int w, int h, int p, int nimg, int step)
{ launch_derivate_t(st, src, dxy, stride, w, h, p, nimg, step); }
void hak_launch_hessian(hipStream_t st, const float* dxy, float* det, long stride, int w, int h, int p, int nimg, int step)
{ launch_hessian_t(st, dxy, det, stride, w, h, p, nimg, step); }
void hak_launch_hessian(hipStream_t st, const int* dxy, int* det, long stride, int w, int h, int p, int nimg, int step)
{ launch_hessian_t(st, dxy, det, stride, w, h, p, nimg, step); }

// interleaved {a, b} plane (pitch 2p) -> two dense planes (pitch p): stage tests and hak_debug_plane only
__global__ __launch_bounds__(256) void k_deinterleave(const float2* __restrict__ ab, float* __restrict__ a, float* __restrict__ b,
                                                      int w, int h, int p)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float2 v = ab[(long)y * p + x];
    a[(long)y * p + x] = v.x;
    b[(long)y * p + x] = v.y;
}
void hak_launch_deinterleave(hipStream_t st, const float* ab, float* a, float* b, int w, int h, int p)
{
    k_deinterleave<<<dim3((w + 255) / 256, h), 256, 0, st>>>(reinterpret_cast<const float2*>(ab), a, b, w, h, p);
}

// ------------------------------------------------------------------ ingest
// uint8 -> float32 [0,1] as main.cpp:149: (float)(v * (1.0 / 255.0)).  One thread converts 16 pixels of a row (one 16-byte load,
// four 16-byte stores) when the row starts and pitches allow it, else pixel by pixel; the threads of an image are a flat
// index over (row, 16-px chunk), so a 1920-px row does not leave a partly idle block at its right end.
__global__ __launch_bounds__(256) void k_ingest_u8(const unsigned char* __restrict__ src, long src_stride, int sp,
                                                   float* __restrict__ dst, long dst_stride, int dp, int w, int h, int cpr, int vec)
{
    const unsigned char* s = src + (long)blockIdx.y * src_stride;
    float* d = dst + (long)blockIdx.y * dst_stride;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int y = (int)(idx / cpr), x = (int)(idx - (long)y * cpr) * 16;
    if (y >= h) return;
    const unsigned char* q = s + (long)y * sp + x;
    float* o = d + (long)y * dp + x;
    if (vec && x + 15 < w) {
        const uint4 v = *reinterpret_cast<const uint4*>(q);
        const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned u = wds[k];
            *reinterpret_cast<float4*>(o + 4 * k) =
                make_float4((float)((u & 255u) * (1.0 / 255.0)), (float)(((u >> 8) & 255u) * (1.0 / 255.0)),
                            (float)(((u >> 16) & 255u) * (1.0 / 255.0)), (float)((u >> 24) * (1.0 / 255.0)));
        }
    } else {
        for (int e = 0; e < 16 && x + e < w; e++) o[e] = (float)(q[e] * (1.0 / 255.0));
    }
}

void hak_launch_ingest_u8(hipStream_t st, const unsigned char* src, long src_stride, int sp, float* dst, long dst_stride,
                          int dp, int w, int h, int nimg)
{
    const int cpr = (w + 15) / 16;                                  // 16-px chunks per row
    const int vec = ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0) && sp % 16 == 0 && src_stride % 16 == 0 &&
                    dp % 4 == 0 && dst_stride % 4 == 0;
    dim3 grid((unsigned)(((long)cpr * h + 255) / 256), nimg);
    k_ingest_u8<<<grid, 256, 0, st>>>(src, src_stride, sp, dst, dst_stride, dp, w, h, cpr, vec);
}

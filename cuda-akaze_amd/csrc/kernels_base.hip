// kernels_base.hip -- octave-0 prologue: base level + contrast factor (akaze.cpp:325-333).
//
//   hLowPass(img -> smooth, var 1, ksz 5)         akazed.cu:2336, 204   (gConv2d<2>)
//   hScharrContrast(smooth -> kcontrast)          akazed.cu:2410, 644, 827, 901
//   hLowPass(img -> Lt(0,0), var soffset^2)       akazed.cu:2336, 204   (gConv2d<R>, R = 4 for soffset 1.6)
//
// The sigma=1 plane is only an intermediate of the contrast factor, so it is never written:
//   pass A  reads the image once and produces Lt(0,0) AND the maximum Scharr magnitude of the
//           sigma=1 image (one atomicMax per block), and leaves that magnitude as a plane;
//   pass B  fills the 300-bin histogram from that plane (needs the global maximum of pass A).
// Pass A is a persistent tile kernel with register prefetch of the next tile (see kernels_hessian.hip
// for why).  As in kernels_smoothflow.hip, tiles are loaded with reflect-101 indices and then indexed
// plainly.  The integer FAST path (akaze.cpp:589-612, uint8 image, int32 planes) has the same two passes:
// kf_base<R> and kf_grad_hist_plane below.  Arithmetic: pixel_rules.h.
#include "hak_internal.h"

#define BS_TX 64
#define BS_TY 32

struct BsTaps { float a[3]; float b[6]; };       // sigma=1 taps (R=2), base taps (R <= 5)

// Scharr magnitude at the centre of a 3x3 neighbourhood in a tile of width W (akazed.cu:664-666 / 3208-3232)
template <int W, typename V>
__device__ __forceinline__ V scharr_mag(const V* q)
{
    V dx, dy;
    hak_scharr(q[-W - 1], q[-W], q[-W + 1], q[-1], q[1], q[W - 1], q[W], q[W + 1], dx, dy);
    return hak_grad_mag(dx, dy);
}

template <int H>                                   // H = tile halo
struct BsGeo {
    static constexpr int RW = BS_TX + 2 * H, RH = BS_TY + 2 * H;    // raw tile
    static constexpr int NPF = (RW * RH + 255) / 256;
    static constexpr int PW = BS_TX + 2, PH = BS_TY + 6;            // sigma=1 row-pass tile (halo 1 in x, 3 in y)
    static constexpr int SH = BS_TY + 2;                            // sigma=1 smooth tile (halo 1)
};

template <int H>
__device__ __forceinline__ void bs_fetch(float (&pf)[BsGeo<H>::NPF], const float* __restrict__ s, int w, int h, int sp,
                                         int x0, int y0, int tid)
{
    using G = BsGeo<H>;
#pragma unroll
    for (int i = 0; i < G::NPF; i++) {
        const int idx = tid + 256 * i;
        if (idx < G::RW * G::RH) {
            const int r = idx / G::RW, c = idx - r * G::RW;
            pf[i] = s[(long)hak_refl(y0 - H + r, h) * sp + hak_refl(x0 - H + c, w)];
        }
    }
}

// sigma=1 row pass (rows y0-3 .. y0+TY+2, columns x0-1 .. x0+TX) from a raw tile with halo H >= 3
template <int H>
__device__ __forceinline__ void bs_rowpass1(const float* raw, float* rowp, const BsTaps& t, int tid)
{
    using G = BsGeo<H>;
    for (int idx = tid; idx < G::PH * G::PW; idx += 256) {
        const int r = idx / G::PW, c = idx - r * G::PW;
        const float* q = raw + (r + H - 3) * G::RW + c + H - 1;
        rowp[idx] = hak_conv<2>(t.a, [&](int k) { return q[k]; });
    }
}

// sigma=1 column pass -> smooth tile (rows y0-1 .. y0+TY, columns x0-1 .. x0+TX)
template <int H>
__device__ __forceinline__ void bs_colpass1(const float* rowp, float* sm, const BsTaps& t, int tid)
{
    using G = BsGeo<H>;
    for (int idx = tid; idx < G::SH * G::PW; idx += 256) {
        const int r = idx / G::PW, c = idx - r * G::PW;
        const float* q = rowp + (r + 2) * G::PW + c;
        sm[idx] = hak_conv<2>(t.a, [&](int k) { return q[k * G::PW]; });
    }
}

// ---- pass A: Lt(0,0) = G(base) * img, and max |Scharr(G(1) * img)|
template <int R>
__global__ __launch_bounds__(256) void k_base_a(const float* __restrict__ img, long img_stride, int sp,
                                                float* __restrict__ lt, float* __restrict__ grad, long stride, int w, int h, int p,
                                                BsTaps t, HakImgState* state, int tiles_per_block, int nbx, int nby, int nimg)
{
    constexpr int H = R < 3 ? 3 : R;
    using G = BsGeo<H>;
    __shared__ float raw[G::RH * G::RW];              // reused for the sigma=1 smooth tile
    __shared__ float rowb[G::RH * BS_TX];             // base row pass (all tile rows, output columns)
    __shared__ float rowp[G::PH * G::PW];             // sigma=1 row pass
    __shared__ float wmax[4];
    int bx, by, im;
    if (!hak_xcd_decode(nbx, nby, nimg, bx, by, im)) return;
    const float* s = img + (long)im * img_stride;
    float* o = lt + (long)im * stride;
    float* go = grad + (long)im * stride;
    const int tid = threadIdx.x;
    const int x0 = bx * BS_TX;
    const int ty0 = by * tiles_per_block;
    const int ty1 = min(ty0 + tiles_per_block, (h + BS_TY - 1) / BS_TY);
    float pf[G::NPF];
    float tmax = 0.f;
    if (ty0 < ty1) bs_fetch<H>(pf, s, w, h, sp, x0, ty0 * BS_TY, tid);
    for (int ty = ty0; ty < ty1; ty++) {
        const int y0 = ty * BS_TY;
        hak_lds_barrier();
#pragma unroll
        for (int i = 0; i < G::NPF; i++)
            if (tid + 256 * i < G::RW * G::RH) raw[tid + 256 * i] = pf[i];
        hak_lds_barrier();
        if (ty + 1 < ty1) bs_fetch<H>(pf, s, w, h, sp, x0, y0 + BS_TY, tid);
        // base row pass on every raw row, output columns only (akazed.cu:227-239)
        for (int idx = tid; idx < G::RH * BS_TX; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            const float* q = raw + r * G::RW + c + H;
            rowb[idx] = hak_conv<R>(t.b, [&](int k) { return q[k]; });
        }
        bs_rowpass1<H>(raw, rowp, t, tid);
        hak_lds_barrier();
        // base column pass -> Lt(0,0) (akazed.cu:283-288)
        for (int idx = tid; idx < BS_TY * BS_TX; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            const int x = x0 + c, y = y0 + r;
            const float* q = rowb + (r + H) * BS_TX + c;
            const float ws = hak_conv<R>(t.b, [&](int k) { return q[k * BS_TX]; });
            if (x < w && y < h) o[(long)y * p + x] = ws;
        }
        float* sm = raw;
        bs_colpass1<H>(rowp, sm, t, tid);
        hak_lds_barrier();
        for (int idx = tid; idx < BS_TY * BS_TX; idx += 256) {
            const int r = idx >> 6, c = idx & 63;
            if (x0 + c < w && y0 + r < h) {
                const float g = scharr_mag<G::PW>(sm + (r + 1) * G::PW + c + 1);
                if (hak_on_lattice(x0 + c, y0 + r, w, h)) tmax = fmaxf(tmax, g);
                go[(long)(y0 + r) * p + x0 + c] = g;      // kept for the histogram pass (k_grad_hist_plane)
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, off));
    if ((tid & 63) == 0) wmax[tid >> 6] = tmax;
    hak_lds_barrier();
    if (tid == 0) {
        const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        if (m > 0.f) atomicMax(&state[im].hmax_bits, __float_as_uint(m));   // lattice maximum (akazed.cu:827-877)
    }
}

// ---- pass B: the histogram from the gradient plane pass A left behind// ---- pass B': the same histogram from the gradient plane pass A left behind (4 B/px read, no recomputation)
#define HIST_COPIES 8          // private LDS histograms per block, selected by lane: smooth images put most pixels into a few
                                // bins, and LDS atomics on one address serialise
// (histogram only: the contrast factor stays a launch of its own, k_kcontrast2.  Letting the last histogram block finish it was
// measured: the fence every block then needs behind its ~300 bin atomics, which are otherwise fire-and-forget, took the kernel
// from 22 to 73 us on a single 1080p image -- far more than the launch it saves)
__global__ __launch_bounds__(256) void k_grad_hist_plane(const float* __restrict__ grad, long stride, int w, int h, int p,
                                                         HakImgState* state, int rows_per_block)
{
    __shared__ int shist[HIST_COPIES * HAK_NBINS];
    const int im = blockIdx.y;
    const float* g0 = grad + (long)im * stride;
    const int tid = threadIdx.x;
    for (int i = tid; i < HIST_COPIES * HAK_NBINS; i += 256) shist[i] = 0;
    const double hfactor = hak_hist_factor(hak_state_hmax<float>(state + im));
    hak_lds_barrier();
    const int y0 = blockIdx.x * rows_per_block, y1 = min(y0 + rows_per_block, h);
    int* mine = shist + (tid & (HIST_COPIES - 1)) * HAK_NBINS;
    auto bin = [&](float g) { atomicAdd(&mine[hak_hist_bin(g, hfactor)], 1); };
    const int w4 = w >> 2;                                          // rows are 16-byte aligned (pitch % 64 == 0)
    for (int y = y0; y < y1; y++) {
        const float* row = g0 + (long)y * p;
        for (int x = tid; x < w4; x += 256) {
            const float4 g = reinterpret_cast<const float4*>(row)[x];
            bin(g.x); bin(g.y); bin(g.z); bin(g.w);
        }
        if (tid < (w & 3)) bin(row[4 * w4 + tid]);
    }
    hak_lds_barrier();
    for (int i = tid; i < HAK_NBINS; i += 256) {
        int sum = 0;
#pragma unroll
        for (int c = 0; c < HIST_COPIES; c++) sum += shist[c * HAK_NBINS + i];
        if (sum) atomicAdd(&state[im].hist[i], sum);
    }
}
// the FAST path's: one int per lane and row step (akazed.cu:3299-3330)
__global__ __launch_bounds__(256) void kf_grad_hist_plane(const int* __restrict__ grad, long stride, int w, int h, int p,
                                                          HakImgState* state, int rows_per_block)
{
    __shared__ int shist[HIST_COPIES * HAK_NBINS];
    const int im = blockIdx.y;
    const int* g0 = grad + (long)im * stride;
    for (int i = threadIdx.x; i < HIST_COPIES * HAK_NBINS; i += 256) shist[i] = 0;
    const int hfactor = hak_hist_factor(hak_state_hmax<int>(state + im));
    __syncthreads();
    int* mine = shist + (threadIdx.x & (HIST_COPIES - 1)) * HAK_NBINS;
    const int y0 = blockIdx.x * rows_per_block, y1 = min(y0 + rows_per_block, h);
    for (int y = y0; y < y1; y++) {
        const int* row = g0 + (long)y * p;
        for (int x = threadIdx.x; x < w; x += 256) atomicAdd(&mine[hak_hist_bin(row[x], hfactor)], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HAK_NBINS; i += 256) {
        int sum = 0;
#pragma unroll
        for (int c = 0; c < HIST_COPIES; c++) sum += shist[c * HAK_NBINS + i];
        if (sum) atomicAdd(&state[im].hist[i], sum);
    }
}

// host half of hScharrContrast, kept on the device (hak_finish_kcontrast, pixel_rules.h)
template <typename V>
__global__ void k_kcontrast2(HakImgState* state, int npix, int extra0, float per, int noct)
{
    if (threadIdx.x != 0) return;
    hak_finish_kcontrast<V>(state + blockIdx.x, state[blockIdx.x].hist, npix, extra0, per, noct);
}

// img -> Lt(0,0) and the per-image contrast factors.  Returns false when R is not supported here.
// `grad_scratch`: a free plane of the arena (same stride / pitch as lt) that receives the gradient magnitude for the histogram pass.
bool hak_launch_base_level(hipStream_t st, const float* img, long img_stride, int sp, float* lt, float* grad_scratch, long stride,
                           int w, int h, int p, int nimg, const float* taps1, const float* taps_base, int R,
                           HakImgState* state, float per, int noct, const HakKnobs& knobs)
{
    if (R < 2 || R > 5) return false;
    if (!grad_scratch) { hak_note_launch_error("the octave-0 prologue needs a plane for the gradient magnitude"); return true; }
    BsTaps t;
    for (int i = 0; i < 3; i++) t.a[i] = taps1[i];
    for (int i = 0; i < 6; i++) t.b[i] = i <= R ? taps_base[i] : 0.f;
    const int ntx = (w + BS_TX - 1) / BS_TX, nty = (h + BS_TY - 1) / BS_TY;
    int tpb = 8;
    while (tpb > 1 && (long)ntx * ((nty + tpb - 1) / tpb) * nimg < 4096) tpb >>= 1;
    const int nby = (nty + tpb - 1) / tpb;
    const unsigned grid = hak_xcd_grid(ntx, nby, nimg);
    // the streaming form with the histogram inside (round 5): contrast maximum first, from the lattice points alone, then ONE pass
    if (knobs.base_hist && hak_launch_base_stream(st, img, img_stride, sp, lt, nullptr, stride, w, h, p, nimg, taps1, taps_base, R, state, knobs.base_stream)) {
        k_kcontrast2<float><<<nimg, 64, 0, st>>>(state, w * h, hak_hist_extra0(w, h), per, noct);
        return true;
    }
    if (hak_launch_base_stream(st, img, img_stride, sp, lt, grad_scratch, stride, w, h, p, nimg, taps1, taps_base, R, state, knobs.base_stream)) {
        // pass A done by the streaming kernel
    } else
    switch (R) {
    case 2: k_base_a<2><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t, state, tpb, ntx, nby, nimg); break;
    case 3: k_base_a<3><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t, state, tpb, ntx, nby, nimg); break;
    case 4: k_base_a<4><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t, state, tpb, ntx, nby, nimg); break;
    default: k_base_a<5><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t, state, tpb, ntx, nby, nimg); break;
    }
    int rpb = knobs.hist_rpb_max;
    while (rpb > 1 && (long)((h + rpb - 1) / rpb) * nimg < knobs.hist_min_blocks) rpb >>= 1;
    // rows per block: 8 unless that leaves fewer than 256 blocks (round 5; 2048 before: a pair's two images then ran 2 160 one-row
    // blocks, each zeroing 2 400 LDS words and flushing its bins with global atomics for 1 920 pixels -- 27 us alone, on the
    // critical chain of the pair call; with 8 rows per block the call is 0.547 instead of 0.567 ms, batches are unchanged)
    k_grad_hist_plane<<<dim3((h + rpb - 1) / rpb, nimg), 256, 0, st>>>(grad_scratch, stride, w, h, p, state, rpb);
    k_kcontrast2<float><<<nimg, 64, 0, st>>>(state, w * h, hak_hist_extra0(w, h), per, noct);
    return true;
}

// ---- the FAST path's prologue (akaze.cpp:589-612): one pass over the uint8 image gives Lt(0,0) = the base Gaussian, the maximum
// Scharr magnitude of the sigma=1 image, and that magnitude as a plane for the histogram pass.  The sigma=1 plane itself is only an
// intermediate of the contrast factor and is never written.  One tile per block (no prefetch ring), raw rows padded by one word.
struct FbTaps { int k[8]; };
template <int R>
__global__ __launch_bounds__(256) void kf_base(const unsigned char* __restrict__ img, long img_stride, int sp, int* __restrict__ lt,
                                               int* __restrict__ grad, long stride, int w, int h, int p, FbTaps t1, FbTaps tb,
                                               HakImgState* state, int nbx, int nby, int nimg)
{
    constexpr int H = R < 3 ? 3 : R;
    using G = BsGeo<H>;
    constexpr int RP = G::RW + 1;                                   // padded raw pitch
    __shared__ int raw[G::RH * RP];                                 // reused for the sigma=1 smooth tile [SH][PW]
    __shared__ int rowb[G::RH * BS_TX];
    __shared__ int rowp[G::PH * G::PW];
    int bx, by, im;
    if (!hak_xcd_decode(nbx, nby, nimg, bx, by, im)) return;
    const unsigned char* s = img + (long)im * img_stride;
    int* o = lt + (long)im * stride;
    int* go = grad + (long)im * stride;
    const int x0 = bx * BS_TX, y0 = by * BS_TY, tid = threadIdx.x;
    for (int i = tid; i < G::RH * G::RW; i += 256) {
        const int r = i / G::RW, c = i - r * G::RW;
        raw[r * RP + c] = (int)s[(long)hak_refl(y0 - H + r, h) * sp + hak_refl(x0 - H + c, w)];
    }
    __syncthreads();
    for (int i = tid; i < G::RH * BS_TX; i += 256) {                // base row pass, output columns only
        const int r = i >> 6, c = i & 63;
        const int* q = raw + r * RP + c + H;
        rowb[i] = hak_conv<R>(tb.k, [&](int k) { return q[k]; });
    }
    for (int i = tid; i < G::PH * G::PW; i += 256) {                // sigma=1 row pass: rows y0-3.., columns x0-1..
        const int r = i / G::PW, c = i - r * G::PW;
        const int* q = raw + (r + H - 3) * RP + c + H - 1;
        rowp[i] = hak_conv<2>(t1.k, [&](int k) { return q[k]; });
    }
    __syncthreads();
    for (int i = tid; i < BS_TY * BS_TX; i += 256) {                // base column pass -> Lt(0,0)
        const int r = i >> 6, c = i & 63;
        const int x = x0 + c, y = y0 + r;
        const int* q = rowb + (r + H) * BS_TX + c;
        const int ws = hak_conv<R>(tb.k, [&](int k) { return q[k * BS_TX]; });
        if (x < w && y < h) o[(long)y * p + x] = ws;
    }
    int* sm = raw;                                                  // raw is dead: both row passes are done
    for (int i = tid; i < G::SH * G::PW; i += 256) {                // sigma=1 column pass -> smooth tile (halo 1)
        const int r = i / G::PW, c = i - r * G::PW;
        const int* q = rowp + (r + 2) * G::PW + c;
        sm[i] = hak_conv<2>(t1.k, [&](int k) { return q[k * G::PW]; });
    }
    __syncthreads();
    int m = 0;
    for (int i = tid; i < BS_TY * BS_TX; i += 256) {                // Scharr magnitude (akazed.cu:3208-3232)
        const int r = i >> 6, c = i & 63;
        const int x = x0 + c, y = y0 + r;
        if (x < w && y < h) {
            const int g = scharr_mag<G::PW>(sm + (r + 1) * G::PW + c + 1);
            go[(long)y * p + x] = g;
            if (hak_on_lattice(x, y, w, h)) m = max(m, g);                                        // akazed.cu:3245-3296
        }
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
    if ((tid & 63) == 0 && m > 1) atomicMax(&state[im].ihmax, m);
}

// img (uint8) -> Lt(0,0), contrast factors; `grad_scratch` = a free int32 plane of the arena.  false: R not covered
// (caller: hak_launch_lowpass x2 + hak_launch_contrast)
bool hak_launch_base_level(hipStream_t st, const unsigned char* img, long img_stride, int sp, int* lt, int* grad_scratch, long stride,
                           int w, int h, int p, int nimg, const int* taps1, const int* taps_base, int R, HakImgState* state,
                           float per, int noct, const HakKnobs& knobs)
{
    if (R < 2 || R > 5) return false;
    FbTaps t1, tb;
    for (int i = 0; i < 8; i++) { t1.k[i] = i <= 2 ? taps1[i] : 0; tb.k[i] = i <= R ? taps_base[i] : 0; }
    const int nbx = (w + BS_TX - 1) / BS_TX, nby = (h + BS_TY - 1) / BS_TY;
    const unsigned grid = hak_xcd_grid(nbx, nby, nimg);
    // the streaming form with the histogram inside (round 5): contrast maximum first, from the lattice points alone, then ONE pass
    if (knobs.base_hist && hak_launch_base_stream(st, img, img_stride, sp, lt, nullptr, stride, w, h, p, nimg, taps1, taps_base, R, state, knobs.base_stream)) {
        k_kcontrast2<int><<<nimg, 64, 0, st>>>(state, w * h, hak_hist_extra0(w, h), per, noct);
        return true;
    }
    if (hak_launch_base_stream(st, img, img_stride, sp, lt, grad_scratch, stride, w, h, p, nimg, taps1, taps_base, R, state, knobs.base_stream)) {
        // pass A done by the streaming kernel
    } else
    switch (R) {
    case 2: kf_base<2><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t1, tb, state, nbx, nby, nimg); break;
    case 3: kf_base<3><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t1, tb, state, nbx, nby, nimg); break;
    case 4: kf_base<4><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t1, tb, state, nbx, nby, nimg); break;
    default: kf_base<5><<<grid, 256, 0, st>>>(img, img_stride, sp, lt, grad_scratch, stride, w, h, p, t1, tb, state, nbx, nby, nimg); break;
    }
    int rpb = 8;
    while (rpb > 1 && (long)((h + rpb - 1) / rpb) * nimg < 2048) rpb >>= 1;
    kf_grad_hist_plane<<<dim3((h + rpb - 1) / rpb, nimg), 256, 0, st>>>(grad_scratch, stride, w, h, p, state, rpb);
    k_kcontrast2<int><<<nimg, 64, 0, st>>>(state, w * h, hak_hist_extra0(w, h), per, noct);
    return true;
}

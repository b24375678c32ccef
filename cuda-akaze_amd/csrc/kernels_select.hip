// kernels_select.hip -- keep the strongest N survivors of an image instead of its raster-order prefix (hak_set_retain_best)
// (gfx950, wave64).
//
// Runs between k_nms_cand and k_row_scan of hak_launch_nms_emit when the mode is on; everything after it (scan, emit, refine,
// orientation, descriptors, download, the map clean-up) is unchanged and simply sees fewer survivor bits.  Per image with
// S survivors and clamp C (the same clamp k_row_scan applies):
//   S <= C: nothing is touched (every kernel below leaves at once on the device-side flag of k_sel_init).
//   S >  C: keep the C survivors that rank highest by (K(response word), then the smaller raster index y * w + x), where K is
//           the order-preserving unsigned map of the key map's high word (sel_key).
// The C-th largest key T is found by a radix select over K: three passes of 11 / 11 / 10 bits, each a walk of the survivor bitmap
// that gathers the key of every set bit and builds a per-block LDS histogram of the next digit, flushed with one integer atomic
// per non-empty bin; a one-wave kernel per image then picks the digit that holds the C-th key.  k_sel_rows clears every bit
// below T and counts, per row, the keys above T and equal to T; k_sel_ties keeps the first C - count(K > T) keys equal to T in
// raster order.  Only integer atomics: the result does not depend on arrival order.
#include "hak_internal.h"

namespace {
constexpr int kShift[HAK_SEL_PASSES] = {21, 10, 0};
constexpr int kWidth[HAK_SEL_PASSES] = {11, 11, 10};
}                                               // (sel_key, sel_cap: hak_internal.h, shared with kernels_grid_select.hip)

// survivors of the image vs its clamp; zeroes the image's digit histograms when it selects.  One block per image.
__global__ __launch_bounds__(256) void k_sel_init(const int* __restrict__ rowcount, int h, int max_pts, int cap0, int cap1,
                                                  HakSelState* sel, unsigned* bins)
{
    __shared__ int part[256];
    __shared__ int active;
    const int img = blockIdx.x;
    const int* rc = rowcount + (long)img * h;
    int sum = 0;
    for (int i = threadIdx.x; i < h; i += 256) sum += rc[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int cap = sel_cap(img, max_pts, cap0, cap1);
        active = part[0] > cap ? 1 : 0;
        HakSelState s;
        s.active = active;
        s.need = cap;
        s.prefix = 0u;
        s.pad = 0;
        sel[img] = s;
    }
    __syncthreads();
    if (!active) return;
    unsigned* b = bins + (long)img * HAK_SEL_PASSES * HAK_SEL_BINS;
    for (int i = threadIdx.x; i < HAK_SEL_PASSES * HAK_SEL_BINS; i += 256) b[i] = 0u;
}

// one radix pass: histogram of digit `pass` over the keys whose earlier digits equal the prefix picked so far.
// grid (nb, nimg): block x of an image walks its share of the image's bitmap words.
__global__ __launch_bounds__(256) void k_sel_hist(const unsigned long long* __restrict__ maps, long map_stride, int p0,
                                                  const unsigned long long* __restrict__ bitmap, int words_per_row, int h,
                                                  const HakSelState* __restrict__ sel, unsigned* bins, int pass, int fast)
{
    __shared__ unsigned hist[HAK_SEL_BINS];
    const int img = blockIdx.y;
    if (!sel[img].active) return;                                   // (block-uniform)
    const unsigned prefix = sel[img].prefix;
    const int shift = kShift[pass], mask = (1 << kWidth[pass]) - 1;
    const int fshift = pass > 0 ? kShift[pass - 1] : 32;            // (pass 0: no filter)
    for (int i = threadIdx.x; i < HAK_SEL_BINS; i += 256) hist[i] = 0u;
    __syncthreads();
    const long total = (long)h * words_per_row;
    const long beg = total * blockIdx.x / gridDim.x, end = total * (blockIdx.x + 1) / gridDim.x;
    const unsigned long long* bm = bitmap + (long)img * total;
    const unsigned long long* map = maps + (long)img * map_stride;
    for (long i = beg + threadIdx.x; i < end; i += 256) {
        unsigned long long word = bm[i];
        if (!word) continue;
        const int y = (int)(i / words_per_row), x0 = (int)(i - (long)y * words_per_row) * 64;
        while (word) {
            const int bit = __ffsll((long long)word) - 1;
            word &= word - 1;
            const unsigned k = sel_key(hak_key_word(map[(long)y * p0 + x0 + bit]), fast);
            if (fshift == 32 || (k >> fshift) == prefix) atomicAdd(&hist[(k >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    unsigned* b = bins + ((long)img * HAK_SEL_PASSES + pass) * HAK_SEL_BINS;
    for (int i = threadIdx.x; i <= mask; i += 256)
        if (hist[i]) atomicAdd(&b[i], hist[i]);
}

// one wave per image: the digit of pass `pass` that holds the need-th largest key among those matching the prefix
__global__ __launch_bounds__(64) void k_sel_pick(HakSelState* sel, const unsigned* __restrict__ bins, int pass)
{
    const int img = blockIdx.x;
    const int lane = threadIdx.x;
    if (!sel[img].active) return;
    const int need = sel[img].need;
    const int nbins = 1 << kWidth[pass];
    const int per = nbins / 64;
    const unsigned* b = bins + ((long)img * HAK_SEL_PASSES + pass) * HAK_SEL_BINS;
    // lane l owns the bins [nbins - (l + 1) * per, nbins - l * per): lane order is descending digit order
    const int top = nbins - 1 - lane * per;
    int s = 0;
    for (int j = 0; j < per; j++) s += (int)b[top - j];
    int incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned long long m = __ballot(incl >= need);
    if (!m) {                                                       // (cannot happen: the bins hold >= need keys) keep the raster clamp
        if (lane == 0) sel[img].active = 0;
        return;
    }
    const int owner = __ffsll((long long)m) - 1;
    if (lane == owner) {
        int rem = need - (incl - s);
        int d = top - per + 1;
        for (int j = 0; j < per; j++) {
            const int c = (int)b[top - j];
            if (rem <= c) { d = top - j; break; }
            rem -= c;
        }
        sel[img].need = rem;
        sel[img].prefix = (sel[img].prefix << kWidth[pass]) | (unsigned)d;
    }
}

// clear every survivor below T; per row: rowcount = keys above T, tie = keys equal to T.  grid (nb, nimg), one wave per row.
__global__ __launch_bounds__(256) void k_sel_rows(const unsigned long long* __restrict__ maps, long map_stride, int p0,
                                                  unsigned long long* bitmap, int words_per_row, int h, int* rowcount, int* tie,
                                                  const HakSelState* __restrict__ sel, int fast)
{
    const int img = blockIdx.y;
    if (!sel[img].active) return;
    const unsigned T = sel[img].prefix;
    const int lane = threadIdx.x & 63;
    const unsigned long long* map = maps + (long)img * map_stride;
    for (int y = blockIdx.x * 4 + (threadIdx.x >> 6); y < h; y += gridDim.x * 4) {      // (wave-uniform)
        int* rc = rowcount + (long)img * h + y;
        int gt = 0, eq = 0;
        if (*rc) {
            unsigned long long* row = bitmap + ((long)img * h + y) * words_per_row;
            for (int w0 = 0; w0 < words_per_row; w0 += 64) {
                if (w0 + lane >= words_per_row) continue;
                const unsigned long long orig = row[w0 + lane];
                unsigned long long word = orig, keep = orig;
                while (word) {
                    const int bit = __ffsll((long long)word) - 1;
                    word &= word - 1;
                    const unsigned k = sel_key(hak_key_word(map[(long)y * p0 + (w0 + lane) * 64 + bit]), fast);
                    if (k < T) keep &= ~(1ull << bit);
                    gt += k > T;
                    eq += k == T;
                }
                if (keep != orig) row[w0 + lane] = keep;
            }
            for (int o = 32; o > 0; o >>= 1) {
                gt += __shfl_xor(gt, o);
                eq += __shfl_xor(eq, o);
            }
        }
        if (lane == 0) {
            *rc = gt;
            tie[(long)img * h + y] = eq;
        }
    }
}

// the keys equal to T: the first `need` of them in raster order stay.  One block per image: exclusive scan of the per-row tie
// counts, then each thread finishes its own rows (only rows that hold a key equal to T are touched).
__global__ __launch_bounds__(1024) void k_sel_ties(const unsigned long long* __restrict__ maps, long map_stride, int p0,
                                                   unsigned long long* bitmap, int words_per_row, int h, int* rowcount,
                                                   const int* __restrict__ tie, const HakSelState* __restrict__ sel, int fast)
{
    __shared__ int part[1024];
    const int img = blockIdx.x;
    if (!sel[img].active) return;
    const unsigned T = sel[img].prefix;
    const int need = sel[img].need;
    const int* tc = tie + (long)img * h;
    const int per = (h + 1023) / 1024;
    const int beg = threadIdx.x * per, end = min(beg + per, h);
    int sum = 0;
    for (int i = beg; i < end; i++) sum += tc[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                            // inclusive Hillis-Steele scan
        const int t = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;                              // ties in the rows before this thread's first row
    const unsigned long long* map = maps + (long)img * map_stride;
    for (int y = beg; y < end; y++) {
        const int t = tc[y];
        if (!t) continue;
        int keep = need - run;
        keep = keep < 0 ? 0 : (keep > t ? t : keep);
        run += t;
        if (keep) rowcount[(long)img * h + y] += keep;
        if (keep == t) continue;
        unsigned long long* row = bitmap + ((long)img * h + y) * words_per_row;
        int seen = 0;
        for (int wi = 0; wi < words_per_row; wi++) {
            const unsigned long long orig = row[wi];
            unsigned long long word = orig, out = orig;
            while (word) {
                const int bit = __ffsll((long long)word) - 1;
                word &= word - 1;
                if (sel_key(hak_key_word(map[(long)y * p0 + wi * 64 + bit]), fast) == T && seen++ >= keep) out &= ~(1ull << bit);
            }
            if (out != orig) row[wi] = out;
        }
    }
}

void hak_launch_select(hipStream_t st, const HakBatch& b, const HakLayout& L, int max_pts, int cap0, int cap1, int fast)
{
    const int w = L.oct[0].w, h = L.oct[0].h, p = L.oct[0].p;
    const int words = (w + 63) / 64;
    const HakSelScratch& s = b.sel;
    // blocks per image: about 8 bitmap words per thread, at most 256 per image and 2048 in all (a 256-image batch: 8 per image)
    long nb = (long)h * words / 2048;
    nb = nb < 1 ? 1 : (nb > 256 ? 256 : nb);
    if (nb * b.nimg > 2048) nb = 2048 / b.nimg > 1 ? 2048 / b.nimg : 1;
    k_sel_init<<<b.nimg, 256, 0, st>>>(b.rowcount, h, max_pts, cap0, cap1, s.st, s.bins);
    for (int pass = 0; pass < HAK_SEL_PASSES; pass++) {
        k_sel_hist<<<dim3((unsigned)nb, b.nimg), 256, 0, st>>>(b.maps, b.map_stride, p, b.bitmap, words, h, s.st, s.bins, pass, fast);
        k_sel_pick<<<b.nimg, 64, 0, st>>>(s.st, s.bins, pass);
    }
    k_sel_rows<<<dim3((unsigned)nb, b.nimg), 256, 0, st>>>(b.maps, b.map_stride, p, b.bitmap, words, h, b.rowcount, s.tie, s.st, fast);
    k_sel_ties<<<b.nimg, 1024, 0, st>>>(b.maps, b.map_stride, p, b.bitmap, words, h, b.rowcount, s.tie, s.st, fast);
}

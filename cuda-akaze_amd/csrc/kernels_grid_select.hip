// kernels_grid_select.hip -- spread an overflowing image's keypoint budget over a grid of square cells (hak_set_retain_grid)
// (gfx950, wave64).
//
// Runs where hak_launch_select runs, instead of it: between k_nms_cand and k_row_scan of hak_launch_nms_emit.  Everything after it
// sees fewer survivor bits and exact per-row counts, nothing else.  Per image with S survivors and clamp C (k_row_scan's clamp):
//   S <= C: nothing is touched (every kernel below leaves at once on the device-side flag of k_grid_init).
//   S >  C: a survivor at integer position (x, y) lies in cell c = (y / G) * ncx + x / G; inside a cell and between cells alike
//           survivors rank by the composite  K(response word) << 32 | (0xFFFFFFFF - raster index y * w + x),  larger first: K
//           descending, then the smaller raster index (K: sel_key, the map of the strongest-N mode).  Composites of an image are
//           distinct.  With n_c the survivors of cell c, q is the largest quota with sum min(n_c, q) <= C; every cell keeps its
//           min(n_c, q) highest, and of the rank-q survivors (0-based) of the cells with n_c > q -- one candidate per cell -- the
//           R = C - sum min(n_c, q) highest are kept as well.
//   k_grid_count   one wave per cell: n_c = popcount of the cell's part of the bitmap (G rows, at most three words per row).
//   k_grid_quota   one block per image: q by bisection over [0, G * G] on the block sum of min(n_c, q); R.
//   k_grid_rank    one wave per cell with n_c > q: the cell's rank-q composite T_c (counting comparisons over the cell's composites,
//                  staged in LDS up to kStage of them, read again from the key map above that -- slower, never truncated), published
//                  as the cell's candidate; every bit of the cell below T_c is cleared.
//   k_grid_extras  one block per image: the R-th largest candidate T, bit by bit from the top on the block count of candidates
//                  >= T | bit; the candidates below T are cleared.
// A cleared bit is one atomicAnd on its bitmap word (words and rows cross cells) and one atomicSub on its row's count.  Only integer
// atomics, every operand decided by the rule alone: the result does not depend on arrival order.
#include "hak_internal.h"

namespace {
typedef unsigned long long u64;
constexpr int kStage = 512;                     // composites a wave stages in LDS (4 KB)

struct Cell { int x0, x1, y0, rows, w0, nw; };  // columns [x0, x1), rows from y0, bitmap words w0 .. w0 + nw - 1 of each row
__device__ __forceinline__ Cell cell_of(int c, int ncx, int G, int w, int h)
{
    const int cy = c / ncx, cx = c - cy * ncx;
    Cell k;
    k.x0 = cx * G;
    k.x1 = min(k.x0 + G, w);
    k.y0 = cy * G;
    k.rows = min(k.y0 + G, h) - k.y0;
    k.w0 = k.x0 >> 6;
    k.nw = ((k.x1 - 1) >> 6) - k.w0 + 1;
    return k;
}
// item i of a cell = word w0 + i % nw of row y0 + i / nw, cut to the cell's columns
__device__ __forceinline__ u64 cell_word(const u64* bm, int words_per_row, const Cell& k, int i, int* y, int* wi)
{
    const int r = i / k.nw;
    *y = k.y0 + r;
    *wi = k.w0 + (i - r * k.nw);
    const int lo = max(k.x0 - *wi * 64, 0), hi = min(k.x1 - *wi * 64, 64);         // (0 <= lo < hi <= 64)
    const u64 mask = (hi >= 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
    return bm[(long)*y * words_per_row + *wi] & mask;
}
__device__ __forceinline__ u64 composite(u64 key, int y, int x, int w, int fast)
{
    return ((u64)sel_key(hak_key_word(key), fast) << 32) | (u64)(0xFFFFFFFFu - ((unsigned)y * (unsigned)w + (unsigned)x));
}
// removes the survivor a composite names from the bitmap and from its row's count
__device__ __forceinline__ void clear_survivor(u64 comp, u64* bm, int words_per_row, int* rc, int w)
{
    const unsigned idx = 0xFFFFFFFFu - (unsigned)comp;
    const int y = (int)(idx / (unsigned)w), x = (int)(idx - (unsigned)y * (unsigned)w);
    atomicAnd(&bm[(long)y * words_per_row + (x >> 6)], ~(1ull << (x & 63)));
    atomicSub(&rc[y], 1);
}
// sum over the block's 1024 threads, returned to every thread
__device__ __forceinline__ long long block_sum(long long v, long long* part)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                                // (part may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
    for (int i = 0; i < 16; i++) s += part[i];
    return s;
}
}

// survivors of the image vs its clamp.  One block per image.
__global__ __launch_bounds__(256) void k_grid_init(const int* __restrict__ rowcount, int h, int max_pts, int cap0, int cap1, HakGridState* gs)
{
    __shared__ int part[256];
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
        HakGridState s;
        s.cap = sel_cap(img, max_pts, cap0, cap1);
        s.active = part[0] > s.cap ? 1 : 0;
        s.q = 0;
        s.rem = 0;
        gs[img] = s;
    }
}

// n_c of every cell.  grid (nb, nimg), one wave per block: block x takes the cells x, x + nb, ...
__global__ __launch_bounds__(64) void k_grid_count(const u64* __restrict__ bitmap, int words_per_row, int w, int h, int G, int ncx, int ncells,
                                                   const HakGridState* __restrict__ gs, int* count, long cell_cap)
{
    const int img = blockIdx.y;
    if (!gs[img].active) return;
    const int lane = threadIdx.x;
    const u64* bm = bitmap + (long)img * h * words_per_row;
    for (int c = blockIdx.x; c < ncells; c += gridDim.x) {
        const Cell k = cell_of(c, ncx, G, w, h);
        const int nitems = k.rows * k.nw;
        int n = 0;
        for (int i = lane; i < nitems; i += 64) {
            int y, wi;
            n += __popcll(cell_word(bm, words_per_row, k, i, &y, &wi));
        }
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        if (lane == 0) count[(long)img * cell_cap + c] = n;
    }
}

// q = the largest quota with sum min(n_c, q) <= C, and R = C - that sum.  One block per image.
__global__ __launch_bounds__(1024) void k_grid_quota(const int* __restrict__ count, long cell_cap, int ncells, int G, HakGridState* gs)
{
    __shared__ long long part[16];
    const int img = blockIdx.x;
    if (!gs[img].active) return;
    const int cap = gs[img].cap;
    const int* cnt = count + (long)img * cell_cap;
    auto kept = [&](int q) {
        long long s = 0;
        for (int c = threadIdx.x; c < ncells; c += 1024) s += min(cnt[c], q);
        return block_sum(s, part);
    };
    int lo = 0, hi = G * G;                                         // kept(lo) <= C < kept(hi): n_c <= G * G, so kept(G * G) = S > C
    while (hi - lo > 1) {                                           // (block-uniform: every thread holds the same sums)
        const int mid = (lo + hi) >> 1;
        if (kept(mid) <= cap) lo = mid; else hi = mid;
    }
    const long long s = kept(lo);
    if (threadIdx.x == 0) {
        gs[img].q = lo;
        gs[img].rem = (int)(cap - s);
    }
}

// cells with n_c > q: find the rank-q composite T_c, publish it, clear every survivor of the cell below it.
// grid (nb, nimg), one wave per block.
__global__ __launch_bounds__(64) void k_grid_rank(const u64* __restrict__ maps, long map_stride, int p0, u64* bitmap, int words_per_row,
                                                  int w, int h, int G, int ncx, int ncells, int* rowcount,
                                                  const HakGridState* __restrict__ gs, const int* __restrict__ count, u64* comp, long cell_cap,
                                                  int fast)
{
    __shared__ u64 stage[kStage];
    __shared__ u64 tc;
    const int img = blockIdx.y;
    if (!gs[img].active) return;
    const int q = gs[img].q;
    const int lane = threadIdx.x;
    const u64* map = maps + (long)img * map_stride;
    u64* bm = bitmap + (long)img * h * words_per_row;
    int* rc = rowcount + (long)img * h;
    for (int c = blockIdx.x; c < ncells; c += gridDim.x) {          // (block-uniform, and so is every branch on n)
        const int n = count[(long)img * cell_cap + c];
        if (n <= q) continue;
        const Cell k = cell_of(c, ncx, G, w, h);
        const int nitems = k.rows * k.nw;
        if (n <= kStage) {
            int base = 0;
            for (int i0 = 0; i0 < nitems; i0 += 64) {
                int y = 0, wi = 0;
                u64 word = i0 + lane < nitems ? cell_word(bm, words_per_row, k, i0 + lane, &y, &wi) : 0ull;
                const int cnt = __popcll(word);
                int incl = cnt;
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(incl, o);
                    if (lane >= o) incl += t;
                }
                int pos = base + incl - cnt;
                while (word) {
                    const int x = wi * 64 + __ffsll((long long)word) - 1;
                    word &= word - 1;
                    if (pos < kStage) stage[pos] = composite(map[(long)y * p0 + x], y, x, w, fast);     // (always: pos < n)
                    pos++;
                }
                base += __shfl(incl, 63);
            }
            __syncthreads();
            for (int e = lane; e < n; e += 64) {
                const u64 my = stage[e];
                int r = 0;
                for (int j = 0; j < n; j++) r += stage[j] > my;
                if (r == q) tc = my;                                // (distinct composites: exactly one)
            }
            __syncthreads();
            const u64 T = tc;
            for (int e = lane; e < n; e += 64)
                if (stage[e] < T) clear_survivor(stage[e], bm, words_per_row, rc, w);
            if (lane == 0) comp[(long)img * cell_cap + c] = T;
            __syncthreads();                                        // (stage and tc are written again for the next cell)
        } else {
            // more survivors than the LDS stage holds: each lane ranks the survivors of its own words against the whole cell, read
            // from the bitmap and the key map again.  Nothing of the cell is cleared before every rank is known.
            for (int i = lane; i < nitems; i += 64) {
                int y, wi;
                u64 word = cell_word(bm, words_per_row, k, i, &y, &wi);
                while (word) {
                    const int x = wi * 64 + __ffsll((long long)word) - 1;
                    word &= word - 1;
                    const u64 my = composite(map[(long)y * p0 + x], y, x, w, fast);
                    int r = 0;
                    for (int j = 0; j < nitems; j++) {
                        int yj, wj;
                        u64 other = cell_word(bm, words_per_row, k, j, &yj, &wj);
                        while (other) {
                            const int xj = wj * 64 + __ffsll((long long)other) - 1;
                            other &= other - 1;
                            r += composite(map[(long)yj * p0 + xj], yj, xj, w, fast) > my;
                        }
                    }
                    if (r == q) tc = my;
                }
            }
            __syncthreads();
            const u64 T = tc;
            for (int i = lane; i < nitems; i += 64) {
                int y, wi;
                u64 word = cell_word(bm, words_per_row, k, i, &y, &wi);
                while (word) {
                    const int x = wi * 64 + __ffsll((long long)word) - 1;
                    word &= word - 1;
                    const u64 v = composite(map[(long)y * p0 + x], y, x, w, fast);
                    if (v < T) clear_survivor(v, bm, words_per_row, rc, w);
                }
            }
            if (lane == 0) comp[(long)img * cell_cap + c] = T;
            __syncthreads();
        }
    }
}

// the R highest candidates stay, the others are cleared.  One block per image.
__global__ __launch_bounds__(1024) void k_grid_extras(u64* bitmap, int words_per_row, int w, int h, int ncells, int* rowcount,
                                                      const HakGridState* __restrict__ gs, const int* __restrict__ count,
                                                      const u64* __restrict__ comp, long cell_cap)
{
    __shared__ long long part[16];
    const int img = blockIdx.x;
    if (!gs[img].active) return;
    const int q = gs[img].q, R = gs[img].rem;
    const int* cnt = count + (long)img * cell_cap;
    const u64* cm = comp + (long)img * cell_cap;
    u64 T = 0ull;                                                   // the R-th largest candidate: the largest T with R candidates >= T
    if (R > 0)
        for (int b = 63; b >= 0; b--) {                             // (block-uniform)
            const u64 t = T | (1ull << b);
            long long s = 0;
            for (int c = threadIdx.x; c < ncells; c += 1024) s += (cnt[c] > q && cm[c] >= t) ? 1 : 0;
            if (block_sum(s, part) >= R) T = t;
        }
    u64* bm = bitmap + (long)img * h * words_per_row;
    int* rc = rowcount + (long)img * h;
    for (int c = threadIdx.x; c < ncells; c += 1024)
        if (cnt[c] > q && (R == 0 || cm[c] < T)) clear_survivor(cm[c], bm, words_per_row, rc, w);
}

void hak_launch_grid_select(hipStream_t st, const HakBatch& b, const HakLayout& L, int max_pts, int cap0, int cap1, int fast)
{
    const int w = L.oct[0].w, h = L.oct[0].h, p = L.oct[0].p;
    const int words = (w + 63) / 64;
    const HakGridScratch& g = b.grid;
    const int G = g.G, ncx = (w + G - 1) / G, ncells = ncx * ((h + G - 1) / G);     // (<= cell_cap: G >= HAK_GRID_MIN)
    // one-wave blocks per image: a cell each up to 1024 per image and 8192 in all, the other cells in turn
    int nb = ncells < 1024 ? ncells : 1024;
    if ((long)nb * b.nimg > 8192) nb = 8192 / b.nimg > 1 ? 8192 / b.nimg : 1;
    k_grid_init<<<b.nimg, 256, 0, st>>>(b.rowcount, h, max_pts, cap0, cap1, g.st);
    k_grid_count<<<dim3((unsigned)nb, b.nimg), 64, 0, st>>>(b.bitmap, words, w, h, G, ncx, ncells, g.st, g.count, g.cell_cap);
    k_grid_quota<<<b.nimg, 1024, 0, st>>>(g.count, g.cell_cap, ncells, G, g.st);
    k_grid_rank<<<dim3((unsigned)nb, b.nimg), 64, 0, st>>>(b.maps, b.map_stride, p, b.bitmap, words, w, h, G, ncx, ncells, b.rowcount, g.st,
                                                          g.count, g.comp, g.cell_cap, fast);
    k_grid_extras<<<b.nimg, 1024, 0, st>>>(b.bitmap, words, w, h, ncells, b.rowcount, g.st, g.count, g.comp, g.cell_cap);
}

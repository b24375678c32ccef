// ransac_common.h -- the RANSAC scaffold of the three estimators (kernels_homography.hip, kernels_fundamental.hip, kernels_pnp.hip):
// everything that is not a minimal solver or an inlier test, stated once.
//
//   rs_sample<K, DRAWS>   the counter-based sample generator: K distinct indices from at most DRAWS splitmix64 draws
//   rs_word / rs_write_model / rs_read_model / rs_read_models
//                         the models scratch of the estimators with a models kernel, word-major so that every kernel touches it
//                         coalesced: words [pair][w][iterations], w = NW r + q word q of model r, w = NM NW the mask of the models
//                         that exist (bit r = model r)
//   rs_score_block<E>     the body of a score kernel: grid (pair, hypothesis block), RS_THREADS threads.  A block owns `hp` hypotheses
//                         (16 .. 256, a power of two: hak_homography_blocks) and RS_THREADS / hp slices of the list: thread t scores
//                         the up to NM models of hypothesis t mod hp against the records j = t / hp (mod RS_THREADS / hp) of each
//                         chunk.  The list streams through LDS in chunks of RS_CHUNK records, read back with ds_read_b128 where the
//                         lanes of a wave share one address (hp >= 64) or four consecutive ones (hp = 16).  Only integer counts are
//                         reduced.  Each block writes its best key (inliers << 32 | ~(4 h + r), 0 = none) to its own slot
//                         [pair][block]: no atomics and nothing to clear before a call.  The largest key is the largest count, then
//                         the smallest hypothesis, then the smallest model of it, whatever hp is.
//   rs_best_slot / rs_decode / rs_write_mask / rs_write_result
//                         head and tail of a finish kernel (one wave per pair): the pair's best key, its (inliers, hypothesis, model),
//                         the inlier mask of the winning model and the record.
//   rs_finish<E>          the body of k_fund_finish and k_pnp_finish: all of the above around a read of the winner from scratch.
//
// An estimator E supplies: list_t (the list's element), rec_t (what the tests read of one), load(list, i), struct lds with put(j, rec) /
// get(j) (a chunk's staging), NM models of NW float32 words per hypothesis, UNROLL (of the count loop, chosen per estimator),
// inlier(model, rec) const, and for its record out_t, store(record, model, inliers, hypothesis, tag, n) and no_model(model).
// Every file that includes this is built with -ffp-contract=off.
#pragma once
#include "geom_common.h"

#define RS_CHUNK 1024            // records per LDS chunk: 16 KB of float4, so that several blocks share a CU
#define RS_THREADS 256           // a score block
#define RS_MTHREADS 64           // a models block: one wave (1024 hypotheses of one pair spread over 16 CUs)

__device__ __forceinline__ unsigned long long rs_mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the sample of hypothesis h of a list with n records: draw d = 0 .. DRAWS - 1 is floor(n * hi32(mix64(seed + (DRAWS h + d + 1) GOLD))
// / 2^32) and is taken if it differs from every index taken so far; false if fewer than K were found.  idx is only ever indexed by
// compile-time values (selects, no dynamic register indexing).
template <int K, int DRAWS>
__device__ __forceinline__ bool rs_sample(unsigned seed, int h, int n, int idx[K])
{
#pragma unroll
    for (int q = 0; q < K; q++) idx[q] = -1;
    int k = 0;
#pragma unroll 1
    for (int d = 0; d < DRAWS && k < K; d++) {
        const unsigned long long r =
            rs_mix64((unsigned long long)seed + (unsigned long long)(DRAWS * (unsigned)h + d + 1) * 0x9E3779B97F4A7C15ull);
        const int j = (int)(((r >> 32) * (unsigned long long)n) >> 32);
        bool fresh = true;
#pragma unroll
        for (int q = 0; q < K - 1; q++) fresh = fresh && j != idx[q];
        if (fresh) {
#pragma unroll
            for (int q = 0; q < K; q++) idx[q] = q == k ? j : idx[q];
            k++;
        }
    }
    return k == K;
}

// ------------------------------------------------------------------------------------------------------------ models scratch
template <class E>
constexpr int rs_words() { return E::NM * E::NW + 1; }              // scratch words per hypothesis

template <class E, class W>
__device__ __forceinline__ W& rs_word(W* models, int pair, int iterations, int h, int w)
{
    return models[((long)pair * rs_words<E>() + w) * iterations + h];
}

template <class E>
__device__ __forceinline__ void rs_write_valid(unsigned* models, int pair, int iterations, int h, int valid)
{
    rs_word<E>(models, pair, iterations, h, E::NM * E::NW) = (unsigned)valid;
}

template <class E>
__device__ __forceinline__ void rs_write_model(unsigned* models, int pair, int iterations, int h, int r, const float M[E::NW])
{
#pragma unroll
    for (int q = 0; q < E::NW; q++) rs_word<E>(models, pair, iterations, h, E::NW * r + q) = __float_as_uint(M[q]);
}

template <class E>
__device__ __forceinline__ void rs_read_model(const unsigned* models, int pair, int iterations, int h, int r, float M[E::NW])
{
#pragma unroll
    for (int q = 0; q < E::NW; q++) M[q] = __uint_as_float(rs_word<E>(models, pair, iterations, h, E::NW * r + q));
}

// all models of hypothesis h to registers (zeros past the last hypothesis), returns their mask
template <class E>
__device__ __forceinline__ int rs_read_models(const unsigned* models, int pair, int iterations, int h, float M[E::NM][E::NW])
{
    const bool in = h < iterations;
#pragma unroll
    for (int r = 0; r < E::NM; r++) {
        if (in) rs_read_model<E>(models, pair, iterations, h, r, M[r]);
        else {
#pragma unroll
            for (int q = 0; q < E::NW; q++) M[r][q] = 0.0f;
        }
    }
    return in ? (int)rs_word<E>(models, pair, iterations, h, E::NM * E::NW) : 0;
}

// ------------------------------------------------------------------------------------------------------------------- score
// the staging of the estimators on match lists: float4 {x1, y1, x2, y2}
struct rs_match_records {
    typedef hak_match_pair list_t;
    typedef float4 rec_t;
    struct lds {
        float4 a[RS_CHUNK];
        __device__ __forceinline__ void put(int j, const float4 r) { a[j] = r; }
        __device__ __forceinline__ float4 get(int j) const { return a[j]; }
    };
    static __device__ __forceinline__ float4 load(const hak_match_pair* m, int i) { return fd_load(m, i); }
};

// the views of the two estimators on match lists.  Beside what the score block needs, a view states its record: out_t, store and
// no_model (the model of a record without one); those whose refit starts from a record (refit_common.h) add load_model (false
// unless the record holds a finite model with hypothesis >= 0) and tag (the record's third int: root / solution).
// homography: one model of 9 words per hypothesis; its refit runs inside the finish kernel, so no record is ever read
struct hg_est : rs_match_records {
    static constexpr int NM = 1, NW = 9, UNROLL = 4;
    typedef hak_homography out_t;
    float t2;
    __device__ __forceinline__ bool inlier(const float H[9], const float4 r) const { return hg_inlier(H, r, t2); }
    static __device__ __forceinline__ void store(hak_homography& o, const float H[9], int inliers, int hypothesis, int tag, int n)
    {
#pragma unroll
        for (int k = 0; k < 9; k++) o.H[k] = H[k];
        o.inliers = inliers; o.hypothesis = hypothesis; o.refined = tag; o.n = n;
    }
    static __device__ __forceinline__ void no_model(float H[9])
    {
#pragma unroll
        for (int k = 0; k < 9; k++) H[k] = k % 4 == 0 ? 1.0f : 0.0f;
    }
};

// fundamental matrix: three models (the cubic's roots) of 9 words per hypothesis
struct fd_est : rs_match_records {
    static constexpr int NM = 3, NW = 9, UNROLL = 2;
    typedef hak_fundamental out_t;
    float t2;
    __device__ __forceinline__ bool inlier(const float F[9], const float4 r) const { return fd_inlier(F, r, t2); }
    static __device__ __forceinline__ bool load_model(const hak_fundamental& o, float F[9])
    {
        bool model = o.hypothesis >= 0;
#pragma unroll
        for (int k = 0; k < 9; k++) { F[k] = o.F[k]; model = model && __builtin_isfinite(F[k]); }
        return model;
    }
    static __device__ __forceinline__ int tag(const hak_fundamental& o) { return o.root; }
    static __device__ __forceinline__ void store(hak_fundamental& o, const float F[9], int inliers, int hypothesis, int tag, int n)
    {
#pragma unroll
        for (int k = 0; k < 9; k++) o.F[k] = F[k];
        o.inliers = inliers; o.hypothesis = hypothesis; o.root = tag; o.n = n;
    }
    static __device__ __forceinline__ void no_model(float F[9])
    {
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = 0.0f;
    }
};

__device__ __forceinline__ unsigned long long rs_wmax(unsigned long long key)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    return key;
}

// the hypothesis of this thread in a score block
__device__ __forceinline__ int rs_block_hypothesis(int hp) { return blockIdx.y * hp + (threadIdx.x & (hp - 1)); }

// M, valid: the models of rs_block_hypothesis(hp) and the mask of those that exist
template <class E>
__device__ __forceinline__ void rs_score_block(const E est, const typename E::list_t* m, int n, int hp, const float M[E::NM][E::NW],
                                               int valid, unsigned long long* slots)
{
    __shared__ typename E::lds rec;
    __shared__ int part[E::NM][RS_THREADS];
    __shared__ unsigned long long wbest[RS_THREADS / HAK_WAVE];
    const int pair = blockIdx.x, t = threadIdx.x;
    const int h = rs_block_hypothesis(hp);
    const int slice = t / hp, nslice = RS_THREADS / hp;
    static_assert(E::NM >= 1 && E::NM <= 4, "a key holds the model's number in two bits");
    // (scalars: a counter array indexed by a loop is turned into a vector before that loop is unrolled, and the loop vectoriser then
    // leaves the count loop alone)
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int b0 = 0; b0 < n; b0 += RS_CHUNK) {
        const int len = min(RS_CHUNK, n - b0);
        __syncthreads();                                            // the previous chunk is consumed
        for (int j = t; j < len; j += RS_THREADS) rec.put(j, E::load(m, b0 + j));
        __syncthreads();
        if (valid) {
#pragma unroll E::UNROLL
            for (int j = slice; j < len; j += nslice) {
                const typename E::rec_t x = rec.get(j);
                c0 += est.inlier(M[0], x) ? 1 : 0;
                if constexpr (E::NM > 1) c1 += est.inlier(M[1], x) ? 1 : 0;
                if constexpr (E::NM > 2) c2 += est.inlier(M[2], x) ? 1 : 0;
                if constexpr (E::NM > 3) c3 += est.inlier(M[3], x) ? 1 : 0;
            }
        }
    }
    const int cnt[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int r = 0; r < E::NM; r++) part[r][t] = cnt[r];
    __syncthreads();
    unsigned long long key = 0;
    if (t < hp) {
#pragma unroll
        for (int r = 0; r < E::NM; r++) {
            int s = 0;
            for (int k = 0; k < nslice; k++) s += part[r][t + k * hp];
            const unsigned long long kr = ((unsigned long long)s << 32) | (unsigned)~(4u * (unsigned)h + (unsigned)r);
            if ((valid >> r & 1) && kr > key) key = kr;
        }
    }
    key = rs_wmax(key);
    if ((t & (HAK_WAVE - 1)) == 0) wbest[t / HAK_WAVE] = key;
    __syncthreads();
    if (t == 0) {
        unsigned long long b = wbest[0];
#pragma unroll
        for (int w = 1; w < RS_THREADS / HAK_WAVE; w++) b = wbest[w] > b ? wbest[w] : b;
        slots[(long)pair * gridDim.y + blockIdx.y] = b;
    }
}

// ------------------------------------------------------------------------------------------------------------------ finish
// the largest key of the pair's slots (one wave, every lane returns it)
__device__ __forceinline__ unsigned long long rs_best_slot(const unsigned long long* slots, int hblocks)
{
    const unsigned long long* s = slots + (long)blockIdx.x * hblocks;
    unsigned long long key = 0;
    for (int k = threadIdx.x; k < hblocks; k += HAK_WAVE) key = s[k] > key ? s[k] : key;
    return rs_wmax(key);
}

// false: no model (inliers 0, hypothesis -1, model 0)
__device__ __forceinline__ bool rs_decode(unsigned long long key, int& inliers, int& hyp, int& r)
{
    const unsigned id = ~(unsigned)key;                             // 4 h + r
    inliers = (int)(key >> 32);
    hyp = key != 0 ? (int)(id >> 2) : -1;
    r = key != 0 ? (int)(id & 3u) : 0;
    return key != 0;
}

// mask[i] = record i passes the test of M (all 0 when there is no model); one wave
template <class E>
__device__ __forceinline__ void rs_write_mask(const E est, unsigned char* masks, long mask_stride, const typename E::list_t* m, int n,
                                              const float M[E::NW], bool has)
{
    if (!masks) return;
    unsigned char* mk = masks + (long)blockIdx.x * mask_stride;
    for (int i = threadIdx.x; i < n; i += HAK_WAVE) mk[i] = (has && est.inlier(M, E::load(m, i))) ? 1 : 0;
}

// the end of every finish and refit kernel (one wave per pair): the mask of M, then lane 0 writes the pair's record.  Without a model
// the caller passes E::no_model, inliers 0, hypothesis -1, tag 0.
template <class E>
__device__ __forceinline__ void rs_write_result(const E est, const typename E::list_t* m, int n, const float M[E::NW], int inliers,
                                                int hypothesis, int tag, typename E::out_t* out, unsigned char* masks,
                                                long mask_stride)
{
    rs_write_mask(est, masks, mask_stride, m, n, M, hypothesis >= 0);
    if (threadIdx.x == 0) {
        typename E::out_t o;
        E::store(o, M, inliers, hypothesis, tag, n);
        out[blockIdx.x] = o;
    }
}

// the body of a finish kernel behind a models kernel: the winner is read back from scratch (its hypothesis is below `iterations`)
template <class E>
__device__ __forceinline__ void rs_finish(const E est, const typename E::list_t* m, int n, int iterations, int hblocks,
                                          const unsigned* models, const unsigned long long* slots, typename E::out_t* out,
                                          unsigned char* masks, long mask_stride)
{
    float M[E::NW];
    E::no_model(M);
    int inl, hyp, r;
    if (rs_decode(rs_best_slot(slots, hblocks), inl, hyp, r)) rs_read_model<E>(models, blockIdx.x, iterations, hyp, r, M);
    rs_write_result(est, m, n, M, inl, hyp, r, out, masks, mask_stride);
}

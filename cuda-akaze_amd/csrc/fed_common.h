// fed_common.h -- element traits, DPP wave shifts and the one-row FED update shared by the streaming kernels
// (kernels_fed.hip: FED steps only; kernels_fedsf.hip: low-pass + conductivity + FED steps in one pass).
#pragma once
#include "hak_internal.h"
#include <type_traits>
#include <utility>

// The same streaming kernel serves both pipelines: V = float (akaze) and V = int (fastakaze, 16.16 fixed point,
// akazed.cu:3448-3470).  Integer arithmetic wraps (unsigned add / mul), so every regrouping used below for the float
// path (shared pair sums, shared flux products, tE + tW = P[x+1] - P[x]) is exact for the int path as well.
template <typename V> struct FedV;
template <> struct FedV<float> { using V4 = float4; };
template <> struct FedV<int> { using V4 = int4; };
// (vadd / vsub / vmul / vneg, wrapping for int: pixel_rules.h)
__device__ __forceinline__ float4 mk4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
__device__ __forceinline__ int4 mk4(int a, int b, int c, int d) { return make_int4(a, b, c, d); }
// L' from the flux sum:  float: fma(0.5*tau, sum, L) (akazed.cu:1263);  int: ((stepfac * (sum >> 16)) >> 16) + L (akazed.cu:3468-3469)
__device__ __forceinline__ float vstep(float f, float sum, float L) { return fmaf(f, sum, L); }
__device__ __forceinline__ int vstep(int f, int sum, int L) { return vadd(vmul(f, sum >> 16) >> 16, L); }

template <typename V, int NS>
struct FedFacs { V f[NS]; };

// bound_ctrl = 1 with a zero `old`: the end lane (no source) reads 0 -- lanes 0 and 63 are strip margin -- and the
// compiler needs no copy of `v` to seed the destination (an `old = v` shift costs one extra v_mov each)
__device__ __forceinline__ int hak_dpp_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }   // lane i <- lane i-1
__device__ __forceinline__ int hak_dpp_shl1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true); }   // lane i <- lane i+1
__device__ __forceinline__ float wave_shr1(float v) { return __int_as_float(hak_dpp_shr1(__float_as_int(v))); }
__device__ __forceinline__ float wave_shl1(float v) { return __int_as_float(hak_dpp_shl1(__float_as_int(v))); }
// Integer shifts are made opaque to the optimiser: ROCm 7.2's DPP-combine pass folded `a - shift(b)` into
// `v_sub_u32_dpp shift(b), a` (operands swapped, no v_subrev) in k_hessian_stream<int>: Lx came out with the sign of its
// second term flipped in every lane's first column.  The empty asm keeps the shift a plain v_mov_b32_dpp.
__device__ __forceinline__ int wave_shr1(int v)
{
    int r = hak_dpp_shr1(v);
    asm volatile("" : "+v"(r));
    return r;
}
__device__ __forceinline__ int wave_shl1(int v)
{
    int r = hak_dpp_shl1(v);
    asm volatile("" : "+v"(r));
    return r;
}
// The same shifts with the end lane (no source) keeping `keep` instead of reading 0 (bound_ctrl off): a strip's end lane takes a
// value from outside the strip (kernels_hessian_stream.hip).  The integer form stays opaque like the one above.
__device__ __forceinline__ float wave_shr1_keep(float keep, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(keep), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1_keep(float keep, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(keep), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ int wave_shr1_keep(int keep, int v)
{
    int r = __builtin_amdgcn_update_dpp(keep, v, 0x138, 0xf, 0xf, false);
    asm volatile("" : "+v"(r));
    return r;
}
__device__ __forceinline__ int wave_shl1_keep(int keep, int v)
{
    int r = __builtin_amdgcn_update_dpp(keep, v, 0x130, 0xf, 0xf, false);
    asm volatile("" : "+v"(r));
    return r;
}

// 16-byte store with the `nt` bit: planes that are written once and next read sparsely or much later should not displace
// the streams other kernels are reading from L2 / Infinity Cache (measured: Hessian -3 %, +3 % end to end)
typedef float hak_v4f __attribute__((ext_vector_type(4)));
typedef int hak_v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void hak_store_nt(float4* p, const float4 v)
{
    const hak_v4f t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<hak_v4f*>(p));
}
__device__ __forceinline__ void hak_store_nt(int4* p, const int4 v)
{
    const hak_v4i t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<hak_v4i*>(p));
}

// ---- predicated 16-byte stores without a branch.  A store inside `if (row in segment && lane owns its columns)` makes the
// compiler's s_waitcnt insertion assume it was NOT issued, so the wait for a prefetched row becomes vmcnt(<loads in flight>)
// and -- vmcnt retiring in order -- every row then also waits for all earlier stores of the wave to complete: the streaming
// kernels exposed the full store latency once per row.  A raw buffer store drops lanes whose offset is out of range in
// hardware, so the predicate moves into the offset (HAK_BUF_OOB) and the instruction is unconditional and countable.
typedef unsigned hak_v4u __attribute__((ext_vector_type(4)));
// out-of-range marker = num_records of every resource made below.  Offsets are SUMS of a lane part (column + plane offset)
// and a wave-uniform row part, either of which may carry the marker: valid sums stay below 2^30 (launchers check plane
// offset + plane size), one marker gives [2^30, 2^31), two give 2^31 -- all out of range, none wraps.
constexpr unsigned HAK_BUF_OOB = 0x40000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t hak_buf_rsrc(void* base)
{
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, HAK_BUF_OOB, 0x00020000);     // raw buffer, gfx9 dword-3 format bits
}
// voff: byte offset per lane (>= HAK_BUF_OOB = the lane writes nothing).  aux 2 = nt (see hak_store_nt).
// The scalar offset field is deliberately the constant 0: with an SGPR there, LLVM's hazard recognizer assumes that a
// following VALU write of the 128-bit store data needs no wait state (GCNHazardRecognizer::createsVALUHazard), but on
// gfx950 the next instruction did overwrite the data of the last four lanes of each 16-lane pass before the store had
// read them (lanes 12-15 / 28-31 / ... of one row wrong, only in some code shapes).  Plane offsets therefore go into voff.
__device__ __forceinline__ void hak_buf_store_nt(__amdgpu_buffer_rsrc_t r, unsigned voff, const float4 v)
{
    const hak_v4u d = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(d, r, voff, 0, 2);
}
__device__ __forceinline__ void hak_buf_store_nt(__amdgpu_buffer_rsrc_t r, unsigned voff, const int4 v)
{
    const hak_v4u d = {(unsigned)v.x, (unsigned)v.y, (unsigned)v.z, (unsigned)v.w};
    __builtin_amdgcn_raw_buffer_store_b128(d, r, voff, 0, 2);
}

// 16-byte streaming load of a row piece.  HAK_NT_LOADS (A/B builds only) marks it non-temporal.
__device__ __forceinline__ float4 hak_load_stream(const float4* p)
{
#ifdef HAK_NT_LOADS
    const hak_v4f t = __builtin_nontemporal_load(reinterpret_cast<const hak_v4f*>(p));
    return make_float4(t.x, t.y, t.z, t.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ int4 hak_load_stream(const int4* p)
{
#ifdef HAK_NT_LOADS
    const hak_v4i t = __builtin_nontemporal_load(reinterpret_cast<const hak_v4i*>(p));
    return make_int4(t.x, t.y, t.z, t.w);
#else
    return *p;
#endif
}

constexpr int pmod(int a, int m) { return ((a % m) + m) % m; }

// ---- the lane vector of the FED kernels: the W consecutive pixels of one row that a lane owns.  W = 4 (a wave's strip is 256 px
// wide, 16 bytes per lane and row) or W = 2 (128 px, 8 bytes): every ring of the streaming kernels costs W registers per slot, so
// the 2-px form keeps twice as many fused levels in the same register budget (kernels_fed.hip).  A wave moves 64 W contiguous
// elements per row either way.
template <typename V, int W> struct alignas(sizeof(V) * W) FedPx { V e[W]; };
template <typename V, int W> __device__ __forceinline__ FedPx<V, W> px_fill(const V a)
{
    FedPx<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.e[j] = a;
    return r;
}
template <typename V, int W> __device__ __forceinline__ FedPx<V, W> px_add(const FedPx<V, W>& a, const FedPx<V, W>& b)
{
    FedPx<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.e[j] = vadd(a.e[j], b.e[j]);
    return r;
}
template <typename V, int W> __device__ __forceinline__ FedPx<V, W> px_neg(const FedPx<V, W>& a)
{
    FedPx<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.e[j] = vneg(a.e[j]);
    return r;
}
template <typename V, int W> __device__ __forceinline__ FedPx<V, W> px_sel(const bool c, const FedPx<V, W>& a, const FedPx<V, W>& b)
{
    FedPx<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.e[j] = c ? a.e[j] : b.e[j];
    return r;
}
// one row piece as ONE 16- or 8-byte access (p aligned to it).  HAK_NT_LOADS (A/B builds only) marks the load non-temporal.
template <typename V, int W> __device__ __forceinline__ FedPx<V, W> px_load(const V* p)
{
    typedef V vec __attribute__((ext_vector_type(W)));
#ifdef HAK_NT_LOADS
    const vec t = __builtin_nontemporal_load(reinterpret_cast<const vec*>(p));
#else
    const vec t = *reinterpret_cast<const vec*>(p);
#endif
    FedPx<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.e[j] = t[j];
    return r;
}
template <typename V, int W> __device__ __forceinline__ void px_store_nt(V* p, const FedPx<V, W>& v)    // (see hak_store_nt)
{
    typedef V vec __attribute__((ext_vector_type(W)));
    vec t;
#pragma unroll
    for (int j = 0; j < W; j++) t[j] = v.e[j];
    __builtin_nontemporal_store(t, reinterpret_cast<vec*>(p));
}
__device__ __forceinline__ unsigned px_bits(float a) { return __float_as_uint(a); }
__device__ __forceinline__ unsigned px_bits(int a) { return (unsigned)a; }
template <typename V, int W> __device__ __forceinline__ void px_buf_store_nt(__amdgpu_buffer_rsrc_t r, unsigned voff, const FedPx<V, W>& v)
{                                                                                                       // (see hak_buf_store_nt)
    if constexpr (W == 4) {
        const hak_v4u d = {px_bits(v.e[0]), px_bits(v.e[1]), px_bits(v.e[2]), px_bits(v.e[3])};
        __builtin_amdgcn_raw_buffer_store_b128(d, r, voff, 0, 2);
    } else {
        static_assert(W == 2, "a lane owns 4 or 2 pixels");
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        const v2u d = {px_bits(v.e[0]), px_bits(v.e[1])};
        __builtin_amdgcn_raw_buffer_store_b64(d, r, voff, 0, 2);
    }
}

// horizontal pair sums of one g row as seen by a lane: h[j] = g[x0+j] + g[x0+j+1], j = 0..W-1 (the last needs the right lane's g[0])
template <typename V, int W> struct GHrow { V h[W]; };
template <typename V, int W> __device__ __forceinline__ GHrow<V, W> fed_gh(const FedPx<V, W>& g)
{
    const V gr = wave_shl1(g.e[0]);
    GHrow<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.h[j] = vadd(g.e[j], j + 1 < W ? g.e[(j + 1) % W] : gr);
    return r;
}

// One output row (W px per lane) of one FED level from shared flux products.
//   horizontal: P[j] = (g[x0+j-1] + g[x0+j]) * (L[x0+j] - L[x0+j-1]);  term_E(x) = P[x+1], term_W(x) = -P[x] exactly, so
//               (tE + tW) = P[j+1] - P[j] bit for bit.  P[0] is the left lane's P[W] -- the same two operands in the same
//               order -- and arrives by ONE wave shift instead of being recomputed (shift + subtract + multiply).
//   vertical:   Q[r] = (g[r] + g[r+1]) * (L[r+1] - L[r]);  term_S(r) = Q[r], term_N(r) = -Q[r-1] exactly (IEEE addition
//               commutes, negating a factor negates the product), so  ((tE + tW) + tS) + tN = ((P[j+1] - P[j]) + Qn) - Qp.
//               Each Q row is formed once and serves the row above and the row below it.
// Reflect-101 (akazed.cu:1251-1254): x == 0: tW = tE -> P[0] := -P[1];  x == w-1: tE = tW -> P[W] := -P[W-1];  the callers
// do the same in y: row 0: Qp := -Qn, row h-1: Qn := -Qp.  Same value and same rounding as the reference expression
//   (f+fE)(LE-L) + (f+fW)(LW-L) + (f+fS)(LS-L) + (f+fN)(LN-L)  then  fma(stepfac, sum, L)    (akazed.cu:1259-1263)
// for both element types (integer arithmetic wraps, so the regroupings are exact there too).
template <bool XEDGE, typename V, int W>
__device__ __forceinline__ FedPx<V, W> fed_row(const FedPx<V, W>& Lc, const GHrow<V, W>& gh, const FedPx<V, W>& Qn, const FedPx<V, W>& Qp,
                                               int x0, int w, V stepfac)
{
    const V Lr = wave_shl1(Lc.e[0]);
    V P[W + 1];
#pragma unroll
    for (int j = 1; j <= W; j++) P[j] = vmul(gh.h[j - 1], vsub(j < W ? Lc.e[j % W] : Lr, Lc.e[j - 1]));
    if (XEDGE) P[W] = x0 + W - 1 == w - 1 ? vneg(P[W - 1]) : P[W];   // borderAdd(x,1,w) = w-2 (w % 4 == 0: x == w-1 is a lane's last pixel)
    P[0] = wave_shr1(P[W]);                                 // (executes with every lane active: not inside the select)
    if (XEDGE) P[0] = x0 == 0 ? vneg(P[1]) : P[0];          // abs(x-1) = 1
    FedPx<V, W> o;
#pragma unroll
    for (int j = 0; j < W; j++) o.e[j] = vstep(stepfac, vsub(vadd(vsub(P[j + 1], P[j]), Qn.e[j]), Qp.e[j]), Lc.e[j]);
    return o;
}
// Q[r] of one level: gv = g[r] + g[r+1], Ln = row r+1, Lc = row r
template <typename V, int W>
__device__ __forceinline__ FedPx<V, W> fed_q(const FedPx<V, W>& gv, const FedPx<V, W>& Ln, const FedPx<V, W>& Lc)
{
    FedPx<V, W> r;
#pragma unroll
    for (int j = 0; j < W; j++) r.e[j] = vmul(gv.e[j], vsub(Ln.e[j], Lc.e[j]));
    return r;
}
// the float4 / int4 select of the other streaming kernels (kernels_hessian_stream.hip)
template <typename V4> __device__ __forceinline__ V4 vsel4(const bool c, const V4 a, const V4 b)
{
    return mk4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

// ---- FED steps per launch (hak_fed_groups / hak_fed_group_size state how a cycle is cut): a group of at most HAK_FED_WIDE_STEPS
// steps runs on 4-px lanes, a longer one (up to HAK_FED_MAX_FUSE) on 2-px lanes
constexpr int HAK_FED_WIDE_STEPS = 4;
constexpr int fed_lane_px(int ns) { return ns <= HAK_FED_WIDE_STEPS ? 4 : 2; }
// ring geometry of a launch that fuses NS levels: the g-sum rings need NS + 1 slots, and every ring size (2 L / Q rows per level,
// the prefetch distance 3, the 6- and 3-row rings of kernels_fedsf.hip) divides the number of rows one unrolled loop body handles
constexpr int fed_gsum_slots(int ns) { return ns + 1 <= 6 ? 6 : 9; }
constexpr int fed_unroll(int ns) { return ns + 1 <= 6 ? 6 : 18; }


// (the sigma=1 low-pass hak_conv5 / SfTaps, the gradient energy hak_dif2 and the conductivity as the element type hak_g_as: pixel_rules.h)

// ---- 1 / d for the PM_G2 conductivity g = 1 / (1 + dif2).  hipcc's correctly rounded float division costs ~11 instructions
// (v_div_scale x2, v_rcp, four fmas, v_div_fmas, v_div_fixup).  For 1 <= d < 2^64 the three-instruction sequence below --
// v_rcp_f32 plus one Newton step with explicit fmas -- returns the identical bits: checked exhaustively over all 2^29
// floats of that range on gfx950 (tools/rcp_exhaustive.hip; the library's own copy is re-checked by hak_op_rcp_check in
// the GPU tests).  Callers must send anything else (NaN, inf, >= 2^64) through the IEEE division.
__device__ __forceinline__ float hak_rcp_newton(float d)
{
    const float y0 = __builtin_amdgcn_rcpf(d);
    const float e = fmaf(-d, y0, 1.0f);
    return fmaf(e, y0, y0);
}

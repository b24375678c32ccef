// hak_sequence.hip -- the launch sequence of libhipakaze: which kernels one detect + describe call enqueues, on which streams, and
// (float pipeline) the captured graph it is replayed from.  Host code only: the kernels and their launchers live in kernels_*.hip.
// Host orchestration restates Akazer::detectAndCompute / detect (akaze.cpp:101-150, 240-503) and fastDetectAndCompute / fastDetect
// (akaze.cpp:153-201, 506-743) with every per-image scalar kept on the device (kcontrast, point counts), one launch sequence per
// BATCH of images (blockIdx.z = image) and no host synchronisation inside the sequence.  The two pipelines share one level
// sequence, build_level<V> / hessian_level<V>: V = float (AKAZE) or int (FAST, 16.16 fixed point on int32 planes of the same arena).
#include "hak_internal.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>

#include "hak_ctx.h"

static thread_local const char* g_launch_err = nullptr;
void hak_note_launch_error(const char* msg) { if (!g_launch_err) g_launch_err = msg; }

// The reference issues everything on stream 0 (akaze.cpp:101-150, 55-64): whatever its caller enqueued on the default stream before a call
// -- a hipMemset of an output array, an asynchronous upload, a kernel of its own -- is finished when the call's first kernel starts.  A
// context's streams are non-blocking; this makes the call's stream wait for the NULL stream's work enqueued so far (device-side: an event
// record there, a wait here; nothing when the context runs on the NULL stream itself).  Never inside a stream capture: every caller sits
// in front of run_detect_inner's capture.
void order_after_null_stream(hak_ctx* c, hipStream_t st)
{
    if (!c || !c->null_order || !c->ev_null || st == nullptr) return;
    // (an idle NULL stream -- the reference's own call pattern with its blocking copies -- costs one query; the cross-queue dependency
    // itself was measured at ~15 us per call: 0.54 -> 0.55 ms for the pair call when taken unconditionally)
    const hipError_t q = hipStreamQuery(nullptr);
    if (q == hipSuccess) return;
    (void)hipGetLastError();
    if (hipEventRecord(c->ev_null, nullptr) != hipSuccess || hipStreamWaitEvent(st, c->ev_null, 0) != hipSuccess) (void)hipGetLastError();
}

// ------------------------------------------------------- the launch sequence
// The key map must be all zero when a launch sequence starts; every sequence restores that itself (k_clear_cand_maps).  If a
// call fails between writing the map and cleaning it up, the flag stays set and the next call clears the map in full -- eagerly
// on the context's stream and never inside a stream capture, so a replayed graph cannot miss (or needlessly carry) the clear.
void maps_guard_begin(hak_ctx* c)
{
    if (c->maps_dirty) {
        const size_t h = c->L.oct[0].h, words = (c->L.oct[0].w + 63) / 64, B = c->cfg.batch;
        (void)hipMemsetAsync(c->maps, 0, sizeof(unsigned long long) * (size_t)c->L.oct[0].plane * B, c->stream);
        (void)hipMemsetAsync(c->bitmap, 0, sizeof(unsigned long long) * h * words * B, c->stream);
        (void)hipMemsetAsync(c->rowcount, 0, sizeof(int) * h * B, c->stream);
    }
    c->maps_dirty = true;
}
int maps_guard_end(hak_ctx* c, int rc)
{
    if (!rc) c->maps_dirty = false;
    // (on the stream the sequence ended on: a marker on the caller's idle stream would make the next call's idle test fail)
    if (c->ev_last) (void)hipEventRecord(c->ev_last, c->sync_stream ? c->sync_stream : c->stream);
    return rc;
}

// kernels_level.hip's one-launch sublevel: by the size rule unless a test forces the streaming kernels (fuse_sf == 2)
static bool level_tile_pays(const hak_ctx* c, const HakOct& oc, int nimg)
{
    const int mode = c->knobs.level_tile;
    if (mode != 1) return mode != 0;
    // (round 4, measured: taking the tile kernel for the latency-bound small octaves of a LARGE batch as well -- octave 3, or octaves
    // 2-3, of 512 images -- cuts the FED launches from 46 to 26 / 18 and costs 8-17 ms per sequence: its halo work, (T + 2n)^2 / T^2
    // of the useful work, is only worth paying where launches, not bytes or arithmetic, are the cost)
    return c->knobs.fuse_sf != 2 && (long)oc.w * oc.h * nimg <= HAK_LEVEL_TILE_MAX_PX;
}

// Launch-bound sequences -- a single image: octave 0 small enough for k_level_tile -- are issued in SPINE order (enqueue_detect) and
// eagerly instead of as a replayed graph: their time is the longest dependency chain, not bytes.  Round 4 tried the same for a PAIR
// (two to four images; HAK_SPINE_MAX_PX widens the rule): with four chains of two-image kernels in flight the kernels slow each other
// down and the call got slower, 0.60 -> 0.635 ms (8 hardware queues) / 0.675 (4) -- a pair is bound by the GPU time of its small
// kernels, the replayed per-octave order is the better one for it (profiles/r04_pair_timeline.txt).
static bool spine_pays(const hak_ctx* c, int nimg)
{
    const long max_px = c->knobs.spine_max_px;
    if (max_px > 0 && c->knobs.level_tile == 1) return c->knobs.fuse_sf != 2 && (long)c->L.oct[0].w * c->L.oct[0].h * nimg <= max_px;
    return level_tile_pays(c, c->L.oct[0], nimg);
}

// ------------------------------------------------------- one level, both pipelines: what it needs besides (o, s) and the stream
struct LevelArgs {
    hak_ctx* c;
    HakBatch b;
    const void* images;             // float (AKAZE) or uint8 (FAST) images, image_stride elements apart, rows of `pitch` elements
    long image_stride;
    int pitch, nimg;
    bool hess_fused[HAK_MAX_OCTAVES * HAK_MAX_SCALES];      // the level's Hessian ran inside k_level_tile
    bool hess_lp[HAK_MAX_OCTAVES * HAK_MAX_SCALES];         // the level's Hessian low-passes Lt(o,s-1) itself: `smooth` was not written
};

static LevelArgs level_args(hak_ctx* c, const void* images, long image_stride, int pitch, int nimg)
{
    const HakLayout& L = c->L;
    LevelArgs a{c, HakBatch{c->arena, L.arena, nimg, c->state, c->maps, L.oct[0].plane, c->bitmap, c->rowcount, c->cand, c->cand_cap, &c->knobs,
                            c->perm, c->cfg.max_pts},
                images, image_stride, pitch, nimg, {}, {}};
    hak_batch_selection(c, a.b);
    return a;
}

template <typename V> constexpr bool is_fast = std::is_same_v<V, int>;
template <typename V> static const V* taps_of(const float* f, const int* i) { if constexpr (is_fast<V>) return i; else return f; }
// extrema threshold: cfg.dthreshold, FAST: idthreshold = 65 (akaze.cpp:559)
template <typename V> static V dthreshold_of(const hak_ctx* c) { if constexpr (is_fast<V>) return 65; else return c->cfg.dthreshold; }

// ---- part A of level (o, s): build Lt(o, s) and the sigma=1 low-pass `smooth` the level's Hessian reads (akaze.cpp:325-421; FAST:
// akaze.cpp:589-695).  smooth_alt != nullptr: the level's sigma=1 low-pass goes there instead of the octave's `smooth` plane
// (side-stream Hessians of enqueue_detect)
template <typename V>
static void build_level(LevelArgs& a, int o, int s, hipStream_t st, V* smooth_alt = nullptr)
{
    hak_ctx* const c = a.c;
    hak_ctx* const pc = is_fast<V> ? nullptr : c;           // FAST records no ProfScope
    const hak_config& cfg = c->cfg;
    const HakLayout& L = c->L;
    const HakKnobs& kn = c->knobs;
    const int nimg = a.nimg;
    V* const A = reinterpret_cast<V*>(c->arena);
    const long S = L.arena;
    const HakOct oc = L.oct[o];
    V* smooth = smooth_alt ? smooth_alt : A + L.smooth_off[o];
    V* flow = A + L.flow_off[o];
    V* tmp = A + L.tmp_off[o];
    const LevelPlan& lp = c->plan[(size_t)o * L.ms + s];
    V* Lt = A + L.lt(o, s);
    const V* taps1 = taps_of<V>(c->taps1, c->itaps1);
    // FAST does not touch fed_launches / fed_fused_bytes (hak_query_traffic reports the float sequence)
    auto count_fed = [&](int nl, double bytes) { if constexpr (!is_fast<V>) { c->fed_launches += nl; c->fed_fused_bytes += bytes; } };
    if (o == 0 && s == 0) {                                                   // akaze.cpp:325-332 in two passes over img
        ProfScope ps(pc, HAK_PROF_CONTRAST, st);
        // `tmp` is free until the FED cycle of (0,1): it takes the gradient plane the histogram pass reads
        const auto* img = static_cast<const std::conditional_t<is_fast<V>, unsigned char, float>*>(a.images);
        const V* taps_base = taps_of<V>(c->taps_base, c->itaps_base);
        const bool based = hak_launch_base_level(st, img, a.image_stride, a.pitch, Lt, tmp, S, oc.w, oc.h, oc.p, nimg, taps1, taps_base, c->base_R,
                                                 c->state, cfg.per, L.noct, kn);
        if constexpr (is_fast<V>) {                                           // akaze.cpp:589-623 when the fused prologue does not cover base_R
            if (!based) {
                hak_launch_lowpass(st, img, a.image_stride, a.pitch, smooth, S, oc.w, oc.h, oc.p, nimg, taps1, 2);
                hak_launch_contrast(st, smooth, S, oc.w, oc.h, oc.p, nimg, c->state, cfg.per, L.noct);
                hak_launch_lowpass(st, img, a.image_stride, a.pitch, Lt, S, oc.w, oc.h, oc.p, nimg, taps_base, c->base_R);
            }
        } else (void)based;
        return;
    }
    const int n = lp.nsteps;
    // small launches (single images, small octaves of small batches): the whole sublevel in one launch out of LDS tiles --
    // octave heads (one launch instead of decimation + conductivity + FED groups) and every cycle long enough that the tile
    // kernel's halo work costs less than the launches it saves (by the size rule: n >= 8, i.e. octaves 2 and up of the demo
    // schedule; shorter cycles keep k_smooth_flow + k_fed_multi, which spend less GPU time per pixel)
    // FAST takes the tile kernel for every cycle, without the level_min_steps condition: as it has been since round 3; not re-measured here
    if (level_tile_pays(c, oc, nimg) && (is_fast<V> || s == 0 || n >= kn.level_min_steps || kn.level_tile == 2)) {
        ProfScope ps(pc, HAK_PROF_FED, st);
        // (the level's Hessian rides along when the cycle is long enough: hess_fused tells hessian_level below)
        const int nl = hak_launch_level_tile(st, s == 0 ? A + L.lt(o - 1, 0) : A + L.lt(o, s - 1), s == 0 ? L.oct[o - 1] : oc, s == 0, smooth, Lt, tmp, S,
                                             oc, nimg, taps1, cfg.diffusivity, lp.tau.data(), n, c->state, o,
                                             kn.level_hess ? A + L.dxy(o, s) : nullptr, lp.sigma_size, &a.b, &L, &c->htab, s, dthreshold_of<V>(c),
                                             &a.hess_fused[o * HAK_MAX_SCALES + s]);
        count_fed(nl, (s == 0 ? 1.0 * L.oct[o - 1].w * L.oct[o - 1].h : 4.0 * oc.w * oc.h) + 8.0 * oc.w * oc.h + (nl - 1) * 12.0 * oc.w * oc.h);
        return;
    }
    // the FED cycle in G fused launches, ping-pong Lt <-> tmp so that the last one lands in Lt (widths that do not allow 16-byte
    // rows: G = n, one step per launch)
    // FAST keeps the 4-px groups: the deeper 2-px kernels are built and measured for the float sequence only
    const int G = hak_fed_groups(n, is_fast<V> && kn.max_fuse > 4 ? 4 : kn.max_fuse, oc.w, hak_fed_wide_only(o, oc.w));
    const int ns0 = hak_fed_group_size(n, G, 0);
    V* dst0 = (G % 2 == 1) ? Lt : tmp;
    const V* fsrc;              // input of the first FED launch
    bool fused_first = false;
    if (s == 0) {                                                             // akaze.cpp:369-392 (FAST: 640-662)
        // octave head: decimation + low-pass + conductivity + the first FED group in one streaming pass when covered
        if (hak_fed_sf_covers(kn, cfg.diffusivity, oc, nimg, &L.oct[o - 1])) {
            ProfScope ps(pc, HAK_PROF_FED, st);
            fused_first = hak_launch_fed_sf_head(st, A + L.lt(o - 1, 0), L.oct[o - 1], smooth, flow, dst0, S, oc, nimg, taps1, cfg.diffusivity,
                                                 lp.tau.data(), ns0, c->state, o, G > 1);
            // reads the even rows of Lt(o-1,0), writes smooth, L' (+ g for later launches)
            if (fused_first) count_fed(1, 2.0 * L.oct[o - 1].w * L.oct[o - 1].h + (G > 1 ? 12.0 : 8.0) * oc.w * oc.h);
        }
        // otherwise decimate Lt(o-1,0) so that the last of G ping-pong launches lands in Lt(o,0)
        V* first = (G % 2 == 0) ? Lt : tmp;
        if (!fused_first) {
            { ProfScope ps(pc, HAK_PROF_DOWN, st);
              hak_launch_down_smooth(st, A + L.lt(o - 1, 0), first, smooth, S, L.oct[o - 1], oc, nimg, taps1); }
            ProfScope ps(pc, HAK_PROF_FLOW, st);
            hak_launch_flow(st, smooth, flow, S, oc.w, oc.h, oc.p, nimg, cfg.diffusivity, c->state, o);
        }
        fsrc = first;
    } else {                                                                  // akaze.cpp:393-421 (FAST: 664-695)
        fsrc = A + L.lt(o, s - 1);
        // sublevels > 0: low-pass + conductivity + the first FED group in one streaming pass when the case is covered
        // (PM_G2, 16-byte rows); the conductivity plane is written only if later groups of the cycle need it
        if (hak_fed_sf_covers(kn, cfg.diffusivity, oc, nimg)) {
            ProfScope ps(pc, HAK_PROF_FED, st);
            if constexpr (is_fast<V>) {                                       // FAST has no LP Hessian: `smooth` is always stored
                fused_first = hak_launch_fed_sf(st, fsrc, smooth, flow, dst0, S, oc.w, oc.h, oc.p, nimg, taps1, cfg.diffusivity, lp.tau.data(),
                                                ns0, c->state, o, G > 1);
            } else {
                // the low-pass has one reader, the level's Hessian: when that runs as the streaming kernel it low-passes Lt(o,s-1)
                // itself (LP variant) and the plane is not written at all
                const bool lp_hess = kn.hess_lp != 0 && hak_stream_pays(kn.hess_stream, oc.w, oc.h, nimg) &&
                                     hak_hessian_stream_covers(oc.w, oc.h, lp.sigma_size, true);
                fused_first = hak_launch_fed_sf(st, fsrc, smooth, flow, dst0, S, oc.w, oc.h, oc.p, nimg, taps1, cfg.diffusivity, lp.tau.data(),
                                                ns0, c->state, o, G > 1, !lp_hess);
                if (fused_first) {
                    a.hess_lp[o * HAK_MAX_SCALES + s] = lp_hess;
                    // reads L, writes L' (+ smooth unless the Hessian is LP, + g for later launches)
                    count_fed(1, ((G > 1 ? 16.0 : 12.0) - (lp_hess ? 4.0 : 0.0)) * oc.w * oc.h);
                }
            }
        }
        if (!fused_first) {                                                   // akaze.cpp:403-404 in one pass
            ProfScope ps(pc, HAK_PROF_LOWPASS, st);
            hak_launch_smooth_flow(st, fsrc, smooth, flow, S, oc.w, oc.h, oc.p, nimg, taps1, cfg.diffusivity, c->state, o);
        }
    }
    // the n explicit steps of the cycle in G fused launches, ping-pong Lt <-> tmp, ending in Lt
    const V* src = fsrc;
    int done = 0;
    for (int g = 0; g < G; g++) {
        const int ns = hak_fed_group_size(n, G, g);
        V* dst = ((G - g) % 2 == 1) ? Lt : tmp;
        if (!(g == 0 && fused_first)) {
            ProfScope ps(pc, HAK_PROF_FED, st);
            hak_launch_fed_group(st, src, flow, dst, S, oc.w, oc.h, oc.p, nimg, lp.tau.data() + done, ns);
            count_fed(1, 12.0 * oc.w * oc.h);                                 // reads L and g, writes L'
        }
        done += ns;
        src = dst;
    }
}

// ---- part B of level (o, s): derivatives + determinant + extrema (akaze.cpp:354, 423, 431-433).  Level (0, 0) differentiates
// Lt itself, every other level the low-pass of its predecessor (D13).  (The determinant goes to HBM only in the dilation > 4
// fallback: `flow` is free at every call.)
template <typename V>
static void hessian_level(LevelArgs& a, int o, int s, hipStream_t st, const V* smooth_alt = nullptr)
{
    if (a.hess_fused[o * HAK_MAX_SCALES + s]) return;                // done inside k_level_tile
    hak_ctx* const c = a.c;
    const HakLayout& L = c->L;
    V* const A = reinterpret_cast<V*>(c->arena);
    const HakOct oc = L.oct[o];
    const LevelPlan& lp = c->plan[(size_t)o * L.ms + s];
    const bool lph = a.hess_lp[o * HAK_MAX_SCALES + s];              // (never set by FAST)
    const V* hsrc = (o == 0 && s == 0) ? A + L.lt(0, 0) : lph ? A + L.lt(o, s - 1) : smooth_alt ? smooth_alt : A + L.smooth_off[o];
    const V thr = dthreshold_of<V>(c);
    ProfScope ps(is_fast<V> ? nullptr : c, HAK_PROF_HESSIAN, st);
    bool done;
    if constexpr (is_fast<V>)
        done = hak_launch_hessian_level(st, hsrc, A + L.dxy(o, s), A + L.flow_off[o], false, L.arena, oc.w, oc.h, oc.p, a.nimg, lp.sigma_size,
                                        &a.b, &L, &c->htab, o, s, thr);
    else
        done = hak_launch_hessian_level(st, hsrc, A + L.dxy(o, s), A + L.flow_off[o], false, L.arena, oc.w, oc.h, oc.p, a.nimg, lp.sigma_size,
                                        &a.b, &L, &c->htab, o, s, thr, lph ? c->taps1 : nullptr);
    if (!done) hak_launch_extrema_level(st, a.b, L, &c->htab, o, s, thr, L.flow_off[o]);
}

static int enqueue_detect(hak_ctx* c, const float* d_images, long image_stride, int pitch, int nimg,
                          hak_point* d_points, int* d_num_pts, int desc, int max_pts, hak_point* h_points = nullptr, int cap0 = 0, int cap1 = 0)
{
    const hak_config& cfg = c->cfg;
    const HakLayout& L = c->L;
    // Octave o+1 depends only on Lt(o, 0) (the reference decimates from sublevel 0, akaze.cpp:371-375).
    const bool spine = c->concurrent && L.noct > 1 && spine_pays(c, nimg);
    const hipStream_t main_st = c->stream;
    c->sync_stream = c->stream;
    float* A = c->arena;
    LevelArgs a = level_args(c, d_images, image_stride, pitch, nimg);
    HakBatch& b = a.b;
    b.cap0 = cap0; b.cap1 = cap1;
    c->last_fast = false;
    c->fed_launches = 0;
    c->fed_fused_bytes = 0;

    hak_launch_reset_state(main_st, c->state, nimg);   // (the key map is all zero here: hak_create / k_clear_cand_maps / maps_guard)

    if (spine) {
        // Launch-bound calls (a single image): the dependency chain base -> head(1) -> head(2) -> ... -> every sublevel of the
        // last octave is the critical path, so it runs on ONE stream without cross-queue waits (each costs 15-35 us in a replayed
        // graph, profiles/r03_single_*); what hangs off it -- the remaining sublevels and all Hessians of octaves 0 .. noct-2 --
        // goes to side streams, one per octave.
        const int last = L.noct - 1;
        hipGraphNode_t head_node[HAK_MAX_OCTAVES] = {};
        hipGraph_t cap_graph = nullptr;
        for (int o = 0; o <= last; o++) {
            build_level<float>(a, o, 0, main_st);
            if (o < last) {
                (void)hipEventRecord(c->ev_ready[o], main_st);                    // Lt(o,0) + its low-pass ready: side stream o may start
                // while capturing: remember the head's graph node (see below)
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                const hipGraphNode_t* deps = nullptr;
                size_t ndeps = 0;
                if (hipStreamGetCaptureInfo_v2(main_st, &cs, nullptr, &cap_graph, &deps, &ndeps) == hipSuccess &&
                    cs == hipStreamCaptureStatusActive && ndeps == 1) head_node[o] = deps[0];
                else (void)hipGetLastError();
            }
        }
        // The graph executor deals a fork's branches to its queues by position: the first outgoing edge of a node stays on the
        // node's queue, the k-th goes k-1 queues further (of four).  Every side stream forks from the spine as some head's SECOND
        // edge, so all three would share one queue and run one after the other (measured: 440 us of side work in a row).  Empty
        // nodes in front of a fork move its side branch further along.  The replay submits queue by queue -- the spine's first, then
        // the others from the last to the first -- so the longest side chain (octave 0's) gets the last queue, the shortest the
        // first.  Pure placement: results and ordering are unaffected, and a runtime that places nodes differently merely ignores
        // the hint (HAK_GRAPH_PADS=0 switches it off).
        for (int o = 0; o < last && c->knobs.graph_pads; o++)
            for (int k = 0; k < last - 1 - o && head_node[o] && cap_graph; k++) {
                hipGraphNode_t pad = nullptr;
                if (hipGraphAddEmptyNode(&pad, cap_graph, &head_node[o], 1) != hipSuccess) (void)hipGetLastError();
            }
        // Side streams: one per remaining octave by default.  The chain + noct-1 side streams want noct hardware queues besides the
        // null stream's; the runtime gives a process four (GPU_MAX_HW_QUEUES), so at four octaves two side chains share a queue and
        // run one after the other (C++ demo: 1.08 instead of 0.91 ms per 1080p pair).  A process that makes single-image calls
        // should start with GPU_MAX_HW_QUEUES=8 (the demo does) -- the library does not set it itself, because a
        // process that runs BATCHES loses 2 % (1080p) to 13 % (720p) with eight queues.  HAK_SIDE_STREAMS = n < noct-1 makes
        // octaves n-1 .. noct-2 share the last side stream by design (same time as the shared queue).
        const int nside = c->knobs.side_streams < last ? c->knobs.side_streams : (last > 0 ? last : 1);
        auto side_of = [&](int o) { return c->oct_stream[1 + (o < nside ? o : nside - 1)]; };
        // the remaining work, one level per octave in turn, each octave's first node behind the wait for its head
        for (int s = 0; s < L.ms; s++)
            for (int k = 0; k <= last; k++) {
                const int o = k == 0 ? last : k - 1;                              // the spine's own octave first
                const hipStream_t st = o == last ? main_st : side_of(o);
                if (s == 0 && o != last && hipStreamWaitEvent(st, c->ev_ready[o], 0) != hipSuccess) return fail("stream wait");
                if (s > 0) build_level<float>(a, o, s, st);
                hessian_level<float>(a, o, s, st);
            }
        for (int i = 0; i < nside && last > 0; i++) {
            (void)hipEventRecord(c->ev_done[i + 1], c->oct_stream[i + 1]);
            if (hipStreamWaitEvent(main_st, c->ev_done[i + 1], 0) != hipSuccess) return fail("stream join");
        }
    } else {
        // each octave on its own stream, chained by events: the small octaves' launches are latency chains of a few hundred waves
        // and hide under octave 0's chip-filling kernels
        // Small launches in the tile-kernel regime (a pair, a handful of images): octave 0 is the longest chain, and a third of it
        // are its four Hessians, which nothing in the scale space waits for.  They move to a stream of their own.  The only
        // hazard is the `smooth` plane (level s's Hessian reads it, level s+1's low-pass overwrites it): the levels alternate
        // between `smooth` and `tmp`, which is free in an octave whose FED cycles are single launches (G = 1: the cycle lands in
        // Lt directly), so level s+1's low-pass only waits for the Hessian of level s-1.  profiles/r05_pair_serial_timeline.txt:
        // 292 us of chain (alone) become 183 + the last Hessian.
        // MEASURED, OFF BY DEFAULT (HAK_HESS_SIDE=1): the pair call gets SLOWER, 0.567-0.572 -> 0.620-0.623 ms (4 or 5 hardware
        // queues alike; 6: 0.82): as with the spine order of round 4, a fifth chain of two-image kernels stretches the other four by
        // more than the critical chain shrinks -- the call is bound by the chip's throughput on these small kernels, not by the
        // order they are issued in.
        bool side0 = c->knobs.hess_side != 0 && c->concurrent && L.noct > 1 && c->hess_stream && L.ms <= HAK_MAX_SCALES &&
                     !hak_stream_pays(c->knobs.hess_stream, L.oct[0].w, L.oct[0].h, nimg) && !level_tile_pays(c, L.oct[0], nimg) &&
                     !hak_stream_pays(c->knobs.fuse_sf, L.oct[0].w, L.oct[0].h, nimg);
        for (int s = 1; s < L.ms && side0; s++)
            side0 = hak_fed_groups(c->plan[s].nsteps, c->knobs.max_fuse, L.oct[0].w, true) == 1 && c->plan[s].sigma_size <= 4;
        hipStream_t st = main_st;
        for (int o = 0; o < L.noct; o++) {
            if (c->concurrent && o > 0) {                       // this octave's chain waits only for Lt(o-1,0)
                st = c->oct_stream[o];
                if (hipStreamWaitEvent(st, c->ev_ready[o - 1], 0) != hipSuccess) return fail("stream wait");
            }
            for (int s = 0; s < L.ms; s++) {
                if (o == 0 && side0) {
                    float* sm = (s & 1) ? A + L.tmp_off[0] : A + L.smooth_off[0];
                    // (level s's low-pass target was last read by the Hessian of level s - 2)
                    if (s >= 2 && hipStreamWaitEvent(st, c->ev_hd[s - 2], 0) != hipSuccess) return fail("stream wait");
                    build_level<float>(a, 0, s, st, sm);
                    if (s == 0) (void)hipEventRecord(c->ev_ready[0], st);
                    (void)hipEventRecord(c->ev_hs[s], st);
                    if (hipStreamWaitEvent(c->hess_stream, c->ev_hs[s], 0) != hipSuccess) return fail("stream wait");
                    hessian_level<float>(a, 0, s, c->hess_stream, sm);
                    (void)hipEventRecord(c->ev_hd[s], c->hess_stream);
                    continue;
                }
                build_level<float>(a, o, s, st);
                if (c->concurrent && s == 0) (void)hipEventRecord(c->ev_ready[o], st);   // Lt(o,0) final: octave o+1 may start
                hessian_level<float>(a, o, s, st);
            }
            if (c->concurrent && o > 0) (void)hipEventRecord(c->ev_done[o], st);
        }
        if (c->concurrent)
            for (int o = 1; o < L.noct; o++)
                if (hipStreamWaitEvent(main_st, c->ev_done[o], 0) != hipSuccess) return fail("stream join");
        if (side0)                                              // (the stream runs in order: its last event covers all four)
            if (hipStreamWaitEvent(main_st, c->ev_hd[L.ms - 1], 0) != hipSuccess) return fail("stream join");
    }
    // the scale space (bound by HBM stores) is done, the keypoint stages (bound by gathers and integer work) begin: a caller that
    // runs two contexts lets the other one start its scale space here (hak_phase_event)
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hipGraph_t g = nullptr;
        const hipGraphNode_t* deps = nullptr;
        size_t ndeps = 0;
        if (hipStreamGetCaptureInfo_v2(main_st, &cs, nullptr, &g, &deps, &ndeps) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        hipError_t pe;
        if (cs == hipStreamCaptureStatusActive) {
            // inside a capture a plain record would be a capture-internal dependency: the record becomes an event-record NODE behind
            // the stream's current frontier, and the frontier moves to it
            hipGraphNode_t node = nullptr;
            pe = hipGraphAddEventRecordNode(&node, g, deps, ndeps, c->ev_phase);
            if (pe == hipSuccess) pe = hipStreamUpdateCaptureDependencies(main_st, &node, 1, hipStreamSetCaptureDependencies);
        } else pe = hipEventRecord(c->ev_phase, main_st);
        if (pe != hipSuccess) { fprintf(stderr, "hipakaze: phase event record: %s\n", hipGetErrorString(pe)); (void)hipGetLastError(); }
    }
    bool tail_fork = false;
    { ProfScope ps(c, HAK_PROF_NMS);                                              // akaze.cpp:449-455
      hak_launch_nms_emit(main_st, b, L, c->dtab, c->psz, d_points, max_pts, d_num_pts);
      // the clean-up for the next sequence needs only the candidate list: beside the descriptor kernels, not in front of them
      // (batches: no gain beside 5 ms of descriptor kernels, A/B 5 640 vs 5 710 pairs/s; the pair call: the fork's two cross-stream
      // waits in the replayed graph cost more than the 5 us kernel they move aside, 0.571 vs 0.544 ms, round 5)
      tail_fork = spine && c->knobs.tail_fork;
      if (tail_fork) {
          (void)hipEventRecord(c->ev_tail_fork, main_st);
          if (hipStreamWaitEvent(c->oct_stream[1], c->ev_tail_fork, 0) != hipSuccess) return fail("stream wait");
          hak_launch_clear_maps(c->oct_stream[1], b, L);
          (void)hipEventRecord(c->ev_tail_join, c->oct_stream[1]);
      } else hak_launch_clear_maps(main_st, b, L); }
    { ProfScope ps(c, HAK_PROF_DESCRIBE);                                         // akaze.cpp:124-131
      hak_launch_describe(main_st, b, L, c->dtab, d_points, max_pts, cfg.descriptor_pattern_size, cfg.upright, desc, c->htab.dsc_plan_ok); }
    if (h_points)                                                                 // pinned destination: records and count go out in the same sequence
        hak_launch_download(main_st, d_points, d_num_pts, max_pts, nimg, h_points, c->h_num);
    if (tail_fork && hipStreamWaitEvent(main_st, c->ev_tail_join, 0) != hipSuccess) return fail("stream join");
    if (hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    if (g_launch_err) { const char* m = g_launch_err; g_launch_err = nullptr; return fail(m); }
    return 0;
}

// ------------------------------------------------------- integer FAST path
// Akazer::fastDetectAndCompute / fastDetect (akaze.cpp:153-201, 506-743): the same levels on int32 planes, one after the other on
// c->stream -- never captured or replayed, no side streams, no per-image caps, no profile classes.
int enqueue_fast_detect(hak_ctx* c, const unsigned char* d_images, long image_stride, int pitch, int nimg,
                        hak_point* d_points, int* d_num_pts, int desc, int max_pts)
{
    const hak_config& cfg = c->cfg;
    const HakLayout& L = c->L;
    const hipStream_t st = c->stream;
    LevelArgs a = level_args(c, d_images, image_stride, pitch, nimg);
    c->last_fast = true;
    c->sync_stream = c->stream;
    hak_launch_reset_state(st, c->state, nimg);              // (the key map is all zero here: hak_create / k_clear_cand_maps / maps_guard)
    for (int o = 0; o < L.noct; o++)
        for (int s = 0; s < L.ms; s++) {
            build_level<int>(a, o, s, st);
            hessian_level<int>(a, o, s, st);
        }
    hak_launch_nms_emit(st, a.b, L, c->dtab, c->psz, d_points, max_pts, d_num_pts, 1);
    hak_launch_clear_maps(st, a.b, L);
    hakf_launch_describe(st, a.b, L, c->dtab, d_points, max_pts, cfg.descriptor_pattern_size, cfg.upright, desc, c->htab.dsc_plan_ok);
    if (hipGetLastError() != hipSuccess) return fail("kernel launch failed");
    return 0;
}

// enqueue one detect+describe sequence: replay the captured graph when the arguments repeat, else capture it
static int run_detect_inner(hak_ctx* c, const float* d_images, long image_stride, int pitch, int nimg,
                            hak_point* d_points, int* d_num_pts, int desc, int max_pts, hak_point* h_pinned, int cap0, int cap1)
{
    // A launch-bound sequence (single images: the spine order of enqueue_detect) is issued eagerly: with ~50 launches on four
    // streams the host keeps ahead of the GPU, and the graph replay of ROCm 7.2 submits queue by queue in an order of its own
    // (measured on the C++ demo, ms per 1080p pair: eager 1.18, replay 1.31; HAK_GRAPH=2 forces the replay).
    const bool launch_bound = c->concurrent && c->L.noct > 1 && spine_pays(c, nimg);
    if (!c->use_graph || c->prof_on || (launch_bound && c->knobs.graph != 2))
        return enqueue_detect(c, d_images, image_stride, pitch, nimg, d_points, d_num_pts, desc, max_pts, h_pinned, cap0, cap1);
    hak_ctx::GraphKey key;
    memset(&key, 0, sizeof(key));
    key.img = d_images; key.stride = image_stride; key.pitch = pitch; key.nimg = nimg; key.pts = d_points;
    key.num = d_num_pts; key.desc = desc; key.max_pts = max_pts; key.conc = c->concurrent ? 1 : 0; key.st = c->stream; key.hpts = h_pinned; key.cap0 = cap0; key.cap1 = cap1;
    key.retain = (c->retain_best ? 1 : 0) | (c->retain_grid << 1);     // (both selection modes: what hak_batch_selection reads)
    int slot = -1, victim = 0;
    for (int i = 0; i < hak_ctx::NGRAPH; i++) {
        if (c->graph_exec[i] && memcmp(&key, &c->gkey[i], sizeof(key)) == 0) slot = i;
        if (c->graph_age[i] < c->graph_age[victim]) victim = i;
    }
    if (slot >= 0) {
        c->graph_age[slot] = ++c->graph_clock;
        if (hipGraphLaunch(c->graph_exec[slot], c->stream) != hipSuccess) return fail("hipGraphLaunch");
        return 0;
    }
    slot = victim;                                              // least recently used (or empty) slot
    if (c->graph_exec[slot]) { (void)hipGraphExecDestroy(c->graph_exec[slot]); c->graph_exec[slot] = nullptr; }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        c->use_graph = false;                                   // e.g. legacy default stream: fall back to eager launches
        return enqueue_detect(c, d_images, image_stride, pitch, nimg, d_points, d_num_pts, desc, max_pts, h_pinned, cap0, cap1);
    }
    const int rc = enqueue_detect(c, d_images, image_stride, pitch, nimg, d_points, d_num_pts, desc, max_pts, h_pinned, cap0, cap1);
    const hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess || !graph) return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(&c->graph_exec[slot], graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { c->graph_exec[slot] = nullptr; return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
    c->gkey[slot] = key;
    c->graph_age[slot] = ++c->graph_clock;
    if (hipGraphLaunch(c->graph_exec[slot], c->stream) != hipSuccess) return fail("hipGraphLaunch");
    return 0;
}

int run_detect(hak_ctx* c, const float* d_images, long image_stride, int pitch, int nimg,
               hak_point* d_points, int* d_num_pts, int desc, int max_pts, hak_point* h_pinned, int cap0, int cap1)
{
    order_after_null_stream(c, c->stream);
    maps_guard_begin(c);
    return maps_guard_end(c, run_detect_inner(c, d_images, image_stride, pitch, nimg, d_points, d_num_pts, desc, max_pts, h_pinned, cap0, cap1));
}

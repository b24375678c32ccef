// hak_api.hip -- C ABI of libhipakaze: context, FED schedule and the extern "C" entry points.  The launch sequence they enqueue
// is hak_sequence.hip.
#include "hak_internal.h"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "hak_ctx.h"

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int hak_fail(const std::string& m) { g_err = m; return 1; }

extern "C" const char* hak_last_error(void) { return g_err.c_str(); }

extern "C" int hak_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int hak_set_device(int dev)
{
    int n = hak_device_count();
    if (n == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    dev = dev < 0 ? 0 : (dev >= n ? n - 1 : dev);                   // cuda_utils.h:50
    HIP_TRY(hipSetDevice(dev));
    return 0;
}

extern "C" void hak_default_config(hak_config* c)
{
    c->noctaves = 4; c->max_scale = 4; c->per = 0.7f; c->kcontrast = 0.03f; c->soffset = 1.6f;
    c->reordering = 1; c->derivative_factor = 1.5f; c->dthreshold = 0.001f; c->diffusivity = HAK_PM_G2;
    c->descriptor_pattern_size = 10; c->max_pts = 10000; c->upright = 0; c->batch = 1;
}

// --------------------------------------------------- host-side schedule math
static bool fed_is_prime(int number)                                // fed.cpp:128-148
{
    if (number <= 1) return false;
    if (number == 2 || number == 3 || number == 5 || number == 7) return true;
    if (number % 2 == 0 || number % 3 == 0 || number % 5 == 0 || number % 7 == 0) return false;
    int upper = (int)std::sqrt(number + 1.0);
    for (int d = 11; d <= upper; d += 2)
        if (number % d == 0) return false;
    return true;
}

extern "C" int hak_fed_tau(float T, int M, float tau_max, int reordering, float* tau, int cap)
{
    // fed.cpp:41-119; mixed float/double arithmetic as in the source
    const float t = T / (float)M;
    const int n = (int)(std::ceil(std::sqrt(3.0 * t / tau_max + 0.25f) - 0.5f - 1.0e-8f) + 0.5f);
    if (n <= 0) return 0;
    if (n > cap) return -n;
    const float scale = (float)(3.0 * t / (tau_max * (float)(n * (n + 1))));
    const float c = 1.0f / (4.0f * (float)n + 2.0f);
    const float d = scale * tau_max / 2.0f;
    std::vector<float> tauh(n);
    for (int k = 0; k < n; ++k) {
        float hh = (float)std::cos(HAK_PI_D * (2.0f * (float)k + 1.0f) * c);
        tauh[k] = d / (hh * hh);
    }
    if (!reordering) {
        for (int k = 0; k < n; k++) tau[k] = tauh[k];
        return n;
    }
    const int kappa = n / 2;
    int prime = n + 1;
    while (!fed_is_prime(prime)) prime++;
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return n;
}

extern "C" void hak_gauss_taps(float var, int radius, float* taps)
{
    // akazed.cu:2298-2333
    const float denom = 1.f / (2.f * var);
    float ksum = 0;
    for (int i = 0; i <= radius; i++) {
        taps[i] = expf(-i * i * denom);
        ksum += (i == 0) ? taps[i] : taps[i] + taps[i];
    }
    ksum = 1 / ksum;
    for (int i = 0; i <= radius; i++) taps[i] *= ksum;
}

extern "C" int hak_describe_plan_query(int pattern_size, unsigned int* pos, unsigned int* cell)
{
    static HakTables t;                                     // (too large for the stack of a small thread; host-only scratch)
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (pattern_size < 1) return 0;
    memset(&t, 0, sizeof(t));
    hak_describe_plan(&t, pattern_size);
    if (pos)                                                // the window-order row of the gather table, without the index bits
        for (int j = 0; j < 7 * 64; j++) pos[j] = t.dsc_ord[HAK_DSC_NB * 7 * 64 + j] & 0x1FFFFu;
    if (cell) memcpy(cell, t.dsc_cell, sizeof(t.dsc_cell));
    return t.dsc_plan_ok;
}

extern "C" int hak_describe_order_query(int pattern_size, int row, unsigned int* slots)
{
    static HakTables t;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (pattern_size < 1 || row < 0 || row > HAK_DSC_NB) return 0;
    memset(&t, 0, sizeof(t));
    hak_describe_plan(&t, pattern_size);
    if (!t.dsc_plan_ok) return 0;
    if (slots) memcpy(slots, t.dsc_ord + (size_t)row * 7 * 64, sizeof(unsigned int) * 7 * 64);
    return HAK_DSC_NB;
}

extern "C" int hak_describe_order_bin(float angle) { return hak_dsc_bin(angle); }

extern "C" void hak_compare_indices(int* idx1, int* idx2)
{
    // akazed.cu:65-159: per grid (2x2 cells 0-3, 3x3 cells 4-12, 4x4 cells 13-28), channel-major, pairs j<i
    static const int lo[3] = {0, 4, 13}, hi[3] = {4, 13, 29};
    int n = 0;
    for (int g = 0; g < 3; g++)
        for (int ch = 0; ch < 3; ch++)
            for (int j = lo[g]; j < hi[g] - 1; ++j)
                for (int i = j + 1; i < hi[g]; ++i) {
                    idx1[n] = 3 * j + ch;
                    idx2[n] = 3 * i + ch;
                    n++;
                }
    for (; n < 488; n++) idx1[n] = idx2[n] = 0;
}

static inline int align_up(int a, int b) { return (a + b - 1) / b * b; }

static int build_plan(hak_ctx* c, int w, int h)
{
    const hak_config& cfg = c->cfg;
    if (cfg.noctaves < 1 || cfg.noctaves > HAK_MAX_OCTAVES) return fail("noctaves out of range");
    if (cfg.max_scale < 1 || cfg.max_scale > HAK_MAX_SCALES) return fail("max_scale out of range");
    if (w < 80 || h < 80) return fail("image smaller than 80 px");
    // candidate entries carry 16 bits per full-resolution coordinate (hak_cand_word, hak_internal.h)
    if (w > 65535 || h > 65535) return fail("image larger than 65535 px in one dimension");
    // the key map orders responses by their bits: the order of positive floats only (hak_ext_key, hak_internal.h; hipakaze.h)
    if (!(cfg.dthreshold >= 0.f)) return fail("dthreshold must be >= 0 (and not a NaN): the key map orders positive responses only");
    HakLayout& L = c->L;
    memset(&L, 0, sizeof(L));
    L.ms = cfg.max_scale;
    // akaze.cpp:204-237 allocMemory; octave count fixed up front
    int noct = 1;
    L.oct[0] = {w, h, align_up(w, 64), 0};
    for (int j = 1; j < cfg.noctaves; j++) {
        int ww = L.oct[j - 1].w >> 1, hh = L.oct[j - 1].h >> 1;
        if (ww < 80 || hh < 80) break;
        L.oct[j] = {ww, hh, align_up(ww, 64), 0};
        noct = j + 1;
    }
    L.noct = noct;
    long off = 0;
    for (int o = 0; o < noct; o++) {
        L.oct[o].plane = (long)L.oct[o].h * L.oct[o].p;
        L.lvl_off[o] = off;       off += 3L * L.ms * L.oct[o].plane;      // Lt[ms] + interleaved {Lx, Ly}[ms] (2 planes each)
        L.smooth_off[o] = off;    off += L.oct[o].plane;
        L.flow_off[o] = off;      off += L.oct[o].plane;
        L.tmp_off[o] = off;       off += L.oct[o].plane;
    }
    L.arena = off;

    // akaze.cpp:268-439 schedule
    c->plan.assign((size_t)noct * L.ms, LevelPlan());
    const float tmax = 0.25f;
    float esigma = cfg.soffset;
    float last_etime = (float)(0.5 * cfg.soffset * cfg.soffset);                 // akaze.cpp:270
    const float smax = (float)(10.0 * sqrtf(2.0f));                               // akaze.cpp:279 (MLDB)
    int oratio = 1;
    float psz = 10000;
    float tau[4096];
    for (int i = 0; i < noct; i++) {
        for (int j = 0; j < L.ms; j++) {
            LevelPlan& lp = c->plan[(size_t)i * L.ms + j];
            if (i == 0 && j == 0) {
                lp.size = esigma * cfg.derivative_factor;                         // akaze.cpp:336-338
                lp.sigma_size = (int)(esigma * cfg.derivative_factor + 0.5f);
                lp.border = smax * lp.sigma_size;
                continue;
            }
            esigma = cfg.soffset * powf(2, (float)j / L.ms + i);                  // akaze.cpp:357
            float curr_etime = 0.5f * esigma * esigma;
            float ttime = curr_etime - last_etime;
            int n = hak_fed_tau(ttime, 1, tmax, cfg.reordering, tau, 4096);
            if (n < 0) return fail("FED cycle longer than 4096 steps");
            if (n == 0) return fail("FED cycle with zero steps (non-increasing scale schedule)");
            lp.nsteps = n;
            lp.tau.assign(tau, tau + n);
            lp.size = esigma * cfg.derivative_factor / oratio;
            lp.sigma_size = (int)(lp.size + 0.5f);
            lp.border = smax * lp.sigma_size;
            last_etime = curr_etime;
        }
        float b0 = c->plan[(size_t)i * L.ms].border * oratio;
        psz = psz < b0 ? psz : b0;                                                // akaze.cpp:434
        oratio *= 2;
    }
    c->psz = (int)psz;
    memset(&c->htab, 0, sizeof(c->htab));
    for (int l = 0; l < noct * L.ms; l++) {
        c->htab.sizes[l] = c->plan[l].size;
        c->htab.borders[l] = c->plan[l].border;
        c->htab.sigma_size[l] = c->plan[l].sigma_size;
    }
    for (int r2 = 0; r2 < 36; r2++) c->htab.orient_w[r2] = hak_expf(-r2 * 0.08f);  // akazed.cu:1697
    hak_deriv_factors(&c->htab.fac1, &c->htab.fac2);
    c->htab.ifac1 = hak_fix16(c->htab.fac1);                                      // akazed.cu:4183-4184
    c->htab.ifac2 = hak_fix16(c->htab.fac2);
    hak_compare_indices(c->htab.comp1, c->htab.comp2);
    for (int b = 0; b < 61; b++)
        for (int i = 0; i < 8; i++) {
            c->htab.comp_packed[b * 16 + 2 * i] = (unsigned char)c->htab.comp1[b * 8 + i];
            c->htab.comp_packed[b * 16 + 2 * i + 1] = (unsigned char)c->htab.comp2[b * 8 + i];
        }
    hak_describe_plan(&c->htab, cfg.descriptor_pattern_size);
    hak_gauss_taps(1.f, 2, c->taps1);
    int ksz = (int)(2 * ceilf((cfg.soffset - 0.8f) / 0.3f) + 3);                 // akaze.cpp:328
    c->base_R = ksz <= 5 ? 2 : ksz <= 7 ? 3 : ksz <= 9 ? 4 : 5;                   // akazed.cu:2345-2377
    if (ksz > 11) return fail("Kernels larger than 11 not implemented");
    hak_gauss_taps(cfg.soffset * cfg.soffset, c->base_R, c->taps_base);
    for (int i = 0; i < 8; i++) {
        c->itaps1[i] = i <= 2 ? hak_fix16(c->taps1[i]) : 0;
        c->itaps_base[i] = i <= c->base_R ? hak_fix16(c->taps_base[i]) : 0;
    }
    return 0;
}

extern "C" int hak_create(const hak_config* cfg, int w, int h, hak_ctx** out)
{
    if (!cfg || !out) return fail("null argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    hak_ctx* c = new hak_ctx();
    c->cfg = *cfg;
    if (c->cfg.batch < 1) c->cfg.batch = 1;
    if (c->cfg.max_pts < 1) c->cfg.max_pts = 1;
    c->knobs = hak_knobs_from_env();                // the environment is read here and nowhere else
    c->concurrent = c->knobs.serial == 0;
    c->use_graph = c->knobs.graph != 0;
    c->null_order = c->knobs.null_order != 0;
    if (build_plan(c, w, h)) { delete c; return 1; }
    const int B = c->cfg.batch;
    const HakLayout& L = c->L;
    const int words = (L.oct[0].w + 63) / 64;
    hipError_t e = hipSuccess;
    auto A = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    A((void**)&c->arena, sizeof(float) * (size_t)L.arena * B);
    A((void**)&c->maps, sizeof(unsigned long long) * (size_t)L.oct[0].plane * B);
    A((void**)&c->bitmap, sizeof(unsigned long long) * (size_t)L.oct[0].h * words * B);
    A((void**)&c->rowcount, sizeof(int) * (size_t)L.oct[0].h * B);
    // a 3x3 strict maximum occurs at most once per 2x2 block: the list can never overflow
    c->cand_cap = 0;
    for (int o = 0; o < L.noct; o++) c->cand_cap += (long)L.ms * ((L.oct[o].w + 1) / 2) * ((L.oct[o].h + 1) / 2);
    A((void**)&c->cand, sizeof(unsigned long long) * (size_t)c->cand_cap * B);
    A((void**)&c->perm, sizeof(int) * (size_t)c->cfg.max_pts * B);
    A((void**)&c->state, sizeof(HakImgState) * (size_t)B);
    A((void**)&c->sel.st, sizeof(HakSelState) * (size_t)B);
    A((void**)&c->sel.bins, sizeof(unsigned) * HAK_SEL_PASSES * HAK_SEL_BINS * (size_t)B);
    A((void**)&c->sel.tie, sizeof(int) * (size_t)L.oct[0].h * B);
    A((void**)&c->d_num, sizeof(int) * (size_t)B);
    A((void**)&c->dtab, sizeof(HakTables));
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_num, sizeof(int) * (size_t)B);
    if (e == hipSuccess) e = hipMemcpy(c->dtab, &c->htab, sizeof(HakTables), hipMemcpyHostToDevice);
    // the key map must be all zero at the start of every call; calls restore that themselves (k_clear_cand_maps)
    if (e == hipSuccess) e = hipMemset(c->maps, 0, sizeof(unsigned long long) * (size_t)L.oct[0].plane * B);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_tail_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_phase, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_null, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_tail_join, hipEventDisableTiming);
    // ... and so must the survivor bitmap and the row counts (hak_launch_clear_maps restores all three)
    if (e == hipSuccess) e = hipMemset(c->bitmap, 0, sizeof(unsigned long long) * (size_t)L.oct[0].h * words * B);
    if (e == hipSuccess) e = hipMemset(c->rowcount, 0, sizeof(int) * (size_t)L.oct[0].h * B);
    // (hipMemset fills on the NULL stream and may return before the fill has run; the context's streams are non-blocking and would
    // not wait for it)
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    for (int o = 0; o < L.noct && e == hipSuccess; o++) {
        if (o > 0) e = hipStreamCreateWithFlags(&c->oct_stream[o], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_ready[o], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_done[o], hipEventDisableTiming);
    }
    // (only when asked for, and behind the octave streams: the runtime deals a process's streams to its four hardware queues in
    // creation order, so one more stream per context moves every later stream to another queue -- creating it unconditionally put
    // the two pipeline contexts of the bench on ONE queue: 45.0 instead of 41-42 ms per step, single-image calls 1.12 instead of 0.94 ms)
    if (c->knobs.hess_side && e == hipSuccess) {
        e = hipStreamCreateWithFlags(&c->hess_stream, hipStreamNonBlocking);
        for (int s = 0; s < HAK_MAX_SCALES && e == hipSuccess; s++) {
            e = hipEventCreateWithFlags(&c->ev_hs[s], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_hd[s], hipEventDisableTiming);
        }
    }
    if (e != hipSuccess) {
        fail(std::string("hak_create: ") + hipGetErrorString(e));
        hak_destroy(c);
        return 1;
    }
    c->stream = c->own_stream;
    *out = c;
    return 0;
}

extern "C" void hak_destroy(hak_ctx* c)
{
    if (!c) return;
    // work may still be queued on a caller-provided stream (hak_set_stream), which may itself be gone by now: wait for the
    // event recorded after the context's last enqueue instead of touching that stream
    if (c->ev_last) { (void)hipEventSynchronize(c->ev_last); (void)hipEventDestroy(c->ev_last); }
    if (c->ev_tail_fork) (void)hipEventDestroy(c->ev_tail_fork);
    if (c->ev_phase) (void)hipEventDestroy(c->ev_phase);
    if (c->ev_null) (void)hipEventDestroy(c->ev_null);
    if (c->ev_tail_join) (void)hipEventDestroy(c->ev_tail_join);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (auto& g : c->graph_exec) if (g) (void)hipGraphExecDestroy(g);
    for (int o = 0; o < HAK_MAX_OCTAVES; o++) {
        if (c->oct_stream[o]) { (void)hipStreamSynchronize(c->oct_stream[o]); (void)hipStreamDestroy(c->oct_stream[o]); }
        if (c->ev_ready[o]) (void)hipEventDestroy(c->ev_ready[o]);
        if (c->ev_done[o]) (void)hipEventDestroy(c->ev_done[o]);
    }
    if (c->hess_stream) { (void)hipStreamSynchronize(c->hess_stream); (void)hipStreamDestroy(c->hess_stream); }
    for (int s = 0; s < HAK_MAX_SCALES; s++) {
        if (c->ev_hs[s]) (void)hipEventDestroy(c->ev_hs[s]);
        if (c->ev_hd[s]) (void)hipEventDestroy(c->ev_hd[s]);
    }
    for (auto& p : c->prof)
        for (auto ev : p.ev) (void)hipEventDestroy(ev);
    hak_match_scratch_free(&c->msc);
    void* bufs[] = {c->arena, c->maps, c->bitmap, c->rowcount, c->cand, c->state, c->d_num, c->dtab, c->knn, c->d_cnt, c->perm, c->pair_pts,
                    c->ransac_slots, c->ransac_models, c->geom_rec, c->link_tab, c->sel.st, c->sel.bins, c->sel.tie, c->grid.st, c->grid.count, c->grid.comp, c->guided};
    for (void* b : bufs) (void)hipFree(b);
    if (c->h_num) (void)hipHostFree(c->h_num);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" int hak_set_stream(hak_ctx* c, void* s)
{
    if (!c) return fail("null context");
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return 0;
}

extern "C" int hak_set_concurrency(hak_ctx* c, int on)
{
    if (!c) return fail("null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->concurrent = on != 0;
    return 0;
}

extern "C" int hak_set_null_order(hak_ctx* c, int on)
{
    if (!c) return fail("null context");
    c->null_order = on != 0;
    return 0;
}

// (the flag is read when a call enqueues its sequence: it is part of the graph key, so a sequence captured in one mode is never
// replayed in the other; the scratch exists from hak_create on, so turning it on allocates nothing)
extern "C" int hak_set_retain_best(hak_ctx* c, int on)
{
    if (!c) return fail("null context");
    c->retain_best = on != 0;
    return 0;
}

// (read like hak_set_retain_best's flag and part of the graph key with it.  The scratch is sized for the smallest cell, so a later
// change of G allocates nothing and a sequence captured earlier keeps valid pointers; it is allocated here, at the first G > 0)
extern "C" int hak_set_retain_grid(hak_ctx* c, int G)
{
    if (!c) return fail("null context");
    if (G != 0 && (G < HAK_GRID_MIN || G > HAK_GRID_MAX))
        return fail("hak_set_retain_grid: the cell size must be 0 (off) or between " + std::to_string(HAK_GRID_MIN) + " and " + std::to_string(HAK_GRID_MAX));
    if (G > 0 && !c->grid.st) {
        const int B = c->cfg.batch;
        HakGridScratch g;
        g.cell_cap = (long)((c->L.oct[0].w + HAK_GRID_MIN - 1) / HAK_GRID_MIN) * ((c->L.oct[0].h + HAK_GRID_MIN - 1) / HAK_GRID_MIN);
        hipError_t e = hipMalloc((void**)&g.st, sizeof(HakGridState) * (size_t)B);
        if (e == hipSuccess) e = hipMalloc((void**)&g.count, sizeof(int) * (size_t)g.cell_cap * B);
        if (e == hipSuccess) e = hipMalloc((void**)&g.comp, sizeof(unsigned long long) * (size_t)g.cell_cap * B);
        if (e != hipSuccess) {
            (void)hipFree(g.st); (void)hipFree(g.count); (void)hipFree(g.comp);
            return fail(std::string("hak_set_retain_grid: ") + hipGetErrorString(e));
        }
        c->grid = g;
    }
    c->retain_grid = G;
    return 0;
}

extern "C" int hak_phase_event(hak_ctx* c, void** ev)
{
    if (!c || !ev) return fail("null argument");
    *ev = (void*)c->ev_phase;
    return 0;
}

extern "C" int hak_wait_event(hak_ctx* c, void* ev)
{
    if (!c || !ev) return fail("null argument");
    HIP_TRY(hipStreamWaitEvent(c->stream, (hipEvent_t)ev, 0));
    return 0;
}

extern "C" int hak_sync(hak_ctx* c)
{
    if (!c) return fail("null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------- entry points of the detect sequences (hak_sequence.hip)
extern "C" int hak_fast_detect_and_compute_batch(hak_ctx* c, const unsigned char* d_images, long image_stride, int pitch,
                                                 int nimg, hak_point* d_points, int* d_num_pts, int desc)
{
    if (!c || !d_images || !d_points || !d_num_pts) return fail("null argument");
    if (nimg < 1 || nimg > c->cfg.batch) return fail("nimg exceeds the context's batch capacity");
    if (pitch < c->L.oct[0].w) return fail("pitch smaller than width");
    order_after_null_stream(c, c->stream);
    maps_guard_begin(c);
    return maps_guard_end(c, enqueue_fast_detect(c, d_images, image_stride, pitch, nimg, d_points, d_num_pts, desc, c->cfg.max_pts));
}

extern "C" int hak_fast_detect_and_compute(hak_ctx* c, const unsigned char* d_image, int pitch, hak_point* d_points, int max_pts,
                                           int* num_pts, hak_point* h_points, int desc)
{
    if (!c || !d_image || !d_points || !num_pts) return fail("null argument");
    if (max_pts < 1) return fail("max_pts < 1");
    if (pitch < c->L.oct[0].w) return fail("pitch smaller than width");
    order_after_null_stream(c, c->stream);
    maps_guard_begin(c);
    if (maps_guard_end(c, enqueue_fast_detect(c, d_image, 0, pitch, 1, d_points, c->d_num, desc, max_pts))) return 1;
    HIP_TRY(hipMemcpyAsync(c->h_num, c->d_num, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *num_pts = c->h_num[0];
    if (h_points && *num_pts > 0)
        HIP_TRY(hipMemcpy(h_points, d_points, sizeof(hak_point) * (size_t)*num_pts, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hak_detect_and_compute_batch(hak_ctx* c, const float* d_images, long image_stride, int pitch,
                                            int nimg, hak_point* d_points, int* d_num_pts, int desc)
{
    if (!c || !d_images || !d_points || !d_num_pts) return fail("null argument");
    if (nimg < 1 || nimg > c->cfg.batch) return fail("nimg exceeds the context's batch capacity");
    if (pitch < c->L.oct[0].w) return fail("pitch smaller than width");
    return run_detect(c, d_images, image_stride, pitch, nimg, d_points, d_num_pts, desc, c->cfg.max_pts);
}

// is p device-visible (pinned) host memory?  A pageable pointer makes the query fail: not an error here.
// ... and may the download kernel write it directly?  k_download stores 8-byte words through the pointer itself, so it must be
// 8-byte aligned and mapped into this device at the same address (hipHostMalloc memory is; an offset into a pinned buffer or
// hipHostRegister'd memory need not be) -- anything else takes the count + hipMemcpy route.
static bool host_pinned(const void* p)
{
    hipPointerAttribute_t a{};
    bool pinned = p && ((uintptr_t)p & 7) == 0 && hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    if (pinned) {
        void* dp = nullptr;
        pinned = hipHostGetDevicePointer(&dp, const_cast<void*>(p), 0) == hipSuccess && dp == p;
    }
    (void)hipGetLastError();
    return pinned;
}

extern "C" int hak_detect_and_compute(hak_ctx* c, const float* d_image, int pitch, hak_point* d_points, int max_pts,
                                      int* num_pts, hak_point* h_points, int desc)
{
    if (!c || !d_image || !d_points || !num_pts) return fail("null argument");
    if (max_pts < 1) return fail("max_pts < 1");
    if (pitch < c->L.oct[0].w) return fail("pitch smaller than width");
    // A pinned h_points (hak_host_alloc: what initAkazeData of the C++ layer hands out) is filled by the launch sequence itself,
    // count included: one synchronisation and the results are there.  A pageable one takes the reference's route
    // (akaze.cpp:134-139): count first, then a copy of the valid records.
    // HAK_TIMING=1: host-side split of the call (submission vs waiting), printed every 100 calls -- diagnosis only
    const bool timing = c->knobs.timing != 0;
    static double t_sub = 0, t_wait = 0; static int t_n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    hak_point* h_pinned = host_pinned(h_points) ? h_points : nullptr;
    if (run_detect(c, d_image, 0, pitch, 1, d_points, c->d_num, desc, max_pts, h_pinned)) return 1;
    if (!h_pinned) HIP_TRY(hipMemcpyAsync(c->h_num, c->d_num, sizeof(int), hipMemcpyDeviceToHost, c->sync_stream));
    const auto t1 = std::chrono::steady_clock::now();
    HIP_TRY(hipStreamSynchronize(c->sync_stream));
    if (timing) {
        const auto t2 = std::chrono::steady_clock::now();
        t_sub += std::chrono::duration<double, std::micro>(t1 - t0).count();
        t_wait += std::chrono::duration<double, std::micro>(t2 - t1).count();
        if (++t_n % 100 == 0) { fprintf(stderr, "hak timing: submit %.1f us, wait %.1f us per call\n", t_sub / 100, t_wait / 100); t_sub = t_wait = 0; }
    }
    *num_pts = c->h_num[0];
    if (h_points && !h_pinned && *num_pts > 0)                                    // akaze.cpp:134-139
        HIP_TRY(hipMemcpy(h_points, d_points, sizeof(hak_point) * (size_t)*num_pts, hipMemcpyDeviceToHost));
    return 0;
}

// Scratch for callers without a context (cuMatch is a free function in the reference, so hak_match / hak_match_knn2 accept
// ctx == NULL): a pool per device, guarded by a mutex.  A call takes a scratch of the CURRENT device for its duration -- both
// entry points synchronise before they return -- and puts it back; concurrent callers get different ones.
namespace {
std::mutex g_pool_mu;
std::vector<HakMatchScratch*> g_pool;
HakMatchScratch* pool_acquire()
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); i++)
        if (g_pool[i]->device == dev) { HakMatchScratch* sc = g_pool[i]; g_pool.erase(g_pool.begin() + (long)i); return sc; }
    HakMatchScratch* sc = new HakMatchScratch();
    sc->device = dev;
    return sc;
}
void pool_release(HakMatchScratch* sc, bool ok)
{
    // a call that failed may have left keys / tickets behind: such a scratch is not handed out again
    if (!ok) { hak_match_scratch_free(sc); delete sc; return; }
    std::lock_guard<std::mutex> lock(g_pool_mu);
    g_pool.push_back(sc);
}
}

// the 16 match bytes (match, distance, match_x, match_y) of n1 device records -> the host records, as akaze.cpp:58-63
static int download_match_fields(hak_point* h_pts1, const hak_point* d_pts1, int n1)
{
    HIP_TRY(hipMemcpy2D(&h_pts1[0].match, sizeof(hak_point), &d_pts1[0].match, sizeof(hak_point), 16, n1,
                        hipMemcpyDeviceToHost));
    return 0;
}

// The tail of a single-pair call that returns a match list (hak_match_knn2, hak_match_guided), behind its synchronisation: the
// count, the scratch back to its owner, the list and the match fields to the host.  rc: the call's state so far.
static int match_list_tail(hak_ctx* c, HakMatchScratch* sc, int rc, hak_point* h_pts1, const hak_point* d_pts1, int n1,
                           const hak_match_pair* d_out, int* count, hak_match_pair* h_out)
{
    // the multi-block finish leaves the count in the scratch's pinned word; the one-block finish only in device memory
    if (!rc && *sc->h_cnt < 0 && hipMemcpy(sc->h_cnt, sc->d_cnt, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = fail("count download");
    if (!rc) *count = *sc->h_cnt;
    if (!c) pool_release(sc, rc == 0);
    else if (rc) hak_match_scratch_free(sc);
    if (!rc && h_out && *count > 0 &&
        hipMemcpy(h_out, d_out, sizeof(hak_match_pair) * (size_t)*count, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail("match list download");
    if (!rc && h_pts1 && download_match_fields(h_pts1, d_pts1, n1)) rc = fail("match field download");      // (names the step, as before)
    return rc;
}

// One PAIR per call (include/hipakaze.h): both images through ONE launch sequence (the batch path with two images: every launch
// covers both), the match appended, the records scattered to the caller's arrays by one more kernel, ONE synchronisation --
// instead of the three synchronous calls of main.cpp:201-209 (43 + 43 + 1 launches, three waits).
extern "C" int hak_detect_and_compute_pair(hak_ctx* c, const float* d_image1, const float* d_image2, int pitch,
                                           hak_point* d_points1, hak_point* d_points2, int max_pts1, int max_pts2,
                                           int* num_pts1, int* num_pts2, hak_point* h_points1, hak_point* h_points2, int desc, int match)
{
    if (!c || !d_image1 || !d_image2 || !d_points1 || !d_points2 || !num_pts1 || !num_pts2) return fail("null argument");
    if (c->cfg.batch < 2) return fail("hak_detect_and_compute_pair needs a context created with batch >= 2");
    if (max_pts1 < 1 || max_pts2 < 1) return fail("max_pts < 1");
    if (pitch < c->L.oct[0].w) return fail("pitch smaller than width");
    const long mp = c->cfg.max_pts;
    if (!hak_mkey_fits(mp)) return fail("max_pts must stay below 2^20 for the matcher");
    if (!c->pair_pts) HIP_TRY(hipMalloc((void**)&c->pair_pts, sizeof(hak_point) * 2 * (size_t)mp));
    // each image keeps its own clamp, as in the three calls (setMaxNumPoints(result.max_pts), akaze.cpp:246, 451), bounded by the
    // context's max_pts -- the record stride of the pair buffer, which every kernel of the sequence and the matcher index with
    const int cap0 = max_pts1 < mp ? max_pts1 : (int)mp, cap1 = max_pts2 < mp ? max_pts2 : (int)mp;
    if (run_detect(c, d_image1, (long)(d_image2 - d_image1), pitch, 2, c->pair_pts, c->d_num, desc, (int)mp, nullptr, cap0, cap1)) return 1;
    if (match) {
        ProfScope ps(c, HAK_PROF_MATCH);
        hak_launch_match(c->sync_stream, c->pair_pts, c->pair_pts + mp, c->d_num, c->d_num + 1, (int)mp, (int)mp, 2 * mp, 2 * mp, 1, &c->msc);
    }
    HakPairDst dst{{d_points1, d_points2}, {host_pinned(h_points1) ? h_points1 : nullptr, host_pinned(h_points2) ? h_points2 : nullptr},
                   {max_pts1, max_pts2}};
    hak_launch_download_pair(c->sync_stream, c->pair_pts, c->d_num, mp, dst, c->h_num);
    if (hipGetLastError() != hipSuccess) return fail("pair launch failed");
    HIP_TRY(hipStreamSynchronize(c->sync_stream));
    *num_pts1 = c->h_num[0];
    *num_pts2 = c->h_num[1];
    // pageable host arrays take the reference's route (akaze.cpp:134-139): a copy of the valid records
    if (h_points1 && !dst.h[0] && *num_pts1 > 0)
        HIP_TRY(hipMemcpy(h_points1, d_points1, sizeof(hak_point) * (size_t)*num_pts1, hipMemcpyDeviceToHost));
    if (h_points2 && !dst.h[1] && *num_pts2 > 0)
        HIP_TRY(hipMemcpy(h_points2, d_points2, sizeof(hak_point) * (size_t)*num_pts2, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hak_match(hak_ctx* c, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2, hak_point* h_pts1)
{
    // ctx may be NULL (cuMatch is a free function in the reference): default stream, no profiling
    if (!d_pts1 || (!d_pts2 && n2 > 0)) return fail("null argument");
    if (n1 <= 0) return 0;
    if (!hak_mkey_fits(n2)) return fail("more than 2^20 - 1 train points");      // the packed key (hak_mkey, hak_internal.h)
    // one big pair takes the sliced search (kernels_match.hip), whose scratch belongs to the context (its device) or, without
    // one, comes from the per-device pool above for the duration of the call -- no process-wide buffer
    hipStream_t st = c ? c->stream : nullptr;
    HakMatchScratch* sc = c ? &c->msc : pool_acquire();
    order_after_null_stream(c, st);
    {
        ProfScope ps(c, HAK_PROF_MATCH);
        hak_launch_match(st, d_pts1, d_pts2, nullptr, nullptr, n1, n2, 0, 0, 1, sc);
    }
    int rc = 0;
    if (hipGetLastError() != hipSuccess) rc = fail("match launch failed");
    if (hipStreamSynchronize(st) != hipSuccess) rc = fail("hipStreamSynchronize(match)");
    if (!c) pool_release(sc, rc == 0);
    else if (rc) hak_match_scratch_free(sc);
    if (rc) return rc;
    return h_pts1 ? download_match_fields(h_pts1, d_pts1, n1) : 0;
}

extern "C" int hak_match_batch(hak_ctx* c, hak_point* d_points, const int* d_num_pts, int npairs)
{
    if (!c || !d_points || !d_num_pts || npairs < 1) return fail("bad argument");
    const long mp = c->cfg.max_pts;
    if (!hak_mkey_fits(mp)) return fail("max_pts must stay below 2^20 for the matcher");
    order_after_null_stream(c, c->stream);
    { ProfScope ps(c, HAK_PROF_MATCH);
      hak_launch_match(c->stream, d_points, d_points + mp, d_num_pts, d_num_pts + 1, (int)mp, (int)mp, 2 * mp, 2 * mp, npairs, &c->msc); }
    if (hipGetLastError() != hipSuccess) return fail("match launch failed");
    return 0;
}

// ----------------------------------------------------------- match post-processing
static int knn_scratch(hak_ctx* c)
{
    if (c->knn) return 0;
    const size_t npair = (size_t)(c->cfg.batch + 1) / 2;
    HIP_TRY(hipMalloc((void**)&c->knn, sizeof(int4) * 2 * npair * (size_t)c->cfg.max_pts));
    HIP_TRY(hipMalloc((void**)&c->d_cnt, sizeof(int) * npair));
    return 0;
}

extern "C" int hak_match_knn2(hak_ctx* c, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2, int ratio_num,
                              int ratio_den, int cross_check, int max_dist, hak_point* h_pts1, hak_match_pair* d_out,
                              int* count, hak_match_pair* h_out)
{
    if (!d_pts1 || (!d_pts2 && n2 > 0) || !count) return fail("null argument");
    if (ratio_num <= 0 || ratio_den <= 0) return fail("ratio must be a positive fraction");
    if (h_out && !d_out) return fail("h_out needs d_out");
    // (both sets are a train set once: the reverse search of the cross-check packs query indices into the same key)
    if (!hak_mkey_fits(n1) || !hak_mkey_fits(n2)) return fail("more than 2^20 - 1 points");
    *count = 0;
    if (n1 <= 0) return 0;
    if (max_dist <= 0) max_dist = HAK_MAX_DIST;
    hipStream_t st = c ? c->stream : nullptr;
    HakMatchScratch* sc = c ? &c->msc : pool_acquire();
    order_after_null_stream(c, st);
    const int nb = (n1 + 1023) / 1024;
    if (!hak_match_scratch_reserve(sc, st, 0, 0, 0, (long)n1 + (long)(n2 > 0 ? n2 : 1), nb)) {
        if (!c) pool_release(sc, false);
        return fail("hak_match_knn2: out of device memory for the 2-NN scratch");
    }
    int4* fwd = sc->knn;
    int4* rev = sc->knn + n1;
    *sc->h_cnt = -1;
    {
        hak_launch_knn2(st, d_pts1, d_pts2, nullptr, nullptr, n1, n2, 0, 0, 1, fwd, 0, sc);
        if (cross_check && n2 > 0) hak_launch_knn2(st, d_pts2, d_pts1, nullptr, nullptr, n2, n1, 0, 0, 1, rev, 0, sc);
        hak_launch_knn2_finish(st, d_pts1, d_pts2, nullptr, n1, 0, 0, 1, fwd, cross_check ? rev : nullptr, 0, ratio_num, ratio_den,
                               cross_check ? 1 : 0, max_dist, d_out, 0, sc->d_cnt, sc);
    }
    int rc = 0;
    if (hipGetLastError() != hipSuccess) rc = fail("knn2 launch failed");
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail("sync");
    return match_list_tail(c, sc, rc, h_pts1, d_pts1, n1, d_out, count, h_out);
}

extern "C" int hak_match_knn2_batch(hak_ctx* c, hak_point* d_points, const int* d_num_pts, int npairs, int ratio_num,
                                    int ratio_den, int cross_check, int max_dist, hak_match_pair* d_out, int* d_counts)
{
    if (!c || !d_points || !d_num_pts || !d_counts || npairs < 1) return fail("bad argument");
    if (2 * npairs > c->cfg.batch + 1) return fail("npairs exceeds the context's batch capacity");
    if (ratio_num <= 0 || ratio_den <= 0) return fail("ratio must be a positive fraction");
    if (max_dist <= 0) max_dist = HAK_MAX_DIST;
    const long mp = c->cfg.max_pts;
    if (!hak_mkey_fits(mp)) return fail("max_pts must stay below 2^20 for the matcher");
    if (knn_scratch(c)) return 1;
    order_after_null_stream(c, c->stream);
    int4* fwd = c->knn;
    int4* rev = c->knn + (size_t)((c->cfg.batch + 1) / 2) * mp;
    { ProfScope ps(c, HAK_PROF_MATCH);
      hak_launch_knn2(c->stream, d_points, d_points + mp, d_num_pts, d_num_pts + 1, (int)mp, (int)mp, 2 * mp, 2 * mp, npairs, fwd, mp);
      if (cross_check)
          hak_launch_knn2(c->stream, d_points + mp, d_points, d_num_pts + 1, d_num_pts, (int)mp, (int)mp, 2 * mp, 2 * mp, npairs, rev, mp);
      hak_launch_knn2_finish(c->stream, d_points, d_points + mp, d_num_pts, 0, 2 * mp, 2 * mp, npairs, fwd, cross_check ? rev : nullptr,
                             mp, ratio_num, ratio_den, cross_check ? 1 : 0, max_dist, d_out, mp, d_counts); }
    if (hipGetLastError() != hipSuccess) return fail("knn2 launch failed");
    return 0;
}

// ----------------------------------------------------------- geometric verification: what its entry points share
static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// the list of a single call / the lists of a batch call; `unaligned`, and for the batch forms that tell them apart `no_ctx`, `null`
// and `shape`, are the call's own messages
static int list_args(const void* h_out, const void* d_list, int n, const char* unaligned)
{
    if (!h_out || (!d_list && n > 0)) return fail("null argument");
    if (n < 0) return fail("n < 0");
    if (misaligned16(d_list)) return fail(unaligned);
    return 0;
}
static int list_args_batch(const hak_ctx* c, const void* d_list, const int* d_counts, const void* d_out, int npairs, long stride,
                           const char* unaligned, const char* no_ctx = "bad argument", const char* null = "bad argument",
                           const char* shape = "bad argument")
{
    if (!c) return fail(no_ctx);
    if (!d_list || !d_counts || !d_out) return fail(null);
    if (npairs < 1 || stride < 1) return fail(shape);
    if (misaligned16(d_list)) return fail(unaligned);
    return 0;
}

static int ransac_args(int iterations, float threshold, int refine)
{
    if (iterations < 1 || iterations > 65536) return fail("iterations must be in 1 .. 65536");
    if (!std::isfinite(threshold) || !(threshold > 0.f)) return fail("threshold must be finite and > 0");
    if (refine != 0 && refine != 1) return fail("refine must be 0 or 1");
    return 0;
}

static int intrinsics_args(const hak_intrinsics* K)
{
    if (!K) return fail("null intrinsics");
    if (!std::isfinite(K->fx) || !std::isfinite(K->fy) || K->fx == 0.f || K->fy == 0.f) return fail("fx and fy must be finite and non-zero");
    if (!std::isfinite(K->cx) || !std::isfinite(K->cy)) return fail("cx and cy must be finite");
    return 0;
}

// a context's buffer of `need` elements, grow-only and outside a launch sequence; a buffer being replaced may still be read by an
// earlier call on the context's stream (hipFree waits for the device)
template <typename T>
static int grow_scratch(T*& p, long& cap, long need, size_t elem = sizeof(T))
{
    if (need <= cap) return 0;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc((void**)&p, elem * (size_t)need));
    cap = need;
    return 0;
}

// the context's record: HAK_REC_BYTES (hak_internal.h); hak_link_tracks' count follows it
static int geom_record(hak_ctx* c)
{
    if (!c->geom_rec) HIP_TRY(hipMalloc((void**)&c->geom_rec, HAK_REC_BYTES + 16));
    return 0;
}

// the scratch of one RANSAC call (words = 0: no models kernel): the context's, or without a context one block slots | record | models
// that single_tail frees
struct RansacScratch { unsigned long long* slots = nullptr; void* rec = nullptr; unsigned* models = nullptr; void* block = nullptr; };
static int ransac_scratch(hak_ctx* c, long slots, long words, RansacScratch& s)
{
    if (c) {
        if (grow_scratch(c->ransac_slots, c->ransac_slots_cap, slots) || grow_scratch(c->ransac_models, c->ransac_models_cap, words) ||
            geom_record(c))
            return 1;
        s.slots = c->ransac_slots; s.rec = c->geom_rec; s.models = c->ransac_models;
        return 0;
    }
    char* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, sizeof(unsigned long long) * (size_t)slots + HAK_REC_BYTES + sizeof(unsigned) * (size_t)words));
    s.block = s.slots = reinterpret_cast<unsigned long long*>(p);
    s.rec = p + sizeof(unsigned long long) * (size_t)slots;
    s.models = reinterpret_cast<unsigned*>(p + sizeof(unsigned long long) * (size_t)slots + HAK_REC_BYTES);
    return 0;
}

// the end of a single call after its launches (rc: what went wrong before them): launch error, sync, download of `bytes` from d_rec
// to h_out, release of the call's own block
static int single_tail(int rc, hipStream_t st, const std::string& what, const char* download, void* h_out, const void* d_rec,
                       size_t bytes, void* block = nullptr)
{
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(what + " launch failed");
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = fail("hipStreamSynchronize(" + what + ")");
    if (!rc && hipMemcpy(h_out, d_rec, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(download);
    if (block) (void)hipFree(block);
    return rc;
}

// ----------------------------------------------------------- RANSAC homography (kernels_homography.hip)
extern "C" int hak_find_homography(hak_ctx* c, const hak_match_pair* d_matches, int n, int iterations, float threshold,
                                   unsigned seed, int refine, unsigned char* d_mask, hak_homography* h_out)
{
    if (list_args(h_out, d_matches, n, "d_matches must be 16-byte aligned") || ransac_args(iterations, threshold, refine)) return 1;
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    RansacScratch s;
    if (ransac_scratch(c, hak_homography_blocks(1, iterations, nullptr), 0, s)) return 1;
    hipStream_t st = c ? c->stream : nullptr;
    order_after_null_stream(c, st);
    hak_launch_homography(st, d_matches, n > 0 ? n : 1, nullptr, n, 1, iterations, threshold, seed, refine, s.slots,
                          static_cast<hak_homography*>(s.rec), d_mask, 0);
    return single_tail(0, st, "homography", "homography download", h_out, s.rec, sizeof(hak_homography), s.block);
}

extern "C" int hak_find_homography_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                                         int iterations, float threshold, unsigned seed, int refine, hak_homography* d_out,
                                         unsigned char* d_masks)
{
    if (list_args_batch(c, d_matches, d_counts, d_out, npairs, stride, "d_matches must be 16-byte aligned")) return 1;
    if (ransac_args(iterations, threshold, refine)) return 1;
    RansacScratch s;
    if (ransac_scratch(c, (long)npairs * hak_homography_blocks(npairs, iterations, nullptr), 0, s)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_homography(c->stream, d_matches, stride, d_counts, 0, npairs, iterations, threshold, seed, refine, s.slots, d_out,
                          d_masks, stride);
    if (hipGetLastError() != hipSuccess) return fail("homography launch failed");
    return 0;
}

// ----------------------------------------------------------- RANSAC fundamental matrix (kernels_fundamental.hip)
extern "C" int hak_find_fundamental(hak_ctx* c, const hak_match_pair* d_matches, int n, int iterations, float threshold,
                                    unsigned seed, unsigned char* d_mask, hak_fundamental* h_out)
{
    if (list_args(h_out, d_matches, n, "d_matches must be 16-byte aligned") || ransac_args(iterations, threshold, 0)) return 1;
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    RansacScratch s;
    if (ransac_scratch(c, hak_homography_blocks(1, iterations, nullptr), hak_fundamental_words(1, iterations), s)) return 1;
    hipStream_t st = c ? c->stream : nullptr;
    order_after_null_stream(c, st);
    hak_launch_fundamental(st, d_matches, n > 0 ? n : 1, nullptr, n, 1, iterations, threshold, seed, s.models, s.slots,
                           static_cast<hak_fundamental*>(s.rec), d_mask, 0);
    return single_tail(0, st, "fundamental", "fundamental download", h_out, s.rec, sizeof(hak_fundamental), s.block);
}

extern "C" int hak_find_fundamental_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                                          int iterations, float threshold, unsigned seed, hak_fundamental* d_out,
                                          unsigned char* d_masks)
{
    if (list_args_batch(c, d_matches, d_counts, d_out, npairs, stride, "d_matches must be 16-byte aligned")) return 1;
    if (ransac_args(iterations, threshold, 0)) return 1;
    RansacScratch s;
    if (ransac_scratch(c, (long)npairs * hak_homography_blocks(npairs, iterations, nullptr), hak_fundamental_words(npairs, iterations), s))
        return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_fundamental(c->stream, d_matches, stride, d_counts, 0, npairs, iterations, threshold, seed, s.models, s.slots, d_out,
                           d_masks, stride);
    if (hipGetLastError() != hipSuccess) return fail("fundamental launch failed");
    return 0;
}

// ----------------------------------------------------------- rank-2 refit of a fundamental matrix (kernels_fundrefit.hip)
static int refine_args(float threshold, int rounds)
{
    if (rounds < 1 || rounds > 8) return fail("rounds must be in 1 .. 8");
    if (!std::isfinite(threshold) || !(threshold > 0.f)) return fail("threshold must be finite and > 0");
    return 0;
}

// one synchronous one-list call on one record, after its argument checks, on c's stream (c may be NULL).  No scratch: the record's
// device copy is `owner`'s geom_rec, or with owner = NULL the device global hak_shared_record(), so nothing is allocated.  The refits
// pass their context as the owner; hak_recover_pose and hak_triangulate never name one.  h_in != NULL: the record is in/out and is
// uploaded first.  launch(stream, d_rec) enqueues the kernel, and the record comes back to h_out.
// The shared record has one mutex: calls without an owner take it in turn, whatever their kind.  Each of them synchronises its
// stream before it returns anyway, so no two of them could have overlapped on the device.
static std::mutex g_shared_record_turn;
template <class Rec, class Launch>
static int record_single(hak_ctx* c, hak_ctx* owner, const void* h_in, Rec* h_out, const char* what, Launch launch)
{
    static_assert(sizeof(Rec) <= HAK_REC_BYTES, "the one record holds every record type");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    std::unique_lock<std::mutex> turn(g_shared_record_turn, std::defer_lock);
    void* d_rec = nullptr;
    if (owner) {
        if (geom_record(owner)) return 1;
        d_rec = owner->geom_rec;
    } else {
        turn.lock();
        d_rec = hak_shared_record();
        if (!d_rec) return fail("hipGetSymbolAddress(shared record)");
    }
    hipStream_t st = c ? c->stream : nullptr;
    order_after_null_stream(c, st);
    int rc = 0;
    if (h_in && hipMemcpyAsync(d_rec, h_in, sizeof(Rec), hipMemcpyHostToDevice, st) != hipSuccess) rc = fail("record upload");
    if (!rc) launch(st, static_cast<Rec*>(d_rec));
    return single_tail(rc, st, what, "record download", h_out, d_rec, sizeof(Rec));
}

extern "C" int hak_refine_fundamental(hak_ctx* c, const hak_match_pair* d_matches, int n, float threshold, int rounds,
                                      unsigned char* d_mask, hak_fundamental* h_inout)
{
    if (list_args(h_inout, d_matches, n, "d_matches must be 16-byte aligned") || refine_args(threshold, rounds)) return 1;
    return record_single(c, c, h_inout, h_inout, "fundamental refit", [&](hipStream_t st, hak_fundamental* d_rec) {
        hak_launch_fundamental_refit(st, d_matches, n, nullptr, n, 1, threshold, rounds, d_rec, d_mask, 0);
    });
}

extern "C" int hak_refine_fundamental_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts,
                                            int npairs, float threshold, int rounds, hak_fundamental* d_inout,
                                            unsigned char* d_masks)
{
    if (list_args_batch(c, d_matches, d_counts, d_inout, npairs, stride, "d_matches must be 16-byte aligned")) return 1;
    if (refine_args(threshold, rounds)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_fundamental_refit(c->stream, d_matches, stride, d_counts, 0, npairs, threshold, rounds, d_inout, d_masks, stride);
    if (hipGetLastError() != hipSuccess) return fail("fundamental refit launch failed");
    return 0;
}

// ----------------------------------------------------------- relative pose from a fundamental matrix (kernels_pose.hip)
static int pose_args(const hak_intrinsics* K1, const hak_intrinsics* K2, float threshold, float max_depth)
{
    if (!K1 || !K2) return fail("null intrinsics");
    if (!std::isfinite(threshold) || !(threshold > 0.f)) return fail("threshold must be finite and > 0");
    if (!(max_depth > 0.f)) return fail("max_depth must be > 0 (+inf allowed)");
    return intrinsics_args(K1) || intrinsics_args(K2);
}

extern "C" int hak_recover_pose(hak_ctx* c, const hak_match_pair* d_matches, int n, const float F[9], const hak_intrinsics* K1,
                                const hak_intrinsics* K2, float threshold, float max_depth, unsigned char* d_mask, float* d_xyz,
                                hak_pose* h_out)
{
    if (list_args(F ? h_out : nullptr, d_matches, n, "d_matches must be 16-byte aligned")) return 1;
    if (pose_args(K1, K2, threshold, max_depth)) return 1;
    return record_single(c, nullptr, nullptr, h_out, "pose", [&](hipStream_t st, hak_pose* d_rec) {
        hak_launch_pose(st, d_matches, n > 0 ? n : 1, nullptr, n, 1, nullptr, F, *K1, *K2, threshold, max_depth, d_rec, d_mask, d_xyz);
    });
}

extern "C" int hak_recover_pose_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                                      const hak_fundamental* d_F, const hak_intrinsics* K1, const hak_intrinsics* K2,
                                      float threshold, float max_depth, hak_pose* d_out, unsigned char* d_masks, float* d_xyz)
{
    if (list_args_batch(c, d_matches, d_counts, d_F ? d_out : nullptr, npairs, stride, "d_matches must be 16-byte aligned")) return 1;
    if (pose_args(K1, K2, threshold, max_depth)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_pose(c->stream, d_matches, stride, d_counts, 0, npairs, d_F, nullptr, *K1, *K2, threshold, max_depth, d_out, d_masks,
                    d_xyz);
    if (hipGetLastError() != hipSuccess) return fail("pose launch failed");
    return 0;
}

// ----------------------------------------------------------- five-point RANSAC essential matrix (kernels_essential.hip)
static int essential_args(const hak_intrinsics* K1, const hak_intrinsics* K2, int iterations, float threshold)
{
    if (!K1 || !K2) return fail("null intrinsics");
    return ransac_args(iterations, threshold, 0) || intrinsics_args(K1) || intrinsics_args(K2);
}

extern "C" int hak_find_essential(hak_ctx* c, const hak_match_pair* d_matches, int n, const hak_intrinsics* K1, const hak_intrinsics* K2,
                                  int iterations, float threshold, unsigned seed, unsigned char* d_mask, hak_fundamental* h_out)
{
    if (list_args(h_out, d_matches, n, "d_matches must be 16-byte aligned") || essential_args(K1, K2, iterations, threshold)) return 1;
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    RansacScratch s;
    if (ransac_scratch(c, hak_essential_blocks(1, iterations), hak_essential_words(1, iterations), s)) return 1;
    hipStream_t st = c ? c->stream : nullptr;
    order_after_null_stream(c, st);
    hak_launch_essential(st, d_matches, n > 0 ? n : 1, nullptr, n, 1, *K1, *K2, iterations, threshold, seed, s.models, s.slots,
                         static_cast<hak_fundamental*>(s.rec), d_mask, 0);
    return single_tail(0, st, "essential", "essential download", h_out, s.rec, sizeof(hak_fundamental), s.block);
}

extern "C" int hak_find_essential_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                                        const hak_intrinsics* K1, const hak_intrinsics* K2, int iterations, float threshold,
                                        unsigned seed, hak_fundamental* d_out, unsigned char* d_masks)
{
    if (list_args_batch(c, d_matches, d_counts, d_out, npairs, stride, "d_matches must be 16-byte aligned")) return 1;
    if (essential_args(K1, K2, iterations, threshold)) return 1;
    RansacScratch s;
    if (ransac_scratch(c, (long)npairs * hak_essential_blocks(npairs, iterations), hak_essential_words(npairs, iterations), s)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_essential(c->stream, d_matches, stride, d_counts, 0, npairs, *K1, *K2, iterations, threshold, seed, s.models, s.slots,
                         d_out, d_masks, stride);
    if (hipGetLastError() != hipSuccess) return fail("essential launch failed");
    return 0;
}

// ----------------------------------------------------------- Gauss-Newton refit of a relative pose (kernels_poserefit.hip)
extern "C" int hak_refine_pose(hak_ctx* c, const hak_match_pair* d_matches, int n, const hak_intrinsics* K1, const hak_intrinsics* K2,
                               float threshold, float max_depth, int rounds, unsigned char* d_mask, float* d_xyz, hak_pose* h_inout)
{
    if (list_args(h_inout, d_matches, n, "d_matches must be 16-byte aligned")) return 1;
    if (pose_args(K1, K2, threshold, max_depth) || refine_args(threshold, rounds)) return 1;
    return record_single(c, c, h_inout, h_inout, "pose refit", [&](hipStream_t st, hak_pose* d_rec) {
        hak_launch_pose_refit(st, d_matches, n > 0 ? n : 1, nullptr, n, 1, *K1, *K2, threshold, max_depth, rounds, d_rec, d_mask, d_xyz);
    });
}

extern "C" int hak_refine_pose_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts, int npairs,
                                     const hak_intrinsics* K1, const hak_intrinsics* K2, float threshold, float max_depth, int rounds,
                                     hak_pose* d_inout, unsigned char* d_masks, float* d_xyz)
{
    if (list_args_batch(c, d_matches, d_counts, d_inout, npairs, stride, "d_matches must be 16-byte aligned")) return 1;
    if (pose_args(K1, K2, threshold, max_depth) || refine_args(threshold, rounds)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_pose_refit(c->stream, d_matches, stride, d_counts, 0, npairs, *K1, *K2, threshold, max_depth, rounds, d_inout, d_masks,
                          d_xyz);
    if (hipGetLastError() != hipSuccess) return fail("pose refit launch failed");
    return 0;
}

// ----------------------------------------------------------- track linking and RANSAC absolute pose (kernels_pnp.hip)
extern "C" int hak_link_tracks(hak_ctx* c, const hak_match_pair* d_A, int nA, const unsigned char* d_maskA, const float* d_xyzA,
                               const hak_match_pair* d_B, int nB, int max_index, hak_corr3d* d_out, int* count, hak_corr3d* h_out)
{
    if (!count || (!d_A && nA > 0) || (!d_xyzA && nA > 0) || (!d_B && nB > 0) || (!d_out && nB > 0)) return fail("null argument");
    if (nA < 0 || nB < 0 || nA >= (1 << 30) || nB >= (1 << 30)) return fail("a count is negative or not below 2^30");
    if (max_index < 1) return fail("max_index < 1");
    if (misaligned16(d_A) || misaligned16(d_B) || misaligned16(d_out)) return fail("the lists must be 16-byte aligned");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    int* d_tab = nullptr;
    int* d_cnt = nullptr;
    char* block = nullptr;
    if (c) {
        if (grow_scratch(c->link_tab, c->link_cap, max_index) || geom_record(c)) return 1;
        d_tab = c->link_tab;
        d_cnt = reinterpret_cast<int*>(c->geom_rec + HAK_REC_BYTES);
    } else {
        // one allocation: count (16 bytes) | table
        HIP_TRY(hipMalloc((void**)&block, 16 + sizeof(int) * (size_t)max_index));
        d_cnt = reinterpret_cast<int*>(block);
        d_tab = reinterpret_cast<int*>(block + 16);
    }
    hipStream_t st = c ? c->stream : nullptr;
    order_after_null_stream(c, st);
    hak_launch_link(st, d_A, nA > 0 ? nA : 1, nullptr, 1, nA, d_maskA, d_xyzA, d_B, nB > 0 ? nB : 1, nullptr, 1, nB, 1, max_index, d_tab,
                    d_out, nB > 0 ? nB : 1, d_cnt);
    int rc = single_tail(0, st, "link", "count download", count, d_cnt, sizeof(int), block);
    if (!rc && h_out && *count > 0 &&
        hipMemcpy(h_out, d_out, sizeof(hak_corr3d) * (size_t)*count, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail("list download");
    return rc;
}

extern "C" int hak_link_tracks_batch(hak_ctx* c, const hak_match_pair* d_A, long strideA, const int* d_countsA, int count_stepA,
                                     const unsigned char* d_masksA, const float* d_xyzA, const hak_match_pair* d_B, long strideB,
                                     const int* d_countsB, int count_stepB, int npairs, hak_corr3d* d_out, long out_stride,
                                     int* d_counts)
{
    if (!c) return fail("null context");
    if (!d_A || !d_countsA || !d_xyzA || !d_B || !d_countsB || !d_out || !d_counts) return fail("null argument");
    if (npairs < 1 || strideA < 1 || strideB < 1 || out_stride < 1 || count_stepA < 1 || count_stepB < 1)
        return fail("npairs, the strides and the count steps must be >= 1");
    if (misaligned16(d_A) || misaligned16(d_B) || misaligned16(d_out)) return fail("the lists must be 16-byte aligned");
    if (c->cfg.max_pts < 1) return fail("max_index < 1");
    if (grow_scratch(c->link_tab, c->link_cap, (long)npairs * c->cfg.max_pts)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_link(c->stream, d_A, strideA, d_countsA, count_stepA, 0, d_masksA, d_xyzA, d_B, strideB, d_countsB, count_stepB, 0,
                    npairs, c->cfg.max_pts, c->link_tab, d_out, out_stride, d_counts);
    if (hipGetLastError() != hipSuccess) return fail("link launch failed");
    return 0;
}

static int pnp_args(const hak_intrinsics* K, int iterations, float threshold)
{
    if (!K) return fail("null intrinsics");
    return ransac_args(iterations, threshold, 0) || intrinsics_args(K);
}

extern "C" int hak_solve_pnp(hak_ctx* c, const hak_corr3d* d_corr, int n, const hak_intrinsics* K, int iterations, float threshold,
                             unsigned seed, unsigned char* d_mask, hak_abs_pose* h_out)
{
    if (list_args(h_out, d_corr, n, "d_corr must be 16-byte aligned") || pnp_args(K, iterations, threshold)) return 1;
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    RansacScratch s;
    if (ransac_scratch(c, hak_homography_blocks(1, iterations, nullptr), hak_pnp_words(1, iterations), s)) return 1;
    hipStream_t st = c ? c->stream : nullptr;
    order_after_null_stream(c, st);
    hak_launch_pnp(st, d_corr, n > 0 ? n : 1, nullptr, n, 1, *K, iterations, threshold, seed, s.models, s.slots,
                   static_cast<hak_abs_pose*>(s.rec), d_mask, 0);
    return single_tail(0, st, "pnp", "pnp download", h_out, s.rec, sizeof(hak_abs_pose), s.block);
}

extern "C" int hak_solve_pnp_batch(hak_ctx* c, const hak_corr3d* d_corr, long stride, const int* d_counts, int npairs,
                                   const hak_intrinsics* K, int iterations, float threshold, unsigned seed, hak_abs_pose* d_out,
                                   unsigned char* d_masks)
{
    if (list_args_batch(c, d_corr, d_counts, d_out, npairs, stride, "d_corr must be 16-byte aligned", "null context", "null argument",
                        "npairs and the stride must be >= 1"))
        return 1;
    if (pnp_args(K, iterations, threshold)) return 1;
    RansacScratch s;
    if (ransac_scratch(c, (long)npairs * hak_homography_blocks(npairs, iterations, nullptr), hak_pnp_words(npairs, iterations), s)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_pnp(c->stream, d_corr, stride, d_counts, 0, npairs, *K, iterations, threshold, seed, s.models, s.slots, d_out, d_masks,
                   stride);
    if (hipGetLastError() != hipSuccess) return fail("pnp launch failed");
    return 0;
}

// ----------------------------------------------------------- Gauss-Newton refit of an absolute pose (kernels_pnprefit.hip)
extern "C" int hak_refine_pnp(hak_ctx* c, const hak_corr3d* d_corr, int n, const hak_intrinsics* K, float threshold, int rounds,
                              unsigned char* d_mask, hak_abs_pose* h_inout)
{
    if (list_args(h_inout, d_corr, n, "d_corr must be 16-byte aligned") || refine_args(threshold, rounds) || intrinsics_args(K))
        return 1;
    return record_single(c, c, h_inout, h_inout, "pnp refit", [&](hipStream_t st, hak_abs_pose* d_rec) {
        hak_launch_pnp_refit(st, d_corr, n, nullptr, n, 1, *K, threshold, rounds, d_rec, d_mask, 0);
    });
}

extern "C" int hak_refine_pnp_batch(hak_ctx* c, const hak_corr3d* d_corr, long stride, const int* d_counts, int npairs,
                                    const hak_intrinsics* K, float threshold, int rounds, hak_abs_pose* d_inout,
                                    unsigned char* d_masks)
{
    if (list_args_batch(c, d_corr, d_counts, d_inout, npairs, stride, "d_corr must be 16-byte aligned", "null context", "null argument",
                        "npairs and the stride must be >= 1"))
        return 1;
    if (refine_args(threshold, rounds) || intrinsics_args(K)) return 1;
    order_after_null_stream(c, c->stream);
    hak_launch_pnp_refit(c->stream, d_corr, stride, d_counts, 0, npairs, *K, threshold, rounds, d_inout, d_masks, stride);
    if (hipGetLastError() != hipSuccess) return fail("pnp refit launch failed");
    return 0;
}

// ----------------------------------------------------------- triangulation under two known views (kernels_triangulate.hip)
static int triangulate_args(const hak_intrinsics* KA, const hak_intrinsics* KB, float threshold, float max_depth, float min_sin)
{
    if (pose_args(KA, KB, threshold, max_depth)) return 1;
    if (!(min_sin >= 0.f && min_sin < 1.f)) return fail("min_sin must be in [0, 1)");
    return 0;
}

static int host_view_args(const float* Rt)
{
    for (int k = 0; Rt && k < 12; k++)
        if (!std::isfinite(Rt[k])) return fail("a host view has a non-finite entry");
    return 0;
}

static int device_view_args(const void* d_views, int kind, int step)
{
    if (kind < HAK_VIEW_IDENTITY || kind > HAK_VIEW_ABSOLUTE) return fail("a view kind must be 0, 1 or 2");
    if (kind != HAK_VIEW_IDENTITY && !d_views) return fail("null view array");
    if (step < 0) return fail("a view step must be >= 0");
    return 0;
}

extern "C" int hak_triangulate(hak_ctx* c, const hak_match_pair* d_matches, int n, const float* RtA, const float* RtB,
                               const hak_intrinsics* KA, const hak_intrinsics* KB, float threshold, float max_depth, float min_sin,
                               unsigned char* d_mask, float* d_xyz, hak_triangulation* h_out)
{
    if (list_args(h_out, d_matches, n, "d_matches must be 16-byte aligned")) return 1;
    if (triangulate_args(KA, KB, threshold, max_depth, min_sin) || host_view_args(RtA) || host_view_args(RtB)) return 1;
    return record_single(c, nullptr, nullptr, h_out, "triangulation", [&](hipStream_t st, hak_triangulation* d_rec) {
        hak_launch_triangulate(st, d_matches, n > 0 ? n : 1, nullptr, 1, n, 1, nullptr, HAK_VIEW_IDENTITY, 0, RtA, nullptr,
                               HAK_VIEW_IDENTITY, 0, RtB, *KA, *KB, threshold, max_depth, min_sin, d_rec, d_mask, d_xyz);
    });
}

extern "C" int hak_triangulate_batch(hak_ctx* c, const hak_match_pair* d_matches, long stride, const int* d_counts, int count_step,
                                     int npairs, const void* d_viewsA, int kindA, int view_stepA, const void* d_viewsB, int kindB,
                                     int view_stepB, const hak_intrinsics* KA, const hak_intrinsics* KB, float threshold,
                                     float max_depth, float min_sin, hak_triangulation* d_out, unsigned char* d_masks, float* d_xyz)
{
    // the context is looked at last, so that every other refusal can be told from it
    if (!d_matches || !d_counts || !d_out) return fail("null argument");
    if (npairs < 1 || stride < 1) return fail("npairs and the stride must be >= 1");
    if (count_step < 1) return fail("the count step must be >= 1");
    if (misaligned16(d_matches)) return fail("d_matches must be 16-byte aligned");
    if (device_view_args(d_viewsA, kindA, view_stepA) || device_view_args(d_viewsB, kindB, view_stepB)) return 1;
    if (triangulate_args(KA, KB, threshold, max_depth, min_sin)) return 1;
    if (!c) return fail("null context");
    order_after_null_stream(c, c->stream);
    hak_launch_triangulate(c->stream, d_matches, stride, d_counts, count_step, 0, npairs, d_viewsA, kindA, view_stepA, nullptr, d_viewsB,
                           kindB, view_stepB, nullptr, *KA, *KB, threshold, max_depth, min_sin, d_out, d_masks, d_xyz);
    if (hipGetLastError() != hipSuccess) return fail("triangulation launch failed");
    return 0;
}

// ----------------------------------------------------------- guided matching (kernels_guided.hip; the rule: include/hipakaze.h)
static int guided_args(float radius, int ratio_num, int ratio_den)
{
    if (!std::isfinite(radius) || !(radius > 0.f)) return fail("radius must be finite and > 0");
    if (!std::isfinite(radius * radius)) return fail("radius * radius must be finite in float32");
    if (ratio_num <= 0 || ratio_den <= 0) return fail("ratio must be a positive fraction");
    return 0;
}

static int guided_scratch(hak_ctx* c, size_t bytes) { return grow_scratch(c->guided, c->guided_cap, (long)bytes, 1); }

// The scratch of a one-list gated call (gated_match_single, hak_match_projected): the grid's buffer -- the context's, or without a
// context a hipMalloc that lives as long as the holder -- and the 2-NN scratch (the context's or the pool's) with room for nq + cap2
// search records and `blks` block counts.  Without a context the holder gives back what it still holds when it goes: a caller whose
// tail releases msc itself clears the pointer, the others say through `ok` how the pool gets it back.
struct GatedScratch {
    hak_ctx* c;
    hipStream_t st;
    long cap2;
    void* buf = nullptr;
    HakMatchScratch* msc = nullptr;
    bool ok = false;

    GatedScratch(hak_ctx* c, int n2) : c(c), st(c ? c->stream : nullptr), cap2(n2 > 0 ? n2 : 1) {}
    GatedScratch(const GatedScratch&) = delete;
    GatedScratch& operator=(const GatedScratch&) = delete;
    ~GatedScratch()
    {
        if (!c && msc) pool_release(msc, ok);
        if (!c) (void)hipFree(buf);
    }
    int acquire(const char* what, long nq, long blks)
    {
        const size_t bytes = hak_guided_scratch_bytes(1, cap2);
        if (c) {
            if (guided_scratch(c, bytes)) return 1;
            buf = c->guided;
        } else
            HIP_TRY(hipMalloc(&buf, bytes));
        msc = c ? &c->msc : pool_acquire();
        order_after_null_stream(c, st);
        if (!hak_match_scratch_reserve(msc, st, 0, 0, 0, nq + cap2, blks))
            return fail(std::string(what) + ": out of device memory for the search scratch");
        return 0;
    }
    // forward records at msc->knn, the reverse words of the nq queries' train set behind them
    HakGuidedScratch carve(long nq) const { return hak_guided_scratch_carve(buf, 1, cap2, msc->knn + nq, 0); }
};
// ... and of a batch call, on the context: its 2-NN records split into a forward and a reverse half of the context's pair capacity
// times max_pts (mp) each, and its grid buffer for as many pairs of max_pts train points
static int gated_batch_scratch(hak_ctx* c, long& mp, int4*& fwd, int4*& rev)
{
    mp = c->cfg.max_pts;
    if (!hak_mkey_fits(mp)) return fail("max_pts must stay below 2^20 for the matcher");
    if (knn_scratch(c)) return 1;
    const long npair_cap = (c->cfg.batch + 1) / 2;
    if (guided_scratch(c, hak_guided_scratch_bytes(npair_cap, mp))) return 1;
    order_after_null_stream(c, c->stream);
    fwd = c->knn;
    rev = c->knn + (size_t)npair_cap * mp;
    return 0;
}

// What the matchers gated by a model of nine floats (hak_match_guided, hak_match_epipolar) share behind their own model checks;
// hak_match_projected has lists of its own around the same scratch.  Single pair, synchronous: search(stream, scratch, fwd)
// enqueues the bin step, the search and the reverse step.
static int gated_args_single(const hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2, const int* count)
{
    if (!count) return fail("null argument");
    if (n1 < 0 || n2 < 0) return fail("negative point count");
    if ((!d_pts1 && n1 > 0) || (!d_pts2 && n2 > 0)) return fail("null point array");
    return 0;
}
template <typename Search>
static int gated_match_single(hak_ctx* c, const char* what, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2, float radius,
                              int ratio_num, int ratio_den, int cross_check, int max_dist, hak_point* h_pts1, hak_match_pair* d_out,
                              int* count, hak_match_pair* h_out, Search search)
{
    if (guided_args(radius, ratio_num, ratio_den)) return 1;
    if (h_out && !d_out) return fail("h_out needs d_out");
    if (!hak_mkey_fits(n1) || !hak_mkey_fits(n2)) return fail("more than 2^20 - 1 points");
    *count = 0;
    if (n1 == 0) return 0;
    if (max_dist <= 0) max_dist = HAK_MAX_DIST;
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    GatedScratch g(c, n2);
    if (g.acquire(what, n1, (n1 + 1023) / 1024)) return 1;
    hipStream_t st = g.st;
    HakMatchScratch* sc = g.msc;
    int4* fwd = sc->knn;
    int4* rev = sc->knn + n1;
    *sc->h_cnt = -1;
    {
        ProfScope ps(c, HAK_PROF_MATCH);
        search(st, g.carve(n1), fwd);
        hak_launch_knn2_finish(st, d_pts1, d_pts2, nullptr, n1, 0, 0, 1, fwd, cross_check ? rev : nullptr, 0, ratio_num, ratio_den,
                               cross_check ? 1 : 0, max_dist, d_out, 0, sc->d_cnt, sc);
    }
    int rc = 0;
    if (hipGetLastError() != hipSuccess) rc = fail(std::string(what) + ": launch failed");
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(std::string(what) + ": hipStreamSynchronize");
    g.msc = nullptr;                                                    // (match_list_tail releases it)
    return match_list_tail(c, sc, rc, h_pts1, d_pts1, n1, d_out, count, h_out);
}
// ... and the batch form, asynchronous on the context's stream: search(scratch, fwd, mp)
template <typename Search>
static int gated_match_batch(hak_ctx* c, const char* what, hak_point* d_points, const int* d_num_pts, int npairs, const void* d_model,
                             float radius, int ratio_num, int ratio_den, int cross_check, int max_dist, hak_match_pair* d_out,
                             int* d_counts, Search search)
{
    if (!c) return fail(std::string(what) + " needs a context");
    if (!d_points || !d_num_pts || !d_model || !d_counts || npairs < 1) return fail("bad argument");
    if (2 * npairs > c->cfg.batch + 1) return fail("npairs exceeds the context's batch capacity");
    if (guided_args(radius, ratio_num, ratio_den)) return 1;
    if (max_dist <= 0) max_dist = HAK_MAX_DIST;
    long mp;
    int4 *fwd, *rev;
    if (gated_batch_scratch(c, mp, fwd, rev)) return 1;
    { ProfScope ps(c, HAK_PROF_MATCH);
      search(hak_guided_scratch_carve(c->guided, (c->cfg.batch + 1) / 2, mp, rev, mp), fwd, mp);
      hak_launch_knn2_finish(c->stream, d_points, d_points + mp, d_num_pts, 0, 2 * mp, 2 * mp, npairs, fwd, cross_check ? rev : nullptr,
                             mp, ratio_num, ratio_den, cross_check ? 1 : 0, max_dist, d_out, mp, d_counts); }
    if (hipGetLastError() != hipSuccess) return fail(std::string(what) + ": launch failed");
    return 0;
}

extern "C" int hak_match_guided(hak_ctx* c, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2, const float* H, float radius,
                                int ratio_num, int ratio_den, int cross_check, int max_dist, hak_point* h_pts1, hak_match_pair* d_out,
                                int* count, hak_match_pair* h_out)
{
    if (gated_args_single(d_pts1, n1, d_pts2, n2, count)) return 1;
    if (!H) return fail("H is NULL");
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(H[k])) return fail("H has a non-finite entry");
    return gated_match_single(c, "hak_match_guided", d_pts1, n1, d_pts2, n2, radius, ratio_num, ratio_den, cross_check, max_dist, h_pts1,
                              d_out, count, h_out, [&](hipStream_t st, const HakGuidedScratch& gs, int4* fwd) {
                                  hak_launch_guided(st, d_pts1, d_pts2, nullptr, nullptr, 1, n1, n2, 0, 0, 1, nullptr, H, radius,
                                                    cross_check ? 1 : 0, gs, fwd, 0);
                              });
}

extern "C" int hak_match_guided_batch(hak_ctx* c, hak_point* d_points, const int* d_num_pts, int npairs, const hak_homography* d_H,
                                      float radius, int ratio_num, int ratio_den, int cross_check, int max_dist, hak_match_pair* d_out,
                                      int* d_counts)
{
    return gated_match_batch(c, "hak_match_guided_batch", d_points, d_num_pts, npairs, d_H, radius, ratio_num, ratio_den, cross_check,
                             max_dist, d_out, d_counts, [&](const HakGuidedScratch& gs, int4* fwd, long mp) {
                                 hak_launch_guided(c->stream, d_points, d_points + mp, d_num_pts, d_num_pts + 1, 2, (int)mp, (int)mp,
                                                   2 * mp, 2 * mp, npairs, d_H, nullptr, radius, cross_check ? 1 : 0, gs, fwd, mp);
                             });
}

// epipolar guided matching (kernels_epipolar.hip): a fundamental matrix in the homography's place
extern "C" int hak_match_epipolar(hak_ctx* c, hak_point* d_pts1, int n1, const hak_point* d_pts2, int n2, const float* F, float radius,
                                  int ratio_num, int ratio_den, int cross_check, int max_dist, hak_point* h_pts1, hak_match_pair* d_out,
                                  int* count, hak_match_pair* h_out)
{
    if (gated_args_single(d_pts1, n1, d_pts2, n2, count)) return 1;
    if (!F) return fail("F is NULL");
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(F[k])) return fail("F has a non-finite entry");
    return gated_match_single(c, "hak_match_epipolar", d_pts1, n1, d_pts2, n2, radius, ratio_num, ratio_den, cross_check, max_dist, h_pts1,
                              d_out, count, h_out, [&](hipStream_t st, const HakGuidedScratch& gs, int4* fwd) {
                                  hak_launch_epipolar(st, d_pts1, d_pts2, nullptr, nullptr, 1, n1, n2, 0, 0, 1, nullptr, F, radius,
                                                      cross_check ? 1 : 0, gs, fwd, 0);
                              });
}

extern "C" int hak_match_epipolar_batch(hak_ctx* c, hak_point* d_points, const int* d_num_pts, int npairs, const hak_fundamental* d_F,
                                        float radius, int ratio_num, int ratio_den, int cross_check, int max_dist, hak_match_pair* d_out,
                                        int* d_counts)
{
    return gated_match_batch(c, "hak_match_epipolar_batch", d_points, d_num_pts, npairs, d_F, radius, ratio_num, ratio_den, cross_check,
                             max_dist, d_out, d_counts, [&](const HakGuidedScratch& gs, int4* fwd, long mp) {
                                 hak_launch_epipolar(c->stream, d_points, d_points + mp, d_num_pts, d_num_pts + 1, 2, (int)mp, (int)mp,
                                                     2 * mp, 2 * mp, npairs, d_F, nullptr, radius, cross_check ? 1 : 0, gs, fwd, mp);
                             });
}

// ----------------------------------------------------------- projection-guided matching (kernels_projected.hip; the rule: include/hipakaze.h)
static int projected_args(const hak_intrinsics* K, float radius, int ratio_num, int ratio_den)
{
    if (!K) return fail("null intrinsics");
    return guided_args(radius, ratio_num, ratio_den) || intrinsics_args(K);
}

extern "C" int hak_match_projected(hak_ctx* c, const hak_match_pair* d_A, int nA, const unsigned char* d_maskA, const float* d_xyzA,
                                   const hak_point* d_desc, int n_desc, const hak_point* d_pts2, int n2, const float* Rt,
                                   const hak_intrinsics* K, float radius, int ratio_num, int ratio_den, int cross_check, int max_dist,
                                   hak_corr3d* d_out, int* count, hak_corr3d* h_out)
{
    if (!count) return fail("null argument");
    if (nA < 0 || n_desc < 0 || n2 < 0) return fail("negative count");
    if (!hak_mkey_fits(nA) || !hak_mkey_fits(n_desc) || !hak_mkey_fits(n2)) return fail("more than 2^20 - 1 records");
    if (((!d_A || !d_xyzA) && nA > 0) || (!d_desc && n_desc > 0) || (!d_pts2 && n2 > 0)) return fail("null array with a positive count");
    if (h_out && !d_out) return fail("h_out needs d_out");
    if (misaligned16(d_A) || misaligned16(d_out)) return fail("the lists must be 16-byte aligned");
    if (projected_args(K, radius, ratio_num, ratio_den) || host_view_args(Rt)) return 1;
    *count = 0;
    if (nA == 0) return 0;
    if (max_dist <= 0) max_dist = HAK_MAX_DIST;
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    GatedScratch g(c, n2);
    if (g.acquire("hak_match_projected", nA, 1)) return 1;
    {
        ProfScope ps(c, HAK_PROF_MATCH);
        hak_launch_projected(g.st, d_A, nA, nullptr, 1, nA, nA, d_maskA, d_xyzA, d_desc, n_desc > 0 ? n_desc : 1, nullptr, 1, n_desc,
                             n_desc, d_pts2, g.cap2, nullptr, 1, n2, 1, nullptr, HAK_VIEW_IDENTITY, 0, Rt, *K, radius, ratio_num, ratio_den,
                             cross_check ? 1 : 0, max_dist, g.carve(nA), g.msc->knn, 0, d_out, nA, g.msc->d_cnt);
    }
    int rc = single_tail(0, g.st, "hak_match_projected", "count download", count, g.msc->d_cnt, sizeof(int));
    g.ok = rc == 0;
    if (!rc && h_out && *count > 0 &&
        hipMemcpy(h_out, d_out, sizeof(hak_corr3d) * (size_t)*count, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail("list download");
    return rc;
}

extern "C" int hak_match_projected_batch(hak_ctx* c, const hak_match_pair* d_A, long strideA, const int* d_countsA, int count_stepA,
                                         const unsigned char* d_masksA, const float* d_xyzA, const hak_point* d_desc, long desc_stride,
                                         const int* d_desc_counts, int desc_count_step, const hak_point* d_pts2, long stride2,
                                         const int* d_counts2, int count_step2, int npairs, const void* d_views, int kind, int view_step,
                                         const hak_intrinsics* K, float radius, int ratio_num, int ratio_den, int cross_check,
                                         int max_dist, hak_corr3d* d_out, long out_stride, int* d_counts)
{
    // the context is looked at last, so that every other refusal can be told from it
    if (!d_A || !d_countsA || !d_xyzA || !d_desc || !d_desc_counts || !d_pts2 || !d_counts2 || !d_out || !d_counts)
        return fail("null argument");
    if (npairs < 1 || strideA < 1 || desc_stride < 1 || stride2 < 1 || out_stride < 1 || count_stepA < 1 || desc_count_step < 1 ||
        count_step2 < 1)
        return fail("npairs, the strides and the count steps must be >= 1");
    if (misaligned16(d_A) || misaligned16(d_out)) return fail("the lists must be 16-byte aligned");
    if (device_view_args(d_views, kind, view_step)) return 1;
    if (projected_args(K, radius, ratio_num, ratio_den)) return 1;
    if (!c) return fail("hak_match_projected_batch needs a context");
    if (npairs > (c->cfg.batch + 1) / 2) return fail("npairs exceeds the context's pair capacity");
    if (max_dist <= 0) max_dist = HAK_MAX_DIST;
    long mp;
    int4 *fwd, *rev;
    if (gated_batch_scratch(c, mp, fwd, rev)) return 1;
    const long capA = std::min(std::min(strideA, out_stride), mp), capD = std::min(desc_stride, mp), cap2 = std::min(stride2, mp);
    { ProfScope ps(c, HAK_PROF_MATCH);
      hak_launch_projected(c->stream, d_A, strideA, d_countsA, count_stepA, 0, capA, d_masksA, d_xyzA, d_desc, desc_stride, d_desc_counts,
                           desc_count_step, 0, capD, d_pts2, stride2, d_counts2, count_step2, (int)cap2, npairs, d_views, kind, view_step,
                           nullptr, *K, radius, ratio_num, ratio_den, cross_check ? 1 : 0, max_dist,
                           hak_guided_scratch_carve(c->guided, npairs, cap2, rev, mp), fwd, mp, d_out, out_stride, d_counts); }
    if (hipGetLastError() != hipSuccess) return fail("hak_match_projected_batch: launch failed");
    return 0;
}

// ----------------------------------------------------------- memory helpers
extern "C" int hak_points_alloc(hak_point** d, int count)
{
    HIP_TRY(hipMalloc((void**)d, sizeof(hak_point) * (size_t)count));
    HIP_TRY(hipMemset(*d, 0, sizeof(hak_point) * (size_t)count));
    HIP_TRY(hipStreamSynchronize(nullptr));                     // (the fill runs on the NULL stream; the caller's streams need not wait for that one)
    return 0;
}
extern "C" int hak_points_free(hak_point* d) { HIP_TRY(hipFree(d)); return 0; }

extern "C" int hak_image_alloc(float** d, int w, int h, int* pitch)
{
    int p = (w % 128 != 0) ? (w - w % 128 + 128) : w;                             // cuda_utils.h:160, main.cpp:174
    HIP_TRY(hipMalloc((void**)d, sizeof(float) * (size_t)p * h));
    if (pitch) *pitch = p;
    return 0;
}
extern "C" int hak_image_upload(float* d, int pitch, const float* hsrc, int w, int h)
{
    HIP_TRY(hipMemcpy2D(d, sizeof(float) * pitch, hsrc, sizeof(float) * w, sizeof(float) * w, h, hipMemcpyHostToDevice));
    return 0;
}
extern "C" int hak_image_free(float* d) { HIP_TRY(hipFree(d)); return 0; }

extern "C" int hak_ingest_u8(hak_ctx* c, const unsigned char* d_src, long src_stride, int src_pitch,
                             float* d_dst, long dst_stride, int dst_pitch, int w, int h, int nimg)
{
    if (!d_src || !d_dst || w < 1 || h < 1 || nimg < 1 || src_pitch < w || dst_pitch < w) return fail("bad ingest argument");
    if (hak_device_count() == 0) return fail("no HIP device: libhipakaze has no CPU fallback");
    order_after_null_stream(c, c ? c->stream : nullptr);
    hak_launch_ingest_u8(c ? c->stream : nullptr, d_src, src_stride, src_pitch, d_dst, dst_stride, dst_pitch, w, h, nimg);
    if (hipGetLastError() != hipSuccess) return fail("ingest launch failed");
    return 0;
}
extern "C" int hak_host_alloc(void** p, long bytes) { HIP_TRY(hipHostMalloc(p, (size_t)bytes)); return 0; }
extern "C" int hak_host_free(void* p) { HIP_TRY(hipHostFree(p)); return 0; }

extern "C" int hak_download_batch(hak_ctx* c, const hak_point* d_points, const int* d_num_pts, int nimg,
                                  hak_point* h_points, int* h_num_pts)
{
    if (!c || !d_points || !d_num_pts || !h_points || !h_num_pts) return fail("null argument");
    // pinned (device-visible) destination buffers -- hak_host_alloc -- take one kernel that stores counts and records over PCIe
    {
        hipPointerAttribute_t ap{}, an{};
        const bool pinned = hipPointerGetAttributes(&ap, h_points) == hipSuccess && ap.type == hipMemoryTypeHost &&
                            hipPointerGetAttributes(&an, h_num_pts) == hipSuccess && an.type == hipMemoryTypeHost;
        (void)hipGetLastError();                                    // a pageable pointer makes the query fail: not an error here
        if (pinned) {
            hak_launch_download(c->stream, d_points, d_num_pts, c->cfg.max_pts, nimg, h_points, h_num_pts);
            if (hipGetLastError() != hipSuccess) return fail("download launch failed");
            HIP_TRY(hipStreamSynchronize(c->stream));
            return 0;
        }
    }
    HIP_TRY(hipMemcpyAsync(h_num_pts, d_num_pts, sizeof(int) * (size_t)nimg, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long mp = c->cfg.max_pts;
    for (int i = 0; i < nimg; i++)
        if (h_num_pts[i] > 0)
            HIP_TRY(hipMemcpyAsync(h_points + i * mp, d_points + i * mp, sizeof(hak_point) * (size_t)h_num_pts[i],
                                   hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int hak_memcpy_d2h(void* dst, const void* src, long bytes)
{
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int hak_memcpy_h2d(void* dst, const void* src, long bytes)
{
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return 0;
}

// ------------------------------------------------------------ introspection
extern "C" int hak_query_schedule(const hak_ctx* c, int* nsteps, int* sigma_size, float* sizes, float* borders)
{
    if (!c) return -1;
    for (size_t l = 0; l < c->plan.size(); l++) {
        if (nsteps) nsteps[l] = c->plan[l].nsteps;
        if (sigma_size) sigma_size[l] = c->plan[l].sigma_size;
        if (sizes) sizes[l] = c->plan[l].size;
        if (borders) borders[l] = c->plan[l].border;
    }
    return c->L.noct;
}

extern "C" int hak_query_geometry(const hak_ctx* c, int* whp)
{
    if (!c) return -1;
    for (int o = 0; o < c->L.noct; o++) {
        whp[3 * o] = c->L.oct[o].w; whp[3 * o + 1] = c->L.oct[o].h; whp[3 * o + 2] = c->L.oct[o].p;
    }
    return c->L.noct;
}

extern "C" int hak_query_traffic(const hak_ctx* c, int npts_hint, hak_traffic* out)
{
    if (!c || !out) return fail("null argument");
    const HakLayout& L = c->L;
    double pxsteps = 0, all = 0, folded = 0;
    int launches = 0;
    for (int o = 0; o < L.noct; o++) {
        const double N = (double)L.oct[o].w * L.oct[o].h;
        for (int s = 0; s < L.ms; s++) {
            const LevelPlan& lp = c->plan[(size_t)o * L.ms + s];
            pxsteps += N * lp.nsteps;
            launches += lp.nsteps ? hak_fed_groups(lp.nsteps, c->knobs.max_fuse, L.oct[o].w, hak_fed_wide_only(o, L.oct[o].w)) : 0;
            // sublevels whose low-pass (8 B/px) + conductivity (8 B/px) run inside the first FED launch (k_fed_sf), and octave
            // heads whose decimation + low-pass (4 N_{o-1} + 8 N_o) + conductivity (8 N_o) do
            if (s > 0 && hak_fed_sf_covers(c->knobs, c->cfg.diffusivity, L.oct[o], c->cfg.batch)) folded += 16.0 * N;
            if (s == 0 && o > 0 && hak_fed_sf_covers(c->knobs, c->cfg.diffusivity, L.oct[o], c->cfg.batch, &L.oct[o - 1]))
                folded += 4.0 * L.oct[o - 1].w * L.oct[o - 1].h + 16.0 * N;
            if (o == 0 && s == 0) all += 56.0 * N;                                // o0 prologue
            else if (s == 0) all += 4.0 * L.oct[o - 1].w * L.oct[o - 1].h + 8.0 * N + 8.0 * N + 24.0 * N + 4.0 * N;
            else all += 44.0 * N;
        }
    }
    all += 16.0 * L.oct[0].w * L.oct[0].h;                                        // maps init + NMS scan
    all += 12.0 * pxsteps;
    all += (872.0 + 5292.0 + 104.0) * npts_hint;
    out->fed_px_steps = pxsteps;
    out->fed_bytes = 12.0 * pxsteps + folded;
    out->all_stage_bytes = all;
    out->fed_launches = launches;
    // per-class compulsory bytes of the launches AS BUILT (fused): what each class must move per image even with perfect
    // reuse inside a launch.  The FED figure is accumulated by the launch sequence itself (valid after the first detect call).
    out->fed_fused_bytes = c->fed_fused_bytes;
    double lvl_px = 0;
    for (int o = 0; o < L.noct; o++) lvl_px += (double)L.ms * L.oct[o].w * L.oct[o].h;
    out->hessian_bytes = 12.0 * lvl_px;                                           // read smooth, write the interleaved {Lx, Ly} plane
    out->prologue_bytes = 16.0 * L.oct[0].w * L.oct[0].h;                         // read img, write Lt + gradient; re-read gradient (histogram)
    out->describe_bytes = (872.0 + 5292.0) * npts_hint;                           // sampled bytes per keypoint (orientation + MLDB)
    out->nms_bytes = 104.0 * npts_hint;
    return 0;
}

extern "C" int hak_prof_enable(hak_ctx* c, int on) { if (!c) return 1; c->prof_on = on != 0; return 0; }
extern "C" int hak_prof_reset(hak_ctx* c)
{
    if (!c) return 1;
    for (auto& p : c->prof) { p.used = 0; p.acc_ms = 0; p.launches = 0; }
    return 0;
}
extern "C" int hak_prof_read(hak_ctx* c, int k, double* total_ms, int* launches)
{
    if (!c || k < 0 || k >= HAK_PROF_COUNT) return fail("bad profile class");
    HIP_TRY(hipStreamSynchronize(c->stream));
    ProfClass& p = c->prof[k];
    for (size_t i = 0; i + 1 < p.used; i += 2) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
        p.acc_ms += ms;
    }
    p.used = 0;
    if (total_ms) *total_ms = p.acc_ms;
    if (launches) *launches = p.launches;
    return 0;
}

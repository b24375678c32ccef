// hak_knobs.hip -- the one place that reads the environment: name, field and clamp of every HAK_* variable (defaults: hak_knobs.h)
#include "hak_knobs.h"
#include <climits>
#include <cstdlib>

// the variable's value clamped to lo..hi, or dflt when it is not set (text that is no number counts as 0, as with atoi)
static int env_int(const char* name, int dflt, int lo = INT_MIN, int hi = INT_MAX)
{
    const char* e = getenv(name);
    if (!e) return dflt;
    const long v = strtol(e, nullptr, 10);
    return v < lo ? lo : (v > hi ? hi : (int)v);
}

HakKnobs hak_knobs_from_env()
{
    static const struct { const char* name; int HakKnobs::*field; int lo, hi; } rows[] = {
        {"HAK_HESS_STREAM", &HakKnobs::hess_stream, INT_MIN, INT_MAX},
        {"HAK_BASE_STREAM", &HakKnobs::base_stream, INT_MIN, INT_MAX},
        {"HAK_BASE_HIST", &HakKnobs::base_hist, INT_MIN, INT_MAX},
        {"HAK_HESS_CBUF", &HakKnobs::hess_cbuf, 1, 256},
        {"HAK_DESC_ORDER", &HakKnobs::desc_order, 0, 255},
        {"HAK_DESC_PLAN", &HakKnobs::desc_plan, INT_MIN, INT_MAX},
        {"HAK_DESC_SORT", &HakKnobs::desc_sort, INT_MIN, INT_MAX},
        {"HAK_DESC_GATHER", &HakKnobs::desc_gather, INT_MIN, INT_MAX},
        {"HAK_HESS_LP", &HakKnobs::hess_lp, INT_MIN, INT_MAX},
        {"HAK_LEVEL_TILE", &HakKnobs::level_tile, INT_MIN, INT_MAX},
        {"HAK_LEVEL_HESS", &HakKnobs::level_hess, INT_MIN, INT_MAX},
        {"HAK_LEVEL_MIN_STEPS", &HakKnobs::level_min_steps, INT_MIN, INT_MAX},
        {"HAK_LEVEL_MIN_BLOCKS", &HakKnobs::level_min_blocks, 1, INT_MAX},
        {"HAK_FUSE_SF", &HakKnobs::fuse_sf, INT_MIN, INT_MAX},
        {"HAK_FUSE_HEAD", &HakKnobs::fuse_head, INT_MIN, INT_MAX},
        {"HAK_FED_MAX_FUSE", &HakKnobs::max_fuse, 1, HAK_FED_MAX_FUSE},
        {"HAK_HIST_MIN_BLOCKS", &HakKnobs::hist_min_blocks, 1, INT_MAX},
        {"HAK_HIST_RPB_MAX", &HakKnobs::hist_rpb_max, 1, INT_MAX},
        {"HAK_HESS_SIDE", &HakKnobs::hess_side, INT_MIN, INT_MAX},
        {"HAK_SPINE_MAX_PX", &HakKnobs::spine_max_px, INT_MIN, INT_MAX},
        {"HAK_SIDE_STREAMS", &HakKnobs::side_streams, 1, INT_MAX},
        {"HAK_GRAPH_PADS", &HakKnobs::graph_pads, INT_MIN, INT_MAX},
        {"HAK_TAIL_FORK", &HakKnobs::tail_fork, INT_MIN, INT_MAX},
        {"HAK_GRAPH", &HakKnobs::graph, INT_MIN, INT_MAX},
        {"HAK_SERIAL", &HakKnobs::serial, INT_MIN, INT_MAX},
        {"HAK_NULL_ORDER", &HakKnobs::null_order, INT_MIN, INT_MAX},
        {"HAK_TIMING", &HakKnobs::timing, INT_MIN, INT_MAX},
        {"HAK_PROF_FENCE", &HakKnobs::prof_fence, INT_MIN, INT_MAX},
        {"HAK_STREAM_MIN_WAVES", &HakKnobs::stream_min_waves, 1, INT_MAX},
        {"HAK_DOWNLOAD_BLOCKS", &HakKnobs::download_blocks, 1, INT_MAX},
    };
    HakKnobs k;
    for (const auto& r : rows) k.*r.field = env_int(r.name, k.*r.field, r.lo, r.hi);
    return k;
}

const HakKnobs& hak_process_knobs()
{
    static const HakKnobs k = hak_knobs_from_env();
    return k;
}

HakMatchKnobs hak_match_knobs_from_env()
{
    HakMatchKnobs m;
    m.valu = env_int("HAK_MATCH_VALU", m.valu);
    m.qt = env_int("HAK_MATCH_QT", m.qt) == 2 ? 2 : 1;
    m.slices = env_int("HAK_MATCH_SLICES", m.slices);
    return m;
}

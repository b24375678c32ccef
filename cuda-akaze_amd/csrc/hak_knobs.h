// hak_knobs.h -- every HAK_* tuning variable of the library: the field it fills and its default (here), its name and its clamp
// (the table in hak_knobs.hip, the only file of the library that reads the environment).  Internal.
// The variables never change results, only which of two bit-identical kernels or launch orders runs.
#pragma once
#include "../../include/hipakaze.h"

#define HAK_FED_MAX_FUSE 8        // most FED steps one launch fuses: 4 on 4-px lanes, 8 on 2-px lanes, whose rings cost half the
                                  // registers per fused step (kernels_fed.hip)

// PER CONTEXT: hak_create reads them once, into hak_ctx::knobs (two contexts of a process may differ; tests and A/B runs set the
// variables before they create a context).  The launchers get them through the context, its HakBatch or a const HakKnobs&.
// A HakBatch without a context (the stage operators of the test library) reads them per call: hak_knobs_of().
struct HakKnobs {
    int hess_stream = 1;          // HAK_HESS_STREAM: register-streaming Hessian kernel 0 never / 1 by the size rule / 2 always where it applies
    int base_stream = 1;          // HAK_BASE_STREAM: same for pass A of the octave-0 prologue
    int base_hist = 0;            // HAK_BASE_HIST=1: the streaming prologue finds the (lattice) contrast maximum first and bins the gradient on the
                                  // fly (no gradient plane, no histogram pass).  Off by default: half the bytes, 4 % SLOWER (the pass is bound by
                                  // vector issue; kernels_base_stream.hip)
    int hess_cbuf = 256;          // HAK_HESS_CBUF: staged candidates per block of the tile kernel (1..256; tests drive the overflow path)
    int desc_order = 4;           // HAK_DESC_ORDER: image group size of the describe kernels' block order (0..255)
    int desc_plan = 1;            // HAK_DESC_PLAN: planned MLDB kernel (k_describe_runs) on / off
    int desc_sort = 1;            // HAK_DESC_SORT: the keypoint kernels visit an image's keypoints level by level (raster order within a
                                  // level) instead of in output order: 0 never / 1 in batches of 8 images and more / 2 always
    int desc_gather = 1;          // HAK_DESC_GATHER: samples that share a gather instruction of k_describe_runs: 1 neighbours along image
                                  // rows (the order table of the keypoint's angle bin) / 0 consecutive window samples
    int hess_lp = 0;             // HAK_HESS_LP=1: the streaming Hessian low-passes Lt(o,s-1) itself and k_fed_sf stops storing `smooth`.
                                  // Off by default: measured 0.6 ms per 384 x 1080p SLOWER (FED -1.2 ms, Hessian +1.9 ms)
    int level_tile = 1;           // HAK_LEVEL_TILE: one launch per sublevel out of LDS tiles (k_level_tile) 0 never / 1 for launches of at
                                  // most HAK_LEVEL_TILE_MAX_PX pixels unless the streaming kernels are forced / 2 always
    int level_hess = 1;           // HAK_LEVEL_HESS=0: the level's Hessian as a launch of its own instead of inside k_level_tile
    int level_min_steps = 8;      // HAK_LEVEL_MIN_STEPS: shortest FED cycle that goes through k_level_tile under the size rule
    int level_min_blocks = 96;    // HAK_LEVEL_MIN_BLOCKS: k_level_tile's tiles shrink until a launch has this many blocks (>= 1)
    int fuse_sf = 1;              // HAK_FUSE_SF: low-pass + conductivity fused into the first FED launch of a sublevel: 0 never, 1 by size
                                  // (hak_stream_pays), 2 always where covered
    int fuse_head = 1;            // HAK_FUSE_HEAD=0: octave heads not through the decimating k_fed_sf variant
    int max_fuse = 8;             // HAK_FED_MAX_FUSE: FED steps fused per launch (1..HAK_FED_MAX_FUSE).  Above 4 a cycle takes the deeper 2-px
                                  // groups where they save launches (hak_fed_groups); 1, 2 and 4 give the 4-px sequence
    int hist_min_blocks = 256;    // HAK_HIST_MIN_BLOCKS: the prologue's histogram pass halves its rows per block below this many blocks (>= 1)
    int hist_rpb_max = 8;         // HAK_HIST_RPB_MAX: ... starting from this many rows per block (>= 1)
    int hess_side = 0;            // HAK_HESS_SIDE=1: octave 0's Hessians on a stream of their own for launches in the tile-kernel regime.  Off by
                                  // default: measured SLOWER (pair call 0.62 vs 0.57 ms) -- a fifth concurrent chain stretches the other four
                                  // more than the shorter chain gains
    int spine_max_px = 0;         // HAK_SPINE_MAX_PX > 0: spine order for launches of at most this many octave-0 pixels (hak_sequence.hip, spine_pays)
    int side_streams = HAK_MAX_OCTAVES;   // HAK_SIDE_STREAMS: side streams of the spine order (>= 1; more than there are octaves: one each)
    int graph_pads = 1;           // HAK_GRAPH_PADS=0: no empty nodes that steer the captured spine's side chains to queues of their own
    int tail_fork = 1;            // HAK_TAIL_FORK=0: the map clean-up of a spine sequence in front of the descriptor kernels, not beside them
    int graph = 1;                // HAK_GRAPH: 0 never replay a captured graph, 1 replay except for launch-bound single-image sequences, 2 always
    int serial = 0;               // HAK_SERIAL=1: the octaves one after the other on one stream (initial value of hak_set_concurrency)
    int null_order = 1;           // HAK_NULL_ORDER=0: calls do not order themselves behind the NULL stream (initial value of hak_set_null_order)
    int timing = 0;               // HAK_TIMING=1: hak_detect_and_compute prints its host-side split every 100 calls -- diagnosis only
    int prof_fence = 0;           // HAK_PROF_FENCE=1: the profiling events keep their system-scope fence (A/B; hak_ctx.h, ProfScope)
    // ONCE PER PROCESS: geometry constants of launchers that see neither a context nor a HakBatch.  They are used through
    // hak_process_knobs() only; a context's copy of these two fields is not looked at.
    int stream_min_waves = 2048;  // HAK_STREAM_MIN_WAVES: hak_stream_rows halves the row segments below this many waves (>= 1)
    int download_blocks = 128;    // HAK_DOWNLOAD_BLOCKS: blocks per image of k_download_pair (>= 1)
};
HakKnobs hak_knobs_from_env();            // the defaults above, overridden and clamped by the table in hak_knobs.hip
const HakKnobs& hak_process_knobs();      // hak_knobs_from_env() at first use (the two ONCE PER PROCESS fields)

// PER CALL: the matcher works without a context (hak_match(NULL, ...)) and the tests run all its kernels in one process.
struct HakMatchKnobs {
    int valu = 0;                 // HAK_MATCH_VALU=1: the VALU / LDS kernel k_match instead of the matrix-core kernel k_match_mfma
    int qt = 1;                   // HAK_MATCH_QT = 1 | 2: query tiles per wave of k_match_mfma (2 measured slower; anything else: 1)
    int slices = 0;               // HAK_MATCH_SLICES > 0: train-set slices of a sliced search instead of the rule (tuning)
};
HakMatchKnobs hak_match_knobs_from_env();

// orbfe_extractor.h -- the extractor handle (orbfe_handle), private to the files that implement its entry points: orbfe_api.hip
// (create / destroy, options, the batched call) and orbfe_taps.hip (the pyramid read-back and the stage taps).
#pragma once

#include "orbfe_common.h"
#include "orbfe_host.h"
#include "orbfe_kernels.h"
#include "orbfe_plan.h"

#define ORBFE_PROF_RING 64
// event marks of one profiled call: 0 start, 1 pyramid done, 2 FAST done, 3 quadtree done, 4 describe start, 5 end (launch
// stream); 6 / 7 around the blur (on whichever stream it ran)
#define ORBFE_EV_N 8
// auto FAST mode: above this share of pixel pairs passing the necessary test the dense form is the cheaper one.  Measured per
// 1024 frames of 640x480 (tools/compact_ab.py, profiles/r05_compact_ab.json; dense / lane-compacting, ms): pass rate 0.84 (S)
// 1.47 / 2.14; 0.43 1.40 / 1.62; 0.38 1.42 / 1.55; 0.29 1.36 / 1.39; 0.18 (S_tum) 1.33 / 1.12; 0.076 1.26 / 0.92;
// 0.02 1.22 / 0.74 -- break-even near 0.27
#define ORBFE_AUTO_DENSE_RATE 0.25
// ... and a launch that does not fill the GPU is bound by its longest wave, not by issue slots, and the dense form has the shorter
// wave (FAST stage of ONE 640x480 frame: 18 us dense / 21 us compacting on S_tum, 20 / 26 on S; 8 frames: 29 / 34 and 31 / 44 --
// tools/fast_mode_latency.py): below this many wave row steps per call (about 29 frames of 640x480 with 8 levels: 4 890 each) auto is dense
#define ORBFE_AUTO_MIN_ROW_STEPS 140000
#define ORBFE_AUTO_HOLD_MIN 16    // dense calls after a probe above the rate; doubles with every such probe in a row ...
#define ORBFE_AUTO_HOLD_MAX 256   // ... up to this (a probe call on corner-saturated frames costs +45 % of its FAST stage)
#define ORBFE_AUTO_PROBE_EVERY 8  // compacting calls between two looks at the pass rate

struct orbfe_handle {
    orbfe_params prm;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;      // false: the stream belongs to a pipeline (orbfe_internal_create_on_stream); no host copy streams then
    bool own_side = true;        // false: the side stream (blur) is one the pipeline shares among its pipes
    // constructor tables (src/ORBextractor.cc:404-439) and the plan-shaping options (orbfe_set_option; 0 / -1 = built-in choice;
    // changing one invalidates the plan): what the planner reads (orbfe_plan.h)
    OrbPlanIn pin;
    float sigma2[ORBFE_MAX_LEVELS], inv_sigma2[ORBFE_MAX_LEVELS];
    // plan for the current frame size
    OrbPlan plan;
    bool plan_valid = false;
    DevBuf d_plan, d_tabs, d_flanes, d_flanes_c, d_blanes, d_blanesR;
    // per-batch blocks
    DevBuf d_pyr, d_blur, d_skeys, d_scount, d_knode, d_qtbox, d_qtnodes, d_sel, d_nsel, d_nkeys, d_pad;
    // sticky overflow word + FAST sparse-variant statistics: [0] int32 overflow bits, [2..7] 3 x uint64 counters
    DevBuf d_misc;
    int fast_mode = 3;            // 0 dense, 1 sparse shortcuts, 2 lane-compacting, 3 auto (default): 2 or 0 by batch size and observed pass rate (orbfe_set_fast_mode)
    bool fast_stats = false;
    // auto mode: the lane-compacting kernel reports {row steps, batches, parked pairs} of a sample of its waves; the counters are
    // copied to pinned host memory behind the kernel and looked at -- without waiting -- by a later call
    PinBuf h_auto;                // 3 x uint64
    hipEvent_t ev_auto = nullptr;
    bool auto_pending = false;
    int auto_dense_left = 0;      // calls still to run dense before the pass rate is probed again
    int auto_hold = ORBFE_AUTO_HOLD_MIN;   // length of the next dense run
    int auto_since = 0;           // compacting calls since the last probe
    int auto_form = 2;            // the form the last probe chose (before the first answer: compacting, the probe's own form)
    uint64_t auto_last[3] = {0, 0, 0};
    int64_t fast_row_steps = 0;
    // The most recent batched call: its stream (only compared, never dereferenced: the caller may have destroyed it) and an
    // event recorded behind its last launch.  All calls of a handle share the scratch blocks, so a call on another stream
    // waits for that event first, and whoever needs the results on the host (taps, mvImagePyramid, re-planning, the
    // overflow word, destroy) synchronises the event, not the stream.
    hipStream_t last_stream = nullptr;
    bool last_stream_valid = false;
    hipEvent_t ev_last = nullptr;
    // host-API staging
    // two sets, so that the H2D of chunk i+1, the kernels of chunk i and the D2H of chunk i-1 overlap
    DevBuf d_stage[2], d_okps[2], d_odesc[2], d_on[2];
    PinBuf h_stage[2], h_okps[2], h_odesc[2], h_on[2], h_ovf;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_cmp[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    // last call (for taps / mvImagePyramid)
    const uint8_t *last_gray = nullptr;
    int64_t last_gray_fstride = 0;
    int32_t last_gray_pitch = 0;
    int32_t last_nframes = 0;
    // profiling: ring of event sets so a timed region of many asynchronous calls can be averaged afterwards
    bool profiling = false;
    hipEvent_t ev[ORBFE_PROF_RING][ORBFE_EV_N];
    int prof_calls = 0;  // calls recorded since profiling was (re-)enabled
    bool ev_ok = false;
    // blur depends on the pyramid only, the quadtree on FAST only: the blur runs on a side stream next to the
    // latency-bound quadtree (overlap 2), next to FAST + quadtree (1), or in line (0).  -1 = by batch size: 2 for
    // batches that fill the chip (>= 128 frames: 3.71 -> 3.62 ms per 1024 frames, the HBM-bound blur fills the
    // quadtree's idle VALU / memory slots; next to the VALU-bound FAST pass it gains nothing), 0 for small ones
    int overlap = -1;
    int fuse_fast_pyr = 0;   // 1 / 2: FAST(l) + resize(l -> l + 1) in one launch per level (ORBFE_FUSE_FAST_PYR; 2 = the two kinds of
                             // workgroups dealt out proportionally over the grid, 1 = resize workgroups first)
    int fuse_fast_pyr_levels = ORBFE_MAX_LEVELS;   // levels fused that way; the rest: plain resizes + one FAST launch
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr;   // the side-stream FAST of ORBFE_OPT_FUSE_FAST_PYR = 3 (developer builds)
    // tuning options that shape launches, not the plan (orbfe_set_option; 0 = built-in choice)
    OrbOpts kopts = {0, 0, {0, 0, 0}};
    // ORBFE_OPT_REUSE_IDENTICAL_INPUT (orbfe_extract only): the frame of the last single-frame host call is still in the pinned
    // staging block h_stage[0] and its results in h_okps[0]; a call that brings the same pixels gets those results back without
    // touching the GPU.  reuse_valid is dropped by every other use of the handle (run_batch) and by every option change.
    int opt_reuse = 0;
    bool reuse_valid = false, last_reused = false;
    int reuse_w = 0, reuse_h = 0, reuse_cap = 0;
    int64_t reuse_hits = 0;
};

// waits until the last batched call of the handle has finished, on whichever stream it ran
static inline hipError_t wait_last_call(orbfe_handle *h)
{
    if (!h->last_stream_valid) return hipSuccess;
    return hipEventSynchronize(h->ev_last);
}

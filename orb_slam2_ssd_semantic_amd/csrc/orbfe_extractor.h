// orbfe_extractor.h -- the extractor handle (orbfe_handle), private to the files that implement its entry points: orbfe_api.hip
// (create / destroy, options, the batched call) and orbfe_taps.hip (the pyramid read-back and the stage taps).
#pragma once

#include <stddef.h>

#include "orbfe_common.h"
#include "orbfe_fast_auto.h"
#include "orbfe_host.h"
#include "orbfe_kernels.h"
#include "orbfe_plan.h"

#define ORBFE_PROF_RING 64
// event marks of one profiled call: 0 start, 1 pyramid done, 2 FAST done, 3 quadtree done, 4 describe start, 5 end (launch
// stream); 6 / 7 around the blur (on whichever stream it ran)
#define ORBFE_EV_N 8

// The handle's block of sticky device words (d_misc), zeroed when it is made.
struct OrbMisc {
    int32_t overflow;          // byte 0: sticky overflow bits (OrbLaunch::d_ovf; orbfe_get_overflow reads and clears them)
    int32_t pad0[3];
    uint64_t fast_stat[3];     // byte 16: counters of the FAST kernel (OrbLaunch::d_fstat): orbfe_set_fast_mode's statistics, or the
                               // sample an automatic-mode probe takes
    uint64_t pad1[3];
    uint64_t qt_phase[120];    // byte 64: k_octree's per-phase clock sums, [level][8] (-DQT_PROFILE builds; orbfe_internal_read_misc)
};
static_assert(sizeof(OrbMisc) == 1024 && offsetof(OrbMisc, fast_stat) == 16 && offsetof(OrbMisc, qt_phase) == 64,
              "k_octree's QT_STAMP and tools/octree_phases.py address the block by these offsets");

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
    DevBuf d_plan, d_tabs, d_flanes, d_flanes_c, d_blanes;
    // per-batch blocks
    DevBuf d_pyr, d_blur, d_skeys, d_scount, d_knode, d_qtbox, d_qtnodes, d_sel, d_nsel, d_nkeys, d_pad;
    DevBuf d_misc;                // one OrbMisc
    int fast_mode = 3;            // 0 dense, 1 sparse shortcuts, 2 lane-compacting, 3 auto (default): 2 or 0 by batch size and observed pass rate (orbfe_set_fast_mode)
    bool fast_stats = false;
    // auto mode: the lane-compacting kernel reports {row steps, batches, parked pairs} of a sample of its waves; the counters are
    // copied to pinned host memory behind the kernel and looked at -- without waiting -- by a later call
    PinBuf h_auto;                // 3 x uint64
    hipEvent_t ev_auto = nullptr;
    bool auto_pending = false;
    OrbFastAuto fauto;            // what the probes said so far (orbfe_fast_auto.h)
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
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_fork2 = nullptr;   // FAST -> quadtree, when the stages of a call run on streams of their own
    // tuning options that shape launches, not the plan (orbfe_set_option; 0 = built-in choice)
    OrbOpts kopts = {0, {0, 0, 0}};
    // ORBFE_OPT_REUSE_IDENTICAL_INPUT (orbfe_extract only): the frame of the last single-frame host call is still in the pinned
    // staging block h_stage[0] and its results in h_okps[0]; a call that brings the same pixels gets those results back without
    // touching the GPU.  reuse_valid is dropped by every other use of the handle (run_batch) and by every option change.
    int opt_reuse = 0;
    bool reuse_valid = false, last_reused = false;
    int reuse_w = 0, reuse_h = 0, reuse_cap = 0;
    int64_t reuse_hits = 0;
};

static inline OrbMisc *misc_block(orbfe_handle *h) { return (OrbMisc *)h->d_misc.p; }   // device pointer: for addresses only

// waits until the last batched call of the handle has finished, on whichever stream it ran
static inline hipError_t wait_last_call(orbfe_handle *h)
{
    if (!h->last_stream_valid) return hipSuccess;
    return hipEventSynchronize(h->ev_last);
}

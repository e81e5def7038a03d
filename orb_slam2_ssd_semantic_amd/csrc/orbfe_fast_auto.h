// orbfe_fast_auto.h -- the automatic FAST mode (orbfe_set_fast_mode 3, the default): which form of the FAST kernel a call of the
// extractor takes, dense (0) or lane-compacting (2), and whether it samples the pass rate for the calls after it.  Pure host
// arithmetic, no HIP: orbfe_api.hip feeds it the probes it collects and the size of each call; tests/test_fast_auto.py reaches it
// through orbfe_internal_fast_auto without a GPU.
//
// A call of fewer than ORBFE_AUTO_MIN_ROW_STEPS wave row steps is dense.  Any other call is lane-compacting unless the last probe
// found more than ORBFE_AUTO_DENSE_RATE of the pixel pairs passing the necessary test -- then the next `hold` calls are dense (16,
// doubling up to 256 while the probes keep saying so), after which one compacting call probes again.  While compacting, every
// ORBFE_AUTO_PROBE_EVERY-th call probes.  A probe's answer arrives some calls later (the host runs ahead of the GPU): the calls in
// between follow the LAST answer, and nothing probes while an answer is outstanding.
#pragma once
#include <stdint.h>

// above this share of pixel pairs passing the necessary test the dense form is the cheaper one.  Measured per
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

struct OrbFastAuto {
    int dense_left = 0;              // calls still to run dense before the pass rate is probed again
    int hold = ORBFE_AUTO_HOLD_MIN;  // length of the next dense run
    int since = 0;                   // compacting calls since the last probe
    int form = 2;                    // the form the last probe chose (before the first answer: compacting, the probe's own form)
};

struct OrbFastChoice {
    int form;     // 0 dense, 2 lane-compacting
    bool probe;   // this call samples {row steps, batches, parked pairs} for a later call to look at
};

// A probe has answered: c = {row steps, batches, parked pairs} of the waves the compacting kernel sampled (128 pixel pairs a step).
inline void orb_fast_auto_answer(OrbFastAuto &s, const uint64_t c[3])
{
    if (c[0] > 0 && (double)c[2] > ORBFE_AUTO_DENSE_RATE * 128.0 * (double)c[0]) {
        s.form = 0;
        s.dense_left = s.hold;
        s.hold = 2 * s.hold < ORBFE_AUTO_HOLD_MAX ? 2 * s.hold : ORBFE_AUTO_HOLD_MAX;
    } else {
        s.form = 2;
        s.hold = ORBFE_AUTO_HOLD_MIN;
        s.since = 1;
    }
}

// true: a call of this many wave row steps is dense whatever the probes said; it takes no answer and leaves the state alone
inline bool orb_fast_auto_small(int64_t row_steps) { return row_steps < ORBFE_AUTO_MIN_ROW_STEPS; }

// The form of the next call (row_steps = frames x row steps of one frame); `pending`: a probe's answer is still outstanding.
inline OrbFastChoice orb_fast_auto_choose(OrbFastAuto &s, int64_t row_steps, bool pending)
{
    if (orb_fast_auto_small(row_steps)) return {0, false};
    if (s.form == 0) {
        if (s.dense_left > 0) {
            s.dense_left--;
            return {0, false};
        }
        // the dense run is over: one compacting call looks again -- unless a look is already under way
        if (pending) return {0, false};
        return {2, true};
    }
    return {2, !pending && (s.since++ % ORBFE_AUTO_PROBE_EVERY) == 0};
}

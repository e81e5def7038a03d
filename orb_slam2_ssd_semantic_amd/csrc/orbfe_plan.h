// orbfe_plan.h -- the extractor's launch plan, built on the host without a device (csrc/orbfe_plan.hip): the constructor
// tables, and for one frame size the level geometry, the FAST cell table, the cv::resize tap tables and the lane lists of the
// FAST, blur and pyramid kernels.  orbfe_api.hip uploads what orb_plan_build returns; tests/test_plan.py and
// tests/cpp/test_plan_sanitize.cpp reach it without a GPU.
#pragma once

#include <vector>

#include "orbfe_common.h"

// everything the plan depends on besides the frame size: the constructor tables and the plan-shaping options of a handle
struct OrbPlanIn {
    int32_t nlevels;
    float scale[ORBFE_MAX_LEVELS], inv_scale[ORBFE_MAX_LEVELS];   // src/ORBextractor.cc:404-421
    int32_t feat[ORBFE_MAX_LEVELS];                               // mnFeaturesPerLevel (:426-439)
    int32_t ini_th_fast, min_th_fast, blur_rounding, max_batch;
    // tuning options (orbfe_set_option; 0 = built-in choice)
    int32_t opt_rows, opt_rows_fast, opt_rows_blur;
    int32_t opt_blur_pieces, opt_blur_updown, opt_debug;
};

// the plan and the tables behind it, as the kernels read them
struct OrbPlanTables {
    OrbPlan plan;
    std::vector<OrbCell> cells;
    std::vector<OrbTab> tabs;
    std::vector<OrbLane> flanes, clanes, blanes;   // dense FAST, lane-compacting FAST, blur
    int64_t fast_row_steps;                        // wave row steps one frame costs k_fast_map (VALU model of bench.py's roofline)
};

// Checks `p` as orbfe_create does and fills the constructor tables (src/ORBextractor.cc:404-439) and the options' defaults.
// sigma2 / inv_sigma2 (ORBFE_MAX_LEVELS floats each) may be null.
orbfe_status orb_ctor_tables(const orbfe_params *p, OrbPlanIn *in, float *sigma2, float *inv_sigma2);
void orb_host_umax(int umax[16]);   // src/ORBextractor.cc:449-465

// The plan of a w x h frame.  Pure integer / float arithmetic on the host; on failure the error text is set and *out is
// unspecified.
orbfe_status orb_plan_build(const OrbPlanIn &in, int w, int h, OrbPlanTables *out);

// Test hook (not in include/orbfe.h): builds the plan on the host and copies out the raw bytes of table `which`: 0 OrbPlan,
// 1 cells, 2 tabs, 3 flanes, 4 clanes, 5 blanes, 6 fast_row_steps.  knobs: opt_rows, opt_rows_fast, opt_rows_blur,
// opt_blur_pieces, opt_blur_updown, opt_debug, taken raw (orbfe_set_option's range checks are not repeated).  *bytes = the table's size; dst == NULL is the sizing call.  Touches no device.
extern "C" orbfe_status orbfe_internal_plan_table(const orbfe_params *p, const int32_t knobs[6], int32_t w, int32_t h, int32_t which,
                                                  void *dst, size_t cap, size_t *bytes);

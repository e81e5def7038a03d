// Flow_orbfe.cc -- replaces the fork's perfect/src/Flow.cc.  FlowSLAM::Flow::ComputeMask on the GPU (orbfe_flow_compute_mask):
// the same mask bits as the restated OpenCV path (tests/flow_oracle.py), the previous half-size frame kept on the device.
#include "Flow.h"

#include <stdexcept>
#include <string>

#include "orbfe.h"

namespace FlowSLAM {

static void check(orbfe_status s, const char *what)
{
    if (s != ORBFE_OK) throw std::runtime_error(std::string(what) + ": " + orbfe_strerror(s) + " (" + orbfe_last_error() + ")");
}

Flow::Flow() {}

Flow::~Flow() { orbfe_flow_destroy(h_); }

void Flow::ComputeMask(const cv::Mat &GrayImg, cv::Mat &mask, float BInaryThreshold)
{
    if (GrayImg.empty()) return;   // the reference leaves mask and state alone
    int w = GrayImg.cols, h = GrayImg.rows;
    if (!h_ || w > maxw_ || h > maxh_) {
        // a larger frame: a new handle, carrying nothing over (a size change makes the reference's Farneback throw anyway)
        orbfe_flow_destroy(h_);
        h_ = nullptr;
        check(orbfe_flow_create(-1, w, h, 1, &h_), "orbfe_flow_create");
        maxw_ = w;
        maxh_ = h;
    }
    mask.create(h, w, CV_8U);
    check(orbfe_flow_compute_mask(h_, GrayImg.ptr(0), w, h, (int32_t)GrayImg.step, BInaryThreshold, mask.ptr(0), (int32_t)mask.step),
          "orbfe_flow_compute_mask");
}

void Flow::ComputeMask(const cv::Mat &GrayImg, const cv::Mat &Homo, cv::Mat &mask, float BInaryThreshold)
{
#ifdef ORBFE_WITH_OPENCV
    cv::Mat dest;
    cv::warpPerspective(GrayImg, dest, Homo, GrayImg.size());
    ComputeMask(dest, mask, BInaryThreshold);
#else
    (void)GrayImg;
    (void)Homo;
    (void)mask;
    (void)BInaryThreshold;
    throw std::runtime_error("FlowSLAM::Flow::ComputeMask(GrayImg, Homo, ...) needs cv::warpPerspective: build with ORBFE_WITH_OPENCV");
#endif
}

}  // namespace FlowSLAM

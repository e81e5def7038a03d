// Flow_orbfe.cc -- replaces the fork's perfect/src/Flow.cc.  Both FlowSLAM::Flow::ComputeMask overloads on the GPU
// (orbfe_flow_compute_mask, orbfe_flow_compute_mask_homo): the same mask bits as the restated OpenCV path (tests/flow_oracle.py,
// tests/warp_oracle.py), the previous half-size frame kept on the device.
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

// a handle that takes a w x h frame: a larger frame gets a new one, carrying nothing over (a size change makes the reference's
// Farneback throw anyway)
static void fit_handle(orbfe_flow *&f, int &maxw, int &maxh, int w, int h)
{
    if (!f || w > maxw || h > maxh) {
        orbfe_flow_destroy(f);
        f = nullptr;
        check(orbfe_flow_create(-1, w, h, 1, &f), "orbfe_flow_create");
        maxw = w;
        maxh = h;
    }
}

void Flow::ComputeMask(const cv::Mat &GrayImg, cv::Mat &mask, float BInaryThreshold)
{
    if (GrayImg.empty()) return;   // the reference leaves mask and state alone
    int w = GrayImg.cols, h = GrayImg.rows;
    fit_handle(h_, maxw_, maxh_, w, h);
    mask.create(h, w, CV_8U);
    check(orbfe_flow_compute_mask(h_, GrayImg.ptr(0), w, h, (int32_t)GrayImg.step, BInaryThreshold, mask.ptr(0), (int32_t)mask.step),
          "orbfe_flow_compute_mask");
}

void Flow::ComputeMask(const cv::Mat &GrayImg, const cv::Mat &Homo, cv::Mat &mask, float BInaryThreshold)
{
    // warpPerspective's assertions, before any device is touched: a non-empty frame, a 3x3 CV_32F / CV_64F matrix
    if (GrayImg.empty()) throw std::runtime_error("FlowSLAM::Flow::ComputeMask(GrayImg, Homo, ...): empty frame");
    if (Homo.rows != 3 || Homo.cols != 3 || (Homo.type() != CV_32F && Homo.type() != CV_64F))
        throw std::runtime_error("FlowSLAM::Flow::ComputeMask(GrayImg, Homo, ...): Homo must be a 3x3 CV_32F or CV_64F matrix");
    double H[9];   // M0.convertTo(matM, CV_64F)
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) H[r * 3 + c] = Homo.type() == CV_32F ? (double)Homo.at<float>(r, c) : Homo.at<double>(r, c);
    int w = GrayImg.cols, h = GrayImg.rows;
    fit_handle(h_, maxw_, maxh_, w, h);
    mask.create(h, w, CV_8U);
    check(orbfe_flow_compute_mask_homo(h_, GrayImg.ptr(0), w, h, (int32_t)GrayImg.step, H, BInaryThreshold, mask.ptr(0),
                                       (int32_t)mask.step),
          "orbfe_flow_compute_mask_homo");
}

}  // namespace FlowSLAM

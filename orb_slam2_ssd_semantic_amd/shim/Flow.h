// Flow.h -- drop-in replacement for the fork's perfect/include/Flow.h: namespace FlowSLAM, class Flow, the two ComputeMask
// overloads.  Both run on the GPU through the C-ABI (orbfe_flow_*, csrc/orbfe_flow.hip); the homography overload warps the
// frame there with OpenCV 3.2's warpPerspective arithmetic, in every build.
#pragma once

#ifdef ORBFE_WITH_OPENCV
#include <opencv2/opencv.hpp>
#else
#include "cv_stub/orbfe_cv_stub.h"
#endif

struct orbfe_flow;

namespace FlowSLAM {

class Flow {
public:
    Flow();
    ~Flow();
    Flow(const Flow &) = delete;
    Flow &operator=(const Flow &) = delete;

    void ComputeMask(const cv::Mat &GrayImg, cv::Mat &mask, float BInaryThreshold);
    void ComputeMask(const cv::Mat &GrayImg, const cv::Mat &Homo, cv::Mat &mask, float BInaryThreshold);

private:
    orbfe_flow *h_ = nullptr;
    int maxw_ = 0, maxh_ = 0;
};

}  // namespace FlowSLAM

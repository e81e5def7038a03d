// findHomography_orbfe.cc -- cv::findHomography for the OpenCV-free build: Tracking::TrackHomo's
// `homo = findHomography(points_current, points_last, RANSAC, 3);` (perfect/src/Tracking.cc:1331-1399) compiles unchanged
// and runs on the GPU through orbfe_find_homography (csrc/orbfe_homography.hip): the H and mask of the restated OpenCV 3.2
// path (tests/homography_oracle.py).  With ORBFE_WITH_OPENCV the real cv::findHomography is used and this file is empty.
#ifndef ORBFE_WITH_OPENCV
#include "cv_stub/orbfe_cv_stub.h"
#include "orbfe_shim.h"

namespace cv {

using orbfe_shim::check;

// one handle per thread, grown to the largest point count seen
static orbfe_homography *handle_for(int n)
{
    return orbfe_shim::handle_for<orbfe_homography, orbfe_homography_create, orbfe_homography_destroy>(n, "orbfe_homography_create");
}

Mat findHomography(const std::vector<Point2f> &srcPoints, const std::vector<Point2f> &dstPoints, int method,
                   double ransacReprojThreshold, Mat &mask, const int maxIters, const double confidence)
{
    if (srcPoints.size() != dstPoints.size()) throw std::runtime_error("cv::findHomography: point counts differ");
    int n = (int)srcPoints.size();
    Mat m(n, 1, CV_8U);
    double H[9];
    int32_t ok = 0;
    check(orbfe_find_homography(handle_for(n), n ? &srcPoints[0].x : nullptr, n ? &dstPoints[0].x : nullptr, n, method,
                                ransacReprojThreshold, maxIters, confidence, H, n ? m.ptr(0) : nullptr, &ok),
          "orbfe_find_homography");
    mask = m;
    if (!ok) return Mat();
    Mat out(3, 3, CV_64F);
    for (int i = 0; i < 9; i++) out.ptr<double>(i / 3)[i % 3] = H[i];
    return out;
}

Mat findHomography(const std::vector<Point2f> &srcPoints, const std::vector<Point2f> &dstPoints, int method,
                   double ransacReprojThreshold)
{
    Mat mask;
    return findHomography(srcPoints, dstPoints, method, ransacReprojThreshold, mask);
}

}  // namespace cv
#endif

// undistortPoints_orbfe.cc -- cv::undistortPoints for the OpenCV-free build: Frame::UndistortKeyPoints' and
// Frame::ComputeImageBounds' `cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK);` (perfect/src/Frame.cc:769, :799) run
// on the GPU through orbfe_undistort_points (csrc/orbfe_frame.hip): OpenCV 3.2's arithmetic as tests/undistort_oracle.py restates
// it.  The stub Mat has no channels, so the points are an N x 2 CV_32F matrix (the reference's reshape(2) / reshape(1) pair drops
// out).  With ORBFE_WITH_OPENCV the real cv::undistortPoints is used and this file is empty.
#ifndef ORBFE_WITH_OPENCV
#include "cv_stub/orbfe_cv_stub.h"
#include "orbfe_shim.h"

namespace cv {

using orbfe_shim::check;

// one matcher per thread (its stream and scratch carry the call)
static orbfe_matcher *matcher()
{
    static thread_local orbfe_shim::Holder<orbfe_matcher, orbfe_matcher_destroy> hold;
    if (!hold.h) check(orbfe_matcher_create(-1, &hold.h), "orbfe_matcher_create");
    return hold.h;
}

static void read3x3(const Mat &m, const char *name, float out[9])
{
    if (m.rows != 3 || m.cols != 3 || m.type() != CV_32F)
        throw std::runtime_error(std::string("cv::undistortPoints: ") + name + " must be a 3x3 CV_32F matrix");
    for (int i = 0; i < 9; i++) out[i] = m.at<float>(i / 3, i % 3);
}

void undistortPoints(InputArray src, OutputArray dst, InputArray cameraMatrix, InputArray distCoeffs, InputArray R, InputArray P)
{
    if (!src.empty() && (src.cols != 2 || src.type() != CV_32F))
        throw std::runtime_error("cv::undistortPoints: src must be an N x 2 CV_32F matrix");
    if (!R.empty()) throw std::runtime_error("cv::undistortPoints: a rectification R is not supported");
    orbfe_camera cam = {};
    read3x3(cameraMatrix, "cameraMatrix", cam.K);
    if (!P.empty()) {
        read3x3(P, "P", cam.P);
        cam.has_P = 1;
    }
    if (!distCoeffs.empty()) {
        const int nd = distCoeffs.rows * distCoeffs.cols;
        if (distCoeffs.type() != CV_32F || (distCoeffs.rows != 1 && distCoeffs.cols != 1) || nd > 12)
            throw std::runtime_error("cv::undistortPoints: distCoeffs must be a vector of 4, 5, 8 or 12 CV_32F coefficients");
        for (int i = 0; i < nd; i++) cam.dist[i] = distCoeffs.rows == 1 ? distCoeffs.at<float>(0, i) : distCoeffs.at<float>(i, 0);
        cam.ndist = nd;
    }
    const int n = src.empty() ? 0 : src.rows;
    std::vector<float> xy((size_t)n * 2);   // src may be dst: read it all first
    for (int i = 0; i < n; i++) {
        xy[2 * (size_t)i] = src.at<float>(i, 0);
        xy[2 * (size_t)i + 1] = src.at<float>(i, 1);
    }
    if (n) check(orbfe_undistort_points(matcher(), xy.data(), n, &cam, xy.data()), "orbfe_undistort_points");
    else check(orbfe_undistort_points(matcher(), nullptr, 0, &cam, nullptr), "orbfe_undistort_points");
    Mat out(n, 2, CV_32F);
    for (int i = 0; i < n; i++) {
        out.at<float>(i, 0) = xy[2 * (size_t)i];
        out.at<float>(i, 1) = xy[2 * (size_t)i + 1];
    }
    dst = out;
}

}  // namespace cv
#endif

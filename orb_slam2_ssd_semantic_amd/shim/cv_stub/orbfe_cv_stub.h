// orbfe_cv_stub.h -- the handful of OpenCV types the ORB front-end's public signatures mention, for building
// and testing the shim where OpenCV is absent (this container, the GPU box).  With real OpenCV define
// ORBFE_WITH_OPENCV and this file is never included.  Only what the shim touches is modelled.
#pragma once
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#define CV_8U 0
#define CV_8UC1 0
#define CV_32F 5
#define CV_64F 6

struct CvMat;   // the C API's matrix: include/PnPsolver.h names it in private signatures; never defined or used here

namespace cv {
struct Point2f {
    float x = 0, y = 0;
    Point2f() {}
    Point2f(float x_, float y_) : x(x_), y(y_) {}
};
struct KeyPoint {  // field order of cv::KeyPoint (28 bytes)
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};
// single-channel matrices of CV_8U (the default), CV_32F or CV_64F elements
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step = 0;
    uint8_t *data = nullptr;
    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(int r, int c, int type, void *ext, size_t stp) : rows(r), cols(c), step(stp), data((uint8_t *)ext), type_(type) {}
    void create(int r, int c, int type)
    {
        if (r == rows && c == cols && type == type_ && own_) return;
        type_ = type;
        own_.reset(new std::vector<uint8_t>((size_t)r * c * elemSize()));
        rows = r; cols = c; step = (size_t)c * elemSize(); data = own_->data();
    }
    void release() { own_.reset(); rows = cols = 0; step = 0; data = nullptr; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    int type() const { return type_; }
    size_t elemSize() const { return type_ == CV_64F ? 8 : type_ == CV_32F ? 4 : 1; }
    bool isContinuous() const { return step == (size_t)cols * elemSize(); }
    template <typename T> T &at(int r, int c) { return ((T *)(data + (size_t)r * step))[c]; }
    template <typename T> const T &at(int r, int c) const { return ((const T *)(data + (size_t)r * step))[c]; }
    template <typename T> T *ptr(int r = 0) { return (T *)(data + (size_t)r * step); }
    template <typename T> const T *ptr(int r = 0) const { return (const T *)(data + (size_t)r * step); }
    uint8_t *ptr(int r = 0) { return data + (size_t)r * step; }
    const uint8_t *ptr(int r = 0) const { return data + (size_t)r * step; }
    Mat row(int r) const { Mat m; m.rows = 1; m.cols = cols; m.step = step; m.data = data + (size_t)r * step; m.type_ = type_; m.own_ = own_; return m; }
    Mat roi(int x, int y, int w, int h) const { Mat m; m.rows = h; m.cols = w; m.step = step; m.data = data + (size_t)y * step + x * elemSize(); m.type_ = type_; m.own_ = own_; return m; }
    Mat getMat() const { return *this; }
private:
    int type_ = CV_8UC1;
    std::shared_ptr<std::vector<uint8_t>> own_;
};
typedef const Mat &InputArray;
typedef Mat &OutputArray;
// calib3d's findHomography for Point2f vectors, methods 0 and RANSAC (shim/findHomography_orbfe.cc: on the GPU): a 3x3 CV_64F
// matrix, or an empty one when there is no model; mask: n x 1 CV_8U, 1 = inlier
enum { RANSAC = 8 };
Mat findHomography(const std::vector<Point2f> &srcPoints, const std::vector<Point2f> &dstPoints, int method = 0,
                   double ransacReprojThreshold = 3);
Mat findHomography(const std::vector<Point2f> &srcPoints, const std::vector<Point2f> &dstPoints, int method,
                   double ransacReprojThreshold, Mat &mask, const int maxIters = 2000, const double confidence = 0.995);
// imgproc's undistortPoints as Frame::UndistortKeyPoints / ComputeImageBounds call it (shim/undistortPoints_orbfe.cc: on the GPU):
// src N x 2 CV_32F points, dst N x 2 CV_32F (may be src), K 3x3 CV_32F, D 4 / 5 / 8 / 12 CV_32F coefficients or empty, R empty,
// P empty (normalised coordinates) or 3x3 CV_32F
void undistortPoints(InputArray src, OutputArray dst, InputArray cameraMatrix, InputArray distCoeffs, InputArray R = Mat(),
                     InputArray P = Mat());
}  // namespace cv

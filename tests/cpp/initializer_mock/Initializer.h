// Initializer.h -- stand-in for the reference's include/Initializer.h where the reference tree is not at hand (TEST
// INFRASTRUCTURE): the class shim/Initializer_orbfe.cc implements, with the public interface Tracking::MonocularInitialization
// calls and the data members the shim keeps its state in, under the reference's names and types.  Where the reference's header is
// on the include path it is used instead and this file is not.  Frame comes from the mock header the build force-includes.
#pragma once
#include <opencv2/core/core.hpp>

#include <utility>
#include <vector>

namespace ORB_SLAM2
{
class Initializer
{
    typedef std::pair<int, int> Match;

  public:
    Initializer(const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200);
    bool Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                    std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);

  private:
    std::vector<cv::KeyPoint> mvKeys1;
    std::vector<cv::KeyPoint> mvKeys2;
    std::vector<Match> mvMatches12;
    std::vector<bool> mvbMatched1;
    cv::Mat mK;
    float mSigma, mSigma2;
    int mMaxIterations;
    std::vector<std::vector<size_t> > mvSets;
};
}  // namespace ORB_SLAM2

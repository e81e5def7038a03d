// Sim3Solver.h -- stand-in for the reference's include/Sim3Solver.h where the reference tree is not at hand (TEST
// INFRASTRUCTURE): the class shim/Sim3Solver_orbfe.cc implements, with the public interface LoopClosing calls and the data
// members the shim keeps its state in, under the reference's names and types.  Where the reference's header is on the include
// path it is used instead and this file is not.  KeyFrame / MapPoint come from the mock header the build force-includes.
#pragma once
#include <opencv2/opencv.hpp>

#include <vector>

namespace ORB_SLAM2
{
class Sim3Solver
{
  public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true);
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);
    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

  protected:
    // inputs gathered by the constructor
    KeyFrame *mpKF1, *mpKF2;
    std::vector<MapPoint *> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
    std::vector<cv::Mat> mvX3Dc1, mvX3Dc2;
    std::vector<size_t> mvnIndices1, mvSigmaSquare1, mvSigmaSquare2;
    cv::Mat mK1, mK2;
    int N, mN1;
    bool mbFixScale;
    // RANSAC parameters and state
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    int mnIterations, mnBestInliers;
    std::vector<bool> mvbBestInliers;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale;
};
}  // namespace ORB_SLAM2

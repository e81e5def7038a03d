// PnPsolver.h -- stand-in for the reference's include/PnPsolver.h where the reference tree is not at hand (TEST
// INFRASTRUCTURE): the class shim/PnPsolver_orbfe.cc implements, with the public interface Tracking::Relocalization calls and
// the data members the shim keeps its state in, under the reference's names and types.  Where the reference's header is on the
// include path it is used instead and this file is not.  Frame / MapPoint come from the mock header the build force-includes.
#pragma once
#include <opencv2/core/core.hpp>

#include <vector>

namespace ORB_SLAM2
{
class PnPsolver
{
  public:
    PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches);
    ~PnPsolver();
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991);
    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers);
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

  private:
    double uc, vc, fu, fv;
    double *pws, *us, *alphas, *pcs;
    int maximum_number_of_correspondences;
    int number_of_correspondences;
    std::vector<MapPoint *> mvpMapPointMatches;
    std::vector<cv::Point2f> mvP2D;
    std::vector<float> mvSigma2;
    std::vector<cv::Point3f> mvP3Dw;
    std::vector<size_t> mvKeyPointIndices;
    int mnInliersi;
    int mnIterations;
    std::vector<bool> mvbBestInliers;
    int mnBestInliers;
    cv::Mat mBestTcw;
    cv::Mat mRefinedTcw;
    std::vector<bool> mvbRefinedInliers;
    int mnRefinedInliers;
    int N;
    std::vector<size_t> mvAllIndices;
    double mRansacProb;
    int mRansacMinInliers;
    int mRansacMaxIts;
    float mRansacEpsilon;
    float mRansacTh;
    int mRansacMinSet;
    std::vector<float> mvMaxError;
};
}  // namespace ORB_SLAM2

// Sim3Solver_orbfe.cc -- replaces the reference's src/Sim3Solver.cc under its own include/Sim3Solver.h (found on the include
// path): the constructor gathers what the reference's gathers, iterate / find run on the GPU through orbfe_sim3_iterate
// (csrc/orbfe_sim3.hip).  The random draws are rand() used as DUtils' RandomInt(0, size - 1) =
// (int)(((double)r / 2147483648.0) * size); a call hands 3 * nIterations values over, and those of iterations it did not run
// go back to the front of a per-thread queue, so the rand() stream is consumed exactly as the reference consumes it.
// State lives in the members the reference's header declares: mnIterations, mnBestInliers, mBest*, mvbBestInliers.  The level
// sigma^2 values are kept, as float bit patterns, in mvSigmaSquare1 / 2 (declared by the header, never used by the reference):
// the library truncates 9.210 * sigma2 to size_t itself.  The ComputeSim3 / CheckInliers / Project helpers the header declares
// are not defined; nothing calls them.
#include <string.h>

#include <vector>

#include <Sim3Solver.h>

#include "orbfe_shim.h"

namespace ORB_SLAM2
{
namespace
{
using namespace orbfe_shim;

// one handle per thread, grown to the largest correspondence count seen
orbfe_sim3 *handle_for(int n) { return orbfe_shim::handle_for<orbfe_sim3, orbfe_sim3_create, orbfe_sim3_destroy>(n, "orbfe_sim3_create"); }

size_t float_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

float bits_float(size_t b)
{
    const uint32_t u = (uint32_t)b;
    float v;
    memcpy(&v, &u, 4);
    return v;
}

// Rcw * Xw + tcw as a 3x1 CV_32F: float, left to right
cv::Mat to_camera(const cv::Mat &R, const cv::Mat &t, const cv::Mat &X)
{
    cv::Mat c(3, 1, CV_32F);
    for (int k = 0; k < 3; k++)
        c.at<float>(k, 0) = ((R.at<float>(k, 0) * X.at<float>(0, 0) + R.at<float>(k, 1) * X.at<float>(1, 0)) + R.at<float>(k, 2) * X.at<float>(2, 0)) +
                            t.at<float>(k, 0);
    return c;
}

cv::Mat camera_matrix(float fx, float fy, float cx, float cy)
{
    cv::Mat K(3, 3, CV_32F);
    for (int e = 0; e < 9; e++) K.at<float>(e / 3, e % 3) = e % 4 == 0 ? 1.0f : 0.0f;
    K.at<float>(0, 0) = fx;
    K.at<float>(1, 1) = fy;
    K.at<float>(0, 2) = cx;
    K.at<float>(1, 2) = cy;
    return K;
}
}  // namespace

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale)
    : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale)
{
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    const std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    mvpMatches12 = vpMatched12;
    const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation();
    const cv::Mat Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
    for (int i1 = 0; i1 < mN1; i1++) {
        MapPoint *pMP2 = vpMatched12[i1];
        if (!pMP2) continue;
        MapPoint *pMP1 = vpKeyFrameMP1[i1];
        if (!pMP1 || pMP1->isBad() || pMP2->isBad()) continue;
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        mvSigmaSquare1.push_back(float_bits(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]));
        mvSigmaSquare2.push_back(float_bits(pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave]));
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
        mvX3Dc1.push_back(to_camera(Rcw1, tcw1, pMP1->GetWorldPos()));
        mvX3Dc2.push_back(to_camera(Rcw2, tcw2, pMP2->GetWorldPos()));
    }
    mK1 = camera_matrix(pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy);   // the entries of KeyFrame::mK
    mK2 = camera_matrix(pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy);
    mBestScale = 0;
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = (int)mvpMapPoints1.size();
    mRansacMaxIts = orbfe_sim3_ransac_iterations(probability, minInliers, maxIterations, N);
    mnIterations = 0;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    if (nIterations < 0) nIterations = 0;
    std::vector<float> X1(3 * (size_t)N), X2(3 * (size_t)N), s1(N), s2(N);
    for (int i = 0; i < N; i++) {
        for (int k = 0; k < 3; k++) {
            X1[3 * i + k] = mvX3Dc1[i].at<float>(k, 0);
            X2[3 * i + k] = mvX3Dc2[i].at<float>(k, 0);
        }
        s1[i] = bits_float(mvSigmaSquare1[i]);
        s2[i] = bits_float(mvSigmaSquare2[i]);
    }
    const float K1[4] = {mK1.at<float>(0, 0), mK1.at<float>(1, 1), mK1.at<float>(0, 2), mK1.at<float>(1, 2)};
    const float K2[4] = {mK2.at<float>(0, 0), mK2.at<float>(1, 1), mK2.at<float>(0, 2), mK2.at<float>(1, 2)};
    orbfe_sim3_state st;
    memset(&st, 0, sizeof(st));
    st.iterations = mnIterations;
    st.best_inliers = mnBestInliers;
    if (!mBestT12.empty()) {
        for (int e = 0; e < 16; e++) st.best.T12[e] = mBestT12.at<float>(e / 4, e % 4);
        for (int e = 0; e < 9; e++) st.best.R[e] = mBestRotation.at<float>(e / 3, e % 3);
        for (int e = 0; e < 3; e++) st.best.t[e] = mBestTranslation.at<float>(e, 0);
        st.best.s = mBestScale;
    }
    std::vector<uint8_t> best(N, 0), mask(N, 0);
    for (size_t i = 0; i < mvbBestInliers.size() && i < (size_t)N; i++) best[i] = mvbBestInliers[i];
    const std::vector<int32_t> draws = take_draws(3 * (size_t)nIterations);
    orbfe_sim3_result res;
    const orbfe_status status = orbfe_sim3_iterate(handle_for(N), X1.data(), X2.data(), s1.data(), s2.data(), N, K1, K2, mbFixScale, mRansacMinInliers,
                                                   mRansacMaxIts, nIterations, draws.data(), &st, best.data(), &res, mask.data());
    give_back(draws, status == ORBFE_OK ? 3 * (size_t)res.iterations_run : 0);
    check(status, "orbfe_sim3_iterate");
    mnIterations = st.iterations;
    if (res.iterations_run > 0) {   // every iteration that reached the best replaced it; the state says with what
        mnBestInliers = st.best_inliers;
        mBestT12 = cv::Mat(4, 4, CV_32F);
        mBestRotation = cv::Mat(3, 3, CV_32F);
        mBestTranslation = cv::Mat(3, 1, CV_32F);
        for (int e = 0; e < 16; e++) mBestT12.at<float>(e / 4, e % 4) = st.best.T12[e];
        for (int e = 0; e < 9; e++) mBestRotation.at<float>(e / 3, e % 3) = st.best.R[e];
        for (int e = 0; e < 3; e++) mBestTranslation.at<float>(e, 0) = st.best.t[e];
        mBestScale = st.best.s;
        mvbBestInliers.assign(best.begin(), best.end());
    }
    bNoMore = res.no_more != 0;
    if (!res.found) return cv::Mat();
    nInliers = res.n_inliers;
    for (int i = 0; i < N; i++)
        if (mask[i]) vbInliers[mvnIndices1[i]] = true;
    return mBestT12;
}

cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() { return mBestRotation.clone(); }

cv::Mat Sim3Solver::GetEstimatedTranslation() { return mBestTranslation.clone(); }

float Sim3Solver::GetEstimatedScale() { return mBestScale; }

}  // namespace ORB_SLAM2

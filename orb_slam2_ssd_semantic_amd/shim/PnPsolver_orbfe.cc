// PnPsolver_orbfe.cc -- replaces the reference's src/PnPsolver.cc under its own include/PnPsolver.h (found on the include path):
// the constructor gathers what the reference's gathers, iterate / find run on the GPU through orbfe_pnp_iterate
// (csrc/orbfe_pnp.hip).  The random draws are rand() used as DUtils' RandomInt(0, size - 1) =
// (int)(((double)r / 2147483648.0) * size); a call hands over four values for every iteration it can run (the reference's loop
// goes on while mnIterations < mRansacMaxIts OR the call's own count < nIterations), and those of iterations it did not run go
// back to the front of a per-thread queue, so the rand() stream is consumed exactly as the reference consumes it.  State lives
// in the members the reference's header declares: mnIterations, mnBestInliers, mBestTcw, mvbBestInliers, the mRansac* values
// (th2 in mRansacTh).  The EPnP helpers the header declares are not defined; nothing calls them.
#include <string.h>

#include <vector>

struct CvMat;   // named by the header's private signatures only

#include <PnPsolver.h>

#include "orbfe_shim.h"

namespace ORB_SLAM2
{
namespace
{
using namespace orbfe_shim;

// one handle per thread, grown to the largest correspondence count seen
orbfe_pnp *handle_for(int n) { return orbfe_shim::handle_for<orbfe_pnp, orbfe_pnp_create, orbfe_pnp_destroy>(n, "orbfe_pnp_create"); }

cv::Mat mat4(const float *T)
{
    cv::Mat m(4, 4, CV_32F);
    for (int e = 0; e < 16; e++) m.at<float>(e / 4, e % 4) = T[e];
    return m;
}
}  // namespace

PnPsolver::PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches)
    : pws(0), us(0), alphas(0), pcs(0), maximum_number_of_correspondences(0), number_of_correspondences(0), mnInliersi(0), mnIterations(0),
      mnBestInliers(0), N(0)
{
    mvpMapPointMatches = vpMapPointMatches;
    int idx = 0;
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        const cv::KeyPoint &kp = F.mvKeysUn[i];
        mvP2D.push_back(kp.pt);
        mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
        const cv::Mat Pos = pMP->GetWorldPos();
        mvP3Dw.push_back(cv::Point3f(Pos.at<float>(0), Pos.at<float>(1), Pos.at<float>(2)));
        mvKeyPointIndices.push_back(i);
        mvAllIndices.push_back(idx);
        idx++;
    }
    fu = F.fx;
    fv = F.fy;
    uc = F.cx;
    vc = F.cy;
    SetRansacParameters();
}

PnPsolver::~PnPsolver() {}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    mRansacProb = probability;
    mRansacMinSet = minSet;
    mRansacTh = th2;
    N = (int)mvP2D.size();
    orbfe_pnp_params p;
    check(orbfe_pnp_ransac_params(probability, minInliers, maxIterations, minSet, epsilon, N, &p), "orbfe_pnp_ransac_params");
    mRansacMinInliers = p.min_inliers;
    mRansacMaxIts = p.max_its;
    mRansacEpsilon = p.epsilon;
    mvMaxError.resize(mvSigma2.size());
    for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
}

cv::Mat PnPsolver::find(std::vector<bool> &vbInliers, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    if (nIterations < 0) nIterations = 0;
    std::vector<float> P3(3 * (size_t)N), P2(2 * (size_t)N);
    for (int i = 0; i < N; i++) {
        P3[3 * i] = mvP3Dw[i].x;
        P3[3 * i + 1] = mvP3Dw[i].y;
        P3[3 * i + 2] = mvP3Dw[i].z;
        P2[2 * i] = mvP2D[i].x;
        P2[2 * i + 1] = mvP2D[i].y;
    }
    const float K[4] = {(float)fu, (float)fv, (float)uc, (float)vc};   // they were floats (Frame::fx ...)
    orbfe_pnp_params prm;
    prm.min_inliers = mRansacMinInliers;
    prm.max_its = mRansacMaxIts;
    prm.epsilon = mRansacEpsilon;
    prm.th2 = mRansacTh;
    orbfe_pnp_state st;
    memset(&st, 0, sizeof(st));
    st.iterations = mnIterations;
    st.best_inliers = mnBestInliers;
    if (!mBestTcw.empty())
        for (int e = 0; e < 16; e++) st.best_Tcw[e] = mBestTcw.at<float>(e / 4, e % 4);
    std::vector<uint8_t> best(N, 0), mask(N, 0);
    for (size_t i = 0; i < mvbBestInliers.size() && i < (size_t)N; i++) best[i] = mvbBestInliers[i];
    const std::vector<int32_t> draws = take_draws(4 * (size_t)orbfe_pnp_iterations(&st, &prm, nIterations));
    orbfe_pnp_result res;
    memset(&res, 0, sizeof(res));
    const orbfe_status status = orbfe_pnp_iterate(handle_for(N), P3.data(), P2.data(), mvSigma2.data(), N, K, &prm, nIterations, draws.data(), &st,
                                                  best.data(), &res, mask.data());
    give_back(draws, status == ORBFE_OK ? 4 * (size_t)res.iterations_run : 0);
    check(status, "orbfe_pnp_iterate");
    mnIterations = st.iterations;
    if (st.best_inliers > mnBestInliers) {
        mnBestInliers = st.best_inliers;
        mBestTcw = mat4(st.best_Tcw);
        mvbBestInliers.assign(best.begin(), best.end());
    }
    bNoMore = res.no_more != 0;
    if (!res.found) return cv::Mat();
    nInliers = res.n_inliers;
    vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
    for (int i = 0; i < N; i++)
        if (mask[i]) vbInliers[mvKeyPointIndices[i]] = true;
    if (res.refined) {
        mnRefinedInliers = res.n_inliers;
        mvbRefinedInliers.assign(mask.begin(), mask.end());
        mRefinedTcw = mat4(res.Tcw);
        return mRefinedTcw.clone();
    }
    return mBestTcw.clone();
}

}  // namespace ORB_SLAM2

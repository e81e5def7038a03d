// Initializer_orbfe.cc -- replaces the reference's src/Initializer.cc under its own include/Initializer.h (found on the include
// path): the constructor keeps what the reference's keeps, Initialize runs on the GPU through orbfe_initializer_initialize
// (csrc/orbfe_initializer.hip): the H / F RANSAC, the model choice, ReconstructH / ReconstructF with CheckRT
// and Triangulate in one call.  The random draws are rand() used as DUtils' RandomInt(0, size - 1) = (int)(((double)r /
// 2147483648.0) * size).  DUtils::Random::SeedRandOnce(0) is srand(0), once per process, at the first Initialize; every call
// then takes mMaxIterations * 8 values, so the rand() stream is consumed exactly as the reference consumes it.  The GPU
// runtime's start-up (device initialisation, the first launch of each kernel) has been seen to reseed the process's rand(), so
// the first Initialize runs one tiny call through the handle BEFORE it seeds: everything the runtime does once is then behind.
// mvSets is not filled (the sets are replayed on the device); the private helpers the header declares are not defined; nothing
// calls them.
#include <stdlib.h>

#include <mutex>
#include <vector>

#include <Initializer.h>

#include "orbfe_shim.h"

namespace ORB_SLAM2
{
namespace
{
using namespace orbfe_shim;

// one handle per thread, grown to the largest key count seen
orbfe_initializer *handle_for(int n)
{
    return orbfe_shim::handle_for<orbfe_initializer, orbfe_initializer_create, orbfe_initializer_destroy>(n, "orbfe_initializer_create");
}

std::once_flag seeded;

// eight matches, one iteration: initialises the device and loads every kernel a call uses; the answer is not looked at
void warm_up(orbfe_initializer *h)
{
    float k1[16], k2[16];
    int32_t m[8], draws[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 8; i++) {
        k1[2 * i] = 40.0f * i + 7.0f * (i % 3);
        k1[2 * i + 1] = 25.0f * (i % 4) + 3.0f * i;
        k2[2 * i] = k1[2 * i] + 2.0f + 0.5f * (i % 2);
        k2[2 * i + 1] = k1[2 * i + 1] + 1.0f;
        m[i] = i;
    }
    const float K[9] = {500.0f, 0.0f, 320.0f, 0.0f, 500.0f, 240.0f, 0.0f, 0.0f, 1.0f};
    orbfe_initializer_result res;
    float P3D[24];
    uint8_t tri[8];
    check(orbfe_initializer_initialize(h, k1, 8, k2, 8, m, K, 1.0f, 1, draws, &res, P3D, tri), "orbfe_initializer_initialize (warm-up)");
}
}  // namespace

Initializer::Initializer(const Frame &ReferenceFrame, float sigma, int iterations)
{
    mK = ReferenceFrame.mK.clone();
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
}

bool Initializer::Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                             std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated)
{
    mvKeys2 = CurrentFrame.mvKeysUn;
    const int n1 = (int)mvKeys1.size(), n2 = (int)mvKeys2.size();
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    std::vector<int32_t> matches(n1 > 0 ? n1 : 1, -1);
    for (size_t i = 0, iend = vMatches12.size(); i < iend && i < (size_t)n1; i++) {
        if (vMatches12[i] >= 0) {
            mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
            mvbMatched1[i] = true;
            matches[i] = vMatches12[i];
        } else
            mvbMatched1[i] = false;
    }
    std::vector<float> k1(2 * (size_t)(n1 > 0 ? n1 : 1)), k2(2 * (size_t)(n2 > 0 ? n2 : 1));
    for (int i = 0; i < n1; i++) {
        k1[2 * i] = mvKeys1[i].pt.x;
        k1[2 * i + 1] = mvKeys1[i].pt.y;
    }
    for (int i = 0; i < n2; i++) {
        k2[2 * i] = mvKeys2[i].pt.x;
        k2[2 * i + 1] = mvKeys2[i].pt.y;
    }
    float K[9];
    for (int e = 0; e < 9; e++) K[e] = mK.at<float>(e / 3, e % 3);
    orbfe_initializer *h = handle_for(n1 > 0 ? n1 : 1);
    std::call_once(seeded, [h] {
        warm_up(h);
        srand(0);   // DUtils::Random::SeedRandOnce(0)
    });
    const std::vector<int32_t> draws = take_draws(8 * (size_t)(mMaxIterations > 0 ? mMaxIterations : 0));
    orbfe_initializer_result res;
    std::vector<float> P3D(3 * (size_t)(n1 > 0 ? n1 : 1));
    std::vector<uint8_t> tri(n1 > 0 ? n1 : 1);
    check(orbfe_initializer_initialize(h, k1.data(), n1, k2.data(), n2, matches.data(), K, mSigma, mMaxIterations,
                                       draws.data(), &res, P3D.data(), tri.data()),
          "orbfe_initializer_initialize");
    if (!res.ok) {
        if (res.model == 2) {   // ReconstructF empties them before it decides; ReconstructH leaves them
            R21 = cv::Mat();
            t21 = cv::Mat();
        }
        return false;
    }
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int e = 0; e < 9; e++) R21.at<float>(e / 3, e % 3) = res.R21[e];
    for (int e = 0; e < 3; e++) t21.at<float>(e, 0) = res.t21[e];
    vP3D.resize(n1);
    vbTriangulated = std::vector<bool>(n1, false);
    for (int i = 0; i < n1; i++) {
        vP3D[i] = cv::Point3f(P3D[3 * i], P3D[3 * i + 1], P3D[3 * i + 2]);
        vbTriangulated[i] = tri[i] != 0;
    }
    return true;
}

}  // namespace ORB_SLAM2

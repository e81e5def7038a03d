// test_sim3_solver.cpp -- LoopClosing::ComputeSim3's use of Sim3Solver (src/LoopClosing.cc: SetRansacParameters(0.99, 20, 300),
// then iterate(5, ...) round-robin over the candidates' solvers, then the getters) on mock keyframes, through
// shim/Sim3Solver_orbfe.cc.  Built with the mock KeyFrame / MapPoint of oracle/refbuild/ref_mocks.h force-included.
// Input file (int32 / float32): nsolvers, seed, max_rounds; per solver: mN1, nkeys2, fix_scale, K1[4], K2[4], Rcw1[9], tcw1[3],
// Rcw2[9], tcw2[3], sigma2[8], octave1[mN1], octave2[nkeys2], then per keypoint of keyframe 1: has1, Xw1[3], bad1, index1, has2,
// Xw2[3], bad2, index2.  Output file: per iterate call in order: solver, empty, bNoMore, nInliers (int32), T12[16], R[9], t[3],
// s (float32; zeros where empty), then the mN1 bytes of vbInliers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include <Sim3Solver.h>

using namespace ORB_SLAM2;

static FILE *in;
static int32_t geti()
{
    int32_t v = 0;
    if (fread(&v, 4, 1, in) != 1) exit(2);
    return v;
}
static float getf()
{
    float v = 0;
    if (fread(&v, 4, 1, in) != 1) exit(2);
    return v;
}
static cv::Mat getmat(int r, int c)
{
    cv::Mat m(r, c, CV_32F);
    for (int i = 0; i < r; i++)
        for (int j = 0; j < c; j++) m.at<float>(i, j) = getf();
    return m;
}

struct Candidate {
    KeyFrame kf1, kf2;
    std::vector<std::unique_ptr<MapPoint>> points;
    std::vector<MapPoint *> matched;
    std::unique_ptr<Sim3Solver> solver;
    bool discarded = false, done = false;
};

static MapPoint *make_point(Candidate &c, KeyFrame *kf, const cv::Mat &pos, int bad, int index)
{
    c.points.emplace_back(new MapPoint());
    MapPoint *p = c.points.back().get();
    p->world_pos = pos;
    p->mbBad = bad != 0;
    if (index >= 0) p->AddObservation(kf, (size_t)index);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return 2;
    const int nsolvers = geti(), seed = geti(), max_rounds = geti();
    std::vector<std::unique_ptr<Candidate>> cands;
    for (int s = 0; s < nsolvers; s++) {
        cands.emplace_back(new Candidate());
        Candidate &c = *cands.back();
        const int mN1 = geti(), nkeys2 = geti(), fix_scale = geti();
        KeyFrame *kfs[2] = {&c.kf1, &c.kf2};
        for (KeyFrame *kf : kfs) {
            kf->fx = getf();
            kf->fy = getf();
            kf->cx = getf();
            kf->cy = getf();
        }
        for (KeyFrame *kf : kfs) {
            kf->Rcw = getmat(3, 3);
            kf->tcw = getmat(3, 1);
        }
        std::vector<float> sigma2(8);
        for (float &v : sigma2) v = getf();
        c.kf1.mvLevelSigma2 = c.kf2.mvLevelSigma2 = sigma2;
        c.kf1.mvKeysUn.resize(mN1);
        c.kf2.mvKeysUn.resize(nkeys2);
        for (int i = 0; i < mN1; i++) c.kf1.mvKeysUn[i].octave = geti();
        for (int i = 0; i < nkeys2; i++) c.kf2.mvKeysUn[i].octave = geti();
        c.kf1.mvpMapPoints.assign(mN1, nullptr);
        c.matched.assign(mN1, nullptr);
        for (int i = 0; i < mN1; i++) {
            const int has1 = geti();
            const cv::Mat x1 = getmat(3, 1);
            const int bad1 = geti(), index1 = geti(), has2 = geti();
            const cv::Mat x2 = getmat(3, 1);
            const int bad2 = geti(), index2 = geti();
            if (has1) c.kf1.mvpMapPoints[i] = make_point(c, &c.kf1, x1, bad1, index1);
            if (has2) c.matched[i] = make_point(c, &c.kf2, x2, bad2, index2);
        }
        c.solver.reset(new Sim3Solver(&c.kf1, &c.kf2, c.matched, fix_scale != 0));
        c.solver->SetRansacParameters(0.99, 20, 300);
    }
    fclose(in);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    srand((unsigned)seed);
    int calls = 0;
    for (int round = 0; round < max_rounds; round++) {
        bool any = false;
        for (int s = 0; s < nsolvers; s++) {
            Candidate &c = *cands[s];
            if (c.discarded || c.done) continue;
            any = true;
            int nInliers;
            bool bNoMore;
            std::vector<bool> vbInliers;
            Sim3Solver *pSolver = c.solver.get();
            cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
            if (bNoMore) c.discarded = true;
            int32_t head[4] = {s, Scm.empty() ? 1 : 0, bNoMore ? 1 : 0, nInliers};
            float model[29] = {0};
            if (!Scm.empty()) {
                c.done = true;
                const cv::Mat R = pSolver->GetEstimatedRotation();
                const cv::Mat t = pSolver->GetEstimatedTranslation();
                const float sc = pSolver->GetEstimatedScale();
                for (int e = 0; e < 16; e++) model[e] = Scm.at<float>(e / 4, e % 4);
                for (int e = 0; e < 9; e++) model[16 + e] = R.at<float>(e / 3, e % 3);
                for (int e = 0; e < 3; e++) model[25 + e] = t.at<float>(e, 0);
                model[28] = sc;
            }
            fwrite(head, 4, 4, o);
            fwrite(model, 4, 29, o);
            for (size_t i = 0; i < vbInliers.size(); i++) fputc(vbInliers[i] ? 1 : 0, o);
            calls++;
        }
        if (!any) break;
    }
    fclose(o);
    printf("solvers %d calls %d\n", nsolvers, calls);
    return 0;
}

// test_pnp_solver.cpp -- Tracking::Relocalization's use of PnPsolver (perfect/src/Tracking.cc: SetRansacParameters(0.99, 10, 300,
// 4, 0.5, 5.991), then iterate(5, ...) round-robin over the candidates' solvers) on a mock frame, through
// shim/PnPsolver_orbfe.cc.  Built with the mock Frame / MapPoint of oracle/refbuild/ref_mocks.h force-included.
// Input file (int32 / float32): nsolvers, seed, max_rounds; per solver: nkeys, K[4], sigma2[8], then per keypoint: octave, x, y,
// has, Xw[3], bad.  Output file: per iterate call in order: solver, empty, bNoMore, nInliers, size of vbInliers (int32),
// Tcw[16] (float32; zeros where empty), then the bytes of vbInliers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include <PnPsolver.h>

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

struct Candidate {
    Frame frame;
    std::vector<std::unique_ptr<MapPoint>> points;
    std::vector<MapPoint *> matches;
    std::unique_ptr<PnPsolver> solver;
    bool discarded = false, done = false;
};

int main(int argc, char **argv)
{
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return 2;
    const int nsolvers = geti(), seed = geti(), max_rounds = geti();
    std::vector<std::unique_ptr<Candidate>> cands;
    for (int s = 0; s < nsolvers; s++) {
        cands.emplace_back(new Candidate());
        Candidate &c = *cands.back();
        const int nkeys = geti();
        c.frame.fx = getf();
        c.frame.fy = getf();
        c.frame.cx = getf();
        c.frame.cy = getf();
        c.frame.mvLevelSigma2.resize(8);
        for (float &v : c.frame.mvLevelSigma2) v = getf();
        c.frame.mvKeysUn.resize(nkeys);
        c.frame.mvpMapPoints.assign(nkeys, nullptr);
        c.matches.assign(nkeys, nullptr);
        for (int i = 0; i < nkeys; i++) {
            c.frame.mvKeysUn[i].octave = geti();
            c.frame.mvKeysUn[i].pt.x = getf();
            c.frame.mvKeysUn[i].pt.y = getf();
            const int has = geti();
            cv::Mat pos(3, 1, CV_32F);
            for (int k = 0; k < 3; k++) pos.at<float>(k, 0) = getf();
            const int bad = geti();
            if (has) {
                c.points.emplace_back(new MapPoint());
                c.points.back()->world_pos = pos;
                c.points.back()->mbBad = bad != 0;
                c.matches[i] = c.points.back().get();
            }
        }
        c.solver.reset(new PnPsolver(c.frame, c.matches));
        c.solver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
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
            std::vector<bool> vbInliers;
            int nInliers;
            bool bNoMore;
            PnPsolver *pSolver = c.solver.get();
            cv::Mat Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
            if (bNoMore) c.discarded = true;
            int32_t head[5] = {s, Tcw.empty() ? 1 : 0, bNoMore ? 1 : 0, nInliers, (int32_t)vbInliers.size()};
            float model[16] = {0};
            if (!Tcw.empty()) {
                c.done = true;
                for (int e = 0; e < 16; e++) model[e] = Tcw.at<float>(e / 4, e % 4);
            }
            fwrite(head, 4, 5, o);
            fwrite(model, 4, 16, o);
            for (size_t i = 0; i < vbInliers.size(); i++) fputc(vbInliers[i] ? 1 : 0, o);
            calls++;
        }
        if (!any) break;
    }
    fclose(o);
    printf("solvers %d calls %d\n", nsolvers, calls);
    return 0;
}

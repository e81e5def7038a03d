// test_initializer.cpp -- Tracking::MonocularInitialization's use of Initializer (construct on the reference frame with sigma 1.0
// and 200 iterations, Initialize on each following frame until one succeeds) on mock frames, through shim/Initializer_orbfe.cc.
// Built with the mock Frame of oracle/refbuild/ref_mocks.h force-included.
// Input file (int32 / float32): K[9], nframes; per frame: nkeys, then x, y per key; per frame after the first: the vMatches12
// against it (int32 per key of the first frame).  Output file: per Initialize call in order: ok, empty(R21), size of vP3D (int32),
// R21[9], t21[3] (float32; zeros where empty), then vP3D (float32 x 3 each) and the bytes of vbTriangulated.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include <Initializer.h>

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

int main(int argc, char **argv)
{
    if (argc != 3 || !(in = fopen(argv[1], "rb"))) return 2;
    cv::Mat K(3, 3, CV_32F);
    for (int e = 0; e < 9; e++) K.at<float>(e / 3, e % 3) = getf();
    const int nframes = geti();
    std::vector<std::unique_ptr<Frame>> frames;
    for (int f = 0; f < nframes; f++) {
        frames.emplace_back(new Frame());
        Frame &F = *frames.back();
        F.mK = K.clone();
        F.mvKeysUn.resize(geti());
        for (cv::KeyPoint &kp : F.mvKeysUn) {
            kp.pt.x = getf();
            kp.pt.y = getf();
        }
    }
    std::vector<std::vector<int>> matches(nframes);
    for (int f = 1; f < nframes; f++) {
        matches[f].resize(frames[0]->mvKeysUn.size());
        for (int &m : matches[f]) m = geti();
    }
    fclose(in);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    srand(12345);   // whatever the program did before: the first Initialize seeds with 0, once
    Initializer *mpInitializer = new Initializer(*frames[0], 1.0, 200);
    int calls = 0;
    for (int f = 1; f < nframes; f++) {
        cv::Mat Rcw, tcw;
        std::vector<bool> vbTriangulated;
        std::vector<cv::Point3f> mvIniP3D;
        const bool ok = mpInitializer->Initialize(*frames[f], matches[f], Rcw, tcw, mvIniP3D, vbTriangulated);
        int32_t head[3] = {ok ? 1 : 0, Rcw.empty() ? 1 : 0, (int32_t)mvIniP3D.size()};
        float model[12] = {0};
        if (!Rcw.empty()) {
            for (int e = 0; e < 9; e++) model[e] = Rcw.at<float>(e / 3, e % 3);
            for (int e = 0; e < 3; e++) model[9 + e] = tcw.at<float>(e, 0);
        }
        fwrite(head, 4, 3, o);
        fwrite(model, 4, 12, o);
        for (const cv::Point3f &p : mvIniP3D) {
            const float xyz[3] = {p.x, p.y, p.z};
            fwrite(xyz, 4, 3, o);
        }
        for (size_t i = 0; i < vbTriangulated.size(); i++) fputc(vbTriangulated[i] ? 1 : 0, o);
        calls++;
    }
    delete mpInitializer;
    fclose(o);
    printf("frames %d calls %d\n", nframes, calls);
    return 0;
}

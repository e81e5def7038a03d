// test_undistort_points.cpp -- Frame::UndistortKeyPoints' undistortPoints line (perfect/src/Frame.cc:769), against the OpenCV-free
// stub and shim/undistortPoints_orbfe.cc.  The stub Mat has no channels: the points stay N x 2 (the reference's reshape(2) /
// reshape(1) around the call drop out).  Input file: float32 K[9], int32 ndist, float32 dist[ndist], int32 n, n (x, y) float32.
// Output file: n (x, y) float32 of mvKeysUn's positions.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "cv_stub/orbfe_cv_stub.h"

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    float K[9];
    int32_t nd = 0, N = 0;
    if (fread(K, 4, 9, f) != 9 || fread(&nd, 4, 1, f) != 1 || nd < 0 || nd > 12) return 2;
    cv::Mat mK(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) mK.at<float>(i / 3, i % 3) = K[i];
    cv::Mat mDistCoef(nd, 1, CV_32F);
    for (int i = 0; i < nd; i++)
        if (fread(&mDistCoef.at<float>(i, 0), 4, 1, f) != 1) return 2;
    if (fread(&N, 4, 1, f) != 1 || N < 1) return 2;
    std::vector<float> xy((size_t)N * 2);
    if (fread(xy.data(), 8, N, f) != (size_t)N) return 2;
    fclose(f);

    cv::Mat mat(N,2,CV_32F);
    for(int i=0; i<N; i++)
    {
        mat.at<float>(i,0)=xy[2*i];
        mat.at<float>(i,1)=xy[2*i+1];
    }
    cv::undistortPoints(mat,mat,mK,mDistCoef,cv::Mat(),mK);

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int i = 0; i < N; i++) fwrite(&mat.at<float>(i, 0), 4, 2, o);
    fclose(o);
    printf("n %d\n", N);
    return 0;
}

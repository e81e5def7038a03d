// test_find_homography.cpp -- Tracking::TrackHomo's findHomography line (perfect/src/Tracking.cc:1331-1399), verbatim, against
// the OpenCV-free stub and shim/findHomography_orbfe.cc.  Input file: int32 n, then n (x, y) float32 of points_current and n of
// points_last.  Output file: int32 empty flag, 9 float64 of H (zeros when empty), then the n mask bytes of the RANSAC call
// with an explicit mask.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "cv_stub/orbfe_cv_stub.h"

using namespace cv;

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<cv::Point2f> points_current(n), points_last(n);
    if (n && (fread(&points_current[0], 8, n, f) != (size_t)n || fread(&points_last[0], 8, n, f) != (size_t)n)) return 2;
    fclose(f);

    cv::Mat homo;
    homo = findHomography(points_current, points_last, RANSAC, 3);

    cv::Mat mask;
    cv::Mat homo2 = findHomography(points_current, points_last, RANSAC, 3, mask, 2000, 0.995);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    int32_t empty = homo.empty() ? 1 : 0;
    double H[9] = {0};
    if (!empty)
        for (int i = 0; i < 9; i++) H[i] = homo.at<double>(i / 3, i % 3);
    fwrite(&empty, 4, 1, o);
    fwrite(H, 8, 9, o);
    if (n) fwrite(mask.ptr(0), 1, n, o);
    fclose(o);
    printf("n %d empty %d same %d\n", n, empty, (int)(homo2.empty() == homo.empty()));
    return 0;
}

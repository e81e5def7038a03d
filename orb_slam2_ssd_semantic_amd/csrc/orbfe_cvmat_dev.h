// orbfe_cvmat_dev.h -- the two OpenCV 3.2 cv::Mat evaluation rules more than one module restates, host and device alike: what
// cv::gemm's small-matrix shortcut stores and Mat::inv() of a 3x3.  For orbfe_geometry_dev.h (DynaSLAM's Geometry) and
// orbfe_f12.h (LocalMapping::ComputeF12); neither belongs to the other.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define GEO_HD __host__ __device__ inline

// what cv::gemm's float shortcut stores for a float sum t: (float)(t * alpha + c * beta) with alpha = 1, c = 0, beta = 0
// (modules/core/src/matmul.cpp, the 2 <= len <= 4 block of cv::gemm)
GEO_HD float geo_gemm_store(float t) { return (float)((double)t * 1.0 + (double)0.0f * 0.0); }

// Mat::inv() of a 3x3 CV_32F (cv::invert's 3x3 case, modules/core/src/lapack.cpp): determinant and cofactors in double
GEO_HD void geo_inv3(const float *S, float *D)
{
    double d = (double)S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - (double)S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) +
               (double)S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
    if (d != 0.) {
        d = 1. / d;
        D[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
        D[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
        D[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
        D[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
        D[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
        D[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
        D[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
        D[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
        D[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
    } else
        for (int k = 0; k < 9; k++) D[k] = 0.0f;
}

// orbfe_newpoints.h -- the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:446-611) for ONE match, and the
// depth KeyFrame::ComputeSceneMedianDepth takes per MapPoint (src/KeyFrame.cc), as __host__ __device__ functions, so that
// k_np_triangulate (orbfe_newpoints.hip) and the host orbfe_triangulate_match run the same code.  cv::Mat expressions are
// restated as OpenCV 3.2 evaluates them; tests/newpoints_oracle.py restates every step under the rule numbers N1 .. N14 given
// there.  No compiled reference pins either file (LocalMapping.cc is not among the compiled reference sources).  The library is
// built with -ffp-contract=off: one operation at a time.
#pragma once

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "orbfe_track_geom.h"   // trk_div, trk_unproject, TrkCam
#include "orbfe_cvmat_dev.h"    // geo_gemm_store
#include "orbfe_svd.h"          // triangulate, jacobi_svd_f
#include "orbfe_ctrig.h"        // c_atan2, c_cos

// one keypoint of a match is include/orbfe.h's orbfe_newpt_key
typedef orbfe_newpt_key NpKey;

// N3: Rwc * xn with Rwc = Rcw.t() evaluated, a 3x3 . 3x1 product through gemm's float shortcut
ORBFE_HD inline void np_ray(const float *T, float x, float y, float *ray)
{
    for (int i = 0; i < 3; i++) ray[i] = geo_gemm_store(T[i] * x + T[4 + i] * y + T[8 + i] * 1.0f);
}

// N4: Mat::dot, a double sum of (double)a * b from zero, left to right
ORBFE_HD inline double np_dot3(const float *a, const float *b)
{
    double s = 0.;
    for (int k = 0; k < 3; k++) s += (double)a[k] * (double)b[k];
    return s;
}

// N6: Rcw.row(r).dot(x3Dt) + tcw(r) stored to float: the double dot plus the float promoted
ORBFE_HD inline float np_cam_coord(const float *T, int r, const float *x) { return (float)(np_dot3(T + 4 * r, x) + (double)T[4 * r + 3]); }

// N7: cos(2 * atan2(mb / 2, depth)) on floats, by the project's canonical trig
ORBFE_HD inline float np_cos_parallax_stereo(float mb, float depth)
{
    const float a = (float)c_atan2((double)(mb / 2), (double)depth);
    return (float)c_cos((double)(2 * a));
}

// N10, N11: the reprojection error gate of one keyframe; true = `continue`
ORBFE_HD inline bool np_error_gate(const orbfe_track_camera &cam, float x, float y, float z, const NpKey &k, bool stereo, float sigma2)
{
    const float invz = (float)(1.0 / (double)z);
    const float u = cam.fx * x * invz + cam.cx;
    const float v = cam.fy * y * invz + cam.cy;
    const float ex = u - k.ux, ey = v - k.uy;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float ur = u - cam.bf * invz;   // keyframe 1's mbf for both keyframes (sic): one bf serves both
    const float er = ur - k.uright;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// N12: cv::norm(x3D - Ow) stored as float
ORBFE_HD inline float np_dist(const float *x, const float *Ow)
{
    const float n[3] = {x[0] - Ow[0], x[1] - Ow[1], x[2] - Ow[2]};
    return (float)sqrt(np_dot3(n, n));
}

// The loop body for the match (k1, k2) of keyframes (T1, O1), (T2, O2): Tcw row-major 3x4, Ow the camera centres.  At / W / Vt:
// 16 floats, 4 doubles, 16 floats of workspace, anything indexable (csrc/orbfe_svd.h).  Returns ORBFE_NEWPT_*; x3D is the point
// for ORBFE_NEWPT_OK and what the loop held when it left otherwise (zeros before a point exists).  Octaves index the level tables
// unchecked: the caller keeps them inside.
template <class PA, class PW, class PV>
ORBFE_HD inline int np_triangulate_match(const float *T1, const float *O1, const float *T2, const float *O2, const orbfe_track_camera &cam,
                                         float mb, const NpKey &k1, const NpKey &k2, const float *scale_factors, const float *level_sigma2,
                                         float scale_factor, PA At, PW W, PV Vt, float *x3D)
{
    x3D[0] = x3D[1] = x3D[2] = 0.f;
    const bool st1 = k1.uright >= 0, st2 = k2.uright >= 0;
    const float invfx = trk_div(1.0f, cam.fx), invfy = trk_div(1.0f, cam.fy);   // KeyFrame::invfx
    // N2: xn = ((x - cx) * invfx, (y - cy) * invfy, 1)
    const float xn1[2] = {(k1.ux - cam.cx) * invfx, (k1.uy - cam.cy) * invfy}, xn2[2] = {(k2.ux - cam.cx) * invfx, (k2.uy - cam.cy) * invfy};
    float ray1[3], ray2[3];
    np_ray(T1, xn1[0], xn1[1], ray1);
    np_ray(T2, xn2[0], xn2[1], ray2);
    // N5: ray1.dot(ray2) / (norm(ray1) * norm(ray2)) in double, stored as float
    const float cosRays = (float)(np_dot3(ray1, ray2) / (sqrt(np_dot3(ray1, ray1)) * sqrt(np_dot3(ray2, ray2))));
    float cosStereo = cosRays + 1;
    float cosStereo1 = cosStereo, cosStereo2 = cosStereo;
    if (st1) cosStereo1 = np_cos_parallax_stereo(mb, k1.depth);
    else if (st2) cosStereo2 = np_cos_parallax_stereo(mb, k2.depth);   // `else if`: keyframe 2's only when keyframe 1's keypoint is monocular
    cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;     // std::min(a, b)
    if (cosRays < cosStereo && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
        // N8: the linear triangulation on Tcw and xn
        const float w = triangulate(xn1[0], xn1[1], xn2[0], xn2[1], T1, T2, At, W, Vt, x3D);
        if (w == 0) {
            x3D[0] = x3D[1] = x3D[2] = 0.f;
            return ORBFE_NEWPT_W_ZERO;
        }
    } else if (st1 && cosStereo1 < cosStereo2) {
        // N9: KeyFrame::UnprojectStereo; depth <= 0 returns an empty Mat, on which the reference's next line throws -- here DEPTH1
        if (!(k1.depth > 0)) return ORBFE_NEWPT_DEPTH1;
        const TrkCam c = {cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, 0.f, 0.f, 0.f, 0.f};
        trk_unproject(T1, O1, c, invfx, invfy, k1.rx, k1.ry, k1.depth, x3D);
    } else if (st2 && cosStereo2 < cosStereo1) {
        if (!(k2.depth > 0)) return ORBFE_NEWPT_DEPTH2;
        const TrkCam c = {cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, 0.f, 0.f, 0.f, 0.f};
        trk_unproject(T2, O2, c, invfx, invfy, k2.rx, k2.ry, k2.depth, x3D);
    } else
        return ORBFE_NEWPT_LOW_PARALLAX;
    const float z1 = np_cam_coord(T1, 2, x3D);
    if (z1 <= 0) return ORBFE_NEWPT_DEPTH1;
    const float z2 = np_cam_coord(T2, 2, x3D);
    if (z2 <= 0) return ORBFE_NEWPT_DEPTH2;
    if (np_error_gate(cam, np_cam_coord(T1, 0, x3D), np_cam_coord(T1, 1, x3D), z1, k1, st1, level_sigma2[k1.octave])) return ORBFE_NEWPT_ERR1;
    if (np_error_gate(cam, np_cam_coord(T2, 0, x3D), np_cam_coord(T2, 1, x3D), z2, k2, st2, level_sigma2[k2.octave])) return ORBFE_NEWPT_ERR2;
    const float dist1 = np_dist(x3D, O1), dist2 = np_dist(x3D, O2);
    if (dist1 == 0 || dist2 == 0) return ORBFE_NEWPT_DIST_ZERO;
    // N13: the scale gate in float
    const float ratioDist = trk_div(dist2, dist1);
    const float ratioOctave = trk_div(scale_factors[k1.octave], scale_factors[k2.octave]);
    const float ratioFactor = 1.5f * scale_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBFE_NEWPT_SCALE;
    return ORBFE_NEWPT_OK;
}

// N14: the depth ComputeSceneMedianDepth takes for one MapPoint: Rcw2.dot(x3Dw) + zcw with Rcw2 = Tcw.row(2).colRange(0, 3).t()
// and zcw = Tcw(2, 3), a double dot plus the float promoted, stored as float
ORBFE_HD inline float np_scene_depth(const float *T, const float *x) { return np_cam_coord(T, 2, x); }

// orbfe_newpoints_plan_rounds (host only): pair i goes to the earliest round later than the round of every earlier pair that
// shares a keyframe with it; order = the stable permutation into round order; round_off[0 .. nrounds].  Returns nrounds.
inline int32_t np_plan_rounds(const int32_t *kf1, const int32_t *kf2, int32_t npairs, int32_t *round_of, int32_t *order, int32_t *round_off)
{
    std::unordered_map<int32_t, int32_t> last;   // keyframe -> the round of the latest pair so far that holds it
    int32_t nrounds = 0;
    for (int32_t i = 0; i < npairs; ++i) {
        int32_t r = 0;
        for (const int32_t f : {kf1[i], kf2[i]}) {
            const auto it = last.find(f);
            if (it != last.end()) r = std::max(r, it->second + 1);
        }
        last[kf1[i]] = r;
        last[kf2[i]] = r;
        round_of[i] = r;
        nrounds = std::max(nrounds, r + 1);
    }
    std::vector<int32_t> at(nrounds + 1, 0);
    for (int32_t i = 0; i < npairs; ++i) at[round_of[i] + 1]++;
    for (int32_t r = 0; r < nrounds; ++r) at[r + 1] += at[r];
    for (int32_t r = 0; r <= nrounds; ++r) round_off[r] = at[r];
    for (int32_t i = 0; i < npairs; ++i) order[at[round_of[i]]++] = i;   // ascending i inside a round: stable
    return nrounds;
}

// orbfe_track_geom.h -- the per-point arithmetic of the device-resident tracker (orbfe_track.hip), stated ONCE for its kernels
// and for the host entry point orbfe_frustum_points, so that the two cannot drift:
//   Frame::UnprojectStereo                      src/Frame.cc:879-899
//   SearchByProjection(Current, Last) gating    src/ORBmatcher.cc:1590-1644   (operation order: orc_proj_queries_last_frame)
//   Frame::isInFrustum + MapPoint::PredictScale src/Frame.cc:387-451, src/MapPoint.cc:465-480
//   SearchByProjection(F, vpMapPoints) gating   src/ORBmatcher.cc:63-93
//   Fuse x2 gating (orbfe_fuse.hip)             src/ORBmatcher.cc:1060-1097, :1235-1270
//   SearchBySim3 poses + gating (orbfe_sim3_search.hip)   src/ORBmatcher.cc:1355-1357, :1400-1431, :1476-1503
// Float arithmetic in the order the reference's cv::Mat expressions evaluate to -- 3x3 * 3x1 products accumulate left to right
// in float, norms and dot products in double -- nothing fused (the library is built with -ffp-contract=off), IEEE division.
// Poses are row-major 3x4 (Rcw | tcw).  Restated in tests/track_oracle.py.
//
// PcZ == 0 is undefined in the reference's isInFrustum: 1 / 0 is infinite, 0 * inf is NaN, and NaN passes the bounds test
// (every comparison with it is false).  Nothing here defines it either; callers keep such points out.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "orbfe.h"

using TrkCam = orbfe_track_camera;   // fx, fy, cx, cy, bf, then Frame::mnMinX .. mnMaxY as minx, maxx, miny, maxy

__host__ __device__ inline float trk_div(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// r = Rcw * x + tcw
__host__ __device__ inline void trk_to_camera(const float *T, const float *x, float *r)
{
    for (int k = 0; k < 3; ++k) {
        float acc = T[4 * k] * x[0];
        acc += T[4 * k + 1] * x[1];
        acc += T[4 * k + 2] * x[2];
        r[k] = acc + T[4 * k + 3];
    }
}

// Ow = twc = -Rcw^T * tcw (Frame::UpdatePoseMatrices; :1596 of the matcher)
__host__ __device__ inline void trk_camera_centre(const float *T, float *Ow)
{
    for (int k = 0; k < 3; ++k) {
        float acc = -T[k] * T[3];
        acc += -T[4 + k] * T[7];
        acc += -T[8 + k] * T[11];
        Ow[k] = acc;
    }
}

// Frame::UnprojectStereo for a keypoint with depth z > 0: Rwc * (x, y, z) + Ow, Rwc = Rcw^T
__host__ __device__ inline void trk_unproject(const float *T, const float *Ow, const TrkCam &c, float invfx, float invfy, float u,
                                              float v, float z, float *xw)
{
    const float x = (u - c.cx) * z * invfx, y = (v - c.cy) * z * invfy;
    for (int k = 0; k < 3; ++k) {
        float acc = T[k] * x;
        acc += T[4 + k] * y;
        acc += T[8 + k] * z;
        xw[k] = acc + Ow[k];
    }
}

// :1593-1607: tlc = Rlw * twc + tlw against the baseline; bit 0 = bForward, bit 1 = bBackward
__host__ __device__ inline int trk_motion(const float *Tcw_cur, const float *Tcw_last, float mb, int mono)
{
    float twc[3], tlc[3];
    trk_camera_centre(Tcw_cur, twc);
    trk_to_camera(Tcw_last, twc, tlc);
    return ((tlc[2] > mb && !mono) ? 1 : 0) | ((-tlc[2] > mb && !mono) ? 2 : 0);
}

// :1620-1656 for one last-frame MapPoint; false = no query
__host__ __device__ inline bool trk_gate_last(const float *Tcw_cur, const TrkCam &c, const float *xw, int oct, float th,
                                              const float *scale_factors, int motion, int obs_gt0, orbfe_proj_query *q)
{
    float p[3];
    trk_to_camera(Tcw_cur, xw, p);
    const float invzc = trk_div(1.0f, p[2]);
    if (invzc < 0.0f) return false;
    const float u = c.fx * p[0] * invzc + c.cx;
    const float v = c.fy * p[1] * invzc + c.cy;
    if (u < c.minx || u > c.maxx) return false;
    if (v < c.miny || v > c.maxy) return false;
    q->u = u;
    q->v = v;
    q->r = th * scale_factors[oct];
    if (motion & 1) { q->min_level = oct; q->max_level = -1; }
    else if (motion & 2) { q->min_level = 0; q->max_level = oct; }
    else { q->min_level = oct - 1; q->max_level = oct + 1; }
    q->ur = u - c.bf * invzc;
    q->flags = ORBFE_PROJ_RIGHT_GATE | (obs_gt0 ? ORBFE_PROJ_CLAIMS : 0);
    q->pad = 0;
    return true;
}

// MapPoint::PredictScale(currentDist, Frame*): ceil(log(mfMaxDistance / currentDist) / mfLogScaleFactor), clamped
__host__ __device__ inline int trk_predict_scale(float max_dist, float dist, float log_scale_factor, int nlevels)
{
    const float ratio = trk_div(max_dist, dist);
    const float lg = (float)log((double)ratio);
    int n = (int)ceilf(trk_div(lg, log_scale_factor));
    if (n < 0) n = 0;
    else if (n >= nlevels) n = nlevels - 1;
    return n;
}

struct TrkProj {
    float u, v, ur, view_cos;
    int32_t level;
};

// Frame::isInFrustum(pMP, 0.5) for one MapPoint; false = mbTrackInView stays false
__host__ __device__ inline bool trk_frustum(const float *Tcw, const float *Ow, const TrkCam &c, const float *P, const float *Pn,
                                            float min_dist, float max_dist, float log_scale_factor, int nlevels, TrkProj *o)
{
    float pc[3];
    trk_to_camera(Tcw, P, pc);
    if (pc[2] < 0.0f) return false;
    const float invz = trk_div(1.0f, pc[2]);
    const float u = c.fx * pc[0] * invz + c.cx;
    const float v = c.fy * pc[1] * invz + c.cy;
    if (u < c.minx || u > c.maxx) return false;
    if (v < c.miny || v > c.maxy) return false;
    const float po[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist = (float)sqrt((double)po[0] * (double)po[0] + ((double)po[1] * (double)po[1]) + ((double)po[2] * (double)po[2]));
    if (dist < min_dist || dist > max_dist) return false;
    const double dot = (double)po[0] * (double)Pn[0] + ((double)po[1] * (double)Pn[1]) + ((double)po[2] * (double)Pn[2]);
    const float view_cos = (float)(dot / (double)dist);
    if (view_cos < 0.5f) return false;
    o->u = u;
    o->v = v;
    o->ur = u - c.bf * invz;
    o->view_cos = view_cos;
    o->level = trk_predict_scale(max_dist, dist, log_scale_factor, nlevels);
    return true;
}

// :80-93: the query of a MapPoint that isInFrustum kept (orbfe_proj_queries_local_map's rule)
__host__ __device__ inline void trk_query_local_map(const TrkProj &p, float th, const float *scale_factors, int obs_gt0,
                                                    orbfe_proj_query *q)
{
    float r = (double)p.view_cos > 0.998 ? 2.5f : 4.0f;
    if (th != 1.0f) r *= th;
    q->u = p.u;
    q->v = p.v;
    q->r = r * scale_factors[p.level];
    q->min_level = p.level - 1;
    q->max_level = p.level;
    q->ur = p.ur;
    q->flags = ORBFE_PROJ_RIGHT_GATE | (obs_gt0 ? ORBFE_PROJ_CLAIMS : 0);
    q->pad = 0;
}

// ORBmatcher::Fuse, both overloads (src/ORBmatcher.cc:1060-1097 and, identically, :1235-1270): the gating of one MapPoint that is
// neither NULL, bad nor already in the keyframe; false = the reference `continue`s.  Ow is the caller's (GetCameraCenter, or
// -Rcw.t() * tcw of the decomposed Scw), c.minx .. c.maxy are KeyFrame::mnMinX .. mnMaxY (ints, as floats).  The Sim3 body
// writes `1.0 / z` in double and stores it to float: the same value as the float division here, because a double quotient
// rounded to float equals the float quotient when the double has at least 2 * 24 + 2 significand bits (53 >= 50).  z == 0
// gives an infinite invz and a NaN or infinite u: not in the image, so out.  The viewing-angle gate compares the double dot
// product with 0.5 * (double)dist3D -- not trk_frustum's float view_cos < 0.5f.  chi2 != 0: the plain overload, whose
// candidates pass the reprojection-error gate (:1112-1139); 0: the Sim3 overload, which has none.  The distance gate is the
// getters': out iff dist3D < 0.8f * mfMinDistance || dist3D > 1.2f * mfMaxDistance, the values orbfe_project_points is handed.
__host__ __device__ inline bool trk_gate_fuse(const float *Tcw, const float *Ow, const TrkCam &c, const float *P, const float *Pn,
                                              float min_distance, float max_distance, float th, const float *scale_factors,
                                              float log_scale_factor, int nlevels, int chi2, orbfe_proj_query *q, int32_t *level)
{
    float pc[3];
    trk_to_camera(Tcw, P, pc);
    if (pc[2] < 0.0f) return false;
    const float invz = trk_div(1.0f, pc[2]);
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = c.fx * x + c.cx;
    const float v = c.fy * y + c.cy;
    if (!(u >= c.minx && u < c.maxx && v >= c.miny && v < c.maxy)) return false;   // KeyFrame::IsInImage; NaN is out
    const float po[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist = (float)sqrt((double)po[0] * (double)po[0] + ((double)po[1] * (double)po[1]) + ((double)po[2] * (double)po[2]));
    // min_distance / max_distance are mfMinDistance / mfMaxDistance: the getters scale them (src/MapPoint.cc:427-437),
    // PredictScale reads the unscaled mfMaxDistance (:448-463)
    if (dist < 0.8f * min_distance || dist > 1.2f * max_distance) return false;
    const double dot = (double)po[0] * (double)Pn[0] + ((double)po[1] * (double)Pn[1]) + ((double)po[2] * (double)Pn[2]);
    if (dot < 0.5 * (double)dist) return false;
    const int lv = trk_predict_scale(max_distance, dist, log_scale_factor, nlevels);
    q->u = u;
    q->v = v;
    q->r = th * scale_factors[lv];
    q->min_level = lv - 1;
    q->max_level = lv;
    q->ur = u - c.bf * invz;
    q->flags = chi2 ? ORBFE_PROJ_CHI2_GATE : 0;
    q->pad = 0;
    *level = lv;
    return true;
}

// r = A * x + b for a row-major 3x4 (A | b) the way the reference's cv::Mat expression `A * x + b` evaluates: the product's
// accumulator starts at 0.0f (so a product of -0 becomes +0, which trk_to_camera's first term keeps), then one float add of b
__host__ __device__ inline void trk_affine(const float *T, const float *x, float *r)
{
    for (int k = 0; k < 3; ++k) {
        float acc = 0.0f;
        acc += T[4 * k] * x[0];
        acc += T[4 * k + 1] * x[1];
        acc += T[4 * k + 2] * x[2];
        r[k] = acc + T[4 * k + 3];
    }
}

// The two similarity poses of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1355-1357) as row-major 3x4 blocks T12 = (sR12 | t12),
// T21 = (sR21 | t21): sR12 = s12 * R12 and sR21 = (1.0 / s12) * R12.t() are double products rounded to float element by element
// (the scalar is a double in both: `s12 *` promotes the float, `1.0 / s12` is a double quotient), t21 = -sR21 * t12 negates sR21
// first (exact) and accumulates the float product from 0.0f left to right.
__host__ __device__ inline void trk_sim3_pair_pose(float s12, const float *R12, const float *t12, float *T12, float *T21)
{
    const double s = (double)s12, inv = 1.0 / (double)s12;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            T12[4 * r + c] = (float)((double)R12[3 * r + c] * s);
            T21[4 * r + c] = (float)((double)R12[3 * c + r] * inv);
        }
        T12[4 * r + 3] = t12[r];
    }
    for (int r = 0; r < 3; ++r) {
        float acc = 0.0f;
        acc += -T21[4 * r] * t12[0];
        acc += -T21[4 * r + 1] * t12[1];
        acc += -T21[4 * r + 2] * t12[2];
        T21[4 * r + 3] = acc;
    }
}

// ORBmatcher::SearchBySim3, either direction (src/ORBmatcher.cc:1400-1431 and, identically, :1476-1503): the gating of one
// MapPoint of a keyframe that is neither NULL, already matched nor bad; false = the reference `continue`s.  T_own is the pose of
// the keyframe that holds the point (Rcw | tcw), T_to_other the similarity (sR21 | t21) or (sR12 | t12) into the other camera,
// c.minx .. c.maxy are the other keyframe's mnMinX .. mnMaxY.  invz is written `1.0 / z` in double and stored to float: the
// float quotient (see trk_gate_fuse).  z == 0 gives a NaN or infinite u: out.  dist3D is the norm of the point IN THE OTHER CAMERA
// (cv::norm(p3Dc2): a double sum of squares, sqrt, to float) -- not |Pw - Ow| --, there is no viewing-angle gate, and the distance
// gate is the getters': out iff dist3D < 0.8f * mfMinDistance || dist3D > 1.2f * mfMaxDistance, PredictScale from the unscaled
// mfMaxDistance.
__host__ __device__ inline bool trk_gate_sim3(const float *T_own, const float *T_to_other, const TrkCam &c, const float *P,
                                              float min_distance, float max_distance, float th, const float *scale_factors,
                                              float log_scale_factor, int nlevels, orbfe_proj_query *q, int32_t *level)
{
    float pc[3], po[3];
    trk_affine(T_own, P, pc);
    trk_affine(T_to_other, pc, po);
    if (po[2] < 0.0f) return false;
    const float invz = trk_div(1.0f, po[2]);
    const float x = po[0] * invz, y = po[1] * invz;
    const float u = c.fx * x + c.cx;
    const float v = c.fy * y + c.cy;
    if (!(u >= c.minx && u < c.maxx && v >= c.miny && v < c.maxy)) return false;   // KeyFrame::IsInImage; NaN is out
    const float dist = (float)sqrt((double)po[0] * (double)po[0] + ((double)po[1] * (double)po[1]) + ((double)po[2] * (double)po[2]));
    if (dist < 0.8f * min_distance || dist > 1.2f * max_distance) return false;
    const int lv = trk_predict_scale(max_distance, dist, log_scale_factor, nlevels);
    q->u = u;
    q->v = v;
    q->r = th * scale_factors[lv];
    q->min_level = lv - 1;
    q->max_level = lv;
    q->ur = u - c.bf * invz;
    q->flags = 0;
    q->pad = 0;
    *level = lv;
    return true;
}

// orbfe_frame.hip -- the per-frame geometry of the RGB-D Frame on the device:
//   Frame::UndistortKeyPoints      perfect/src/Frame.cc:750-781   (cv::undistortPoints with P = K, skipped when k1 == 0)
//   Frame::ComputeImageBounds      perfect/src/Frame.cc:784-815   (host: orbfe_image_bounds)
//   Frame::ComputeStereoFromRGBD   perfect/src/Frame.cc:1041-1062 (mvDepth / mvuRight from the depth plane)
//   Tracking's depth convertTo     perfect/src/Tracking.cc:681-682
// The undistortion arithmetic is orbfe_undistort.h, shared by the kernels and the host helper.
#include <math.h>

#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_undistort.h"

namespace {

bool cam_ok(const orbfe_camera *cam) { return cam && orb_undistort_ndist_ok(cam->ndist); }

// Tracking.cc:681: (fabs(mDepthMapFactor - 1.0f) > 1e-5) || type != CV_32F -- the float difference, compared in double
__host__ __device__ inline bool depth_scaled(int format, float scale)
{
    return format == ORBFE_DEPTH_U16 || (double)fabsf(scale - 1.0f) > 1e-5;
}

// cvtScale_<T, float, float>: saturate_cast<float>(src * scale + shift), shift = 0, all in float
__device__ inline float depth_value(const void *row, int x, int format, bool scaled, float scale)
{
    const float v = format == ORBFE_DEPTH_U16 ? (float)((const uint16_t *)row)[x] : ((const float *)row)[x];
    return scaled ? v * scale + 0.0f : v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_undistort_points(const float *xy, int n, OrbUndistort u, float *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float x, y;
    orb_undistort_point(u, xy[2 * i], xy[2 * i + 1], &x, &y);
    out[2 * i] = x;
    out[2 * i + 1] = y;
}

// one thread per keypoint slot of the nframes x cap block
__global__ __launch_bounds__(256) void k_frame_geometry(const orbfe_keypoint *kps, const int32_t *d_n, int cap, int64_t nslots,
                                                        OrbUndistort u, int undistort, float bf, const uint8_t *depth, int dw, int dh,
                                                        int format, size_t dstride, size_t dfstride, float scale, orbfe_keypoint *kps_un,
                                                        float *out_depth, float *out_uright)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    const int f = (int)(s / cap), i = (int)(s - (int64_t)f * cap);
    if (i >= d_n[f]) {   // the all-gather invariant: free slots are zero
        kps_un[s] = orbfe_keypoint{0.f, 0.f, 0.f, 0.f, 0.f, 0, 0};
        if (out_depth) {
            out_depth[s] = 0.f;
            out_uright[s] = 0.f;
        }
        return;
    }
    orbfe_keypoint kp = kps[s];
    const float x = kp.x, y = kp.y;
    if (undistort) orb_undistort_point(u, x, y, &kp.x, &kp.y);
    kps_un[s] = kp;
    if (!out_depth) return;
    float dep = -1.f, ur = -1.f;
    // imDepth.at<float>(v, u): both truncated to int; a keypoint outside the plane (or NaN) has no depth
    if (depth && x > -1.f && x < (float)dw && y > -1.f && y < (float)dh) {
        const uint8_t *row = depth + (size_t)f * dfstride + (size_t)(int)y * dstride;
        const float d = depth_value(row, (int)x, format, depth_scaled(format, scale), scale);
        if (d > 0) {
            dep = d;
            ur = kp.x - bf / d;
        }
    }
    out_depth[s] = dep;
    out_uright[s] = ur;
}

// the whole-plane convertTo: one thread per 4 pixels of a row (VEC: 8- / 16-byte accesses), rows of all frames flattened
template <bool VEC>
__global__ __launch_bounds__(256) void k_depth_to_float(const uint8_t *src, int format, int w, int h, size_t sstride, size_t sfstride,
                                                        float scale, int scaled, uint8_t *dst, size_t dstride, size_t dfstride,
                                                        int64_t ngroups)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    const int gpr = (w + 3) >> 2;
    const int64_t r = g / gpr;
    const int x0 = (int)(g - r * gpr) * 4;
    const int f = (int)(r / h), y = (int)(r - (int64_t)f * h);
    const uint8_t *srow = src + (size_t)f * sfstride + (size_t)y * sstride;
    float *drow = (float *)(dst + (size_t)f * dfstride + (size_t)y * dstride);
    if (VEC) {
        float4 o;
        if (format == ORBFE_DEPTH_U16) {
            const ushort4 v = *(const ushort4 *)((const uint16_t *)srow + x0);
            o = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
        } else {
            o = *(const float4 *)((const float *)srow + x0);
        }
        if (scaled) {
            o.x = o.x * scale + 0.0f;
            o.y = o.y * scale + 0.0f;
            o.z = o.z * scale + 0.0f;
            o.w = o.w * scale + 0.0f;
        }
        *(float4 *)(drow + x0) = o;
    } else {
        const int x1 = min(x0 + 4, w);
        for (int x = x0; x < x1; ++x) drow[x] = depth_value(srow, x, format, scaled, scale);
    }
}

extern "C" orbfe_status orbfe_undistort_points(orbfe_matcher *m, const float *xy, int32_t n, const orbfe_camera *cam, float *out_xy)
{
    if (!m || n < 0 || !cam || (n > 0 && (!xy || !out_xy))) {
        orbfe_set_error("bad argument to orbfe_undistort_points");
        return ORBFE_ERR_ARG;
    }
    if (!cam_ok(cam)) {
        orbfe_set_error("orbfe_undistort_points: %d distortion coefficients (0, 4, 5, 8 or 12 are built)", cam->ndist);
        return ORBFE_ERR_ARG;
    }
    if (n == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    const size_t bytes = (size_t)n * 8;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    ORBFE_HIP(m->b[0].ensure(2 * bytes));
    float *d_in = m->b[0].as<float>(), *d_out = d_in + 2 * (size_t)n;
    ORBFE_HIP(hipMemcpyAsync(d_in, xy, bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_undistort_points, dim3((n + 255) / 256), dim3(256), 0, st, (const float *)d_in, n, orb_undistort_prepare(*cam),
                       d_out);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(out_xy, d_out, bytes, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_image_bounds(const orbfe_camera *cam, int32_t w, int32_t ht, float out[6])
{
    if (!out || w < 1 || ht < 1 || !cam_ok(cam)) {
        orbfe_set_error("bad argument to orbfe_image_bounds");
        return ORBFE_ERR_ARG;
    }
    float minx, maxx, miny, maxy;
    if (orb_undistort_k1_zero(*cam)) {
        minx = 0.0f;
        maxx = (float)w;
        miny = 0.0f;
        maxy = (float)ht;
    } else {
        const OrbUndistort u = orb_undistort_prepare(*cam);
        const float cx[4] = {0.0f, (float)w, 0.0f, (float)w}, cy[4] = {0.0f, 0.0f, (float)ht, (float)ht};
        float px[4], py[4];
        for (int i = 0; i < 4; ++i) orb_undistort_point(u, cx[i], cy[i], &px[i], &py[i]);
        minx = std::min(px[0], px[2]);
        maxx = std::max(px[1], px[3]);
        miny = std::min(py[0], py[1]);
        maxy = std::max(py[2], py[3]);
    }
    out[0] = minx;
    out[1] = maxx;
    out[2] = miny;
    out[3] = maxy;
    out[4] = static_cast<float>(ORBFE_GRID_COLS) / static_cast<float>(maxx - minx);
    out[5] = static_cast<float>(ORBFE_GRID_ROWS) / static_cast<float>(maxy - miny);
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_frame_geometry_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const int32_t *d_n, int32_t cap,
                                                          int32_t nframes, const orbfe_camera *cam, const void *d_depth_plane,
                                                          int32_t depth_w, int32_t depth_h, int32_t depth_format, size_t depth_stride,
                                                          size_t depth_frame_stride, float scale, orbfe_keypoint *d_kps_un,
                                                          float *d_depth, float *d_uright, void *stream)
{
    const size_t esz = depth_format == ORBFE_DEPTH_U16 ? 2 : 4;
    if (!m || !cam_ok(cam) || cap < 0 || nframes < 0 || (!d_depth) != (!d_uright) ||
        (nframes > 0 && cap > 0 && (!d_kps || !d_n || !d_kps_un)) ||
        (d_depth_plane && (depth_w < 1 || depth_h < 1 || (depth_format != ORBFE_DEPTH_U16 && depth_format != ORBFE_DEPTH_F32) ||
                           depth_stride < (size_t)depth_w * esz ||
                           (nframes > 1 && depth_frame_stride < depth_stride * (size_t)depth_h)))) {
        orbfe_set_error("bad argument to orbfe_frame_geometry_batch_device");
        return ORBFE_ERR_ARG;
    }
    const int64_t nslots = (int64_t)nframes * cap;
    if (nslots == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    const bool undistort = !orb_undistort_k1_zero(*cam);
    hipLaunchKernelGGL(k_frame_geometry, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_kps, d_n, cap,
                       nslots, orb_undistort_prepare(*cam), undistort ? 1 : 0, cam->bf, (const uint8_t *)d_depth_plane, depth_w,
                       depth_h, depth_format, depth_stride, depth_frame_stride, scale, d_kps_un, d_depth, d_uright);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_depth_to_float_device(const void *d_src, int32_t depth_format, int32_t nframes, int32_t w, int32_t ht,
                                                    size_t src_stride, size_t src_frame_stride, float scale, float *d_dst,
                                                    size_t dst_stride, size_t dst_frame_stride, void *stream)
{
    const size_t esz = depth_format == ORBFE_DEPTH_U16 ? 2 : 4;
    if (!d_src || !d_dst || nframes < 0 || w < 1 || ht < 1 || (depth_format != ORBFE_DEPTH_U16 && depth_format != ORBFE_DEPTH_F32) ||
        src_stride < (size_t)w * esz || dst_stride < (size_t)w * 4 ||
        (nframes > 1 && (src_frame_stride < src_stride * (size_t)ht || dst_frame_stride < dst_stride * (size_t)ht))) {
        orbfe_set_error("bad argument to orbfe_depth_to_float_device");
        return ORBFE_ERR_ARG;
    }
    if (nframes == 0) return ORBFE_OK;
    int32_t device = -1;   // the caller's current device: the buffers are theirs
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    const int64_t ngroups = (int64_t)nframes * ht * ((w + 3) / 4);
    // 4-pixel groups: whole vectors when every row starts on a 16-byte boundary of dst and an 8- / 16-byte one of src
    const size_t sa = 4 * esz;
    const bool vec = (w % 4) == 0 && ((uintptr_t)d_src % sa) == 0 && src_stride % sa == 0 && (nframes == 1 || src_frame_stride % sa == 0) &&
                     ((uintptr_t)d_dst % 16) == 0 && dst_stride % 16 == 0 && (nframes == 1 || dst_frame_stride % 16 == 0);
    const int scaled = depth_scaled(depth_format, scale) ? 1 : 0;
    const dim3 grid((unsigned)((ngroups + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(k_depth_to_float<true>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t *)d_src, depth_format, w, ht,
                           src_stride, src_frame_stride, scale, scaled, (uint8_t *)d_dst, dst_stride, dst_frame_stride, ngroups);
    else
        hipLaunchKernelGGL(k_depth_to_float<false>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t *)d_src, depth_format, w, ht,
                           src_stride, src_frame_stride, scale, scaled, (uint8_t *)d_dst, dst_stride, dst_frame_stride, ngroups);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

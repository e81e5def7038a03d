// orbfe_taps.hip -- what a caller reads back from the extractor handle after a call: level sizes, mvImagePyramid (one level or all
// of them padded), the device view of the pyramid for the matcher's kernels, and the stage taps (blurred level, FAST candidates,
// quadtree selection) the parity tests compare with the oracle.  Host code; the one kernel it launches is orbk_launch_pad_pyramid.
#include <algorithm>

#include "orbfe_extractor.h"

static orbfe_status check_tap(orbfe_handle *h, int frame, int level)
{
    if (!h) return ORBFE_ERR_ARG;
    if (!h->plan_valid || h->last_nframes == 0) { orbfe_set_error("no extract call yet"); return ORBFE_ERR_STATE; }
    if (frame < 0 || frame >= h->last_nframes || level < 0 || level >= h->plan.nlevels) {
        orbfe_set_error("frame/level out of range");
        return ORBFE_ERR_ARG;
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_level_size(const orbfe_handle *h, int32_t level, int32_t *w, int32_t *ht)
{
    if (!h || !h->plan_valid || level < 0 || level >= h->plan.nlevels) return ORBFE_ERR_ARG;
    if (w) *w = h->plan.lv[level].w;
    if (ht) *ht = h->plan.lv[level].h;
    return ORBFE_OK;
}

static inline int host_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

static orbfe_status fetch_level(orbfe_handle *h, const uint8_t *base, int pitch, int w, int ht, uint8_t *dst,
                                int dst_stride, int border)
{
    std::vector<uint8_t> tmp((size_t)w * ht);
    ORBFE_HIP(wait_last_call(h));
    ORBFE_HIP(hipMemcpy2D(tmp.data(), (size_t)w, base, (size_t)pitch, (size_t)w, (size_t)ht, hipMemcpyDeviceToHost));
    for (int y = -border; y < ht + border; ++y) {
        const uint8_t *s = tmp.data() + (size_t)host_reflect101(y, ht) * w;
        uint8_t *d = dst + (size_t)(y + border) * dst_stride;
        if (border == 0) memcpy(d, s, (size_t)w);
        else
            for (int x = -border; x < w + border; ++x) d[x + border] = s[host_reflect101(x, w)];  // :1136-1142
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_pyramid_level(orbfe_handle *h, int32_t frame, int32_t level, uint8_t *dst,
                                                int32_t dst_stride, int32_t with_border)
{
    orbfe_status s = check_tap(h, frame, level);
    if (s != ORBFE_OK) return s;
    if (!dst) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    const OrbLevel &L = h->plan.lv[level];
    const int border = with_border ? ORBFE_EDGE : 0;
    if (dst_stride < L.w + 2 * border) return ORBFE_ERR_ARG;
    if (level == 0)
        return fetch_level(h, h->last_gray + (int64_t)frame * h->last_gray_fstride, h->last_gray_pitch, L.w, L.h, dst,
                           dst_stride, border);
    return fetch_level(h, (uint8_t *)h->d_pyr.p + (int64_t)frame * h->plan.pyr_frame_bytes + L.off, L.pitch, L.w, L.h,
                       dst, dst_stride, border);
}

// The public mvImagePyramid in one go: every level of frame `frame` with its 19-px BORDER_REFLECT_101 frame, level l as a
// (w_l + 38) x (h_l + 38) block with tight rows at offsets[l] of dst.  One kernel builds the blocks on the device, ONE
// device-to-host copy brings them over (the per-level orbfe_get_pyramid_level path made 8 pageable 2-D copies and filled the
// frames on the host: 9.6 ms for a 640x480 frame against 0.18 ms for the extraction itself).
extern "C" orbfe_status orbfe_get_pyramid_padded(orbfe_handle *h, int32_t frame, uint8_t *dst, size_t cap, size_t *offsets, size_t *total)
{
    orbfe_status s = check_tap(h, frame, 0);
    if (s != ORBFE_OK) return s;
    DeviceGuard g(h->device);
    const int nl = h->plan.nlevels;
    uint32_t off[ORBFE_MAX_LEVELS + 1];
    uint32_t at = 0;
    for (int l = 0; l < nl; ++l) {
        off[l] = at;
        const OrbLevel &L = h->plan.lv[l];
        at += (uint32_t)(((size_t)(L.w + 2 * ORBFE_EDGE) * (size_t)(L.h + 2 * ORBFE_EDGE) + 63) & ~(size_t)63);
    }
    off[nl] = at;
    if (offsets)
        for (int l = 0; l < nl; ++l) offsets[l] = off[l];
    if (total) *total = at;
    if (!dst) return ORBFE_OK;   // sizing call
    if (cap < at) { orbfe_set_error("orbfe_get_pyramid_padded: %zu bytes needed, %zu given", (size_t)at, cap); return ORBFE_ERR_CAP; }
    OrbPyrView v;
    s = orbfe_internal_pyramid_view(h, frame, &v);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(wait_last_call(h));
    ORBFE_HIP(h->d_pad.ensure(at));
    ORBFE_HIP(orbk_launch_pad_pyramid(v, off, (uint8_t *)h->d_pad.p, h->stream));
    ORBFE_HIP(hipMemcpyAsync(dst, h->d_pad.p, at, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP(hipStreamSynchronize(h->stream));
    return ORBFE_OK;
}

// makes `stream` (a hipStream_t) wait for the handle's last batched call, wherever it ran: the pyramid readers of the
// matcher (stereo) order themselves behind the extractor with it, without a host synchronisation
int32_t orbfe_internal_order_after_last_call(orbfe_handle *h, void *stream)
{
    if (!h) return ORBFE_ERR_ARG;
    if (!h->last_stream_valid || h->last_stream == (hipStream_t)stream) return ORBFE_OK;
    DeviceGuard g(h->device);
    ORBFE_HIP(hipStreamWaitEvent((hipStream_t)stream, h->ev_last, 0));
    return ORBFE_OK;
}

int32_t orbfe_internal_pyramid_view(orbfe_handle *h, int frame, OrbPyrView *v)
{
    orbfe_status s = check_tap(h, frame, 0);
    if (s != ORBFE_OK) return s;
    DeviceGuard g(h->device);
    v->nlevels = h->plan.nlevels;
    v->device = h->device;
    for (int l = 0; l < h->plan.nlevels; ++l) {
        const OrbLevel &L = h->plan.lv[l];
        v->ptr[l] = l == 0 ? h->last_gray + (int64_t)frame * h->last_gray_fstride
                           : (const uint8_t *)h->d_pyr.p + (int64_t)frame * h->plan.pyr_frame_bytes + L.off;
        v->pitch[l] = l == 0 ? h->last_gray_pitch : L.pitch;
        v->w[l] = L.w;
        v->h[l] = L.h;
        v->scale[l] = h->pin.scale[l];
        v->inv_scale[l] = h->pin.inv_scale[l];
        v->fstride[l] = l == 0 ? h->last_gray_fstride : (int64_t)h->plan.pyr_frame_bytes;
    }
    v->nframes = h->last_nframes;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_tap_blurred_level(orbfe_handle *h, int32_t frame, int32_t level, uint8_t *dst,
                                                int32_t dst_stride)
{
    orbfe_status s = check_tap(h, frame, level);
    if (s != ORBFE_OK) return s;
    if (!dst) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    const OrbLevel &L = h->plan.lv[level];
    if (dst_stride < L.w) return ORBFE_ERR_ARG;
    return fetch_level(h, (uint8_t *)h->d_blur.p + (int64_t)frame * h->plan.pyr_frame_bytes + L.off, L.pitch, L.w, L.h,
                       dst, dst_stride, 0);
}

extern "C" orbfe_status orbfe_tap_candidates(orbfe_handle *h, int32_t frame, int32_t level, float *xyr, int32_t cap,
                                             int32_t *n)
{
    orbfe_status s = check_tap(h, frame, level);
    if (s != ORBFE_OK) return s;
    if (!n) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    const OrbPlan &P = h->plan;
    const OrbLevel &L = P.lv[level];
    ORBFE_HIP(wait_last_call(h));
    int32_t nk = 0, nsv = 0;
    ORBFE_HIP(hipMemcpy(&nk, (int32_t *)h->d_nkeys.p + ((size_t)frame * P.nlevels + level) * ORBFE_NK_STRIDE, sizeof(int32_t),
                        hipMemcpyDeviceToHost));
    ORBFE_HIP(hipMemcpy(&nsv, (int32_t *)h->d_scount.p + ((size_t)frame * P.nlevels + level) * ORBFE_NK_STRIDE, sizeof(int32_t),
                        hipMemcpyDeviceToHost));
    nsv = std::min(nsv, L.key_cap);
    *n = nk;
    if (nk > cap) return ORBFE_ERR_CAP;
    if (nk == 0) return ORBFE_OK;
    if (!xyr) return ORBFE_ERR_ARG;
    // The device keeps the NMS survivors {key, ord} unordered and in place; the per-cell threshold fallback (:818-825) is
    // the same rule k_octree applies: a survivor counts if it is above iniTh or its cell has no survivor above iniTh.
    // `ord` is the rank key of the reference's candidate order.
    std::vector<uint2> sv((size_t)nsv);
    ORBFE_HIP(hipMemcpy(sv.data(), (uint2 *)h->d_skeys.p + (size_t)frame * P.keys_per_frame + L.key_off,
                        sizeof(uint2) * (size_t)nsv, hipMemcpyDeviceToHost));
    std::vector<uint8_t> strong((size_t)L.ncells, 0);
    for (const uint2 &e : sv)
        if ((int)orb_key_r(e.x) >= P.ini_th && (e.y >> 12) < (uint32_t)L.ncells) strong[e.y >> 12] = 1;
    std::vector<uint32_t> kv, ko;
    for (const uint2 &e : sv)
        if ((int)orb_key_r(e.x) >= P.ini_th || ((e.y >> 12) < (uint32_t)L.ncells && !strong[e.y >> 12])) {
            kv.push_back(e.x);
            ko.push_back(e.y);
        }
    if ((int)kv.size() != nk) {
        orbfe_set_error("candidate tap: host filter found %d keys, device counted %d", (int)kv.size(), nk);
        return ORBFE_ERR_STATE;
    }
    std::vector<int> order((size_t)nk);
    for (int i = 0; i < nk; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return ko[a] < ko[b]; });
    for (int i = 0; i < nk; ++i) {
        const uint32_t k = kv[order[i]];
        xyr[3 * i] = (float)orb_key_x(k);
        xyr[3 * i + 1] = (float)orb_key_y(k);
        xyr[3 * i + 2] = (float)orb_key_r(k);
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_tap_selected(orbfe_handle *h, int32_t frame, int32_t level, float *xyr, int32_t cap,
                                           int32_t *n)
{
    orbfe_status s = check_tap(h, frame, level);
    if (s != ORBFE_OK) return s;
    if (!n) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    const OrbPlan &P = h->plan;
    const OrbLevel &L = P.lv[level];
    ORBFE_HIP(wait_last_call(h));
    int32_t ns = 0;
    ORBFE_HIP(hipMemcpy(&ns, (int32_t *)h->d_nsel.p + (size_t)frame * P.nlevels + level, sizeof(int32_t),
                        hipMemcpyDeviceToHost));
    *n = ns;
    if (ns > cap) return ORBFE_ERR_CAP;
    if (ns == 0) return ORBFE_OK;
    if (!xyr) return ORBFE_ERR_ARG;
    std::vector<uint32_t> keys((size_t)ns);
    ORBFE_HIP(hipMemcpy(keys.data(), (uint32_t *)h->d_sel.p + (size_t)frame * P.sel_per_frame + L.sel_off,
                        sizeof(uint32_t) * (size_t)ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < ns; ++i) {
        xyr[3 * i] = (float)orb_key_x(keys[i]);
        xyr[3 * i + 1] = (float)orb_key_y(keys[i]);
        xyr[3 * i + 2] = (float)orb_key_r(keys[i]);
    }
    return ORBFE_OK;
}

// orbfe_api.hip -- host side of the extractor C-ABI (include/orbfe.h): device buffers, stream/event plumbing, the call sequence of
// a batch.  The constructor tables and the per-size plan come from orbfe_plan.hip, which needs no device; this file uploads them.
// All pixel work happens in the kernel files (one per stage: orbfe_kernels.h); there is no CPU path.
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>

#include "orbfe_extractor.h"

// ---------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------
static thread_local char t_err[512] = "";

void orbfe_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof(t_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *orbfe_last_error(void) { return t_err; }
extern "C" int32_t orbfe_version(void) { return ORBFE_VERSION; }

extern "C" const char *orbfe_strerror(orbfe_status s)
{
    switch (s) {
    case ORBFE_OK: return "ok";
    case ORBFE_ERR_ARG: return "invalid argument";
    case ORBFE_ERR_SIZE: return "image size outside the planned range or too small for the pyramid grid";
    case ORBFE_ERR_CAP: return "keypoint capacity too small";
    case ORBFE_ERR_HIP: return "HIP runtime error";
    case ORBFE_ERR_NOMEM: return "out of memory";
    case ORBFE_ERR_NODEVICE: return "no usable HIP device (this library has no CPU path)";
    case ORBFE_ERR_STATE: return "call not valid in the current state";
    default: return "unknown error";
    }
}

extern "C" int32_t orbfe_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// Collects the answer of a finished automatic FAST-mode probe into auto_last; never waits.  true: there was one.
static bool collect_auto_probe(orbfe_handle *h)
{
    if (h->auto_pending && hipEventQuery(h->ev_auto) == hipSuccess) {
        memcpy(h->auto_last, h->h_auto.p, sizeof(h->auto_last));
        h->auto_pending = false;
        return true;
    }
    (void)hipGetLastError();   // hipErrorNotReady is not an error of ours
    return false;
}

// The handle's untimed events and the streams it may own, listed once: create_impl makes them, orbfe_destroy drains the streams
// and destroys both.  A pipe of a pipeline borrows `stream` (and then has no copy streams) and possibly `side`.
struct OwnedStream {
    hipStream_t *s;
    bool own;
};
static std::vector<OwnedStream> handle_streams(orbfe_handle *h)
{
    return {{&h->stream, h->own_stream}, {&h->side, h->own_side}, {&h->s_in, h->own_stream}, {&h->s_out, h->own_stream}};
}
static std::vector<hipEvent_t *> handle_events(orbfe_handle *h)
{
    return {&h->ev_last, &h->ev_fork, &h->ev_join, &h->ev_in[0], &h->ev_cmp[0], &h->ev_out[0], &h->ev_in[1], &h->ev_cmp[1], &h->ev_out[1],
            &h->ev_fork2, &h->ev_auto};
}

// The plan of a w x ht frame (orbfe_plan.hip builds it on the host), uploaded and committed to the handle.
static orbfe_status build_plan(orbfe_handle *h, int w, int ht)
{
    if (h->plan_valid && h->plan.w == w && h->plan.h == ht) return ORBFE_OK;
    OrbPlanTables T;
    const orbfe_status s = orb_plan_build(h->pin, w, ht, &T);
    if (s != ORBFE_OK) return s;
    const struct { DevBuf *buf; const void *p; size_t count, elem; } up[] = {
        {&h->d_plan, &T.plan, 1, sizeof(OrbPlan)},
        {&h->d_tabs, T.tabs.data(), T.tabs.size(), sizeof(OrbTab)},
        {&h->d_flanes, T.flanes.data(), T.flanes.size(), sizeof(OrbLane)},
        {&h->d_flanes_c, T.clanes.data(), T.clanes.size(), sizeof(OrbLane)},
        {&h->d_blanes, T.blanes.data(), T.blanes.size(), sizeof(OrbLane)}};
    for (const auto &u : up) ORBFE_HIP(u.buf->ensure(std::max<size_t>(u.count, 1) * u.elem));
    // synchronous copies: plans change rarely (frame size change), never inside the timed region.  Earlier batches may
    // still be in flight on the handle's stream or on the caller's stream of the previous device call: both are drained
    // before the plan tables they read are overwritten.
    ORBFE_HIP(hipStreamSynchronize(h->stream));
    ORBFE_HIP(wait_last_call(h));
    for (const auto &u : up)
        if (u.count) ORBFE_HIP(hipMemcpy(u.buf->p, u.p, u.count * u.elem, hipMemcpyHostToDevice));
    ORBFE_HIP(orbk_prepare_octree(T.plan.node_cap, T.plan.max_nini, T.plan.w, T.plan.h, T.plan.max_ncells));
    h->plan = T.plan;
    h->fast_row_steps = T.fast_row_steps;
    h->plan_valid = true;
    return ORBFE_OK;
}

static orbfe_status ensure_batch_buffers(orbfe_handle *h, int nframes)
{
    const OrbPlan &P = h->plan;
    const size_t B = (size_t)nframes;
    if (B * (size_t)P.pyr_frame_bytes > h->d_pyr.bytes || B * (size_t)P.keys_per_frame * sizeof(uint2) > h->d_skeys.bytes) {
        // a block is about to be re-allocated: nothing may still be reading the old one
        ORBFE_HIP(hipStreamSynchronize(h->stream));
        ORBFE_HIP(wait_last_call(h));
    }
    ORBFE_HIP(h->d_pyr.ensure(B * (size_t)P.pyr_frame_bytes));
    ORBFE_HIP(h->d_blur.ensure(B * (size_t)P.pyr_frame_bytes));
    ORBFE_HIP(h->d_skeys.ensure(B * (size_t)P.keys_per_frame * sizeof(uint2)));
    // survivor counts and cell flags are zeroed before every FAST pass: one block (counts | flags of the largest batch), so
    // that one memset clears both -- a call with fewer frames passes the flags' offset for ITS frame count (run_batch)
    ORBFE_HIP(h->d_scount.ensure(B * P.nlevels * ORBFE_NK_STRIDE * sizeof(int32_t) +
                                 B * P.nlevels * (size_t)((P.max_ncells + 31) / 32) * sizeof(uint32_t)));
    ORBFE_HIP(h->d_knode.ensure(B * (size_t)P.keys_per_frame * sizeof(uint16_t)));
    ORBFE_HIP(h->d_qtbox.ensure(B * (size_t)P.nlevels * orbk_octree_box_bytes(P.node_cap)));  // deep quadtrees only
    if (orbk_octree_lds_bytes(P.node_cap, std::max(1, P.max_nini), P.w, P.h, P.max_ncells) > (size_t)ORBFE_LDS_MAX)
        ORBFE_HIP(h->d_qtnodes.ensure(B * (size_t)P.nlevels * orbk_octree_node_bytes(P.node_cap)));  // quadtrees beyond the LDS
    ORBFE_HIP(h->d_sel.ensure(B * (size_t)P.sel_per_frame * sizeof(uint32_t)));
    ORBFE_HIP(h->d_nsel.ensure(B * P.nlevels * sizeof(int32_t)));
    ORBFE_HIP(h->d_nkeys.ensure(B * P.nlevels * ORBFE_NK_STRIDE * sizeof(int32_t)));
    if (!h->d_misc.p) {
        ORBFE_HIP(h->d_misc.ensure(sizeof(OrbMisc)));
        ORBFE_HIP(hipMemset(h->d_misc.p, 0, sizeof(OrbMisc)));
    }
    return ORBFE_OK;
}

// reads and clears the sticky overflow word; the stream of the last batched call is drained first
static orbfe_status read_overflow(orbfe_handle *h, int32_t *flags)
{
    *flags = 0;
    if (!h->d_misc.p) return ORBFE_OK;
    ORBFE_HIP(wait_last_call(h));
    ORBFE_HIP(hipMemcpy(flags, &misc_block(h)->overflow, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*flags) ORBFE_HIP(hipMemset(&misc_block(h)->overflow, 0, sizeof(int32_t)));
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// create / destroy / getters
// ---------------------------------------------------------------------------------------------------
static orbfe_status create_impl(const orbfe_params *p, hipStream_t borrowed, hipStream_t borrowed_side, bool borrow, orbfe_handle **out);
extern "C" orbfe_status orbfe_create(const orbfe_params *p, orbfe_handle **out) { return create_impl(p, nullptr, nullptr, false, out); }
// A handle for a pipe of orbfe_pipeline: `st` (the pipe's stream) serves as the handle's own stream and stays the pipeline's;
// the copy streams of the host entry points are not created (orbfe_extract / orbfe_extract_batch answer ORBFE_ERR_STATE).  Every
// stream a process creates is multiplexed onto a few hardware queues: a pipeline of 12 pipes made 74 of them this way, 26 now.
orbfe_status orbfe_internal_create_on_stream(const orbfe_params *p, void *st, void *side, orbfe_handle **out)
{
    return create_impl(p, (hipStream_t)st, (hipStream_t)side, true, out);
}

// The side stream of a pipe's handle from its next call on (null: none).  The pipeline's device and host entry points plan their
// streams apart (orbfe_pipe_plan.h) and hand each call's side stream in; a call joins its blur before it returns, so nothing of
// the handle is left on the stream it gives up.
orbfe_status orbfe_internal_set_side_stream(orbfe_handle *h, void *side)
{
    if (!h || h->own_side) return ORBFE_ERR_ARG;
    h->side = (hipStream_t)side;
    return ORBFE_OK;
}

static orbfe_status create_impl(const orbfe_params *p, hipStream_t borrowed, hipStream_t borrowed_side, bool borrow, orbfe_handle **out)
{
    if (!p || !out) { orbfe_set_error("null argument"); return ORBFE_ERR_ARG; }
    *out = nullptr;
    OrbPlanIn pin;
    float sigma2[ORBFE_MAX_LEVELS] = {0}, inv_sigma2[ORBFE_MAX_LEVELS] = {0};
    const orbfe_status cs = orb_ctor_tables(p, &pin, sigma2, inv_sigma2);
    if (cs != ORBFE_OK) return cs;
    int dev = p->device;
    const orbfe_status rs = orb_resolve_device(&dev);
    if (rs != ORBFE_OK) return rs;

    orbfe_handle *h = new (std::nothrow) orbfe_handle();
    if (!h) return ORBFE_ERR_NOMEM;
    h->prm = *p;
    h->device = dev;
    DeviceGuard g(dev);
    h->pin = pin;
    memcpy(h->sigma2, sigma2, sizeof(sigma2));
    memcpy(h->inv_sigma2, inv_sigma2, sizeof(inv_sigma2));

    auto fail = [&](orbfe_status s) {
        orbfe_destroy(h);
        return s;
    };
    if (borrow) {
        h->stream = borrowed;
        h->own_stream = false;
        h->side = borrowed_side;   // null: the pipeline has no queue to spare for a side stream, the blur runs in `st` (overlap 0)
        h->own_side = false;
    }
    for (int r = 0; r < ORBFE_PROF_RING; ++r)
        for (int i = 0; i < ORBFE_EV_N; ++i) h->ev[r][i] = nullptr;
    h->ev_ok = true;
    bool made = true;
    for (const OwnedStream &s : handle_streams(h))
        if (s.own) made = made && hipStreamCreateWithFlags(s.s, hipStreamNonBlocking) == hipSuccess;
    for (int r = 0; r < ORBFE_PROF_RING; ++r)
        for (int i = 0; i < ORBFE_EV_N; ++i) made = made && hipEventCreate(&h->ev[r][i]) == hipSuccess;
    for (hipEvent_t *e : handle_events(h)) made = made && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!made || h->h_auto.ensure(64) != hipSuccess) {
        orbfe_set_error("stream / event creation failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(ORBFE_ERR_HIP);
    }
#ifdef ORBFE_DEVELOPER
    // a developer build (-DORBFE_DEVELOPER; tools/ab_build.sh) also honours the A/B knobs from the environment, under the
    // names of the options (ORBFE_OPT_OVERLAP -> $ORBFE_OVERLAP ...); the release library takes them through orbfe_set_option only
    {
        static const struct { const char *env; int opt; } kEnv[] = {
            {"ORBFE_OVERLAP", ORBFE_OPT_OVERLAP}, {"ORBFE_ROWS", ORBFE_OPT_ROWS}, {"ORBFE_ROWS_FAST", ORBFE_OPT_ROWS_FAST},
            {"ORBFE_ROWS_BLUR", ORBFE_OPT_ROWS_BLUR}, {"ORBFE_BLUR_PIECES", ORBFE_OPT_BLUR_PIECES},
            {"ORBFE_BLUR_UPDOWN", ORBFE_OPT_BLUR_UPDOWN}, {"ORBFE_PW_ROWS", ORBFE_OPT_PYR_ROWS},
            {"ORBFE_DEBUG", ORBFE_OPT_DEBUG}};
        for (const auto &k : kEnv)
            if (const char *e = getenv(k.env)) (void)orbfe_set_option(h, k.opt, atoi(e));
        if (const char *e = getenv("ORBFE_QT")) {
            int v[3];
            if (sscanf(e, "%d,%d,%d", &v[0], &v[1], &v[2]) == 3)
                for (int i = 0; i < 3; ++i) (void)orbfe_set_option(h, ORBFE_OPT_QT_THREADS_0 + i, v[i]);
        }
    }
#endif
    int umax[16];
    orb_host_umax(umax);
    if (orbk_upload_constants(umax) != hipSuccess) {
        orbfe_set_error("constant upload failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(ORBFE_ERR_HIP);
    }
    orbfe_status s = build_plan(h, p->max_width, p->max_height);
    if (s != ORBFE_OK) return fail(s);
    s = ensure_batch_buffers(h, p->max_batch);
    if (s != ORBFE_OK) return fail(s);
    *out = h;
    return ORBFE_OK;
}

extern "C" void orbfe_destroy(orbfe_handle *h)
{
    if (!h) return;
    DeviceGuard g(h->device);
    // nothing of this handle may still be running when its buffers go: the caller's last stream, the side stream of the
    // blur, the host pipeline's copy streams
    if (h->last_stream_valid && h->ev_last) (void)hipEventSynchronize(h->ev_last);
    for (const OwnedStream &s : handle_streams(h))
        if (*s.s) (void)hipStreamSynchronize(*s.s);
    DevBuf *bufs[] = {&h->d_plan, &h->d_tabs, &h->d_flanes, &h->d_flanes_c, &h->d_blanes, &h->d_pyr, &h->d_blur, &h->d_skeys, &h->d_scount, &h->d_knode, &h->d_qtbox, &h->d_qtnodes, &h->d_sel, &h->d_nsel, &h->d_nkeys, &h->d_pad,
                      &h->d_stage[0], &h->d_okps[0], &h->d_odesc[0], &h->d_on[0], &h->d_stage[1], &h->d_okps[1], &h->d_odesc[1], &h->d_on[1]};
    for (DevBuf *b : bufs) b->release();
    h->d_misc.release();
    PinBuf *pins[] = {&h->h_stage[0], &h->h_okps[0], &h->h_odesc[0], &h->h_on[0], &h->h_stage[1], &h->h_okps[1], &h->h_odesc[1], &h->h_on[1]};
    for (PinBuf *b : pins) b->release();
    h->h_ovf.release();
    if (h->ev_ok)
        for (int r = 0; r < ORBFE_PROF_RING; ++r)
            for (int i = 0; i < ORBFE_EV_N; ++i)
                if (h->ev[r][i]) (void)hipEventDestroy(h->ev[r][i]);
    for (hipEvent_t *e : handle_events(h))
        if (*e) (void)hipEventDestroy(*e);
    h->h_auto.release();
    for (const OwnedStream &s : handle_streams(h))
        if (*s.s && s.own) (void)hipStreamDestroy(*s.s);
    delete h;
}

extern "C" orbfe_status orbfe_get_scales(const orbfe_handle *h, float *scale, float *inv_scale, float *sigma2,
                                         float *inv_sigma2)
{
    if (!h) return ORBFE_ERR_ARG;
    for (int i = 0; i < h->prm.nlevels; ++i) {
        if (scale) scale[i] = h->pin.scale[i];
        if (inv_scale) inv_scale[i] = h->pin.inv_scale[i];
        if (sigma2) sigma2[i] = h->sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = h->inv_sigma2[i];
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_features_per_level(const orbfe_handle *h, int32_t *out)
{
    if (!h || !out) return ORBFE_ERR_ARG;
    for (int i = 0; i < h->prm.nlevels; ++i) out[i] = h->pin.feat[i];
    return ORBFE_OK;
}

extern "C" int32_t orbfe_keypoint_capacity(const orbfe_handle *h)
{
    if (!h) return 0;
    int total = 0;
    for (int l = 0; l < h->plan.nlevels; ++l) total += h->plan.lv[l].sel_cap;
    return orb_align_up(total, 64);
}

extern "C" orbfe_status orbfe_set_profiling(orbfe_handle *h, int32_t enable)
{
    if (!h) return ORBFE_ERR_ARG;
    h->profiling = enable != 0;
    h->prof_calls = 0;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_stage_ms(orbfe_handle *h, float ms[ORBFE_T_COUNT])
{
    if (!h || !ms) return ORBFE_ERR_ARG;
    if (h->prof_calls == 0) { orbfe_set_error("no profiled call yet"); return ORBFE_ERR_STATE; }
    DeviceGuard g(h->device);
    const int ncalls = std::min(h->prof_calls, ORBFE_PROF_RING);
    double acc[ORBFE_T_COUNT] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < ncalls; ++c) {
        hipEvent_t *e = h->ev[(h->prof_calls - 1 - c) % ORBFE_PROF_RING];
        ORBFE_HIP(hipEventSynchronize(e[5]));
        ORBFE_HIP(hipEventSynchronize(e[7]));
        static const int from[ORBFE_T_COUNT] = {0, 1, 2, 6, 4, 0}, to[ORBFE_T_COUNT] = {1, 2, 3, 7, 5, 5};
        for (int i = 0; i < ORBFE_T_COUNT; ++i) {
            float t;
            ORBFE_HIP(hipEventElapsedTime(&t, e[from[i]], e[to[i]]));
            acc[i] += t;
        }
    }
    for (int i = 0; i < ORBFE_T_COUNT; ++i) ms[i] = (float)(acc[i] / ncalls);
    return ORBFE_OK;
}

extern "C" void *orbfe_get_stream(orbfe_handle *h) { return h ? (void *)h->stream : nullptr; }

extern "C" orbfe_status orbfe_synchronize(orbfe_handle *h)
{
    if (!h) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    ORBFE_HIP(hipStreamSynchronize(h->stream));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_work_counts(const orbfe_handle *h, int64_t out[2])
{
    if (!h || !out) return ORBFE_ERR_ARG;
    out[0] = h->fast_row_steps;
    out[1] = h->plan.nfwaves;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_overflow(orbfe_handle *h, int32_t *flags)
{
    if (!h || !flags) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    return read_overflow(h, flags);
}

// developer builds (-DQT_PROFILE): the whole OrbMisc block (1024 bytes); reset != 0 clears the quadtree's phase sums
extern "C" orbfe_status orbfe_internal_read_misc(orbfe_handle *h, void *out, int32_t reset)
{
    if (!h || !out || !h->d_misc.p) return ORBFE_ERR_ARG;
    DeviceGuard g(h->device);
    ORBFE_HIP(wait_last_call(h));
    ORBFE_HIP(hipMemcpy(out, h->d_misc.p, sizeof(OrbMisc), hipMemcpyDeviceToHost));
    if (reset) ORBFE_HIP(hipMemset(misc_block(h)->qt_phase, 0, sizeof(OrbMisc::qt_phase)));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_set_option(orbfe_handle *h, int32_t option, int32_t value)
{
    if (!h) return ORBFE_ERR_ARG;
    auto in = [&](int lo, int hi) { return value >= lo && value <= hi; };
    bool replan = false;
    switch (option) {
    case ORBFE_OPT_OVERLAP: if (!in(-1, 2)) return ORBFE_ERR_ARG; h->overlap = value; break;
    case ORBFE_OPT_ROWS: if (value && !in(8, 512)) return ORBFE_ERR_ARG; h->pin.opt_rows = value; replan = true; break;
    case ORBFE_OPT_ROWS_FAST: if (value && !in(8, 512)) return ORBFE_ERR_ARG; h->pin.opt_rows_fast = value; replan = true; break;
    case ORBFE_OPT_ROWS_BLUR: if (value && !in(8, 512)) return ORBFE_ERR_ARG; h->pin.opt_rows_blur = value; replan = true; break;
    case ORBFE_OPT_BLUR_PIECES: if (!in(0, 1)) return ORBFE_ERR_ARG; h->pin.opt_blur_pieces = value; replan = true; break;
    case ORBFE_OPT_BLUR_UPDOWN: if (!in(0, 2)) return ORBFE_ERR_ARG; h->pin.opt_blur_updown = value; replan = true; break;
    case ORBFE_OPT_PYR_ROWS: if (value && !in(2, ORBFE_PW_ROWS)) return ORBFE_ERR_ARG; h->kopts.pw_rows = value; break;
    case ORBFE_OPT_QT_THREADS_0:
    case ORBFE_OPT_QT_THREADS_1:
    case ORBFE_OPT_QT_THREADS_2:
        if (value && (!in(64, 512) || value % 64)) return ORBFE_ERR_ARG;
        h->kopts.qt[option - ORBFE_OPT_QT_THREADS_0] = value;
        break;
    case ORBFE_OPT_DEBUG:
#ifdef ORBFE_DEVELOPER
        if (value != 0 && value != 50 && value != 51 && value != 60) return ORBFE_ERR_ARG;   // 60: timing-only, FAST without arcs
#else
        if (value != 0 && value != 50 && value != 51) return ORBFE_ERR_ARG;
#endif
        h->pin.opt_debug = value;
        replan = true;
        break;
    case ORBFE_OPT_BLUR_ROUNDING: if (!in(0, 1)) return ORBFE_ERR_ARG; h->pin.blur_rounding = value; replan = true; break;
    case ORBFE_OPT_REUSE_IDENTICAL_INPUT: if (!in(0, 1)) return ORBFE_ERR_ARG; h->opt_reuse = value; break;
    case 12: case 13: case 14: case 15:   // the numbers of four retired kernel variants (profiles/HISTORY.md); "off" is still accepted
        if (value == 0) break;
        orbfe_set_error("option %d is retired: the kernel variant it selected has been removed", option);
        return ORBFE_ERR_ARG;
    default: orbfe_set_error("unknown option %d", option); return ORBFE_ERR_ARG;
    }
    if (replan) h->plan_valid = false;   // rebuilt (behind the handle's outstanding work) by the next call
    h->reuse_valid = false;
    return ORBFE_OK;
}

extern "C" int32_t orbfe_last_call_reused(const orbfe_handle *h) { return h && h->last_reused ? 1 : 0; }

extern "C" orbfe_status orbfe_set_fast_mode(orbfe_handle *h, int32_t mode, int32_t collect_stats)
{
    if (!h || mode < 0 || mode > 3) return ORBFE_ERR_ARG;
    h->fast_mode = mode;
    h->fast_stats = collect_stats != 0;
    h->fauto = OrbFastAuto();
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_get_fast_stats(orbfe_handle *h, uint64_t out[3], int32_t reset)
{
    if (!h || !out) return ORBFE_ERR_ARG;
    out[0] = out[1] = out[2] = 0;
    if (!h->d_misc.p) return ORBFE_OK;
    DeviceGuard g(h->device);
    ORBFE_HIP(wait_last_call(h));
    if (h->fast_mode == 3) {   // auto: the counters belong to the mode selection; report its last completed probe
        (void)collect_auto_probe(h);
        for (int i = 0; i < 3; ++i) out[i] = h->auto_last[i];
        return ORBFE_OK;
    }
    ORBFE_HIP(hipMemcpy(out, misc_block(h)->fast_stat, sizeof(OrbMisc::fast_stat), hipMemcpyDeviceToHost));
    if (reset) ORBFE_HIP(hipMemset(misc_block(h)->fast_stat, 0, sizeof(OrbMisc::fast_stat)));
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// the batched device path (everything else funnels into this)
// ---------------------------------------------------------------------------------------------------
// what the caller of a batched call hands in (orbfe_extract_batch_device's arguments)
struct BatchCall {
    const uint8_t *d_gray;
    int nframes, w, ht, stride;
    size_t frame_stride;
    orbfe_keypoint *d_kps;
    uint8_t *d_desc;
    int cap;
    int32_t *d_n_out;
};

// the launchers' view of a call: the handle's plan tables and scratch blocks, the caller's frames and output arrays
static OrbLaunch launch_args(orbfe_handle *h, const BatchCall &c)
{
    const OrbPlan &P = h->plan;
    OrbLaunch a;
    a.opts = h->kopts;
    a.h_plan = &h->plan;
    a.d_plan = (const OrbPlan *)h->d_plan.p;
    a.d_tabs = (const OrbTab *)h->d_tabs.p;
    a.d_flanes = (const OrbLane *)h->d_flanes.p;
    a.d_flanes_c = (const OrbLane *)h->d_flanes_c.p;
    a.d_blanes = (const OrbLane *)h->d_blanes.p;
    a.nframes = c.nframes;
    a.d_gray = c.d_gray;
    a.gray_fstride = (int64_t)c.frame_stride;
    a.gray_pitch = c.stride;
    a.d_pyr = (uint8_t *)h->d_pyr.p;
    a.d_blur = (uint8_t *)h->d_blur.p;
    a.pyr_fstride = P.pyr_frame_bytes;
    a.d_skeys = (uint2 *)h->d_skeys.p;
    a.d_scount = (int32_t *)h->d_scount.p;
    a.d_cflag = (uint32_t *)(a.d_scount + (size_t)c.nframes * P.nlevels * ORBFE_NK_STRIDE);  // right behind this call's counts
    a.cf_words = (P.max_ncells + 31) / 32;
    a.d_knode = (uint16_t *)h->d_knode.p;
    a.d_qtbox = (int16_t *)h->d_qtbox.p;
    a.qtbox_stride = (int32_t)(orbk_octree_box_bytes(P.node_cap) / sizeof(int16_t));
    a.d_qtnodes = (char *)h->d_qtnodes.p;
    a.qtnodes_stride = (int64_t)orbk_octree_node_bytes(P.node_cap);
    a.d_sel = (uint32_t *)h->d_sel.p;
    a.d_nsel = (int32_t *)h->d_nsel.p;
    a.d_nkeys = (int32_t *)h->d_nkeys.p;
    a.d_kps = c.d_kps;
    a.d_desc = c.d_desc;
    a.cap = c.cap;
    a.d_n_out = c.d_n_out;
    a.d_ovf = &misc_block(h)->overflow;
    a.fast_sparse = 0;     // the FAST form and its counters: run_batch
    a.d_fstat = nullptr;
    return a;
}

// Behind the FAST launch of a probing call, on its stream: the sampled counters -> pinned host memory, cleared for the next
// probe; a later call looks at them (collect_auto_probe).
static orbfe_status hand_off_auto_probe(orbfe_handle *h, hipStream_t st)
{
    ORBFE_HIP(hipMemcpyAsync(h->h_auto.p, misc_block(h)->fast_stat, sizeof(OrbMisc::fast_stat), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemsetAsync(misc_block(h)->fast_stat, 0, sizeof(OrbMisc::fast_stat), st));
    ORBFE_HIP(hipEventRecord(h->ev_auto, st));
    h->auto_pending = true;
    return ORBFE_OK;
}

// The stages of a call on a stream per stage group (orbfe_internal_extract_batch_lanes): lane[0] pyramid, lane[1] FAST, lane[2]
// quadtree + descriptor, lane[3] blur.  pyramid -> FAST and pyramid -> blur (ev_fork), FAST -> quadtree (ev_fork2), blur ->
// descriptor (ev_join); the descriptor is the last launch on the tail stream lane[2], so that the next call of this handle starts
// its pyramid behind everything of this one.  The clear of FAST's survivor counts and cell flags runs on the pyramid's stream, so
// that the FAST stream carries FAST launches and nothing else: run_batch has made lane[0] wait for ev_last of the handle's previous
// call, behind which the last readers of those words (quadtree, taps) lie, and FAST waits for ev_fork, which follows the clear.
static orbfe_status enqueue_lanes(orbfe_handle *h, const OrbLaunch &a, bool auto_probe, const hipStream_t *lane)
{
    const hipStream_t sp = lane[0], sf = lane[1], st = lane[2], sb = lane[3];
    ORBFE_HIP(orbk_launch_pyramid(a, sp));
    ORBFE_HIP(orbk_clear_fast(a, sp));
    ORBFE_HIP(hipEventRecord(h->ev_fork, sp));
    ORBFE_HIP(hipStreamWaitEvent(sf, h->ev_fork, 0));
    if (sb != sp) ORBFE_HIP(hipStreamWaitEvent(sb, h->ev_fork, 0));
    ORBFE_HIP(orbk_launch_fast(a, sf));
    if (auto_probe) {
        const orbfe_status s = hand_off_auto_probe(h, sf);
        if (s != ORBFE_OK) return s;
    }
    ORBFE_HIP(hipEventRecord(h->ev_fork2, sf));
    ORBFE_HIP(orbk_launch_blur(a, sb));
    ORBFE_HIP(hipEventRecord(h->ev_join, sb));
    ORBFE_HIP(hipStreamWaitEvent(st, h->ev_fork2, 0));
    ORBFE_HIP(orbk_launch_octree(a, st));
    if (sb != st) ORBFE_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
    ORBFE_HIP(orbk_launch_describe(a, st));
    return ORBFE_OK;
}

// The stages of a call on one stream, the blur possibly on the handle's side stream (handle.overlap: 1 from before FAST, 2 beside
// the quadtree, 0 in line); ev (null: not profiled): the marks 1 .. 4, 6, 7 of ORBFE_EV_N.
static orbfe_status enqueue_single_stream(orbfe_handle *h, const OrbLaunch &a, bool auto_probe, hipStream_t st, hipEvent_t *ev)
{
    int ov = h->overlap >= 0 ? h->overlap : (a.nframes >= 128 ? 2 : 0);
    if (!h->side) ov = 0;   // a pipe of a pipeline that fits its streams to the hardware queues and has none left for the blur
    auto fork_blur = [&]() -> hipError_t {
        hipError_t e = hipEventRecord(h->ev_fork, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->side, h->ev_fork, 0);
        if (e == hipSuccess && ev) e = hipEventRecord(ev[6], h->side);
        if (e == hipSuccess) e = orbk_launch_blur(a, h->side);
        if (e == hipSuccess && ev) e = hipEventRecord(ev[7], h->side);
        if (e == hipSuccess) e = hipEventRecord(h->ev_join, h->side);
        return e;
    };
    ORBFE_HIP(orbk_launch_pyramid(a, st));
    if (ev) ORBFE_HIP(hipEventRecord(ev[1], st));
    if (ov == 1) ORBFE_HIP(fork_blur());
    ORBFE_HIP(orbk_clear_fast(a, st));
    ORBFE_HIP(orbk_launch_fast(a, st));
    if (auto_probe) {
        const orbfe_status s = hand_off_auto_probe(h, st);
        if (s != ORBFE_OK) return s;
    }
    if (ev) ORBFE_HIP(hipEventRecord(ev[2], st));
    if (ov == 2) ORBFE_HIP(fork_blur());
    ORBFE_HIP(orbk_launch_octree(a, st));
    if (ev) ORBFE_HIP(hipEventRecord(ev[3], st));
    if (ov == 0) {
        if (ev) ORBFE_HIP(hipEventRecord(ev[6], st));
        ORBFE_HIP(orbk_launch_blur(a, st));
        if (ev) ORBFE_HIP(hipEventRecord(ev[7], st));
    } else {
        ORBFE_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
    }
    if (ev) ORBFE_HIP(hipEventRecord(ev[4], st));
    ORBFE_HIP(orbk_launch_describe(a, st));
    return ORBFE_OK;
}

// `lane` (null: everything on `st`, the blur possibly on the handle's side stream): one stream per stage group; `st` is then the
// tail stream lane[2].
static orbfe_status run_batch(orbfe_handle *h, const BatchCall &c, hipStream_t st, const hipStream_t *lane = nullptr)
{
    if (c.w > h->prm.max_width || c.ht > h->prm.max_height) {
        orbfe_set_error("frame %dx%d larger than planned %dx%d", c.w, c.ht, h->prm.max_width, h->prm.max_height);
        return ORBFE_ERR_SIZE;
    }
    h->reuse_valid = false;   // the scratch blocks and taps belong to this call from here on
    h->last_reused = false;
    orbfe_status s = build_plan(h, c.w, c.ht);
    if (s != ORBFE_OK) return s;
    s = ensure_batch_buffers(h, c.nframes);
    if (s != ORBFE_OK) return s;
    OrbLaunch a = launch_args(h, c);
    // FAST form of this call; auto (3, the default): orbfe_fast_auto.h, fed with the probe answers that have arrived
    OrbFastChoice fast = {h->fast_mode, false};
    if (h->fast_mode == 3) {
        const int64_t row_steps = (int64_t)c.nframes * h->fast_row_steps;
        if (!orb_fast_auto_small(row_steps) && collect_auto_probe(h)) orb_fast_auto_answer(h->fauto, h->auto_last);
        fast = orb_fast_auto_choose(h->fauto, row_steps, h->auto_pending);
    }
    a.fast_sparse = fast.form;
    a.d_fstat = (h->fast_stats || fast.probe) ? (unsigned long long *)misc_block(h)->fast_stat : nullptr;
    // every call of a handle uses the same scratch blocks (pyramid, blur, survivor lists, selections): a call on another
    // stream than its predecessor's waits, at stream level, for that predecessor to finish
    const hipStream_t first = lane ? lane[0] : st;   // the stream of the first launch, the pyramid's
    if (h->last_stream_valid && h->last_stream != first) ORBFE_HIP(hipStreamWaitEvent(first, h->ev_last, 0));
    // (a call in lanes is not profiled: the marks of one call would lie on four streams, between other sub-batches' kernels)
    hipEvent_t *ev = (h->profiling && !lane) ? h->ev[h->prof_calls % ORBFE_PROF_RING] : nullptr;
    if (ev) ORBFE_HIP(hipEventRecord(ev[0], st));
    s = lane ? enqueue_lanes(h, a, fast.probe, lane) : enqueue_single_stream(h, a, fast.probe, st, ev);
    if (s != ORBFE_OK) return s;
    // common tail: profiling bookkeeping, the "last call" state of the handle
    if (ev) {
        ORBFE_HIP(hipEventRecord(ev[5], st));
        h->prof_calls++;
    }
    ORBFE_HIP(hipEventRecord(h->ev_last, st));
    h->last_stream = st;
    h->last_stream_valid = true;
    h->last_gray = c.d_gray;
    h->last_gray_fstride = (int64_t)c.frame_stride;
    h->last_gray_pitch = c.stride;
    h->last_nframes = c.nframes;
    return ORBFE_OK;
}

// Test hook (not in include/orbfe.h; tests/test_fast_auto.py): the automatic FAST mode of a fresh handle over n calls, without a
// device.  Call i has row_steps[i] wave row steps and sees a probe outstanding iff pending[i]; has_answer[i] != 0: the counters
// answer[3 * i ..] of a probe arrived before it (a small call leaves them for the next large one, as collect_auto_probe is not
// asked then).  Out: form[i] (0 dense, 2 lane-compacting) and probe[i].
extern "C" orbfe_status orbfe_internal_fast_auto(int32_t n, const int64_t *row_steps, const uint8_t *pending, const uint8_t *has_answer,
                                                 const uint64_t *answer, int32_t *form, uint8_t *probe)
{
    if (n < 0 || !row_steps || !pending || !form || !probe || (has_answer && !answer)) return ORBFE_ERR_ARG;
    OrbFastAuto st;
    const uint64_t *waiting = nullptr;
    for (int i = 0; i < n; ++i) {
        if (has_answer && has_answer[i]) waiting = answer + 3 * (size_t)i;
        if (waiting && !orb_fast_auto_small(row_steps[i])) {
            orb_fast_auto_answer(st, waiting);
            waiting = nullptr;
        }
        const OrbFastChoice c = orb_fast_auto_choose(st, row_steps[i], pending[i] != 0);
        form[i] = c.form;
        probe[i] = c.probe ? 1 : 0;
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_extract_batch_device(orbfe_handle *h, const uint8_t *d_gray, int32_t nframes,
                                                   int32_t w, int32_t ht, int32_t stride, size_t frame_stride,
                                                   orbfe_keypoint *d_kps, uint8_t *d_desc, int32_t cap,
                                                   int32_t *d_n_out, void *stream)
{
    if (!h || !d_gray || !d_kps || !d_desc || !d_n_out || nframes < 1 || w < 1 || ht < 1 || stride < w || cap < 1 ||
        frame_stride < (size_t)stride * (size_t)(ht - 1) + (size_t)w) {
        orbfe_set_error("bad argument to orbfe_extract_batch_device");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(h->device);
    return run_batch(h, BatchCall{d_gray, nframes, w, ht, stride, frame_stride, d_kps, d_desc, cap, d_n_out}, (hipStream_t)stream);
}

// orbfe_extract_batch_device with a stream per stage group, for the pipeline's lanes (orbfe_pipe_plan.h): lane[0] pyramid,
// lane[1] FAST, lane[2] quadtree + descriptor, lane[3] blur (may be lane[0] or lane[2]).  The call has finished when lane[2] has.
orbfe_status orbfe_internal_extract_batch_lanes(orbfe_handle *h, const uint8_t *d_gray, int32_t nframes, int32_t w, int32_t ht,
                                                int32_t stride, size_t frame_stride, orbfe_keypoint *d_kps, uint8_t *d_desc,
                                                int32_t cap, int32_t *d_n_out, void *const lane[4])
{
    if (!h || !d_gray || !d_kps || !d_desc || !d_n_out || nframes < 1 || w < 1 || ht < 1 || stride < w || cap < 1 ||
        frame_stride < (size_t)stride * (size_t)(ht - 1) + (size_t)w || !lane || lane[0] == lane[1] || lane[1] == lane[2] ||
        lane[0] == lane[2] || lane[3] == lane[1]) {
        orbfe_set_error("bad argument to orbfe_internal_extract_batch_lanes");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(h->device);
    const hipStream_t ls[4] = {(hipStream_t)lane[0], (hipStream_t)lane[1], (hipStream_t)lane[2], (hipStream_t)lane[3]};
    return run_batch(h, BatchCall{d_gray, nframes, w, ht, stride, frame_stride, d_kps, d_desc, cap, d_n_out}, ls[2], ls);
}

// host buffers, in chunks of max_batch frames.  A single chunk (the online case: one frame) is a plain H2D -> kernels ->
// D2H sequence on the handle's stream.  Several chunks run as a pipeline over two buffer sets and three streams: while
// the kernels of chunk i run, chunk i+1 is copied in (s_in) and chunk i-1 is copied out (s_out) and unpacked by the host.
// Frames in pinned (page-locked / hipHostRegister'ed) memory with stride == w are copied straight from the caller's
// buffers; pageable frames are first gathered into the pinned staging set (the host memcpy then overlaps the GPU work).
static bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // plain malloc'ed memory: "invalid value", not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

static orbfe_status extract_host(orbfe_handle *h, const uint8_t *const *grays, int nframes, int w, int ht,
                                 int stride, orbfe_keypoint *kps, uint8_t *desc, int cap, int32_t *n_out)
{
    if (!h->own_stream) {
        orbfe_set_error("this extractor is a pipe of an orbfe_pipeline: use orbfe_pipeline_extract_match for host buffers");
        return ORBFE_ERR_STATE;
    }
    DeviceGuard g(h->device);
    const int chunk_max = h->prm.max_batch;
    const int nchunks = (nframes + chunk_max - 1) / chunk_max;
    // The page-locked probes (hipPointerGetAttributes: an error path for plain malloc'ed memory) cost more than they can
    // save on the online single-frame call, which goes through the handle's own pinned staging either way.
    const bool probe = nframes > 1;
    const bool direct = probe && stride == w && is_pinned_host(grays[0]) && is_pinned_host(grays[nframes - 1]);
    // pinned output arrays receive the padded device blocks as they are (slots >= n_out[f] zero-filled): no host unpacking
    const bool direct_out = probe && is_pinned_host(kps) && is_pinned_host(desc) && is_pinned_host(n_out);
    const int pitch = direct ? w : orb_align_up(w, 64);
    const size_t fbytes = (size_t)pitch * ht;
    const int nset = nchunks > 1 ? 2 : 1;
    const size_t nbmax = (size_t)std::min(chunk_max, nframes);
    // Output set k on the device.  When the results go through the handle's pinned staging (the online call), the three
    // arrays are pieces of ONE block -- keypoints | descriptors | counts -- so that they come back in one D2H copy instead
    // of three (each copy is a ~7 us round trip on the stream of a call that takes 0.25 ms in all).
    const size_t kb = orb_align256(sizeof(orbfe_keypoint) * (size_t)cap * nbmax);
    const size_t db = orb_align256((size_t)32 * cap * nbmax);
    const size_t cb = orb_align256(sizeof(int32_t) * nbmax);
    // ORBFE_OPT_REUSE_IDENTICAL_INPUT: perfect/src/Tracking.cc:685 and :716 build two Frames from the SAME mImGray with the same
    // extractor (the second with the dynamic-object mask, which operator() ignores): the second extraction is the first one's
    // result.  The previous frame sits in the pinned staging block (pitch-aligned rows) and its results in the pinned result
    // block; one pass of memcmp over the rows decides, and a hit touches neither the link nor the GPU (pyramid, taps and the
    // device-side state of the handle are still those of that frame).  Bit-exact by construction.
    if (h->opt_reuse && nframes == 1 && h->reuse_valid && h->reuse_w == w && h->reuse_h == ht && h->reuse_cap == cap && h->plan_valid) {
        const uint8_t *prev = (const uint8_t *)h->h_stage[0].p, *src = grays[0];
        bool same = true;
        if (stride == w && pitch == w) same = memcmp(prev, src, fbytes) == 0;
        else
            for (int y = 0; y < ht && same; ++y) same = memcmp(prev + (size_t)y * pitch, src + (size_t)y * stride, (size_t)w) == 0;
        if (same) {
            const uint8_t *hb = (const uint8_t *)h->h_okps[0].p;   // keypoints | descriptors | counts of that call
            const int n = ((const int32_t *)(hb + kb + db))[0];
            n_out[0] = n;
            memcpy(kps, hb, sizeof(orbfe_keypoint) * (size_t)n);
            memcpy(desc, hb + kb, (size_t)32 * n);
            h->last_reused = true;
            h->reuse_hits++;
            return ORBFE_OK;
        }
    }
    uint8_t *d_ok[2] = {nullptr, nullptr}, *d_od[2] = {nullptr, nullptr}, *d_oc[2] = {nullptr, nullptr};
    for (int k = 0; k < nset; ++k) {
        if (!direct) ORBFE_HIP(h->h_stage[k].ensure(fbytes * nbmax));
        ORBFE_HIP(h->d_stage[k].ensure(fbytes * nbmax + 64));
        if (direct_out) {
            ORBFE_HIP(h->d_okps[k].ensure(kb));
            ORBFE_HIP(h->d_odesc[k].ensure(db));
            ORBFE_HIP(h->d_on[k].ensure(cb));
            d_ok[k] = (uint8_t *)h->d_okps[k].p; d_od[k] = (uint8_t *)h->d_odesc[k].p; d_oc[k] = (uint8_t *)h->d_on[k].p;
        } else {
            ORBFE_HIP(h->d_okps[k].ensure(kb + db + cb));
            ORBFE_HIP(h->h_okps[k].ensure(kb + db + cb));
            d_ok[k] = (uint8_t *)h->d_okps[k].p; d_od[k] = d_ok[k] + kb; d_oc[k] = d_od[k] + db;
        }
    }
    // size the plan and the per-batch blocks once, before anything is in flight
    if (w > h->prm.max_width || ht > h->prm.max_height) {
        orbfe_set_error("frame %dx%d larger than planned %dx%d", w, ht, h->prm.max_width, h->prm.max_height);
        return ORBFE_ERR_SIZE;
    }
    orbfe_status sp = build_plan(h, w, ht);
    if (sp != ORBFE_OK) return sp;
    sp = ensure_batch_buffers(h, (int)nbmax);
    if (sp != ORBFE_OK) return sp;

    const bool piped = nchunks > 1;
    hipStream_t s_in = piped ? h->s_in : h->stream, s_cmp = h->stream, s_out = piped ? h->s_out : h->stream;
    orbfe_status worst = ORBFE_OK;
    auto drain = [&]() {
        (void)hipStreamSynchronize(h->s_in);
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->s_out);
    };
    // Every early return below leaves copies / kernels in flight that write into the caller's arrays (direct_out) or read
    // its frames (direct): whatever way the pipeline loop is left, the three streams are drained first.
    struct DrainGuard {
        decltype(drain) &fn;
        bool armed = true;
        ~DrainGuard() { if (armed) fn(); }
    } drain_guard{drain};
    auto unpack = [&](int c) -> orbfe_status {  // results of chunk c: wait for its D2H, hand them to the caller
        const int k = c & (nset - 1), f0 = c * chunk_max, nb = std::min(chunk_max, nframes - f0);
        ORBFE_HIP(hipEventSynchronize(h->ev_out[k]));
        if (direct_out) {
            for (int f = 0; f < nb; ++f)
                if (n_out[f0 + f] > cap) worst = ORBFE_ERR_CAP;
            return ORBFE_OK;
        }
        const uint8_t *hb = (const uint8_t *)h->h_okps[k].p;   // keypoints | descriptors | counts
        for (int f = 0; f < nb; ++f) {
            const int n = ((const int32_t *)(hb + kb + db))[f];
            n_out[f0 + f] = n;
            if (n > cap) { worst = ORBFE_ERR_CAP; continue; }
            memcpy(kps + (size_t)(f0 + f) * cap, (const orbfe_keypoint *)hb + (size_t)f * cap, sizeof(orbfe_keypoint) * (size_t)n);
            memcpy(desc + (size_t)(f0 + f) * cap * 32, hb + kb + (size_t)f * cap * 32, (size_t)32 * n);
        }
        return ORBFE_OK;
    };
    for (int c = 0; c < nchunks; ++c) {
        const int k = c & (nset - 1), f0 = c * chunk_max, nb = std::min(chunk_max, nframes - f0);
        if (c >= 2) {  // set k was last used by chunk c-2: collect its results before its buffers are reused
            orbfe_status su = unpack(c - 2);
            if (su != ORBFE_OK) return su;
        }
        // ---- in ----
        if (piped && c >= 2) ORBFE_HIP(hipStreamWaitEvent(s_in, h->ev_cmp[k], 0));  // kernels of chunk c-2 read d_stage[k]
        if (direct) {
            bool contiguous = true;
            for (int f = 1; f < nb && contiguous; ++f) contiguous = grays[f0 + f] == grays[f0] + fbytes * f;
            if (contiguous) {
                ORBFE_HIP(hipMemcpyAsync(h->d_stage[k].p, grays[f0], fbytes * nb, hipMemcpyHostToDevice, s_in));
            } else {
                for (int f = 0; f < nb; ++f)
                    ORBFE_HIP(hipMemcpyAsync((uint8_t *)h->d_stage[k].p + fbytes * f, grays[f0 + f], fbytes, hipMemcpyHostToDevice, s_in));
            }
        } else {
            // h_stage[k] was read by the H2D of chunk c-2, which the kernels of chunk c-2 waited for and whose results
            // were just unpacked: free to overwrite
            for (int f = 0; f < nb; ++f) {
                uint8_t *dst = (uint8_t *)h->h_stage[k].p + fbytes * f;
                const uint8_t *src = grays[f0 + f];
                if (stride == w && pitch == w) memcpy(dst, src, fbytes);
                else
                    for (int y = 0; y < ht; ++y) memcpy(dst + (size_t)y * pitch, src + (size_t)y * stride, (size_t)w);
            }
            ORBFE_HIP(hipMemcpyAsync(h->d_stage[k].p, h->h_stage[k].p, fbytes * nb, hipMemcpyHostToDevice, s_in));
        }
        if (piped) {
            ORBFE_HIP(hipEventRecord(h->ev_in[k], s_in));
            ORBFE_HIP(hipStreamWaitEvent(s_cmp, h->ev_in[k], 0));
            if (c >= 2) ORBFE_HIP(hipStreamWaitEvent(s_cmp, h->ev_out[k], 0));  // D2H of chunk c-2 read the output set k
        }
        // ---- kernels ----
        orbfe_status s = run_batch(h, BatchCall{(const uint8_t *)h->d_stage[k].p, nb, w, ht, pitch, fbytes, (orbfe_keypoint *)d_ok[k], d_od[k], cap,
                                                (int32_t *)d_oc[k]}, s_cmp);
        if (s != ORBFE_OK) return s;
        if (piped) {
            ORBFE_HIP(hipEventRecord(h->ev_cmp[k], s_cmp));
            ORBFE_HIP(hipStreamWaitEvent(s_out, h->ev_cmp[k], 0));
        }
        // ---- out ----
        if (direct_out) {
            ORBFE_HIP(hipMemcpyAsync(n_out + f0, d_oc[k], sizeof(int32_t) * nb, hipMemcpyDeviceToHost, s_out));
            ORBFE_HIP(hipMemcpyAsync(kps + (size_t)f0 * cap, d_ok[k], sizeof(orbfe_keypoint) * (size_t)cap * nb, hipMemcpyDeviceToHost, s_out));
            ORBFE_HIP(hipMemcpyAsync(desc + (size_t)f0 * cap * 32, d_od[k], (size_t)32 * cap * nb, hipMemcpyDeviceToHost, s_out));
        } else {
            ORBFE_HIP(hipMemcpyAsync(h->h_okps[k].p, d_ok[k], kb + db + sizeof(int32_t) * nb, hipMemcpyDeviceToHost, s_out));
        }
        if (c == nchunks - 1) {
            // the sticky overflow word travels with the results of the last chunk: an asynchronous 4-byte copy into pinned
            // memory behind the last kernels, in flight BEFORE the host starts waiting for results
            ORBFE_HIP(h->h_ovf.ensure(sizeof(int32_t)));
            ORBFE_HIP(hipMemcpyAsync(h->h_ovf.p, &misc_block(h)->overflow, sizeof(int32_t), hipMemcpyDeviceToHost, s_cmp));
        }
        ORBFE_HIP(hipEventRecord(h->ev_out[k], s_out));
    }
    for (int c = std::max(0, nchunks - 2); c < nchunks; ++c) {
        orbfe_status su = unpack(c);
        if (su != ORBFE_OK) return su;
    }
    ORBFE_HIP(hipStreamSynchronize(s_cmp));   // the overflow word (enqueued with the last chunk) has landed
    drain_guard.armed = false;  // everything has been waited for (unpack() synchronised the output events)
    {
        const int32_t ovf = *(const int32_t *)h->h_ovf.p;
        if (ovf) ORBFE_HIP(hipMemset(&misc_block(h)->overflow, 0, sizeof(int32_t)));
        if (ovf & 3) {
            orbfe_set_error("internal capacity exceeded (flags %d: 1 = FAST survivor list, 2 = quadtree selection); "
                            "results of this batch are incomplete", ovf);
            return ORBFE_ERR_CAP;
        }
    }
    if (worst == ORBFE_ERR_CAP) orbfe_set_error("cap=%d too small; n_out holds the required counts", cap);
    if (worst == ORBFE_OK && nframes == 1 && !direct && !direct_out) {   // what a later identical frame can be answered from
        h->reuse_valid = true;
        h->reuse_w = w;
        h->reuse_h = ht;
        h->reuse_cap = cap;
    }
    return worst;
}

extern "C" orbfe_status orbfe_extract(orbfe_handle *h, const uint8_t *gray, int32_t w, int32_t ht, int32_t stride,
                                      orbfe_keypoint *kps, uint8_t *desc, int32_t cap, int32_t *n_out)
{
    if (!h) { orbfe_set_error("null handle"); return ORBFE_ERR_ARG; }
    if (!gray || w == 0 || ht == 0) return ORBFE_OK;  // empty image: silent return, outputs untouched (:1055-1056)
    if (!kps || !desc || !n_out || w < 0 || ht < 0 || stride < w || cap < 1) {
        orbfe_set_error("bad argument to orbfe_extract");
        return ORBFE_ERR_ARG;
    }
    return extract_host(h, &gray, 1, w, ht, stride, kps, desc, cap, n_out);
}

extern "C" orbfe_status orbfe_extract_batch(orbfe_handle *h, const uint8_t *const *grays, int32_t nframes, int32_t w,
                                            int32_t ht, int32_t stride, orbfe_keypoint *kps, uint8_t *desc,
                                            int32_t cap, int32_t *n_out)
{
    if (!h) { orbfe_set_error("null handle"); return ORBFE_ERR_ARG; }
    if (nframes == 0 || w == 0 || ht == 0) return ORBFE_OK;
    if (!grays || !kps || !desc || !n_out || nframes < 0 || w < 0 || ht < 0 || stride < w || cap < 1) {
        orbfe_set_error("bad argument to orbfe_extract_batch");
        return ORBFE_ERR_ARG;
    }
    for (int i = 0; i < nframes; ++i)
        if (!grays[i]) { orbfe_set_error("grays[%d] is null", i); return ORBFE_ERR_ARG; }
    return extract_host(h, grays, nframes, w, ht, stride, kps, desc, cap, n_out);
}

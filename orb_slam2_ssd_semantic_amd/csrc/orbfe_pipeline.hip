// orbfe_pipeline.hip -- the throughput pipeline of the ORB front-end as a product feature (include/orbfe.h "Pipeline").
//
// What it stands for in the reference: the frame loop of perfect/Examples/RGB-D/rgbd_tum.cc:77-119 -- one frame after the
// other through ORBextractor::operator() (Frame constructor) and a match against the previous frame.  Here a whole resident
// SEQUENCE goes through in one call: it is cut into sub-batches of `max_batch` frames, sub-batch j runs on pipe j mod P_eff -- a
// pipe = one extractor handle + one matcher handle + one stream, so that the VALU-bound FAST pass of one sub-batch shares the
// chip with the HBM / LDS-bound stages of its neighbours -- and frame k is matched against frame k - 1 ACROSS sub-batch
// boundaries and across calls (the last frame of a call is carried over), i.e. a real sequence.  How many streams there are, and
// with them P_eff, follows from the hardware queues of the process (orbfe_pipe_plan.h).  The same header has the second way to
// cut a call over the streams, by stage instead of by sub-batch (lanes), taken where its rule and the pipeline's lane mode say so.
//
// What one call enqueues -- which stream every piece runs on, which events it waits for and records, in both cuts -- is stated
// once, in orbfe_pipe_graph.h, without a device call; run_device here walks it with the HIP and library calls (PipeCall).
//
// Host code only: every kernel is launched through the extractor / matcher entry points of this library.
#include <initializer_list>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "orbfe_common.h"
#include "orbfe_kernels.h"
#include "orbfe_matcher.h"
#include "orbfe_pipe_graph.h"

// Streams outlive their pipeline.  Which hardware queue the runtime gives a new stream depends on every stream the process has
// made and destroyed before, and a pipeline whose copy, kernel and side streams landed on queues of their own runs its host
// entry point at 0.95 of the PCIe link where one that shares queues among them reaches 0.68 (profiles/pipe_queues.md).  A
// destroyed pipeline therefore hands its streams, drained, to the next one of the same device, in the same roles.
static std::mutex g_spare_mu;
static std::vector<std::pair<int, hipStream_t>> g_spare;   // (device, stream); taken from the back

static hipStream_t take_spare_stream(int device)
{
    std::lock_guard<std::mutex> lk(g_spare_mu);
    for (size_t i = g_spare.size(); i-- > 0;)
        if (g_spare[i].first == device) {
            hipStream_t s = g_spare[i].second;
            g_spare.erase(g_spare.begin() + (ptrdiff_t)i);
            return s;
        }
    return nullptr;
}

static_assert(sizeof(orbfe_keypoint) == ORB_PIPE_KEYPOINT_BYTES && ORBFE_PIPE_CONTINUE == ORB_PIPE_CONTINUE, "orbfe_pipe_graph.h restates these");

struct orbfe_pipeline {
    orbfe_params prm;
    int device = 0;
    int P = 1;     // pipes (handles); cur.P_eff of them take sub-batches
    int Q = ORBFE_PIPE_DEFAULT_QUEUES;   // hardware queues the streams are fitted to
    OrbPipePlan cur;   // the plan of the call in flight or last made: the device entry point's or the host entry point's
    bool cur_valid = false;
    int F = 1;     // frames per sub-batch (prm.max_batch)
    int cap = 0;   // keypoint slots per frame
    std::vector<orbfe_handle *> ext;
    std::vector<orbfe_matcher *> mat;
    // Every stream of the pipeline, created as a plan first asks for it.  A plan deals the roles in this order: the host entry
    // point's copy streams (s_in, s_out), the kernel streams, the side stream (the extractors' blur, shared by the pipes).
    std::vector<hipStream_t> pool;
    hipStream_t stream_of(int pipe) const { return pool[(size_t)(cur.first + cur.stream_of_pipe[pipe])]; }
    hipStream_t side() const { return cur.side ? pool[(size_t)cur.side_index] : nullptr; }

    // ---- the call graph (orbfe_pipe_graph.h): its state, the events its {kind, index} pairs name, what chooses its route
    OrbPipeState g;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_ext, ev_match;   // per sub-batch index
    std::vector<hipEvent_t> ev_end;             // per pipe
    hipEvent_t ev_carry[2] = {nullptr, nullptr}, ev_m0[2] = {nullptr, nullptr};   // per carry slot
    // lanes (orbfe_pipe_plan.h): -1 automatic, 0 never, 1 wherever the rule allows them (orbfe_internal_pipeline_set_lanes)
    int lane_mode = -1;
    int lane_sets = 0;          // buffer sets of a lane call; 0: ORBFE_PIPE_LANE_SETS
    int lane_place = -1;        // 0: blur behind the pyramid on kernel stream 0, matcher on the side stream; 1: blur on the side
                                // stream, matcher behind the descriptor on kernel stream 2 (where chains have both); 2: blur as 0,
                                // matcher as 1, FAST of odd sub-batches on the side stream; -1: ORBFE_PIPE_LANE_PLACE_AUTO
    int lane_tiles = 0;         // query tiles per wave of a lane call's brute-force matcher (4, 2, 1); 0: ORBFE_PIPE_LANE_MATCH_TILES
    // seq[i] = i - 1: qframe = seq + q0 + 1 (q0, q0 + 1, ...), tframe = seq + q0 (q0 - 1, q0, ...)
    DevBuf d_seq;
    int seq_len = 0;

    // ---- the carry slots: the last frame of the previous call (keypoints, descriptors, count)
    DevBuf d_ckps[2], d_cdesc[2], d_cn[2];

    // ---- host entry point (orbfe_pipeline_extract_match): device input / output sets, copy streams
    int host_pipes = 1;         // pipes the host entry point deals its chunks to (orbfe_pipeline_set_host_pipes)
    static const int NSETS = 3;
    struct HostSet {
        DevBuf in, kps, desc, n, match, nmatch;
        hipEvent_t ev_out = nullptr;   // the set's results have left it
    } host[NSETS];
    hipStream_t s_in() const { return pool[0]; }   // (with a plan that has copy streams)
    hipStream_t s_out() const { return pool[1]; }
};

static orbfe_status drain_streams(orbfe_pipeline *pl)
{
    for (hipStream_t s : pl->pool) ORBFE_HIP(hipStreamSynchronize(s));
    return ORBFE_OK;
}

static hipError_t make_event(hipEvent_t *e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }

static orbfe_status ensure_events(orbfe_pipeline *pl, int nsub)
{
    for (std::vector<hipEvent_t> *v : {&pl->ev_ext, &pl->ev_match})
        while ((int)v->size() < nsub) {
            hipEvent_t e = nullptr;
            ORBFE_HIP(make_event(&e));
            v->push_back(e);
        }
    return ORBFE_OK;
}

static orbfe_status ensure_seq(orbfe_pipeline *pl, int nframes)
{
    if (nframes + 1 <= pl->seq_len) return ORBFE_OK;
    // the index table is about to be replaced: no launch of an earlier call may still read it
    const orbfe_status s = drain_streams(pl);
    if (s != ORBFE_OK) return s;
    pl->seq_len = 0;
    const int len = std::max(nframes + 1, 4096);
    std::vector<int32_t> h((size_t)len);
    for (int i = 0; i < len; ++i) h[(size_t)i] = i - 1;
    ORBFE_HIP(pl->d_seq.ensure((size_t)len * sizeof(int32_t)));
    ORBFE_HIP(hipMemcpy(pl->d_seq.p, h.data(), (size_t)len * sizeof(int32_t), hipMemcpyHostToDevice));
    pl->seq_len = len;
    return ORBFE_OK;
}

extern "C" void orbfe_pipeline_destroy(orbfe_pipeline *pl)
{
    if (!pl) return;
    DeviceGuard g(pl->device);
    for (hipStream_t s : pl->pool)
        if (s) (void)hipStreamSynchronize(s);
    for (orbfe_handle *h : pl->ext) orbfe_destroy(h);
    for (orbfe_matcher *m : pl->mat) orbfe_matcher_destroy(m);
    std::vector<hipEvent_t> ev = {pl->ev_fork, pl->ev_carry[0], pl->ev_carry[1], pl->ev_m0[0], pl->ev_m0[1]};
    for (const std::vector<hipEvent_t> *v : {&pl->ev_ext, &pl->ev_match, &pl->ev_end}) ev.insert(ev.end(), v->begin(), v->end());
    for (orbfe_pipeline::HostSet &h : pl->host) {
        ev.push_back(h.ev_out);
        for (DevBuf *b : {&h.in, &h.kps, &h.desc, &h.n, &h.match, &h.nmatch}) b->release();
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < 2; ++k)
        for (DevBuf *b : {&pl->d_ckps[k], &pl->d_cdesc[k], &pl->d_cn[k]}) b->release();
    pl->d_seq.release();
    {   // (drained above) last stream first, so that the next pipeline's stream i is this one's stream i
        std::lock_guard<std::mutex> lk(g_spare_mu);
        for (size_t i = pl->pool.size(); i-- > 0;)
            if (pl->pool[i]) g_spare.push_back(std::make_pair(pl->device, pl->pool[i]));
    }
    delete pl;
}

// Makes `plan` the pipeline's current one.  A change of plan (the device entry point after the host entry point or the other way
// round, another orbfe_pipeline_set_host_pipes) moves handles to other streams and streams to other roles: everything in flight
// is drained first, which no sequence of calls of one kind ever pays.
static orbfe_status apply_plan(orbfe_pipeline *pl, const OrbPipePlan &plan)
{
    const bool same = pl->cur_valid && pl->cur.copies == plan.copies && pl->cur.S == plan.S && pl->cur.side == plan.side &&
                      pl->cur.P_eff == plan.P_eff;
    if (same) return ORBFE_OK;
    const orbfe_status ds = drain_streams(pl);
    if (ds != ORBFE_OK) return ds;
    while ((int)pl->pool.size() < plan.nstreams) {
        hipStream_t st = take_spare_stream(pl->device);
        if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { orbfe_set_error("pipeline stream creation failed"); return ORBFE_ERR_HIP; }
        pl->pool.push_back(st);
    }
    pl->cur = plan;
    pl->cur_valid = true;
    pl->g.rot %= plan.P_eff;
    for (int i = 0; i < pl->P && i < (int)pl->ext.size(); ++i) {
        const orbfe_status s = orbfe_internal_set_side_stream(pl->ext[(size_t)i], (void *)pl->side());
        if (s != ORBFE_OK) return s;
    }
    return ORBFE_OK;
}

// orbfe_pipeline_create for a process with `queues` hardware queues (not in include/orbfe.h: the tests walk the queue counts
// with it, whatever the environment says)
extern "C" orbfe_status orbfe_internal_pipeline_create_queues(const orbfe_params *p, int32_t npipes, int32_t queues, orbfe_pipeline **out)
{
    if (!p || !out || npipes < 1 || npipes > ORBFE_PIPE_MAX_PIPES) {
        orbfe_set_error("bad argument to orbfe_pipeline_create (1..64 pipes)");
        return ORBFE_ERR_ARG;
    }
    *out = nullptr;
    orbfe_pipeline *pl = new (std::nothrow) orbfe_pipeline();
    if (!pl) return ORBFE_ERR_NOMEM;
    pl->prm = *p;
    pl->P = npipes;
    pl->Q = std::min(std::max(queues, 1), ORBFE_PIPE_MAX_QUEUES);
    pl->F = p->max_batch;
    auto fail = [&](orbfe_status s) {
        orbfe_pipeline_destroy(pl);
        return s;
    };
    {   // the device the handles will use (p->device may be -1 = current)
        int dev = p->device;
        const orbfe_status rs = orb_resolve_device(&dev);
        if (rs != ORBFE_OK) return fail(rs);
        pl->device = dev;
        pl->prm.device = dev;
    }
    DeviceGuard g(pl->device);
    // The streams follow the plan of orbfe_pipe_plan.h: the runtime gives every stream one hardware queue for life, packets of a
    // queue run in submission order, and a cross-stream wait holds everything behind it in its queue, other streams' kernels
    // included -- so the pipeline creates no more kernel-carrying streams than the process has queues, the side stream for the
    // blur among them.  Each of the kernel streams is shared by the extractor and matcher handles of its pipes
    // (which create none of their own); the handles beyond P_eff stay valid for orbfe_pipeline_extractor / _matcher and get
    // no sub-batches.
    {
        OrbPipePlan plan;
        if (!orb_pipe_plan(npipes, pl->Q, false, &plan)) return fail(ORBFE_ERR_ARG);
        const orbfe_status s = apply_plan(pl, plan);
        if (s != ORBFE_OK) return fail(s);
    }
    pl->ev_end.assign((size_t)npipes, nullptr);
    bool events = make_event(&pl->ev_fork) == hipSuccess;
    for (hipEvent_t &e : pl->ev_end) events = events && make_event(&e) == hipSuccess;
    for (int k = 0; k < 2; ++k) events = events && make_event(&pl->ev_carry[k]) == hipSuccess && make_event(&pl->ev_m0[k]) == hipSuccess;
    if (!events) {
        orbfe_set_error("pipeline event creation failed");
        return fail(ORBFE_ERR_HIP);
    }
    for (int i = 0; i < npipes; ++i) {
        orbfe_handle *h = nullptr;
        orbfe_status s = orbfe_internal_create_on_stream(&pl->prm, (void *)pl->stream_of(i), (void *)pl->side(), &h);
        if (s != ORBFE_OK) return fail(s);
        pl->ext.push_back(h);
        orbfe_matcher *m = nullptr;
        s = orbfe_internal_matcher_create_on_stream(pl->device, (void *)pl->stream_of(i), &m);
        if (s != ORBFE_OK) return fail(s);
        pl->mat.push_back(m);
    }
    // Slots per frame of the host sets and the carry blocks: the extractor's capacity for the planned max_width x max_height, and
    // never less than what ANY frame size can ask for -- a level's selection holds max(N_l + 2, 4 * roots) keypoints and the root
    // count follows the frame's aspect ratio (at most ORBFE_MAX_ROOTS): a later call with another w / ht finds room.
    {
        int32_t feat[ORBFE_MAX_LEVELS];
        int worst = 0;
        if (orbfe_get_features_per_level(pl->ext[0], feat) == ORBFE_OK)
            for (int l = 0; l < pl->prm.nlevels; ++l) worst += std::max(feat[l] + 2, 4 * ORBFE_MAX_ROOTS);
        pl->cap = std::max(orbfe_keypoint_capacity(pl->ext[0]), (worst + 63) & ~63);
    }
    for (int k = 0; k < 2; ++k) {
        if (pl->d_ckps[k].ensure((size_t)pl->cap * sizeof(orbfe_keypoint)) != hipSuccess || pl->d_cdesc[k].ensure((size_t)pl->cap * 32) != hipSuccess ||
            pl->d_cn[k].ensure(64) != hipSuccess) {
            orbfe_set_error("pipeline carry buffers: %s", hipGetErrorString(hipGetLastError()));
            return fail(ORBFE_ERR_NOMEM);
        }
        (void)hipMemset(pl->d_cn[k].p, 0, 64);
    }
    orbfe_status s = ensure_seq(pl, 4095);
    if (s != ORBFE_OK) return fail(s);
    *out = pl;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pipeline_create(const orbfe_params *p, int32_t npipes, orbfe_pipeline **out)
{
    return orbfe_internal_pipeline_create_queues(p, npipes, orb_pipe_env_queues(), out);
}

// test hooks (not in include/orbfe.h; no device): the plan of `npipes` pipes on `queues` queues as 9 + ORBFE_PIPE_MAX_PIPES
// int32 -- P, Q, copies, S, P_eff, side, first, side_index, nstreams, stream of every pipe -- and the queue count the
// library makes of a GPU_MAX_HW_QUEUES text / of the environment
extern "C" int32_t orbfe_internal_pipe_plan(int32_t npipes, int32_t queues, int32_t copies, int32_t *out)
{
    OrbPipePlan plan;
    if (!out || !orb_pipe_plan(npipes, queues, copies != 0, &plan)) return ORBFE_ERR_ARG;
    const int32_t head[9] = {plan.P, plan.Q, plan.copies, plan.S, plan.P_eff, plan.side, plan.first, plan.side_index, plan.nstreams};
    for (int i = 0; i < 9; ++i) out[i] = head[i];
    for (int i = 0; i < ORBFE_PIPE_MAX_PIPES; ++i) out[9 + i] = plan.stream_of_pipe[i];
    return ORBFE_OK;
}
extern "C" int32_t orbfe_internal_pipe_parse_queues(const char *text) { return orb_pipe_parse_queues(text); }
extern "C" int32_t orbfe_internal_pipe_env_queues(void) { return orb_pipe_env_queues(); }
// the plan in force: kernel streams, pipes that take sub-batches, side stream or not
extern "C" orbfe_status orbfe_internal_pipeline_streams(const orbfe_pipeline *pl, int32_t *streams, int32_t *eff_pipes, int32_t *side)
{
    if (!pl || !pl->cur_valid) return ORBFE_ERR_ARG;
    if (streams) *streams = pl->cur.S;
    if (eff_pipes) *eff_pipes = pl->cur.P_eff;
    if (side) *side = pl->cur.side;
    return ORBFE_OK;
}

// the lane rule (orb_pipe_lanes) for a call of `nsub` sub-batches on the plan of (npipes, queues, copies): out = {lanes, sets}
extern "C" int32_t orbfe_internal_pipe_lanes(int32_t npipes, int32_t queues, int32_t copies, int32_t nsub, int32_t *out)
{
    OrbPipePlan plan;
    if (!out || !orb_pipe_plan(npipes, queues, copies != 0, &plan)) return ORBFE_ERR_ARG;
    const OrbPipeLanes r = orb_pipe_lanes(plan, nsub);
    out[0] = r.lanes;
    out[1] = r.sets;
    return ORBFE_OK;
}
// -1: lanes where the library chooses them, 0: never, 1: wherever the rule allows them; "on" is an error for a pipeline whose
// device plan lacks the 3 kernel streams + side stream short of its pipes
extern "C" orbfe_status orbfe_internal_pipeline_set_lanes(orbfe_pipeline *pl, int32_t mode)
{
    OrbPipePlan plan;
    if (!pl || mode < -1 || mode > 1 || !orb_pipe_plan(pl->P, pl->Q, false, &plan)) return ORBFE_ERR_ARG;
    if (mode == 1 && !orb_pipe_lanes(plan, 2).lanes) {
        orbfe_set_error("lanes need 3 kernel streams and the side stream for more than 3 pipes: %d pipes on %d queues have %d + %d", pl->P, pl->Q,
                        plan.S, plan.side);
        return ORBFE_ERR_ARG;
    }
    pl->lane_mode = mode;
    return ORBFE_OK;
}
// the A/B knobs of a lane call: buffer sets (0: ORBFE_PIPE_LANE_SETS; at most the pipes) and the placement of blur and matcher
// (0: blur on kernel stream 0, matcher on the side stream; 1: blur on the side stream, matcher on kernel stream 2; 2: blur on kernel
// stream 0, matcher on kernel stream 2, FAST on kernel stream 1 and the side stream in turn; -1: ORBFE_PIPE_LANE_PLACE_AUTO)
extern "C" orbfe_status orbfe_internal_pipeline_set_lane_options(orbfe_pipeline *pl, int32_t sets, int32_t place)
{
    if (!pl || sets < 0 || sets > ORBFE_PIPE_MAX_PIPES || place < -1 || place >= ORBFE_PIPE_LANE_PLACES) return ORBFE_ERR_ARG;
    pl->lane_sets = sets;
    pl->lane_place = place;
    return ORBFE_OK;
}
// ... and the query tiles per wave of a lane call's brute-force matcher (4, 2, 1; 0: ORBFE_PIPE_LANE_MATCH_TILES).  Chain calls and the
// pipes' matcher handles keep their own (orbfe_internal_matcher_set_bf_tiles)
extern "C" orbfe_status orbfe_internal_pipeline_set_lane_match_tiles(orbfe_pipeline *pl, int32_t tiles)
{
    if (!pl || (tiles != 0 && !orb_match_tiles_ok(tiles))) return ORBFE_ERR_ARG;
    pl->lane_tiles = tiles;
    return ORBFE_OK;
}

extern "C" int32_t orbfe_pipeline_pipes(const orbfe_pipeline *pl) { return pl ? pl->P : 0; }
extern "C" int32_t orbfe_pipeline_capacity(const orbfe_pipeline *pl) { return pl ? pl->cap : 0; }
extern "C" int32_t orbfe_pipeline_sub_batch(const orbfe_pipeline *pl) { return pl ? pl->F : 0; }
extern "C" orbfe_handle *orbfe_pipeline_extractor(orbfe_pipeline *pl, int32_t pipe)
{
    return (pl && pipe >= 0 && pipe < pl->P) ? pl->ext[(size_t)pipe] : nullptr;
}
extern "C" orbfe_matcher *orbfe_pipeline_matcher(orbfe_pipeline *pl, int32_t pipe)
{
    return (pl && pipe >= 0 && pipe < pl->P) ? pl->mat[(size_t)pipe] : nullptr;
}

extern "C" orbfe_status orbfe_pipeline_set_host_pipes(orbfe_pipeline *pl, int32_t n)
{
    if (!pl || n < 1) return ORBFE_ERR_ARG;
    pl->host_pipes = std::min(n, pl->P);   // (the host entry point plans its streams for this many pipes)
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pipeline_reset_sequence(orbfe_pipeline *pl)
{
    if (!pl) return ORBFE_ERR_ARG;
    pl->g.new_sequence();
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pipeline_join(orbfe_pipeline *pl, void *stream)
{
    if (!pl) return ORBFE_ERR_ARG;
    DeviceGuard g(pl->device);
    for (int p = 0; p < pl->P; ++p)
        if (pl->g.end_valid[p]) ORBFE_HIP(hipStreamWaitEvent((hipStream_t)stream, pl->ev_end[(size_t)p], 0));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pipeline_synchronize(orbfe_pipeline *pl)
{
    if (!pl) return ORBFE_ERR_ARG;
    DeviceGuard g(pl->device);
    return drain_streams(pl);
}

extern "C" orbfe_status orbfe_pipeline_get_overflow(orbfe_pipeline *pl, int32_t *flags)
{
    if (!pl || !flags) return ORBFE_ERR_ARG;
    *flags = 0;
    for (orbfe_handle *h : pl->ext) {
        int32_t f = 0;
        const orbfe_status s = orbfe_get_overflow(h, &f);
        if (s != ORBFE_OK) return s;
        *flags |= f;
    }
    return ORBFE_OK;
}

// The arguments of one call and what the graph's operations (orbfe_pipe_graph.h) are on the device: streams of the pool, events of
// the pipeline, the extractor and matcher handles' entry points, copies into the carry slots.
struct PipeCall {
    orbfe_pipeline *pl;
    const uint8_t *d_gray;
    int32_t w, ht, stride;
    size_t frame_stride;
    orbfe_keypoint *d_kps;
    uint8_t *d_desc;
    int32_t cap;
    int32_t *d_n_out, *d_match, *d_nmatches;
    float nnratio;
    int32_t th, check_ori;
    hipStream_t caller;
    int32_t lane_tiles = 0;   // run_device: the matcher's query tiles per wave if the call runs in lanes; 0: the matcher handles' own

    hipStream_t stream(int32_t s) const { return s == ORB_PIPE_CALLER ? caller : pl->pool[(size_t)s]; }
    hipEvent_t event(OrbPipeEvent e) const
    {
        switch (e.kind) {
        case ORB_EV_EXT: return pl->ev_ext[(size_t)e.index];
        case ORB_EV_MATCH: return pl->ev_match[(size_t)e.index];
        case ORB_EV_CARRY: return pl->ev_carry[e.index];
        case ORB_EV_M0: return pl->ev_m0[e.index];
        case ORB_EV_END: return pl->ev_end[(size_t)e.index];
        default: return pl->ev_fork;
        }
    }
    const int32_t *seq() const { return pl->d_seq.as<int32_t>(); }
    orbfe_status wait(int32_t s, OrbPipeEvent e) const
    {
        ORBFE_HIP(hipStreamWaitEvent(stream(s), event(e), 0));
        return ORBFE_OK;
    }
    orbfe_status record(int32_t s, OrbPipeEvent e) const
    {
        ORBFE_HIP(hipEventRecord(event(e), stream(s)));
        return ORBFE_OK;
    }
    orbfe_status extract(int32_t h, int32_t lo, int32_t nf, const OrbPipeRoute &r) const
    {
        const uint8_t *gray = d_gray + (size_t)lo * frame_stride;
        orbfe_keypoint *kps = d_kps + (size_t)lo * cap;
        uint8_t *desc = d_desc + (size_t)lo * cap * 32;
        if (!r.lanes)
            return orbfe_extract_batch_device(pl->ext[(size_t)h], gray, nf, w, ht, stride, frame_stride, kps, desc, cap, d_n_out + lo,
                                              (void *)stream(r.start_of[h]));
        void *lane[4] = {(void *)stream(r.lane[0]), (void *)stream(r.lane[1]), (void *)stream(r.lane[2]), (void *)stream(r.lane[3])};
        return orbfe_internal_extract_batch_lanes(pl->ext[(size_t)h], gray, nf, w, ht, stride, frame_stride, kps, desc, cap, d_n_out + lo, lane);
    }
    int32_t tiles(int32_t h) const { return lane_tiles ? lane_tiles : pl->mat[(size_t)h]->bf_tiles; }
    orbfe_status match(int32_t h, int32_t s, int32_t q0, int32_t np) const
    {
        return orbfe_internal_match_bf_blocks_tiles(pl->mat[(size_t)h], d_kps, d_desc, d_n_out, d_kps, d_desc, d_n_out, cap, seq() + q0 + 1, seq() + q0, np,
                                                    nnratio, th, check_ori, d_match + (size_t)q0 * cap, d_nmatches + q0, tiles(h), (void *)stream(s));
    }
    orbfe_status match_carry(int32_t h, int32_t s, int32_t slot) const   // query = frame 0 of this call, train = frame 0 of the carry block
    {
        return orbfe_internal_match_bf_blocks_tiles(pl->mat[(size_t)h], d_kps, d_desc, d_n_out, pl->d_ckps[slot].as<orbfe_keypoint>(),
                                                    pl->d_cdesc[slot].as<uint8_t>(), pl->d_cn[slot].as<int32_t>(), cap, seq() + 1, seq() + 1, 1, nnratio, th,
                                                    check_ori, d_match, d_nmatches, tiles(h), (void *)stream(s));
    }
    orbfe_status clear_row0(int32_t s) const
    {
        ORBFE_HIP(hipMemsetAsync(d_match, 0xFF, (size_t)cap * sizeof(int32_t), stream(s)));
        ORBFE_HIP(hipMemsetAsync(d_nmatches, 0, sizeof(int32_t), stream(s)));
        return ORBFE_OK;
    }
    orbfe_status carry_copy(int32_t s, int32_t slot, int32_t last_frame) const
    {
        const size_t last = (size_t)last_frame, slots = (size_t)std::min(cap, pl->cap);
        ORBFE_HIP(hipMemcpyAsync(pl->d_ckps[slot].p, d_kps + last * cap, slots * sizeof(orbfe_keypoint), hipMemcpyDeviceToDevice, stream(s)));
        ORBFE_HIP(hipMemcpyAsync(pl->d_cdesc[slot].p, d_desc + last * cap * 32, slots * 32, hipMemcpyDeviceToDevice, stream(s)));
        ORBFE_HIP(hipMemcpyAsync(pl->d_cn[slot].p, d_n_out + last, sizeof(int32_t), hipMemcpyDeviceToDevice, stream(s)));
        return ORBFE_OK;
    }
};

// One call on the pipeline's current plan (apply_plan): the device entry point's, or the host entry point's with its copy streams
// (`first_pipe` >= 0: the pipe of its one-sub-batch chunk)
static orbfe_status run_device(orbfe_pipeline *pl, const PipeCall &args, int32_t nframes, int32_t flags, int32_t first_pipe = -1)
{
    const int nsub = (nframes + pl->F - 1) / pl->F;
    orbfe_status s = ensure_events(pl, nsub + 1);
    if (s != ORBFE_OK) return s;
    s = ensure_seq(pl, nframes);
    if (s != ORBFE_OK) return s;
    PipeCall c = args;
    const OrbPipeRoute route(pl->cur, orb_pipe_lanes(pl->cur, nsub, pl->lane_sets), pl->lane_mode, pl->lane_place < 0 ? ORBFE_PIPE_LANE_PLACE_AUTO : pl->lane_place,
                             first_pipe, pl->g);
    const OrbPipeBlocks out{(uintptr_t)c.d_kps, (uintptr_t)c.d_desc, (uintptr_t)c.d_n_out, c.cap};
    const OrbPipeCall call{route, out, pl->F, nframes, c.d_match != nullptr, flags};
    c.lane_tiles = route.lanes ? (pl->lane_tiles ? pl->lane_tiles : ORBFE_PIPE_LANE_MATCH_TILES) : 0;
    s = orb_pipe_call(pl->g, call, c);
    if (s != ORBFE_OK) {
        // launches of this call are in flight and the ledger is half updated: drain the pipes and start the sequence over (the next
        // call has no predecessor frame), then report
        for (hipStream_t x : pl->pool) (void)hipStreamSynchronize(x);
        pl->g.reset();
        return s;
    }
    if (!(flags & ORBFE_PIPE_NO_JOIN)) return orbfe_pipeline_join(pl, (void *)c.caller);
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pipeline_extract_match_device(orbfe_pipeline *pl, const uint8_t *d_gray, int32_t nframes, int32_t w,
                                                            int32_t ht, int32_t stride, size_t frame_stride, orbfe_keypoint *d_kps,
                                                            uint8_t *d_desc, int32_t cap, int32_t *d_n_out, int32_t *d_match,
                                                            int32_t *d_nmatches, float nnratio, int32_t th, int32_t check_ori,
                                                            int32_t flags, void *stream)
{
    if (!pl || !d_gray || !d_kps || !d_desc || !d_n_out || nframes < 1 || cap < 1 || (d_match && !d_nmatches)) {
        orbfe_set_error("bad argument to orbfe_pipeline_extract_match_device");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(pl->device);
    OrbPipePlan plan;
    if (!orb_pipe_plan(pl->P, pl->Q, false, &plan)) return ORBFE_ERR_ARG;
    const orbfe_status s = apply_plan(pl, plan);
    if (s != ORBFE_OK) return s;
    const PipeCall c{pl, d_gray, w, ht, stride, frame_stride, d_kps, d_desc, cap, d_n_out, d_match, d_nmatches, nnratio, th, check_ori, (hipStream_t)stream};
    return run_device(pl, c, nframes, flags);
}

// ---------------------------------------------------------------------------------------------------
// host frames in, host results out: chunks of one sub-batch, H2D / pipes / D2H overlapped over three device buffer sets
// ---------------------------------------------------------------------------------------------------
static orbfe_status ensure_host_sets(orbfe_pipeline *pl, int w, int ht)
{
    // (measured and rejected: copy streams at the highest stream priority -- 159 k frames/s with 3 pipes, 41 k with 12)
    const size_t F = (size_t)pl->F, cap = (size_t)pl->cap;
    const size_t need[6] = {F * w * ht + 64,          F * cap * sizeof(orbfe_keypoint), F * cap * 32,
                            F * sizeof(int32_t),      F * cap * sizeof(int32_t),        F * sizeof(int32_t)};
    // every buffer grows on its own, so a failed allocation leaves the others what they say they are; a buffer is replaced only
    // with nothing in flight
    bool drained = false;
    for (orbfe_pipeline::HostSet &h : pl->host) {
        if (!h.ev_out) ORBFE_HIP(make_event(&h.ev_out));
        DevBuf *const bufs[6] = {&h.in, &h.kps, &h.desc, &h.n, &h.match, &h.nmatch};
        for (int i = 0; i < 6; ++i) {
            if (need[i] <= bufs[i]->bytes) continue;
            if (!drained) {
                const orbfe_status s = drain_streams(pl);
                if (s != ORBFE_OK) return s;
                drained = true;
            }
            ORBFE_HIP(bufs[i]->ensure(need[i]));
        }
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pipeline_extract_match(orbfe_pipeline *pl, const uint8_t *const *grays, int32_t nframes, int32_t w, int32_t ht,
                                                     int32_t stride, orbfe_keypoint *kps, uint8_t *desc, int32_t cap, int32_t *n_out,
                                                     int32_t *match, int32_t *nmatches, float nnratio, int32_t th, int32_t check_ori,
                                                     int32_t flags)
{
    if (!pl || !grays || !kps || !desc || !n_out || nframes < 1 || w < 1 || ht < 1 || stride < w || (match && !nmatches)) {
        orbfe_set_error("bad argument to orbfe_pipeline_extract_match");
        return ORBFE_ERR_ARG;
    }
    if (cap < pl->cap) {
        orbfe_set_error("orbfe_pipeline_extract_match: cap %d below orbfe_pipeline_capacity() = %d", cap, pl->cap);
        return ORBFE_ERR_CAP;
    }
    DeviceGuard g(pl->device);
    // the same planner with the copy streams first: the chunks go to min(host_pipes, P) pipes, which is what the plan is asked for
    OrbPipePlan plan;
    if (!orb_pipe_plan(std::max(1, std::min(pl->host_pipes, pl->P)), pl->Q, true, &plan)) return ORBFE_ERR_ARG;
    orbfe_status s = apply_plan(pl, plan);
    if (s != ORBFE_OK) return s;
    s = ensure_host_sets(pl, w, ht);
    if (s != ORBFE_OK) return s;
    const int F = pl->F, pc = pl->cap;
    const size_t fbytes = (size_t)w * ht;
    const int nchunks = (nframes + F - 1) / F;
    // Whatever way the loop is left, copies that read the caller's frames or write its arrays may be in flight: every exit
    // drains the copy streams and the pipes first.
    struct Drain {
        orbfe_pipeline *pl;
        ~Drain()
        {
            for (hipStream_t st : pl->pool) (void)hipStreamSynchronize(st);
        }
    } drain{pl};
    for (int c = 0; c < nchunks; ++c) {
        const int lo = c * F, nf = std::min(F, nframes - lo);
        orbfe_pipeline::HostSet &hs = pl->host[c % orbfe_pipeline::NSETS];
        // the set is free once the results of chunk c - NSETS have left it
        if (c >= orbfe_pipeline::NSETS) ORBFE_HIP(hipStreamWaitEvent(pl->s_in(), hs.ev_out, 0));
        bool contiguous = stride == w;
        for (int f = 1; f < nf && contiguous; ++f) contiguous = grays[lo + f] == grays[lo + f - 1] + fbytes;
        if (contiguous) {
            ORBFE_HIP(hipMemcpyAsync(hs.in.p, grays[lo], fbytes * nf, hipMemcpyHostToDevice, pl->s_in()));
        } else {
            for (int f = 0; f < nf; ++f)
                ORBFE_HIP(hipMemcpy2DAsync(hs.in.as<uint8_t>() + fbytes * f, (size_t)w, grays[lo + f], (size_t)stride, (size_t)w, (size_t)ht,
                                           hipMemcpyHostToDevice, pl->s_in()));
        }
        // the pipes start behind the copy (the call forks from s_in) and are not joined: the next chunk's copy and pipes follow at once
        const int fl = ((c > 0 || (flags & ORBFE_PIPE_CONTINUE)) ? ORBFE_PIPE_CONTINUE : 0) | ORBFE_PIPE_NO_JOIN;
        const PipeCall call{pl, hs.in.as<uint8_t>(), w, ht, w, fbytes, hs.kps.as<orbfe_keypoint>(), hs.desc.as<uint8_t>(), pc, hs.n.as<int32_t>(),
                            match ? hs.match.as<int32_t>() : nullptr, match ? hs.nmatch.as<int32_t>() : nullptr, nnratio, th, check_ori, pl->s_in()};
        s = run_device(pl, call, nf, fl, c % pl->cur.P_eff);   // the chunk is one sub-batch: this is its pipe
        if (s != ORBFE_OK) return s;
        s = orbfe_pipeline_join(pl, (void *)pl->s_out());   // everything submitted so far, i.e. this chunk and older ones
        if (s != ORBFE_OK) return s;
        // padded blocks straight into the caller's arrays (row pitch cap >= pc)
        ORBFE_HIP(hipMemcpyAsync(n_out + lo, hs.n.p, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, pl->s_out()));
        auto rows_out = [&](void *dst, const void *src, size_t elem) -> hipError_t {   // nf rows of pc elements, host pitch cap
            if (cap == pc) return hipMemcpyAsync(dst, src, (size_t)nf * pc * elem, hipMemcpyDeviceToHost, pl->s_out());   // one linear copy
            return hipMemcpy2DAsync(dst, (size_t)cap * elem, src, (size_t)pc * elem, (size_t)pc * elem, (size_t)nf, hipMemcpyDeviceToHost, pl->s_out());
        };
        ORBFE_HIP(rows_out(kps + (size_t)lo * cap, hs.kps.p, sizeof(orbfe_keypoint)));
        ORBFE_HIP(rows_out(desc + (size_t)lo * cap * 32, hs.desc.p, 32));
        if (match) {
            ORBFE_HIP(rows_out(match + (size_t)lo * cap, hs.match.p, sizeof(int32_t)));
            ORBFE_HIP(hipMemcpyAsync(nmatches + lo, hs.nmatch.p, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, pl->s_out()));
        }
        ORBFE_HIP(hipEventRecord(hs.ev_out, pl->s_out()));
    }
    ORBFE_HIP(hipStreamSynchronize(pl->s_out()));
    int32_t ovf = 0;
    s = orbfe_pipeline_get_overflow(pl, &ovf);
    if (s != ORBFE_OK) return s;
    if (ovf) {
        orbfe_set_error("device-side capacity overflow %d in orbfe_pipeline_extract_match", ovf);
        return ORBFE_ERR_CAP;
    }
    return ORBFE_OK;
}

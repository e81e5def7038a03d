// orbfe_pipe_graph.h -- the sequence pipeline's call graph, written once and without a device call: which stream every piece of a
// call runs on, and what it waits for.  orbfe_pipeline.hip walks it with a sink whose methods are the HIP and library calls;
// tests/cpp/test_pipe_graph.cpp walks it with a sink that prints, and tests/test_pipe_graph.py checks from that log that no two
// operations that touch the same bytes are left unordered.  DESIGN.md section 6 has the two diagrams (chains, lanes).
//
// Three parts:
//   the ledger (OrbPipeState)  what the events of the pipeline stand for: per sub-batch index the output slices that the last
//                              extraction recorded under it wrote, and the two carry slots
//   the route (OrbPipeRoute)   where the work of one call runs, decided once: chains (sub-batch j on the stream of pipe
//                              (rot + j) mod P_eff) or lanes (a stream per stage group, handle (lane_rot + j) mod sets as buffer set)
//   the walk (orb_pipe_call)   the operations of one call in the order they are enqueued, as calls on a sink
// Streams are indices into the pipeline's pool (orbfe_pipe_plan.h deals them), events a {kind, index} pair.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "orbfe_pipe_plan.h"

#define ORB_PIPE_KEYPOINT_BYTES 28   // sizeof(orbfe_keypoint)
#define ORB_PIPE_DESC_BYTES 32
#define ORB_PIPE_CALLER (-1)         // the stream of the caller, which is none of the pool
#define ORB_PIPE_CONTINUE 1          // ORBFE_PIPE_CONTINUE

// ---- the address ledger ---------------------------------------------------------------------------
struct OrbSpan {
    uintptr_t at = 0;   // 0: nothing
    size_t bytes = 0;
};

// the keypoint, descriptor and count bytes of some frames of a call's output blocks
struct OrbSlice {
    OrbSpan k, d, n;
};

static inline bool orb_overlaps(const OrbSpan &a, const OrbSpan &b) { return a.at && b.at && a.at < b.at + b.bytes && b.at < a.at + a.bytes; }
static inline bool orb_overlaps(const OrbSlice &a, const OrbSlice &b) { return orb_overlaps(a.k, b.k) || orb_overlaps(a.d, b.d) || orb_overlaps(a.n, b.n); }

// the output blocks of a call: rows of `cap` keypoints / descriptors and one count per frame
struct OrbPipeBlocks {
    uintptr_t kps = 0, desc = 0, n = 0;
    int32_t cap = 0;
};

// frames lo .. lo + nf - 1 of the blocks
static inline OrbSlice orb_slice(const OrbPipeBlocks &b, int32_t lo, int32_t nf)
{
    const size_t cap = (size_t)b.cap, rows = (size_t)nf * cap;
    OrbSlice s;
    s.k.at = b.kps + (size_t)lo * cap * ORB_PIPE_KEYPOINT_BYTES;
    s.k.bytes = rows * ORB_PIPE_KEYPOINT_BYTES;
    s.d.at = b.desc + (size_t)lo * cap * ORB_PIPE_DESC_BYTES;
    s.d.bytes = rows * ORB_PIPE_DESC_BYTES;
    s.n.at = b.n + (size_t)lo * sizeof(int32_t);
    s.n.bytes = (size_t)nf * sizeof(int32_t);
    return s;
}

enum OrbPipeEventKind {
    ORB_EV_FORK,    // the caller's stream at the start of the call
    ORB_EV_EXT,     // per sub-batch index: behind the extraction last recorded under it
    ORB_EV_MATCH,   // per sub-batch index: behind its matcher
    ORB_EV_CARRY,   // per carry slot: behind the copy that wrote it
    ORB_EV_M0,      // per carry slot: behind the frame-0 match that read it
    ORB_EV_END      // per stream of a call, in the order of OrbPipeRoute::streams: behind its last piece of the most recent call
};

struct OrbPipeEvent {
    OrbPipeEventKind kind;
    int32_t index;
};

struct OrbPipeState {
    // what the events of sub-batch index j stand for.  A later call that lays its sub-batches over other addresses (shifted base
    // pointer, another call size) is ordered by ADDRESS, not by index.  (The events of indices a call does not use keep their last
    // record: a later, longer call still orders itself behind whatever touched those slices last.)
    struct Index {
        OrbSlice slice, before;   // `before`: what `slice` was until the call in flight (or last made) recorded its own
        bool ext_valid = false, match_valid = false;
        int32_t carry = -1;   // the carry slot that the slice's last frame was copied into behind its matcher; -1: none was
    };
    std::vector<Index> index;
    // the last frame of the previous call lives in one of two slots, written alternately
    int32_t carry_cur = 0;        // slot the NEXT call reads
    bool have_carry = false;
    bool m0_valid[2] = {false, false};        // ORB_EV_M0 of the slot has been recorded and not yet waited for by a copy into the slot
    bool carry_written[2] = {false, false};
    bool end_valid[ORBFE_PIPE_MAX_PIPES] = {};   // ORB_EV_END i has been recorded
    int32_t rot = 0;        // chains: pipe of sub-batch 0 of the next call: consecutive short calls take turns on the pipes
    int32_t lane_rot = 0;   // lanes: buffer set of sub-batch 0 of the next call

    void new_sequence() { have_carry = false; }   // the next call has no predecessor frame
    // after a call failed midway and the pipeline's streams have been drained: every event is complete, the sequence starts over
    void reset()
    {
        have_carry = false;
        m0_valid[0] = m0_valid[1] = false;
    }
};

// ---- the route of a call --------------------------------------------------------------------------
struct OrbPipeRoute {
    int32_t lanes;   // 0: chains, 1: lanes (only the extractor call itself differs: a stream, or one per stage group)
    int32_t sets;    // handles that take the sub-batches in turn
    int32_t first;   // handle of sub-batch 0
    int32_t lane[4] = {-1, -1, -1, -1};   // lanes: the streams of pyramid, FAST, quadtree + descriptor, blur
    int32_t fast_odd = -1;                // lanes: the FAST stream of odd sub-batches (lane[1] unless placement 2 gives FAST two streams)
    // per handle: where its extraction starts (what must precede it is waited for there), where it ends, and its matcher's stream
    int32_t start_of[ORBFE_PIPE_MAX_PIPES] = {}, tail_of[ORBFE_PIPE_MAX_PIPES] = {}, match_of[ORBFE_PIPE_MAX_PIPES] = {};
    int32_t nstreams;   // streams that carry work of the call ...
    int32_t streams[ORBFE_PIPE_MAX_PIPES] = {};   // ... (lanes: the side stream last; the rule has P > 3, so there is a fourth ORB_EV_END)
    int32_t OrbPipeState::*turn;   // the rotation the call advances

    // `lane_mode`: -1 the library's choice, 0 never, 1 wherever the rule `lr` allows lanes.  `place` (-1: ORBFE_PIPE_LANE_PLACE) 1: blur
    // on the side stream, matcher behind the descriptor on kernel stream 2; 0: blur behind the pyramid on kernel stream 0, matcher on
    // the side stream; 2: blur behind the pyramid, matcher behind the descriptor, and the side stream takes the FAST launches of odd
    // sub-batches.  `first_pipe` >= 0: the pipe of a chain call's sub-batch 0 instead of the state's rotation.
    OrbPipeRoute(const OrbPipePlan &plan, const OrbPipeLanes &lr, int32_t lane_mode, int32_t place, int32_t first_pipe, const OrbPipeState &g)
    {
        lanes = lr.lanes && (lane_mode < 0 ? ORBFE_PIPE_LANES_AUTO != 0 : lane_mode != 0);
        sets = lanes ? lr.sets : plan.P_eff;
        turn = lanes ? &OrbPipeState::lane_rot : &OrbPipeState::rot;
        first = (lanes || first_pipe < 0 ? g.*turn : first_pipe) % sets;
        const int32_t side = plan.side_index, k0 = plan.first;
        const int32_t pc = place < 0 ? ORBFE_PIPE_LANE_PLACE : place;
        const bool blur_on_side = pc == 1, match_on_side = pc == 0;
        if (lanes) lane[0] = k0, lane[1] = k0 + 1, lane[2] = k0 + 2, lane[3] = blur_on_side ? side : k0, fast_odd = pc == 2 ? side : lane[1];
        for (int32_t h = 0; h < sets; ++h) {
            const int32_t chain = k0 + plan.stream_of_pipe[h];
            start_of[h] = lanes ? lane[0] : chain;
            tail_of[h] = lanes ? lane[2] : chain;
            match_of[h] = lanes ? (match_on_side ? side : lane[2]) : chain;
        }
        nstreams = lanes ? ORBFE_PIPE_LANE_STREAMS + 1 : plan.P_eff;
        for (int32_t i = 0; i < nstreams; ++i) streams[i] = lanes && i == ORBFE_PIPE_LANE_STREAMS ? side : k0 + i;
    }
    int32_t handle(int32_t j) const { return (first + j) % sets; }
    int32_t start(int32_t j) const { return start_of[handle(j)]; }
    int32_t tail(int32_t j) const { return tail_of[handle(j)]; }
    int32_t matcher(int32_t j) const { return match_of[handle(j)]; }
    int32_t fast(int32_t j) const { return (j & 1) ? fast_odd : lane[1]; }   // lanes: the FAST stream of sub-batch j
    int32_t carry(int32_t nsub) const { return matcher(nsub - 1); }   // the carry copy: with the last sub-batch's matcher
};

// ---- the walk -------------------------------------------------------------------------------------
struct OrbPipeCall {
    OrbPipeRoute route;
    OrbPipeBlocks out;
    int32_t F, nframes;    // frames per sub-batch, frames of the call
    bool match;            // the call has match blocks
    int32_t flags;
};

#define ORB_PIPE_DO(call)               \
    do {                                \
        const int32_t s__ = (call);     \
        if (s__ != 0) return s__;       \
    } while (0)

// One call.  The sink's methods answer an orbfe_status; the first that is not ORBFE_OK ends the walk and is returned, with launches
// of the call in flight and the ledger half updated: the caller drains its streams and resets the state.
//   wait(stream, event) / record(stream, event)
//   extract(handle, lo, nf, route)            frames lo .. lo + nf - 1 into their slices, from route.start_of[handle] to .tail_of[handle];
//                                             lanes: route.lane[] holds the stage streams of THIS sub-batch (lane[1] = route.fast(j))
//   match(handle, stream, q0, np)             rows q0 .. q0 + np - 1: frame q against frame q - 1
//   match_carry(handle, stream, slot)         row 0: frame 0 against the frame in the carry slot
//   clear_row0(stream)                        row 0 of a frame without predecessor: all -1, count 0
//   carry_copy(stream, slot, last_frame)      the call's last frame into the slot
template <class Sink>
int32_t orb_pipe_call(OrbPipeState &g, const OrbPipeCall &c, Sink &sink)
{
    const OrbPipeRoute &r = c.route;
    const int32_t nsub = (c.nframes + c.F - 1) / c.F;
    if (g.index.size() < (size_t)nsub + 1) g.index.resize((size_t)nsub + 1);
    const bool cont = (c.flags & ORB_PIPE_CONTINUE) != 0 && g.have_carry && c.match;
    OrbPipeRoute rj = r;   // the route as sub-batch j sees it: its own FAST stream in lane[1]
    const int32_t rd = g.carry_cur, wr = g.carry_cur ^ 1;

    // fork: the streams start behind whatever the caller's stream holds (the producer of the frames, the consumer of the output
    // blocks of an earlier call)
    ORB_PIPE_DO(sink.record(ORB_PIPE_CALLER, OrbPipeEvent{ORB_EV_FORK, 0}));
    for (int32_t i = 0; i < r.nstreams; ++i) ORB_PIPE_DO(sink.wait(r.streams[i], OrbPipeEvent{ORB_EV_FORK, 0}));

    for (int32_t j = 0; j < nsub; ++j) {
        const int32_t h = r.handle(j), st = r.start(j), sx = r.tail(j), sm = r.matcher(j);
        const int32_t lo = j * c.F, nf = c.nframes - lo < c.F ? c.nframes - lo : c.F;
        const OrbSlice mine = orb_slice(c.out, lo, nf);
        // The output blocks may be the ones of the previous call (a host that re-uses its buffers), and the handles take turns: what
        // the PREVIOUS call did with slices j happened on other streams.  This sub-batch overwrites them only after that call's
        // extraction of sub-batch j (write after write), its matcher of sub-batch j (queries) and its matcher of sub-batch j + 1
        // (whose first pair reads the last frame of slice j) have finished.  (Events of finished work cost nothing.)
        auto wait_index = [&](size_t i) -> int32_t {   // everything that wrote or read the slices recorded under index i
            if (g.index[i].ext_valid) ORB_PIPE_DO(sink.wait(st, OrbPipeEvent{ORB_EV_EXT, (int32_t)i}));
            if (g.index[i].match_valid) ORB_PIPE_DO(sink.wait(st, OrbPipeEvent{ORB_EV_MATCH, (int32_t)i}));
            if (i + 1 < g.index.size() && g.index[i + 1].match_valid) ORB_PIPE_DO(sink.wait(st, OrbPipeEvent{ORB_EV_MATCH, (int32_t)i + 1}));
            // ... and the copy of their last frame into a carry slot must have read it (only a sub-batch that writes over these
            // slices waits: no drain at the call boundary)
            if (g.index[i].carry >= 0) ORB_PIPE_DO(sink.wait(st, OrbPipeEvent{ORB_EV_CARRY, g.index[i].carry}));
            return 0;
        };
        // index j (its events are about to be re-recorded), and every other index whose recorded slices overlap this sub-batch's:
        // with the usual re-use of the same buffers and call size that is index j alone.  Recorded BEFORE THIS CALL: an index below j
        // stands for this call's own sub-batch by now, which waited for everything its index stood for and is waited for in its stead.
        ORB_PIPE_DO(wait_index((size_t)j));
        for (size_t i = 0; i < g.index.size(); ++i)
            if ((int32_t)i != j && orb_overlaps((int32_t)i < j ? g.index[i].before : g.index[i].slice, mine)) ORB_PIPE_DO(wait_index(i));
        if (r.lanes) rj.lane[1] = r.fast(j);
        ORB_PIPE_DO(sink.extract(h, lo, nf, rj));
        ORB_PIPE_DO(sink.record(sx, OrbPipeEvent{ORB_EV_EXT, j}));
        g.index[(size_t)j].ext_valid = true;
        g.index[(size_t)j].before = g.index[(size_t)j].slice;
        g.index[(size_t)j].slice = mine;
        g.index[(size_t)j].carry = -1;
        if (!c.match) continue;
        // (lanes: the matcher's writes into the match rows follow the previous call's through this sub-batch's extraction, which
        // waited for them above)
        if (sm != sx) ORB_PIPE_DO(sink.wait(sm, OrbPipeEvent{ORB_EV_EXT, j}));
        if (j > 0) ORB_PIPE_DO(sink.wait(sm, OrbPipeEvent{ORB_EV_EXT, j - 1}));   // frame lo - 1 comes from the neighbour
        const int32_t q0 = lo == 0 ? 1 : lo, np = lo + nf - q0;
        if (np > 0) ORB_PIPE_DO(sink.match(h, sm, q0, np));
        if (lo == 0) {
            if (cont) {
                ORB_PIPE_DO(sink.wait(sm, OrbPipeEvent{ORB_EV_CARRY, rd}));
                ORB_PIPE_DO(sink.match_carry(h, sm, rd));
                ORB_PIPE_DO(sink.record(sm, OrbPipeEvent{ORB_EV_M0, rd}));   // slot rd has been read: the NEXT call may write it
                g.m0_valid[rd] = true;
            } else {   // the first frame of a sequence has no predecessor
                ORB_PIPE_DO(sink.clear_row0(sm));
            }
        }
        ORB_PIPE_DO(sink.record(sm, OrbPipeEvent{ORB_EV_MATCH, j}));
        g.index[(size_t)j].match_valid = true;
    }

    // carry: the last frame of this call, for the first frame of the next one, on the last sub-batch's matcher stream (lanes: behind
    // its extraction on the tail stream).  Slot `wr` was read by the PREVIOUS call's frame-0 match, on whatever stream that call's
    // sub-batch 0 ran: the copy waits for that match's own event ...
    const int32_t cs = r.carry(nsub);
    if (cs != r.tail(nsub - 1)) ORB_PIPE_DO(sink.wait(cs, OrbPipeEvent{ORB_EV_EXT, nsub - 1}));
    if (g.m0_valid[wr]) {
        ORB_PIPE_DO(sink.wait(cs, OrbPipeEvent{ORB_EV_M0, wr}));
        g.m0_valid[wr] = false;
    }
    // ... and behind the previous WRITER of the slot (two calls ago, possibly on another stream): calls without a frame-0 match
    // (extract only, no CONTINUE) record no ORB_EV_M0, and nothing else would order the two copies
    if (g.carry_written[wr]) ORB_PIPE_DO(sink.wait(cs, OrbPipeEvent{ORB_EV_CARRY, wr}));
    ORB_PIPE_DO(sink.carry_copy(cs, wr, c.nframes - 1));
    ORB_PIPE_DO(sink.record(cs, OrbPipeEvent{ORB_EV_CARRY, wr}));
    g.carry_written[wr] = true;
    g.carry_cur = wr;
    g.have_carry = true;
    g.index[(size_t)nsub - 1].carry = wr;

    for (int32_t i = 0; i < r.nstreams; ++i) {
        ORB_PIPE_DO(sink.record(r.streams[i], OrbPipeEvent{ORB_EV_END, i}));
        g.end_valid[i] = true;
    }
    g.*r.turn = (r.first + nsub) % r.sets;
    return 0;
}

#undef ORB_PIPE_DO

// orbfe_pipe_plan.h -- the sequence pipeline's stream plan, made on the host without a device call: how many streams a pipeline
// of P pipes creates on a runtime that has Q hardware queues, and which stream every pipe launches on.  orbfe_pipeline.hip
// creates what orb_pipe_plan returns; tests/test_pipe_plan.py and tests/cpp/test_pipe_plan_sanitize.cpp reach it without a GPU.
//
// Why a plan: the HIP runtime gives every stream one hardware queue for life and, once all Q queues are taken, lets further
// streams share them.  Packets of one queue run in submission order, so a cross-stream wait (hipStreamWaitEvent) of one stream
// holds everything that was submitted behind it to the same queue -- the kernels of the OTHER streams on that queue included.
// Two kernel streams on one queue therefore cannot overlap, and a wait of one of them stalls the other: a pipeline never creates
// more kernel-carrying streams than there are queues.  A queue also runs one kernel at a time, so Q bounds the kernels in flight
// whatever the streams are: what the plan decides is which Q kernels those are.  Measured on 4 queues with 12 pipes asked for
// (profiles/pipe_queues.md): 3 kernel streams + the side stream that puts the blur beside the latency-bound quadtree beat 4 kernel
// streams with the blur in line, which equal 12 streams that share the queues.
// The second half of the file is the other cut over the same four streams, by stage (lanes), with its three placements: since
// profiles/pipe_fast2.md the default gives two of the four streams to the FAST launches of even and odd sub-batches.
#pragma once

#include <errno.h>
#include <stdint.h>
#include <stdlib.h>

#define ORBFE_PIPE_MAX_PIPES 64        // orbfe_pipeline_create's upper bound
#define ORBFE_PIPE_DEFAULT_QUEUES 4    // the runtime's own default of GPU_MAX_HW_QUEUES
#define ORBFE_PIPE_MAX_QUEUES 32       // more queues than this count as this many
#define ORBFE_PIPE_COPY_STREAMS 2      // H2D and D2H stream of the host entry point (orbfe_pipeline_extract_match)

struct OrbPipePlan {
    int32_t P, Q, copies;   // the inputs: pipes asked for, hardware queues (clamped to 1..ORBFE_PIPE_MAX_QUEUES), copy streams in use
    int32_t S;              // kernel streams
    int32_t P_eff;          // pipes that get work = min(P, S): sub-batch j of a call runs on pipe (rot + j) mod P_eff
    int32_t side;           // 1: one side stream, shared by the pipes' blur; 0: every pipe's blur runs in the pipe's own stream
    // the pipeline's streams in creation order: [0, first) the copy streams, [first, first + S) the kernel streams, then the side stream
    int32_t first, side_index /* -1: none */, nstreams;
    int32_t stream_of_pipe[ORBFE_PIPE_MAX_PIPES];   // kernel stream (0 .. S - 1) of pipe i < P; pipes beyond P_eff double up on them
};

// The value of GPU_MAX_HW_QUEUES as the runtime will take it, from the variable's text: null, empty, not a number or below 1 is
// the default, anything above ORBFE_PIPE_MAX_QUEUES counts as ORBFE_PIPE_MAX_QUEUES.
static inline int32_t orb_pipe_parse_queues(const char *text)
{
    if (!text || !*text) return ORBFE_PIPE_DEFAULT_QUEUES;
    char *end = nullptr;
    errno = 0;
    const long long v = strtoll(text, &end, 10);
    if (end == text) return ORBFE_PIPE_DEFAULT_QUEUES;
    while (*end == ' ' || *end == '\t' || *end == '\n' || *end == '\r') ++end;
    if (*end) return ORBFE_PIPE_DEFAULT_QUEUES;   // trailing text: not a number
    if (errno == ERANGE) return v > 0 ? ORBFE_PIPE_MAX_QUEUES : ORBFE_PIPE_DEFAULT_QUEUES;
    if (v < 1) return ORBFE_PIPE_DEFAULT_QUEUES;
    return v > ORBFE_PIPE_MAX_QUEUES ? ORBFE_PIPE_MAX_QUEUES : (int32_t)v;
}

// the process's hardware queues: the environment is read once, here and nowhere else (the runtime reads it once as well)
static inline int32_t orb_pipe_env_queues()
{
    static const int32_t q = orb_pipe_parse_queues(getenv("GPU_MAX_HW_QUEUES"));
    return q;
}

// The plan of P pipes on Q queues.  The copy streams, where in use, come first: they take their queues off the top.  If what is
// left holds P kernel streams and a side stream the plan is the one the pipeline was tuned with on 16 queues (P + 1 streams);
// otherwise the last queue that is left goes to the side stream and every other one to a kernel stream -- with a single queue
// left there is one kernel stream and the blur runs in it.  False (and *out untouched) for a P outside
// 1 .. ORBFE_PIPE_MAX_PIPES; any Q is clamped.
static inline bool orb_pipe_plan(int32_t P, int32_t Q, bool copies, OrbPipePlan *out)
{
    if (!out || P < 1 || P > ORBFE_PIPE_MAX_PIPES) return false;
    OrbPipePlan pl;
    pl.P = P;
    pl.Q = Q < 1 ? 1 : (Q > ORBFE_PIPE_MAX_QUEUES ? ORBFE_PIPE_MAX_QUEUES : Q);
    pl.copies = copies ? 1 : 0;
    pl.first = copies ? ORBFE_PIPE_COPY_STREAMS : 0;
    const int32_t left = pl.Q - pl.first < 1 ? 1 : pl.Q - pl.first;   // queues for kernel-carrying streams
    pl.side = left >= 2 ? 1 : 0;
    pl.S = left >= P + 1 ? P : (pl.side ? left - 1 : 1);
    pl.P_eff = P < pl.S ? P : pl.S;
    pl.side_index = pl.side ? pl.first + pl.S : -1;
    pl.nstreams = pl.first + pl.S + pl.side;
    for (int32_t i = 0; i < ORBFE_PIPE_MAX_PIPES; ++i) pl.stream_of_pipe[i] = i < P ? i % pl.S : -1;
    *out = pl;
    return true;
}

// Lanes: the other way to cut a device-entry call over the same four streams.  A chain (above) runs a whole sub-batch on one
// kernel stream; with 3 chains the VALU-bound FAST pass of some sub-batch is in flight only 59 % of the time and two of them
// compete for the same issue slots a third of it (profiles/pipe_queues.md).  In lanes the streams are dealt by STAGE: one kernel
// stream carries nothing but FAST, back to back, and the other three feed it the pyramid, the blur and the quadtree / descriptor /
// matcher of neighbouring sub-batches; `sets` extractor handles serve as rotating buffer sets, sub-batch j on set
// (rot + j) mod sets.  profiles/pipe_lanes.md has the measurements.
//
// Placement 2 gives FAST two of the four streams: a queue starts a kernel only when its predecessor has drained, so on one FAST
// stream every launch ends in a tail in which FAST's wave slots empty out and FAST cannot refill them.  With the FAST launches of
// even sub-batches on kernel stream 1 and of odd ones on the side stream, launch j + 1 places waves as those of launch j retire;
// the blur moves in behind the pyramid (as in placement 0) and the matcher stays behind the descriptor (as in placement 1).
// Nothing relies on FAST launches being in stream order: consecutive sub-batches use different buffer sets, and a set that comes
// back on the other FAST stream (an odd number of sets) is ordered by its handle's events like any re-use.  The lane defaults
// below can be set on the compiler's command line for A/B builds; profiles/pipe_fast2.md has the measurements.
#ifndef ORBFE_PIPE_LANE_SETS
#define ORBFE_PIPE_LANE_SETS 8         // buffer sets of a lane call (at most P): 3, 4, 6, 8 measured, each a little faster than the last
#endif
// the placements: 0: blur behind the pyramid on kernel stream 0, matcher on the side stream; 1: blur on the side stream, matcher
// behind the descriptor (where chains have both; 0 against 1: a tie at 4 sets); 2: blur behind the pyramid, matcher behind the
// descriptor, FAST on kernel stream 1 and the side stream in turn
#define ORBFE_PIPE_LANE_PLACE 1        // what a route (orbfe_pipe_graph.h) that is given no placement takes
#ifndef ORBFE_PIPE_LANE_PLACE_AUTO
#define ORBFE_PIPE_LANE_PLACE_AUTO 2   // what a pipeline left to itself asks its routes for: +2.4 % over placement 1 with a matcher
                                       // that fits beside two FAST workgroups, -5 % with one that does not (profiles/pipe_fast2.md)
#endif
#ifndef ORBFE_PIPE_LANE_MATCH_TILES
#define ORBFE_PIPE_LANE_MATCH_TILES 4  // query tiles per wave of a lane call's brute-force matcher (4, 2, 1: orbfe_match.hip): fewer
                                       // tiles are fewer registers.  The FP4 kernel's 4-tile form (174 registers) fits where ONE FAST
                                       // workgroup has left, which only the 2-tile form of the int8 kernel (176 against 253) did.
                                       // Measured with placement 2 (profiles/match_fp4.md): 4 tiles +1.1 % over 2, 1 tile -1.3 %
#endif
#define ORBFE_PIPE_LANE_PLACES 3       // placements 0 .. 2
#define ORBFE_PIPE_LANES_AUTO 1        // what a pipeline left to itself does where the rule allows lanes: 1 lanes, 0 chains
#define ORBFE_PIPE_LANE_STREAMS 3      // the kernel streams lanes are defined for; with the side stream: four stage streams

struct OrbPipeLanes {
    int32_t lanes;   // 1: the call runs in lanes; 0: in chains, as orb_pipe_plan lays them out
    int32_t sets;    // lanes: extractor handles in rotation; chains: the plan's P_eff
};

// Whether a call of `nsub` sub-batches on `plan` can run in lanes: the plan has no copy streams (the device entry point), is
// short of queues (S < P: with P + 1 streams every sub-batch has a queue of its own and chains are the faster cut), has exactly
// the 3 kernel streams + side stream that the stages are dealt to, and the call has at least two sub-batches (one sub-batch
// has no neighbour to overlap with).  `want_sets` < 1: ORBFE_PIPE_LANE_SETS.
static inline OrbPipeLanes orb_pipe_lanes(const OrbPipePlan &plan, int32_t nsub, int32_t want_sets = 0)
{
    OrbPipeLanes r;
    r.lanes = (plan.copies == 0 && plan.S < plan.P && plan.S == ORBFE_PIPE_LANE_STREAMS && plan.side == 1 && nsub >= 2) ? 1 : 0;
    const int32_t n = want_sets < 1 ? ORBFE_PIPE_LANE_SETS : want_sets;
    r.sets = r.lanes ? (plan.P < n ? plan.P : n) : plan.P_eff;
    return r;
}

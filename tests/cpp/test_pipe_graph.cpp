// The sequence pipeline's call graph (csrc/orbfe_pipe_graph.h) on its own: a header, no device, no library; built plain and with
// -fsanitize=address,undefined by tests/test_pipe_graph.py.  Reads a script of pipeline calls from stdin, one per line --
//   call <pipes> <queues> <copies> <lane mode> <sets> <place> <F> <cap> <nframes> <base frame> <match blocks 0/1> <flags> [<fail at>]
//   reset_sequence
// -- keeps ONE pipeline state over the whole script, as a pipeline handle does, and prints the operations a logging sink received,
// one per line, then "status <s>" for every call.  Streams are pool indices (-1: the caller's).  <base frame>: the output blocks
// of the call start that many frames into the caller's arrays (all blocks move together).  <fail at> k: the sink's k-th call of
// this script line answers -4 instead of 0; the program then resets the state, as the pipeline does behind its drain.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "orbfe_pipe_graph.h"

static const char *const KIND[] = {"fork", "ext", "match", "carry", "m0", "end"};

struct LogSink {
    int calls = 0, fail_at = 0;
    int32_t step() { return ++calls == fail_at ? -4 : 0; }
    int32_t wait(int32_t s, OrbPipeEvent e)
    {
        if (step()) return -4;
        printf("wait %d %s %d\n", s, KIND[e.kind], e.index);
        return 0;
    }
    int32_t record(int32_t s, OrbPipeEvent e)
    {
        if (step()) return -4;
        printf("record %d %s %d\n", s, KIND[e.kind], e.index);
        return 0;
    }
    int32_t extract(int32_t h, int32_t lo, int32_t nf, const OrbPipeRoute &r)
    {
        if (step()) return -4;
        if (h < 0 || h >= r.sets) abort();
        printf("extract %d %d %d %d %d %d %d %d %d\n", h, lo, nf, r.start_of[h], r.tail_of[h], r.lane[0], r.lane[1], r.lane[2], r.lane[3]);
        return 0;
    }
    int32_t match(int32_t h, int32_t s, int32_t q0, int32_t np)
    {
        if (step()) return -4;
        printf("match %d %d %d %d\n", h, s, q0, np);
        return 0;
    }
    int32_t match_carry(int32_t h, int32_t s, int32_t slot)
    {
        if (step()) return -4;
        printf("match_carry %d %d %d\n", h, s, slot);
        return 0;
    }
    int32_t clear_row0(int32_t s)
    {
        if (step()) return -4;
        printf("clear_row0 %d\n", s);
        return 0;
    }
    int32_t carry_copy(int32_t s, int32_t slot, int32_t last)
    {
        if (step()) return -4;
        printf("carry_copy %d %d %d\n", s, slot, last);
        return 0;
    }
};

static int fail(const char *what, const char *line)
{
    fprintf(stderr, "%s: %s\n", what, line);
    return 1;
}

int main()
{
    char line[512];
    int n = 0;
    OrbPipeState *g = new OrbPipeState();
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\n")] = 0;
        ++n;
        if (!strcmp(line, "reset_sequence")) {
            g->new_sequence();
            printf("reset_sequence\n");
            continue;
        }
        int P, Q, copies, mode, sets, place, F, cap, nframes, base, match, flags, fail_at = 0;
        if (strncmp(line, "call ", 5) || sscanf(line + 5, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &P, &Q, &copies, &mode, &sets, &place, &F, &cap,
                                                &nframes, &base, &match, &flags, &fail_at) < 12)
            return fail("bad request", line);
        if (F < 1 || cap < 1 || nframes < 1 || base < 0) return fail("bad call", line);
        OrbPipePlan plan;
        if (!orb_pipe_plan(P, Q, copies != 0, &plan)) return fail("bad plan", line);
        g->rot %= plan.P_eff;   // (what the pipeline does when it takes a plan)
        const int nsub = (nframes + F - 1) / F;
        // the caller's arrays: far apart, so that only equal blocks overlap
        OrbPipeBlocks out;
        out.cap = cap;
        out.kps = (uintptr_t)0x100000000ull + (uintptr_t)base * cap * ORB_PIPE_KEYPOINT_BYTES;
        out.desc = (uintptr_t)0x200000000ull + (uintptr_t)base * cap * ORB_PIPE_DESC_BYTES;
        out.n = (uintptr_t)0x300000000ull + (uintptr_t)base * sizeof(int32_t);
        OrbPipeCall *c = new OrbPipeCall{OrbPipeRoute(plan, orb_pipe_lanes(plan, nsub, sets), mode, place, -1, *g), out, F, nframes, match != 0, flags};
        const OrbPipeRoute &r = c->route;
        if (r.sets < 1 || r.sets > P || r.first < 0 || r.first >= r.sets || r.nstreams < 1 || r.nstreams > plan.nstreams) return fail("route", line);
        for (int h = 0; h < r.sets; ++h)
            for (int s : {r.start_of[h], r.tail_of[h], r.match_of[h]})
                if (s < plan.first || s >= plan.nstreams) return fail("route stream", line);
        LogSink sink;
        sink.fail_at = fail_at;
        const int32_t s = orb_pipe_call(*g, *c, sink);
        if (s != 0) g->reset();
        if ((s != 0) != (fail_at > 0 && sink.calls == fail_at)) return fail("status", line);
        printf("status %d\n", s);
        delete c;
    }
    delete g;
    return n ? 0 : 2;
}

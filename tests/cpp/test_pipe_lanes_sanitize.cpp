// The pipeline's lane rule (orb_pipe_lanes, csrc/orbfe_pipe_plan.h) on its own, for a host build with -fsanitize=address,undefined:
// a header, no device, no library.  Reads one request per line from stdin --
//   lanes <P> <Q> <copies> <nsub>    -> "<ok> lanes sets" ("0" where the planner refuses P)
// -- and checks the answer's own invariants before printing it.  tests/test_pipe_lanes.py compiles it, feeds it the grid and compares
// the lines with the library's test hook.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "orbfe_pipe_plan.h"

static int fail(const char *what, const char *line)
{
    fprintf(stderr, "%s: %s\n", what, line);
    return 1;
}

int main()
{
    char line[512];
    int n = 0;
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\n")] = 0;
        ++n;
        int P, Q, copies, nsub;
        if (strncmp(line, "lanes ", 6) || sscanf(line + 6, "%d %d %d %d", &P, &Q, &copies, &nsub) != 4) return fail("bad request", line);
        OrbPipePlan *pl = (OrbPipePlan *)malloc(sizeof(OrbPipePlan));   // blocks of exactly their size
        OrbPipeLanes *r = (OrbPipeLanes *)malloc(sizeof(OrbPipeLanes));
        memset(pl, 0x5a, sizeof *pl);
        memset(r, 0x5a, sizeof *r);
        if (!orb_pipe_plan(P, Q, copies != 0, pl)) {
            printf("0\n");
        } else {
            *r = orb_pipe_lanes(*pl, nsub);
            if (r->lanes != 0 && r->lanes != 1) return fail("lanes", line);
            if (r->sets < 1 || r->sets > pl->P) return fail("sets", line);
            if (r->lanes ? (pl->S != ORBFE_PIPE_LANE_STREAMS || !pl->side || pl->copies || r->sets > ORBFE_PIPE_LANE_SETS) : r->sets != pl->P_eff)
                return fail("rule", line);
            for (int want = 1; want <= 8; ++want) {   // another number of buffer sets never leaves the pipes
                const OrbPipeLanes w = orb_pipe_lanes(*pl, nsub, want);
                if (w.lanes != r->lanes || w.sets < 1 || w.sets > pl->P || (w.lanes && w.sets > want)) return fail("asked sets", line);
            }
            printf("1 %d %d\n", r->lanes, r->sets);
        }
        free(r);
        free(pl);
    }
    return n ? 0 : 2;
}

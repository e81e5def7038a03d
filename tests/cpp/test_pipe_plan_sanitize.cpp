// The pipeline's stream planner (csrc/orbfe_pipe_plan.h) on its own, for a host build with -fsanitize=address,undefined: a
// header, no device, no library.  Reads one request per line from stdin --
//   plan <P> <Q> <copies>    -> "<ok> P Q copies S P_eff side first side_index nstreams | stream of pipe 0 .. P - 1"
//   parse <text>             -> the queue count orb_pipe_parse_queues makes of <text> (the rest of the line; may be empty)
//   parse-null               -> ... of a null pointer (the variable is not set)
//   env                      -> orb_pipe_env_queues() and what orb_pipe_parse_queues makes of this process's variable
// -- and checks every plan's own invariants before printing it.  tests/test_pipe_plan.py compiles it, feeds it the grid and compares
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
        if (!strncmp(line, "plan ", 5)) {
            int P, Q, copies;
            if (sscanf(line + 5, "%d %d %d", &P, &Q, &copies) != 3) return fail("bad plan line", line);
            OrbPipePlan *pl = (OrbPipePlan *)malloc(sizeof(OrbPipePlan));   // a block of exactly its size
            memset(pl, 0x5a, sizeof *pl);
            const bool ok = orb_pipe_plan(P, Q, copies != 0, pl);
            if (!ok) {
                printf("0\n");
                free(pl);
                continue;
            }
            if (pl->S < 1 || pl->P_eff < 1 || pl->P_eff > pl->S || pl->nstreams != pl->first + pl->S + pl->side) return fail("counts", line);
            for (int i = 0; i < ORBFE_PIPE_MAX_PIPES; ++i) {
                const int s = pl->stream_of_pipe[i];
                if (i < P ? (s < 0 || s >= pl->S) : s != -1) return fail("stream of pipe", line);
            }
            printf("1 %d %d %d %d %d %d %d %d %d |", pl->P, pl->Q, pl->copies, pl->S, pl->P_eff, pl->side, pl->first, pl->side_index, pl->nstreams);
            for (int i = 0; i < P; ++i) printf(" %d", pl->stream_of_pipe[i]);
            printf("\n");
            free(pl);
        } else if (!strncmp(line, "parse-null", 10)) {
            printf("%d\n", orb_pipe_parse_queues(nullptr));
        } else if (!strncmp(line, "parse", 5)) {
            const char *t = line[5] == ' ' ? line + 6 : line + 5;
            char *copy = (char *)malloc(strlen(t) + 1);   // exactly as long as the text: a read past its end is caught
            strcpy(copy, t);
            printf("%d\n", orb_pipe_parse_queues(copy));
            free(copy);
        } else if (!strcmp(line, "env")) {
            printf("%d %d\n", orb_pipe_env_queues(), orb_pipe_parse_queues(getenv("GPU_MAX_HW_QUEUES")));
        } else {
            return fail("bad request", line);
        }
    }
    return n ? 0 : 2;
}

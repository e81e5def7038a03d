// The automatic FAST mode (csrc/orbfe_fast_auto.h) on its own, for a host build with -fsanitize=address,undefined: a header, no
// device, no library.  Reads the calls of one fresh handle from stdin, one per line --
//   <row steps> <pending> [<c0> <c1> <c2>]     the counters of a probe that answered before the call, if any
// -- and prints "<form> <probe>" per call.  An answer that arrives before a small call waits for the next large one, as in the
// library (orbfe_api.hip does not collect then).  tests/test_fast_auto.py compiles it and compares the lines with the library's hook.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "orbfe_fast_auto.h"

int main()
{
    char line[256];
    int n = 0;
    OrbFastAuto *st = new OrbFastAuto();   // a block of exactly its size
    uint64_t *waiting = nullptr;
    while (fgets(line, sizeof line, stdin)) {
        int64_t steps;
        int pending;
        uint64_t c[3];
        const int got = sscanf(line, "%" SCNd64 " %d %" SCNu64 " %" SCNu64 " %" SCNu64, &steps, &pending, &c[0], &c[1], &c[2]);
        if (got != 2 && got != 5) {
            fprintf(stderr, "bad call line: %s", line);
            return 2;
        }
        if (got == 5) {
            free(waiting);
            waiting = (uint64_t *)malloc(3 * sizeof(uint64_t));
            for (int i = 0; i < 3; ++i) waiting[i] = c[i];
        }
        if (waiting && !orb_fast_auto_small(steps)) {
            orb_fast_auto_answer(*st, waiting);
            free(waiting);
            waiting = nullptr;
        }
        const OrbFastChoice ch = orb_fast_auto_choose(*st, steps, pending != 0);
        if ((ch.form != 0 && ch.form != 2) || (ch.probe && ch.form != 2) || st->dense_left < 0 || st->hold < ORBFE_AUTO_HOLD_MIN ||
            st->hold > ORBFE_AUTO_HOLD_MAX) {
            fprintf(stderr, "state out of range after: %s", line);
            return 1;
        }
        printf("%d %d\n", ch.form, ch.probe ? 1 : 0);
        ++n;
    }
    free(waiting);
    delete st;
    return n ? 0 : 2;
}

// The extractor's planner (csrc/orbfe_plan.hip) on its own, for a host build with -fsanitize=address,undefined: links that one
// translation unit, needs no device.  Reads one case per line from stdin --
//   nfeatures scale_factor nlevels width height max_batch ini_th min_th  rows rows_fast rows_blur pieces updown debug
// -- builds the plan and fetches one table per case (each of the seven in turn) through orbfe_internal_plan_table into a block of
// exactly its size.  Prints one line per case:
// "<status> <total bytes>".  tests/test_plan.py compiles it, feeds it the matrix and compares the sizes with the library's.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "orbfe_plan.h"

static char g_err[512];

void orbfe_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int main()
{
    char line[512];
    int ncases = 0;
    while (fgets(line, sizeof line, stdin)) {
        orbfe_params p;
        memset(&p, 0, sizeof p);
        int w, h, k[6];
        if (sscanf(line, "%d %f %d %d %d %d %d %d %d %d %d %d %d %d", &p.nfeatures, &p.scale_factor, &p.nlevels, &w, &h, &p.max_batch,
                   &p.ini_th_fast, &p.min_th_fast, &k[0], &k[1], &k[2], &k[3], &k[4], &k[5]) != 14) {
            fprintf(stderr, "bad case line: %s", line);
            return 2;
        }
        p.max_width = w;
        p.max_height = h;
        p.device = -1;
        // the plan once, directly ...
        OrbPlanIn in;
        OrbPlanTables T;
        size_t total = 0;
        orbfe_status s = orb_ctor_tables(&p, &in, nullptr, nullptr);
        if (s == ORBFE_OK) {
            in.opt_rows = k[0]; in.opt_rows_fast = k[1]; in.opt_rows_blur = k[2];
            in.opt_blur_pieces = k[3]; in.opt_blur_updown = k[4]; in.opt_debug = k[5];
            s = orb_plan_build(in, w, h, &T);
        }
        if (s == ORBFE_OK) {
            const size_t sizes[7] = {sizeof(OrbPlan), T.cells.size() * sizeof(OrbCell), T.tabs.size() * sizeof(OrbTab),
                                     T.flanes.size() * sizeof(OrbLane), T.clanes.size() * sizeof(OrbLane), T.blanes.size() * sizeof(OrbLane),
                                     sizeof(T.fast_row_steps)};
            for (size_t b : sizes) total += b;
            // ... and one of its tables (each in turn) through the test hook, into a block of exactly its size
            const int32_t knobs[6] = {k[0], k[1], k[2], k[3], k[4], k[5]};
            const int which = ncases % 7;
            size_t bytes = 0;
            void *dst = malloc(sizes[which]);
            s = orbfe_internal_plan_table(&p, knobs, w, h, which, dst, sizes[which], &bytes);
            free(dst);
            if (s != ORBFE_OK || bytes != sizes[which]) {
                fprintf(stderr, "table %d: status %d, %zu bytes copied, %zu built\n", which, (int)s, bytes, sizes[which]);
                return 1;
            }
        }
        if (s != ORBFE_OK && !g_err[0]) {
            fprintf(stderr, "status %d without an error text: %s", (int)s, line);
            return 1;
        }
        printf("%d %zu\n", (int)s, total);
        g_err[0] = 0;
        ++ncases;
    }
    return ncases ? 0 : 2;
}

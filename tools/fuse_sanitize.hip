// fuse_sanitize.hip -- the host path of trk_gate_fuse (csrc/orbfe_track_geom.h), the function k_fuse_search and orbfe_fuse_gate_points
// run, in a stand-alone program, for tools/fuse_sanitize.py to build with -fsanitize=address,undefined (host only; no device code
// is run and no GPU is needed).  Input file: int32 ncases, then per case 12 + 3 + 9 + 2 floats (Tcw, Ow, the camera, th,
// log_scale_factor), int32 nlevels, mode, n, then scale_factors[nlevels], world_pos[n][3], normal[n][3], min_dist[n], max_dist[n].
// Output (stdout): one line per point "ok level" and the eight words of the query as hex bit patterns.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "orbfe.h"
#include "orbfe_track_geom.h"

static bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t ncases = 0;
    if (!read_all(f, &ncases, 4)) return 3;
    for (int32_t c = 0; c < ncases; ++c) {
        float head[26];
        int32_t dims[3];
        if (!read_all(f, head, sizeof(head)) || !read_all(f, dims, sizeof(dims))) return 3;
        const int32_t nlevels = dims[0], mode = dims[1], n = dims[2];
        if (nlevels < 1 || n < 0) return 3;
        TrkCam cam;
        memcpy(&cam, head + 15, sizeof(cam));
        // every array on the heap, exactly sized, so that the sanitizer sees an index past it
        std::vector<float> T(head, head + 12), Ow(head + 12, head + 15), sf((size_t)nlevels), wp((size_t)n * 3), nr((size_t)n * 3), mn((size_t)n),
            mx((size_t)n);
        if (!read_all(f, sf.data(), sf.size() * 4) || !read_all(f, wp.data(), wp.size() * 4) || !read_all(f, nr.data(), nr.size() * 4) ||
            !read_all(f, mn.data(), mn.size() * 4) || !read_all(f, mx.data(), mx.size() * 4))
            return 3;
        for (int32_t i = 0; i < n; ++i) {
            std::vector<orbfe_proj_query> q(1);
            memset(q.data(), 0, sizeof(orbfe_proj_query));
            int32_t level = -1;
            const bool ok = trk_gate_fuse(T.data(), Ow.data(), cam, wp.data() + 3 * (size_t)i, nr.data() + 3 * (size_t)i, mn[(size_t)i], mx[(size_t)i],
                                          head[24], sf.data(), head[25], nlevels, mode == ORBFE_FUSE_PLAIN, q.data(), &level);
            if (!ok) {
                memset(q.data(), 0, sizeof(orbfe_proj_query));
                level = -1;
            }
            uint32_t w[8];
            memcpy(w, q.data(), 32);
            printf("%d %d %08x %08x %08x %08x %08x %08x %08x %08x\n", ok ? 1 : 0, level, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        }
    }
    fclose(f);
    return 0;
}

// newpoints_sanitize.hip -- the host path of csrc/orbfe_newpoints.h (np_triangulate_match, np_scene_depth) and the round planner in
// a stand-alone program, for tools/newpoints_sanitize.py to build with -fsanitize=address,undefined (host only; no device code is
// run and no GPU is needed).  Input file: int32 nmatch, then per match 65 floats + 2 int32 (see Match below); int32 nlists, then
// per list int32 npairs, kf1[npairs], kf2[npairs].  Output (stdout): one line per match "verdict x y z" (x3D as hex bit patterns),
// one line per list "nrounds | round_of .. | order .. | round_off ..".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "orbfe.h"
#include "orbfe_newpoints.h"

struct Match {
    float T1[12], O1[3], T2[12], O2[3], cam[5], mb, k1[6], k2[6], sf[8], s2[8], scale_factor;
    int32_t oct1, oct2;
};

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nmatch = 0, nlists = 0;
    if (!read_all(f, &nmatch, 4)) return 3;
    for (int32_t i = 0; i < nmatch; ++i) {
        Match m;
        if (!read_all(f, &m, sizeof(m))) return 3;
        orbfe_track_camera cam = {m.cam[0], m.cam[1], m.cam[2], m.cam[3], m.cam[4], 0.f, 0.f, 0.f, 0.f};
        orbfe_newpt_key k1 = {m.k1[0], m.k1[1], m.k1[2], m.k1[3], m.k1[4], m.k1[5], m.oct1};
        orbfe_newpt_key k2 = {m.k2[0], m.k2[1], m.k2[2], m.k2[3], m.k2[4], m.k2[5], m.oct2};
        // the workspace on the heap, exactly sized, so that the sanitizer sees an index past it
        std::vector<float> At(16), Vt(16), x(3);
        std::vector<double> W(4);
        std::vector<float> sf(m.sf, m.sf + 8), s2(m.s2, m.s2 + 8);
        const int v = np_triangulate_match(m.T1, m.O1, m.T2, m.O2, cam, m.mb, k1, k2, sf.data(), s2.data(), m.scale_factor, At.data(), W.data(),
                                           Vt.data(), x.data());
        uint32_t b[3];
        memcpy(b, x.data(), 12);
        const float z = np_scene_depth(m.T1, x.data());
        uint32_t zb;
        memcpy(&zb, &z, 4);
        printf("%d %08x %08x %08x %08x\n", v, b[0], b[1], b[2], zb);
    }
    if (!read_all(f, &nlists, 4)) return 3;
    for (int32_t l = 0; l < nlists; ++l) {
        int32_t np = 0;
        if (!read_all(f, &np, 4)) return 3;
        std::vector<int32_t> kf1(np), kf2(np), round_of(np), order(np), round_off(np + 1);
        if (np && (!read_all(f, kf1.data(), 4 * (size_t)np) || !read_all(f, kf2.data(), 4 * (size_t)np))) return 3;
        const int32_t nr = np_plan_rounds(kf1.data(), kf2.data(), np, round_of.data(), order.data(), round_off.data());
        printf("%d |", nr);
        for (int32_t v : round_of) printf(" %d", v);
        printf(" |");
        for (int32_t v : order) printf(" %d", v);
        printf(" |");
        for (int32_t r = 0; r <= nr; ++r) printf(" %d", round_off[r]);
        printf("\n");
    }
    fclose(f);
    return 0;
}

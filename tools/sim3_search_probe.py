"""Time per pair of the two batched LoopClosing searches (orbfe_search_by_sim3_batch_device,
orbfe_search_by_projection_sim3_batch_device) at 1, 16 and 256 pairs of 2000-feature keyframes against the host-gated path the
library offered before them (GPU box).  Data: proj_cases.sim3_pair_case(2000, 2000) / kf_sim3_case(2000, 2000); DISTINCT different
cases are generated and repeated to fill a batch (the device work per pair is the same; the keyframe rows are shared for
SearchBySim3, copied for the projection search).
  batch     one call for all pairs, in / out rows restored before every repeat, outside the timed span.  Stream events, 3 warm-ups,
            median of the repeats with min - max
  a_loop    per pair what shim/ORBmatcher_orbfe.cc does: the host projection (orbfe_project_points, C), the predicted levels and
            the queries (numpy here, a C++ loop in the shim), and one orbfe_search_by_projection[_chi2] call on host buffers per
            direction -- on the library given with --parent-lib (default: the current one).  Wall clock, same repeats; measured
            on min(pairs, 16) pairs and scaled, since every pair costs the same
a_equal says that the loop's result equals the batch's.  Prints one JSON line; --out FILE also writes it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import proj_cases as PC  # noqa: E402
from oracle import oracle_ffi as O  # noqa: E402
from orb_slam2_ssd_semantic_amd import LoopCloser, ORBmatcher, _ffi, loopclosing, mapping  # noqa: E402

F = np.float32
NFEAT, DISTINCT = 2000, 8
PAIRS = (1, 16, 256)
p_ = _ffi.ptr


class Parent:
    """the host-gated path through raw entry points of one library"""

    def __init__(self, path):
        self.L = _ffi.lib()   # the HIP runtime first, as for every second library
        if path:              # an older build lacks the newer entry points: bind only what this path calls
            self.L = C.CDLL(os.path.abspath(path))
            for name in ("orbfe_matcher_create", "orbfe_matcher_destroy", "orbfe_project_points", "orbfe_search_by_projection"):
                f = getattr(self.L, name)
                f.restype, f.argtypes = _ffi.ABI.prototypes[name]
        self.m = C.c_void_p()
        _ffi.check(self.L.orbfe_matcher_create(-1, C.byref(self.m)), "orbfe_matcher_create")

    def close(self):
        self.L.orbfe_matcher_destroy(self.m)

    def project(self, Rm, t, R2, t2, Ow, K, bounds, wp, nr, mn, mx):
        n = len(mn)
        u, v, iz, d, ur = (np.zeros(n, F) for _ in range(5))
        ok = np.zeros(n, np.uint8)
        _ffi.check(self.L.orbfe_project_points(p_(Rm), p_(t), p_(R2), p_(t2), p_(Ow), *[float(x) for x in K[:4]], 0.0, *[float(b) for b in bounds],
                                               _ffi.ABI.ORBFE_PJ_SKIP_NEG_DEPTH, n, p_(wp), p_(nr), p_(mn), p_(mx), p_(u), p_(v), p_(iz), p_(d),
                                               p_(ur), p_(ok)), "orbfe_project_points")
        return u, v, d, ok.astype(bool)

    @staticmethod
    def queries(u, v, d, mx, sel, th, sf, log_sf, flags):
        """LevelQueries of the shim: PredictScale from the unscaled mfMaxDistance, r = th * scale_factors[level]"""
        lg = np.log((mx[sel] / d[sel]).astype(F).astype(np.float64)).astype(F)
        lv = np.clip(np.ceil(lg / F(log_sf)).astype(np.int32), 0, len(sf) - 1)
        q = np.zeros(int(sel.sum()), _ffi.PROJ_QUERY_DTYPE)
        q["u"], q["v"], q["r"], q["min_level"], q["max_level"], q["flags"] = u[sel], v[sel], F(th) * sf[lv], lv - 1, lv, flags
        return q

    def search(self, kf, grid, blocked, q, qd, th):
        m = np.full(len(q), -1, np.int32)
        minx, _, miny, _ = kf["bounds"]
        if len(q):
            _ffi.check(self.L.orbfe_search_by_projection(self.m, p_(kf["desc"]), p_(kf["xy"]), p_(kf["octave"]), len(kf["octave"]), p_(grid[0]),
                                                         p_(grid[1]), float(minx), float(miny), float(kf["gw_inv"]), float(kf["gh_inv"]), None,
                                                         p_(blocked), p_(q), p_(qd), len(q), int(th), 0.0, 0, p_(m), None, None),
                       "orbfe_search_by_projection")
        return m

    def search_by_sim3(self, k1, k2, g1, g2, sim, m_in, th=7.5):
        n1, n2 = len(k1["octave"]), len(k2["octave"])
        T12, T21 = loopclosing.sim3_pair_pose(*sim)   # three cv::Mat expressions in the shim
        T12, T21 = T12.reshape(3, 4), T21.reshape(3, 4)
        done1 = m_in != -1
        done2 = np.zeros(n2, bool)
        done2[m_in[(m_in >= 0) & (m_in < n2)]] = True
        out = []
        for ks, ko, go, done, S in ((k1, k2, g2, done1, T21), (k2, k1, g1, done2, T12)):
            live = (ks["state"] == 1) & ~done
            mn, mx = (F(0.8) * ks["min_dist"]).astype(F), (F(1.2) * ks["max_dist"]).astype(F)
            u, v, d, ok = self.project(np.ascontiguousarray(ks["Rcw"]), ks["tcw"], np.ascontiguousarray(S[:, :3]), np.ascontiguousarray(S[:, 3]), None,
                                       ko["K"], ko["bounds"], ks["world_pos"], None, mn, mx)
            sel = ok & live
            q = self.queries(u, v, d, ks["max_dist"], sel, th, ko["scale_factors"], ko["log_scale"], 0)
            m = self.search(ko, go, None, q, np.ascontiguousarray(ks["mpdesc"][sel]), 100)
            vn = np.full(len(live), -1, np.int32)
            vn[np.flatnonzero(sel)] = m
            out.append(vn)
        vn1, vn2 = out
        res = m_in.copy()
        i1 = np.flatnonzero(vn1 >= 0)
        agree = i1[vn2[vn1[i1]] == i1]
        res[agree] = vn1[agree]
        return res, len(agree)

    def search_by_projection(self, kf, grid, Scw, pts, matched, th=10):
        T, Ow = mapping.sim3_pose(Scw)
        T = T.reshape(3, 4)
        found = np.zeros(len(pts["bad"]), bool)
        found[matched[matched >= 0]] = True
        mn, mx = (F(0.8) * pts["min_dist"]).astype(F), (F(1.2) * pts["max_dist"]).astype(F)
        u, v, d, ok = self.project(np.ascontiguousarray(T[:, :3]), np.ascontiguousarray(T[:, 3]), None, None, Ow, kf["K"], kf["bounds"], pts["world_pos"],
                                   pts["normal"], mn, mx)
        sel = ok & ~found & ~pts["bad"].astype(bool)
        q = self.queries(u, v, d, pts["max_dist"], sel, th, kf["scale_factors"], kf["log_scale"], _ffi.PROJ_CLAIMS)
        m = self.search(kf, grid, (matched != -1).astype(np.uint8), q, np.ascontiguousarray(pts["mpdesc"][sel]), 50)
        res = matched.copy()
        src = np.flatnonzero(sel)
        res[m[m >= 0]] = src[m >= 0]
        return res, int((m >= 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--parent-lib", help="a build of the commit before the batched calls; default: the current library")
    ap.add_argument("--out")
    a = ap.parse_args()
    mt = ORBmatcher(0.75, True)
    lc = LoopCloser(mt)
    par = Parent(a.parent_lib)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(reset, fn):
        ms = []
        for it in range(3 + a.repeats):
            reset()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        return dict(ms=float(np.median(ms)), ms_min_max=[float(min(ms)), float(max(ms))])

    def wall(fn):
        ms = []
        for it in range(3 + a.repeats):
            t0 = time.perf_counter()
            fn()
            if it >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        return dict(ms=float(np.median(ms)), ms_min_max=[float(min(ms)), float(max(ms))])

    def contig(k):
        return {key: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for key, v in k.items()}

    def grid(k):
        minx, _, miny, _ = k["bounds"]
        return tuple(np.ascontiguousarray(g, np.uint32) for g in O.assign_grid(k["xy"], minx, miny, k["gw_inv"], k["gh_inv"]))

    rng = np.random.default_rng(1)
    s_cases = []
    for _ in range(DISTINCT):
        k1, k2, s12, R12, t12, m_in = PC.sim3_pair_case(rng, NFEAT, NFEAT)
        s_cases.append((contig(k1), contig(k2), (s12, R12, t12), m_in))
    p_cases = []
    for _ in range(DISTINCT):
        kf, Scw, pts, m_in = PC.kf_sim3_case(rng, NFEAT, NFEAT)
        p_cases.append((contig(kf), Scw, contig(pts), m_in))
    s_grids = [(grid(c[0]), grid(c[1])) for c in s_cases]
    p_grids = [grid(c[0]) for c in p_cases]
    res = dict(features=NFEAT, repeats=a.repeats, distinct_cases=DISTINCT, parent_lib=bool(a.parent_lib), search_by_sim3={}, search_by_projection_sim3={})
    kfs = [k for c in s_cases for k in c[:2]]
    for P in PAIRS:
        which = [p % DISTINCT for p in range(P)]
        # ---- SearchBySim3
        reset, launch, fetch = lc.search_by_sim3_pairs_device(kfs, [(2 * w, 2 * w + 1) for w in which], [s_cases[w][2] for w in which], 7.5,
                                                              [s_cases[w][3] for w in which], prepared=True)
        r = dict(batch=timed(reset, launch))
        reset()
        launch()
        got = fetch()
        r["found_per_pair"] = float(np.mean([g[1] for g in got]))
        nl = min(P, 16)

        def loop_s():
            return [par.search_by_sim3(s_cases[w][0], s_cases[w][1], s_grids[w][0], s_grids[w][1], s_cases[w][2], s_cases[w][3]) for w in which[:nl]]
        r["a_loop"] = wall(loop_s)
        r["a_loop"]["pairs_measured"] = nl
        r["a_equal"] = bool(all(np.array_equal(x[0], g[0]) and x[1] == g[1] for x, g in zip(loop_s(), got)))
        r["us_per_pair"] = dict(batch=r["batch"]["ms"] * 1e3 / P, a_loop=r["a_loop"]["ms"] * 1e3 / nl)
        r["speedup_vs_a"] = r["us_per_pair"]["a_loop"] / r["us_per_pair"]["batch"]
        res["search_by_sim3"][str(P)] = r
        del reset, launch, fetch
        # ---- SearchByProjection(pKF, Scw, ...)
        cases = [p_cases[w] for w in which]
        reset, launch, fetch = lc.search_by_projection_sim3_pairs_device(cases, 10, ent_cap=P * NFEAT * 32, prepared=True)
        launch()
        got, status = fetch()
        if status[0] > 0:
            reset, launch, fetch = lc.search_by_projection_sim3_pairs_device(cases, 10, ent_cap=int(status[0]), prepared=True)
        r = dict(batch=timed(reset, launch))
        reset()
        launch()
        got, status = fetch()
        r["ent_cap_needed"], r["rounds"] = int(status[0]), int(status[1])
        r["matches_per_pair"] = float(np.mean([g[1] for g in got]))

        def loop_p():
            return [par.search_by_projection(p_cases[w][0], p_grids[w], p_cases[w][1], p_cases[w][2], p_cases[w][3]) for w in which[:nl]]
        r["a_loop"] = wall(loop_p)
        r["a_loop"]["pairs_measured"] = nl
        r["a_equal"] = bool(all(np.array_equal(x[0], g[0]) and x[1] == g[1] for x, g in zip(loop_p(), got)))
        r["us_per_pair"] = dict(batch=r["batch"]["ms"] * 1e3 / P, a_loop=r["a_loop"]["ms"] * 1e3 / nl)
        r["speedup_vs_a"] = r["us_per_pair"]["a_loop"] / r["us_per_pair"]["batch"]
        res["search_by_projection_sim3"][str(P)] = r
        del reset, launch, fetch
    par.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Edge cases of the PnP solver beside tests/pnp_cases.py: Refine's EPnP branches on the cooperative path, Refine sizes on
the 64 / 256 boundaries, returns on the chunk boundaries of the scan, carried state, and the inputs of the batched form and
of the device constructor that the kernel must reject or clamp.  Every case is an oracle replay (pnp_cases.replay_custom),
computed once per process.  Sizes: at most MAX_POINTS correspondences and MAX_ITERATIONS iterations per call.

The Refine branch cases follow pnp_cases.older_replay: a contaminated scene in which chosen outliers get a sigma2 so large
that they are inliers of every pose, iteration 0 steered onto a quad of true inliers, so that the best mask holds the true
inliers and those outliers and Refine's compute_pose sees a contaminated set.  REFINE_BRANCH holds the seeds a bounded search
found (`python tests/pnp_edge_cases.py` prints the table; its bounds are SEARCH below)."""
import functools

import numpy as np

import pnp_cases as PC
import pnp_oracle as oracle

MAX_POINTS, MAX_ITERATIONS = 600, 200
BIG = np.float32(1e6)


def _pk(min_inliers, max_its, epsilon=0.01):
    return dict(probability=0.99, min_inliers=min_inliers, max_its=max_its, min_set=4, epsilon=epsilon, th2=5.991)


# ---- Refine branches ------------------------------------------------------------------------------------------------------------
def refine_scene(seed, n, ratio, n_big):
    """scene(seed, n, ratio) with the first n_big outliers made inliers of every pose; -> (scene, a quad of true inliers)"""
    sc = PC.scene(seed, n, inlier_ratio=ratio)
    outl, inl = np.nonzero(~sc["truth"])[0], np.nonzero(sc["truth"])[0]
    sc["sigma2"] = sc["sigma2"].copy()
    sc["sigma2"][outl[:n_big]] = BIG
    return sc, [int(i) for i in (list(inl) + list(outl))[:4]]


def refine_inputs(seed, n, ratio, n_big):
    """one iteration on the quad, min_inliers 4, the clamp at 1: Refine runs once over the contaminated best mask"""
    sc, quad = refine_scene(seed, n, ratio, n_big)
    return sc, _pk(4, 1), [1], PC.draws_picking([quad], n)


def refine_replay(seed, n, ratio, n_big):
    return PC.replay_custom(*refine_inputs(seed, n, ratio, n_big))


def line_inputs(seed, m=12):
    """qr_solve's singular branch: no contaminated scene of SEARCH / SEARCH_WIDE reaches it; map points on a world line parallel
    to an axis (y = 0.5, z = 0) do, for some seeds, in one of the five Gauss-Newton steps.  Four points of a line give no usable
    pose, so the m line points all carry the large sigma2: every pose counts them, they are the best mask, Refine runs over
    them and, counting them again, returns.  Four ordinary points follow"""
    rng = np.random.default_rng(seed)
    R = PC.rotation(rng, 0.4)
    t = rng.uniform(-0.3, 0.3, 3) + np.array([0, 0, 4.0])
    Pw = np.stack([rng.uniform(-2, 2, m + 4), np.full(m + 4, 0.5), np.zeros(m + 4)], 1)
    Pw[m:, 1:] = rng.uniform(-1, 1, (4, 2))
    P3 = Pw.astype(np.float32)
    Pc = P3.astype(np.float64) @ R.T + t
    uv = np.stack([PC.K[2] + PC.K[0] * Pc[:, 0] / Pc[:, 2], PC.K[3] + PC.K[1] * Pc[:, 1] / Pc[:, 2]], 1)
    sigma2 = np.r_[np.full(m, BIG), PC.SCALE2[:4]].astype(np.float32)
    sc = dict(P3Dw=P3, P2D=uv.astype(np.float32), sigma2=sigma2, truth=np.arange(m + 4) < m, R=R, t=t)
    return sc, _pk(4, 1), [1], PC.draws_picking([[0, 1, 2, 3]], m + 4)


LINE_SEED = 0   # the first seed of range(40) whose Refine over the 12 line points leaves x in a Gauss-Newton step and returns

# census entry -> (n, inlier_ratio, seed, n_big); every one of these Refines returns, so its Tcw is compared
REFINE_BRANCH = {
    "b1_neg": (12, 0.5, 15, 6),
    "k2_b0_neg": (10, 0.5, 82, 5),   # from SEARCH_WIDE; arm 5 at k = 2 and at k = 3
    "k3_b0_neg": (12, 0.5, 12, 6),
    "k3_b0_neg#2": (12, 0.5, 50, 6),
    "det_neg": (12, 0.5, 43, 6),
    "N1": (6, 0.8, 18, 1),
    "N2": (12, 0.5, 5, 6),
    "N3": (12, 0.5, 1, 6),
}
SEARCH = dict(n=(6, 12, 20, 40), ratio=(0.5, 0.8), seeds=range(60))   # with n_big = all outliers and half of them
SEARCH_WIDE = dict(n=(5, 7, 8, 9, 10, 14, 16, 24, 30), ratio=(0.5, 0.65, 0.8), seeds=range(120))   # for what SEARCH missed
# arms of _betas_23 (4 * (b[0] < 0) + 2 * (b[2] < 0) + (b[1] < 0)) that neither stage reached on a returning Refine over more
# than four points; reported by tests/test_pnp_edge_cases.py, not covered.  Arms 4 and 7 of k = 2 were seen only on Refines
# that fail and whose refine_inliers the broken rule does not change.  (At k = 3 the stages saw all of arms 4 - 7; two have a case.)
UNREACHED = ("k2_arm4", "k2_arm6", "k2_arm7")


def refine_trace(runs):
    """the trace of the Refine of iteration 0"""
    return runs[0]["taps"][0]["refine"]


def arms_of(tr):
    """the names of the census entries a compute_pose trace (of one item) shows"""
    out = {f"N{int(tr['N'][0])}"}
    if tr["betas1_neg"][0]:
        out.add("b1_neg")
    for k in (2, 3):
        a = int(tr["betas23_arm"][k][0])
        out.add(f"k{k}_arm{a}")
        if a >= 4:
            out.add(f"k{k}_b0_neg")
    for k in (1, 2, 3):
        if tr["det_neg"][k][0]:
            out.add("det_neg")
        if tr["qr_kept"][k][0]:
            out.add("qr_singular")
        if tr["flip"][k][0]:
            out.add(f"flip{k}")
    return out


# ---- planted scenes: exactly m true inliers ----------------------------------------------------------------------------------------
def planted(seed, m, n_out, noise=0.0):
    """a noiseless scene of m + n_out points in which exactly n_out, at seeded positions, are displaced by 50 - 120 px"""
    n = m + n_out
    sc = PC.scene(seed, n, inlier_ratio=1.0, noise=noise)
    rng = np.random.default_rng(seed + 77)
    out = np.sort(rng.permutation(n)[:n_out])
    ang = rng.uniform(0, 2 * np.pi, n_out)
    sc["P2D"] = sc["P2D"].copy()
    sc["P2D"][out] += (rng.uniform(50, 120, n_out)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    sc["truth"] = np.ones(n, bool)
    sc["truth"][out] = False
    return sc


def good_quad(sc, rng):
    """a quad of true inliers whose EPnP pose counts every true inlier and nothing else (four points do not always give one)"""
    inl = np.nonzero(sc["truth"])[0]
    Kf = tuple(float(np.float32(v)) for v in PC.K)
    for _ in range(200):
        q = [int(i) for i in rng.choice(inl, 4, replace=False)]
        R, t, _, _ = oracle.compute_pose(sc["P3Dw"][q].astype(np.float64)[None], sc["P2D"][q].astype(np.float64)[None], Kf)
        mask, _ = oracle.check_inliers(R[0], t[0], sc["P3Dw"], sc["P2D"], sc["sigma2"] * np.float32(5.991), Kf)
        if np.array_equal(mask, sc["truth"]):
            return q
    raise AssertionError("no quad of this scene recovers its inliers")


def _quads(sc, seed, total, good_at):
    """`total` quads: at the iterations of good_at one that recovers the true inliers, else three outliers and one inlier"""
    rng = np.random.default_rng(seed + 99)
    inl, outl = np.nonzero(sc["truth"])[0], np.nonzero(~sc["truth"])[0]
    q = []
    for it in range(total):
        if it in good_at:
            q.append(good_quad(sc, rng))
        else:
            o = rng.choice(outl, 3, replace=False)
            q.append([int(o[0]), int(rng.choice(inl)), int(o[1]), int(o[2])])
    return q


REFINE_SIZES = (4, 5, 63, 64, 65, 255, 256, 257)
# m -> seed of planted(): iteration 0 counts exactly the m true inliers and (m > 4) its Refine returns with m inliers
SIZE_SEED = {4: 204, 5: 205, 63: 263, 64: 264, 65: 265, 255: 455, 256: 456, 257: 457}


def size_inputs(m, seed):
    """a best mask of exactly m inliers: one steered iteration; min_inliers m - 1 (4 for m = 4, whose Refine cannot return: the
    four points fit both poses and nothing else does)"""
    sc = planted(seed, m, 9)
    return sc, _pk(max(4, m - 1), 1), [1], PC.draws_picking(_quads(sc, seed, 1, (0,)), m + 9)


def size_replay(m, seed):
    return PC.replay_custom(*size_inputs(m, seed))


# ---- the scan ----------------------------------------------------------------------------------------------------------------------
SCAN_SEED = 3


def scan_scene():
    return planted(SCAN_SEED, 20, 10)


def return_at(it, n_iterations=5):
    """every iteration before `it` fits three outliers and counts below min_inliers; `it` returns through Refine.  SetRansacParameters
    clamps max_its to 70 on this scene (epsilon 0.4): a return past that needs n_iterations past it"""
    sc = scan_scene()
    total = max(n_iterations, 70)
    return sc, _pk(12, 200), [n_iterations], PC.draws_picking(_quads(sc, it, total, (it,)), 30)


def two_changes():
    """two best-mask changes inside chunk 0, each with its own Refine, both failing: pnp_cases.older_replay's scene with its two
    hypotheses in the other order.  Iteration 1 fits a quad with off points and becomes the best; iteration 3 fits exact points,
    counts more and replaces it; both Refines land at or below min_inliers.  The clamp at 6 sends the second best out"""
    sc, _, runs, info = PC.older_replay()
    q = [list(t["quad"]) for t in runs[0]["taps"]]
    good, weak, bad = q[0], q[2], q[1]
    return sc, _pk(info["count2"], 6), [5], PC.draws_picking([bad, weak, bad, good, bad, bad], len(sc["truth"]))


def best_survives_clamp():
    """rules_scene: an all-inlier quad at iteration 5 counts == min_inliers, its Refine fails; nothing better follows and the clamp
    ends the call at 70, in chunk 1: the best of chunk 0 goes out unrefined"""
    sc = PC.rules_scene()
    outl = np.nonzero(~sc["truth"])[0]
    bad = [int(outl[0]), PC.GOOD[0], int(outl[1]), int(outl[2])]
    return sc, dict(PC.RULES_PARAMS, max_its=70), [5], PC.draws_picking([bad] * 5 + [PC.GOOD] + [bad] * 64, 30)


def tie_across_chunks():
    """rules_scene: iterations 63 and 64, the last of chunk 0 and the first of chunk 1, fit the same inliers in another order (same
    count, other bits): the later one must not replace the best, which goes out at the clamp of 70"""
    sc = PC.rules_scene()
    outl = np.nonzero(~sc["truth"])[0]
    bad = [int(outl[0]), PC.GOOD[0], int(outl[1]), int(outl[2])]
    return sc, dict(PC.RULES_PARAMS, max_its=70), [5], PC.draws_picking([bad] * 63 + [PC.GOOD, PC.GOOD_PERMUTED] + [bad] * 5, 30)


def older_across_chunks():
    """pnp_cases.older_replay with a chunk boundary between its two hypotheses: the best of iteration 62 is still the best when
    iteration 65 counts fewer, at least min_inliers, with another mask.  Refine belongs to the best mask (the kernel remembers its
    result across the chunk), not to the current one.  SetRansacParameters clamps max_its to 22 here: iterate(70) runs 70"""
    sc, _, runs, info = PC.older_replay()
    q = [list(t["quad"]) for t in runs[0]["taps"]]
    good, weak, bad = q[0], q[2], q[1]
    return sc, _pk(info["count2"], 70), [70], PC.draws_picking([bad] * 62 + [good, bad, bad, weak] + [bad] * 4, len(sc["truth"]))


def carried(first_return, max_its, second, rest):
    """a first call that returns at iteration first_return - 1, then iterate(second) over all-outlier quads, which runs `rest` =
    max(second, max_its - first_return) iterations: (1, 66, 5) runs 65, chunks of 64 and 1; (63, 70, 64) runs 64, one full chunk"""
    sc = scan_scene()
    q = _quads(sc, first_return, max(first_return + rest, max_its), (first_return - 1,))
    return sc, _pk(12, max_its), [1, second], PC.draws_picking(q, 30)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> (scene, SetRansacParameters kwargs, the n_iterations of each call, draws): what pnp_cases.replay_custom takes"""
    t = {}
    for name, (n, ratio, seed, n_big) in REFINE_BRANCH.items():
        t["refine_" + name] = refine_inputs(seed, n, ratio, n_big)
    t["refine_qr_singular"] = line_inputs(LINE_SEED)
    for m in REFINE_SIZES:
        t[f"size_{m}"] = size_inputs(m, SIZE_SEED[m])
    t["return_at_63"] = return_at(63)
    t["return_at_64"] = return_at(64)
    t["return_at_130"] = return_at(130, 140)
    t["two_changes"] = two_changes()
    t["best_survives_clamp"] = best_survives_clamp()
    t["tie_across_chunks"] = tie_across_chunks()
    t["older_across_chunks"] = older_across_chunks()
    t["carried_1"] = carried(1, 66, 5, 65)
    t["carried_63"] = carried(63, 70, 64, 64)
    return t


@functools.lru_cache(maxsize=None)
def table():
    """name -> (scene, params, runs): the oracle's replay of every case, computed once"""
    return {name: PC.replay_custom(*args) for name, args in inputs().items()}


# ---- the device constructor ----------------------------------------------------------------------------------------------------------
N_MAPPOINTS, N_LEVELS = 40, 8


def prepare_inputs(n_keys=400):
    """keys (x, y, octave), mappoint_index and positions with indices n_mappoints and n_mappoints + 1 and octaves -1 and n_levels at
    positions 0, 63, 64, 255, 256 and last, each next to a usable entry -> (x, y, octave, index, positions, usable bool [n_keys])"""
    rng = np.random.default_rng(n_keys)
    x, y = rng.uniform(0, 640, n_keys).astype(np.float32), rng.uniform(0, 480, n_keys).astype(np.float32)
    octave = rng.integers(0, N_LEVELS, n_keys).astype(np.int32)
    idx = rng.integers(0, N_MAPPOINTS, n_keys).astype(np.int32)
    idx[rng.random(n_keys) < 0.1] = -1
    edges = (0, 63, 64, 255, 256, n_keys - 1)
    bad = [("idx", N_MAPPOINTS), ("oct", -1), ("idx", N_MAPPOINTS + 1), ("oct", N_LEVELS), ("oct", -1), ("oct", N_LEVELS)]
    for e, (what, v) in zip(edges, bad):
        idx[e] = 3
        if what == "idx":
            idx[e] = v
        else:
            octave[e] = v
    for e in (1, 62, 65, 254, 257, n_keys - 2):
        idx[e], octave[e] = e % N_MAPPOINTS, e % N_LEVELS
    idx[100], octave[100] = N_MAPPOINTS + 1, N_LEVELS   # both at once
    pos = rng.standard_normal((N_MAPPOINTS, 3)).astype(np.float32)
    usable = (idx >= 0) & (idx < N_MAPPOINTS) & (octave >= 0) & (octave < N_LEVELS)
    return x, y, octave, idx, pos, usable


# ---- the search ----------------------------------------------------------------------------------------------------------------------
_RULE_OF = {"b1_neg": "betas1_sign", "k2_b0_neg": "betas23_b0", "k3_b0_neg": "betas23_b0", "det_neg": "det_neg", "N2": "choose_2",
            "N3": "choose_3"}


def _b(a):
    """the bytes of a float array, every NaN the same one (its sign and payload belong to the processor)"""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def compared(runs):
    """the bytes of everything the GPU test compares of an oracle replay"""
    out = []
    for r in runs:
        o = r["out"]
        out += [_b(np.zeros((4, 4), np.float32) if o["Tcw"] is None else o["Tcw"]), o["mask"].tobytes(),
                str((o["no_more"], o["n_inliers"], o["iterations_run"], r["iterations"], r["best_inliers"])).encode(),
                r["best_mask"].tobytes(), _b(r["best_Tcw"])]
        for t in r["taps"]:
            out += [_b(t["R"]), _b(t["t"]), _b(t["error2"]),
                    str(([int(q) for q in t["quad"]], t["N"], t["n_inliers"], t["refine_inliers"])).encode()]
    return b"".join(out)


def with_break(rule, scope, fn):
    oracle.EPNP_BREAK, oracle.EPNP_BREAK_SCOPE = frozenset([rule]), scope
    try:
        return fn()
    finally:
        oracle.EPNP_BREAK, oracle.EPNP_BREAK_SCOPE = frozenset(), "all"


def _search(space, want, got, seen):
    """fills got[entry] = (n, ratio, seed, n_big) with the first returning Refine over more than four points that shows the entry
    and, where the entry has a break rule, whose compared bytes that rule (Refine scope) changes"""
    k3_arms = {int(refine_trace(refine_replay(*(got[k][2], got[k][0], got[k][1], got[k][3]))[2])["betas23_arm"][3][0])
               for k in ("k3_b0_neg",) if k in got}
    for n in space["n"]:
        for ratio in space["ratio"]:
            for seed in space["seeds"]:
                n_out = int((~PC.scene(seed, n, inlier_ratio=ratio)["truth"]).sum())
                for n_big in sorted({n_out, max(1, n_out // 2)}):
                    args = (seed, n, ratio, n_big)
                    runs = refine_replay(*args)[2]
                    t = runs[0]["taps"][0]
                    if not t["refined"] or t["refine"]["m"] <= 4 or runs[0]["out"]["no_more"]:
                        continue   # no Refine, one over four points, or one that does not return
                    arms = arms_of(t["refine"])
                    seen |= arms
                    for a in sorted(arms):
                        key, arm3 = a, int(t["refine"]["betas23_arm"][3][0])
                        if a == "k3_b0_neg" and a in got:
                            if arm3 in k3_arms:
                                continue
                            key = "k3_b0_neg#2"
                        if key not in want or key in got:
                            continue
                        rule = _RULE_OF.get(a)
                        if rule and compared(with_break(rule, "refine", lambda: refine_replay(*args))[2]) == compared(runs):
                            continue   # the arm is taken but its break does not reach the result
                        got[key] = (n, ratio, seed, n_big)
                        if a == "k3_b0_neg":
                            k3_arms.add(arm3)


if __name__ == "__main__":
    want = ["b1_neg", "k2_b0_neg", "k3_b0_neg", "k3_b0_neg#2", "det_neg", "qr_singular", "N1", "N2", "N3"]
    got, seen = {}, set()
    _search(SEARCH, want, got, seen)
    _search(SEARCH_WIDE, [w for w in want if w not in got], got, seen)   # only for what the first stage missed
    print("REFINE_BRANCH = {")
    for k in want:
        print(f"    {k!r}: {got.get(k)},")
    print("}")
    print("arms seen on a returning Refine:", sorted(seen))
    for seed in range(40):
        runs = PC.replay_custom(*line_inputs(seed))[2]
        t = runs[0]["taps"][0]
        if t["refined"] and "qr_singular" in arms_of(t["refine"]) and not runs[0]["out"]["no_more"]:
            print("LINE_SEED =", seed)
            break
    sizes = {}
    for m in REFINE_SIZES:
        for seed in range(200 + m, 260 + m):
            sc, prm, runs = size_replay(m, seed)
            t, o = runs[0]["taps"][0], runs[0]["out"]
            if t["n_inliers"] == m and t["refine"]["m"] == m and np.array_equal(t["mask"], sc["truth"]) and \
                    ((o["n_inliers"] == m and not o["no_more"]) if m > 4 else (t["refine_inliers"] == 4 and o["no_more"])):
                sizes[m] = seed
                break
    print("SIZE_SEED =", sizes)

"""The scene of the Sim3Solver shim test (tests/cpp/test_sim3_solver.cpp): three loop candidates as mock keyframes and map
points, the input file the C++ program reads, and the oracle's replay of LoopClosing's call sequence with glibc's rand()
stream.  `python tests/sim3_shim_case.py` records the oracle's results in tests/golden/sim3_shim.npz."""
import ctypes
import os

import numpy as np

import sim3_cases as SC
import sim3_oracle as SO

F = np.float32
SEED = 2024
MAX_ROUNDS = 80
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_shim.npz")
SIGMA2 = (F(1.2) ** np.arange(8, dtype=F)) ** 2


def candidates():
    """three candidates: an easy one, one that never finds a model (all outliers) and one with too few correspondences"""
    out = []
    for k, (n_good, n_out, mn1, fix) in enumerate(((90, 30, 150, True), (0, 60, 100, True), (15, 0, 60, False))):
        rng = np.random.default_rng(900 + k)
        n = n_good + n_out
        X1c, X2c, _, _, _ = SC.scene(n, n_out, 700 + k, s=1.0 if fix else 1.4)
        R1, R2 = SC.rodrigues(rng.normal(size=3), 0.4).astype(F), SC.rodrigues(rng.normal(size=3), 1.1).astype(F)
        t1, t2 = rng.uniform(-1, 1, 3).astype(F), rng.uniform(-1, 1, 3).astype(F)
        # world positions whose camera-frame points are (close to) the scene's
        W1 = ((X1c.astype(np.float64) - t1) @ R1.astype(np.float64)).astype(F)
        W2 = ((X2c.astype(np.float64) - t2) @ R2.astype(np.float64)).astype(F)
        nkeys2 = n + 20
        slots = np.sort(rng.permutation(mn1)[:n])
        rec = np.zeros(mn1, [("has1", "<i4"), ("x1", "<f4", 3), ("bad1", "<i4"), ("index1", "<i4"), ("has2", "<i4"), ("x2", "<f4", 3),
                             ("bad2", "<i4"), ("index2", "<i4")])
        rec["has1"] = rng.random(mn1) < 0.8
        rec["x1"] = rng.normal(size=(mn1, 3))
        rec["index1"] = np.arange(mn1)
        idx2 = rng.permutation(nkeys2)[:n]
        for j, i1 in enumerate(slots):
            rec[i1] = (1, W1[j], 0, i1, 1, W2[j], 0, idx2[j])
        if n >= 8:   # the constructor's filters: no map point in keyframe 1, bad points, a point that is not in its keyframe
            for j, f in zip(slots[rng.permutation(n)[:5]], ("has1", "bad1", "bad2", "index1", "index2")):
                rec[f][j] = -1 if f.startswith("index") else (0 if f == "has1" else 1)
        out.append(dict(mN1=mn1, nkeys2=nkeys2, fix_scale=fix, K1=np.array(SC.K_A, F), K2=np.array(SC.K_B, F), R1=R1, t1=t1, R2=R2, t2=t2,
                        oct1=rng.integers(0, 8, mn1).astype(np.int32), oct2=rng.integers(0, 8, nkeys2).astype(np.int32), rec=rec))
    return out


def write_input(path):
    cs = candidates()
    with open(path, "wb") as f:
        np.array([len(cs), SEED, MAX_ROUNDS], np.int32).tofile(f)
        for c in cs:
            np.array([c["mN1"], c["nkeys2"], int(c["fix_scale"])], np.int32).tofile(f)
            for k in ("K1", "K2", "R1", "t1", "R2", "t2"):
                np.ascontiguousarray(c[k], F).tofile(f)
            SIGMA2.astype(F).tofile(f)
            c["oct1"].tofile(f)
            c["oct2"].tofile(f)
            c["rec"].tofile(f)
    return cs


def gather(c):
    """the constructor's loop (src/Sim3Solver.cc:42-88) on the records -> oracle Solver, mvnIndices1"""
    r = c["rec"]
    keep = np.flatnonzero((r["has2"] != 0) & (r["has1"] != 0) & (r["bad1"] == 0) & (r["bad2"] == 0) & (r["index1"] >= 0) & (r["index2"] >= 0))
    X1 = SO.camera_points(r["x1"][keep], c["R1"], c["t1"])
    X2 = SO.camera_points(r["x2"][keep], c["R2"], c["t2"])
    s1 = SIGMA2[c["oct1"][r["index1"][keep]]]
    s2 = SIGMA2[c["oct2"][r["index2"][keep]]]
    return SO.Solver(X1, X2, s1, s2, c["K1"], c["K2"], c["fix_scale"]), keep


def rand_stream(seed, n):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    return np.array([libc.rand() for _ in range(n)], np.int64)


def replay():
    """LoopClosing's sequence through the oracle: a list of (solver, empty, no_more, n_inliers, model float32 [29], inliers uint8 [mN1])"""
    cs = candidates()
    solvers = [gather(c) for c in cs]
    for s, _ in solvers:
        s.set_ransac_parameters(0.99, 20, 300)
    stream = rand_stream(SEED, 3 * 5 * MAX_ROUNDS * len(cs) + 16)
    pos = 0
    off, done, calls = [False] * len(cs), [False] * len(cs), []
    for _ in range(MAX_ROUNDS):
        live = [k for k in range(len(cs)) if not off[k] and not done[k]]
        if not live:
            break
        for k in live:
            s, keep = solvers[k]
            r = s.iterate(5, stream[pos:pos + 15])
            pos += 3 * r["iterations_run"]
            off[k] = r["no_more"]
            model = np.zeros(29, F)
            inl = np.zeros(cs[k]["mN1"], np.uint8)
            if r["found"]:
                done[k] = True
                model[:16] = r["T12"].ravel()
                model[16:25] = s.best["R"].ravel()
                model[25:28] = s.best["t"]
                model[28] = s.best["s"]
                inl[keep[r["mask"].astype(bool)]] = 1
            calls.append((k, int(not r["found"]), int(r["no_more"]), r["n_inliers"], model, inl))
    return calls


def pack(calls):
    return dict(head=np.array([c[:4] for c in calls], np.int32), model=np.array([c[4] for c in calls], F),
                inliers=np.concatenate([c[5] for c in calls]))


def parse_output(blob, cs):
    calls, p = [], 0
    while p < len(blob):
        head = np.frombuffer(blob[p:p + 16], np.int32)
        model = np.frombuffer(blob[p + 16:p + 132], F)
        n1 = cs[int(head[0])]["mN1"]
        calls.append((int(head[0]), int(head[1]), int(head[2]), int(head[3]), model, np.frombuffer(blob[p + 132:p + 132 + n1], np.uint8)))
        p += 132 + n1
    return calls


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **pack(replay()))
    print(GOLDEN, os.path.getsize(GOLDEN))

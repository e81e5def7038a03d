"""The scene of the PnPsolver shim test (tests/cpp/test_pnp_solver.cpp): three relocalization candidates as a mock frame with
map point matches, the input file the C++ program reads, and the oracle's replay of Tracking::Relocalization's call sequence
with glibc's rand() stream.  `python tests/pnp_shim_case.py` records the oracle's results in tests/golden/pnp_shim.npz."""
import ctypes
import os

import numpy as np

import pnp_cases as PC
import pnp_oracle as PO

F = np.float32
SEED = 2025
MAX_ROUNDS = 80
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_shim.npz")
PARAMS = dict(probability=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991)
REC = np.dtype([("octave", "<i4"), ("xy", "<f4", 2), ("has", "<i4"), ("pos", "<f4", 3), ("bad", "<i4")])


def candidates():
    """three candidates: an easy one, one that never finds a model (all outliers) and one with too few correspondences"""
    out = []
    for k, (n, ratio, nkeys) in enumerate(((80, 0.6, 130), (40, 0.0, 70), (7, 1.0, 40))):
        rng = np.random.default_rng(300 + k)
        sc = PC.scene(500 + k, n, inlier_ratio=ratio)
        octave = np.searchsorted(PC.SCALE2, sc["sigma2"]).astype(np.int32)
        assert np.array_equal(PC.SCALE2[octave], sc["sigma2"])
        rec = np.zeros(nkeys, REC)
        rec["octave"] = rng.integers(0, 8, nkeys)
        rec["xy"] = rng.uniform(0, 480, (nkeys, 2))
        rec["has"] = rng.random(nkeys) < 0.3      # matches the constructor has to leave out: bad map points
        rec["bad"] = rec["has"]
        rec["pos"] = rng.normal(size=(nkeys, 3))
        slots = np.sort(rng.permutation(nkeys)[:n])
        for j, i in enumerate(slots):
            rec[i] = (octave[j], sc["P2D"][j], 1, sc["P3Dw"][j], 0)
        out.append(dict(nkeys=nkeys, K=np.array(PC.K, F), rec=rec))
    return out


def write_input(path):
    cs = candidates()
    with open(path, "wb") as f:
        np.array([len(cs), SEED, MAX_ROUNDS], np.int32).tofile(f)
        for c in cs:
            np.array([c["nkeys"]], np.int32).tofile(f)
            c["K"].tofile(f)
            PC.SCALE2.astype(F).tofile(f)
            c["rec"].tofile(f)
    return cs


def gather(c):
    """the constructor's loop (src/PnPsolver.cc:71-93) on the records -> oracle solver, mvKeyPointIndices"""
    r = c["rec"]
    idx = np.where((r["has"] != 0) & (r["bad"] == 0), 0, -1).astype(np.int64)
    idx[idx == 0] = np.flatnonzero(idx == 0)   # the record is its own map point
    P2D, sg, P3, kp = PO.construct(r["xy"], r["octave"], PC.SCALE2, idx, r["pos"])
    s = PO.PnPSolver(P3, P2D, sg, c["K"])
    return s, kp


def rand_stream(seed, n):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    return np.array([libc.rand() for _ in range(n)], np.int64)


def replay():
    """Relocalization's sequence through the oracle: a list of (solver, empty, no_more, n_inliers, size, Tcw float32 [16], inliers)"""
    cs = candidates()
    solvers = [gather(c) for c in cs]
    for s, _ in solvers:
        s.set_ransac_parameters(**PARAMS)
    stream = rand_stream(SEED, 4 * (5 * MAX_ROUNDS + 300) * len(cs) + 16)
    pos = 0
    off, done, calls = [False] * len(cs), [False] * len(cs), []
    for _ in range(MAX_ROUNDS):
        live = [k for k in range(len(cs)) if not off[k] and not done[k]]
        if not live:
            break
        for k in live:
            s, kp = solvers[k]
            can = max(5, s.max_its - s.iterations) if (s.N >= s.min_inliers and s.N >= 4) else 0
            r = s.iterate(5, stream[pos:pos + 4 * can])
            pos += 4 * r["iterations_run"]
            off[k] = r["no_more"]
            found = r["Tcw"] is not None
            T = np.zeros(16, F)
            inl = np.zeros(cs[k]["nkeys"] if found else 0, np.uint8)
            if found:
                done[k] = True
                T[:] = r["Tcw"].ravel()
                inl[kp[r["mask"]]] = 1
            calls.append((k, int(not found), int(r["no_more"]), r["n_inliers"], len(inl), T, inl))
    return calls


def pack(calls):
    return dict(head=np.array([c[:5] for c in calls], np.int32), model=np.array([c[5] for c in calls], F),
                inliers=np.concatenate([c[6] for c in calls]))


def parse_output(blob):
    calls, p = [], 0
    while p < len(blob):
        head = np.frombuffer(blob[p:p + 20], np.int32)
        model = np.frombuffer(blob[p + 20:p + 84], F)
        n1 = int(head[4])
        calls.append((int(head[0]), int(head[1]), int(head[2]), int(head[3]), n1, model, np.frombuffer(blob[p + 84:p + 84 + n1], np.uint8)))
        p += 84 + n1
    return calls


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **pack(replay()))
    print(GOLDEN, os.path.getsize(GOLDEN))

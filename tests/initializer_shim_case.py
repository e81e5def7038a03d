"""The scene of the Initializer shim test (tests/cpp/test_initializer.cpp): a reference frame and two following frames (the first
too close for the parallax test, the second a good one), the input file the C++ program reads, and the oracle's replay of
Tracking::MonocularInitialization's call sequence with glibc's rand() stream after srand(0): 1600 draws per call.
`python tests/initializer_shim_case.py` records the oracle's results in tests/golden/initializer_shim.npz."""
import ctypes
import os

import numpy as np

import initializer_cases as IC
import initializer_oracle as IO

F = np.float32
ITERATIONS = 200
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "initializer_shim.npz")


def frames():
    """-> (K, [keys of frames 1, 2, 3], [matches12 of frame 2, of frame 3])"""
    rng = np.random.default_rng(50)
    X = np.stack([rng.uniform(-2, 2, 120), rng.uniform(-1.5, 1.5, 120), rng.uniform(3, 12, 120)], 1)
    near = IC.pair_from(X, IC.rot(0.01, -0.01, 0.005), np.array([0.08, 0.01, 0.0]), extra1=30, extra2=20, seed=50)
    good = IC.pair_from(X, IC.R_GEN, IC.T_GEN, extra1=30, extra2=20, seed=50)
    assert np.array_equal(near["keys1"], good["keys1"])
    return near["K"], [near["keys1"], near["keys2"], good["keys2"]], [near["matches12"], good["matches12"]]


def write_input(path):
    K, keys, matches = frames()
    with open(path, "wb") as f:
        K.astype(F).tofile(f)
        np.array([len(keys)], np.int32).tofile(f)
        for k in keys:
            np.array([len(k)], np.int32).tofile(f)
            k.astype(F).tofile(f)
        for m in matches:
            m.astype(np.int32).tofile(f)


def rand_stream(seed, n):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    return np.array([libc.rand() for _ in range(n)], np.int64)


def replay():
    """MonocularInitialization's sequence through the oracle: a list of (ok, empty, size, model float32 [12], P3D, triangulated)"""
    K, keys, matches = frames()
    stream = rand_stream(0, 8 * ITERATIONS * len(matches)).astype(np.int32)
    calls = []
    for k, m in enumerate(matches):
        d = stream[8 * ITERATIONS * k:8 * ITERATIONS * (k + 1)]   # the second call consumes the next 1600 draws
        r = IO.initialize(keys[0], keys[k + 1], m, K, 1.0, ITERATIONS, d)
        ok = int(r["ok"])
        model = np.concatenate([r["R21"].ravel(), r["t21"]]).astype(F) if ok else np.zeros(12, F)
        n = len(keys[0]) if ok else 0
        calls.append((ok, int(not ok), n, model, r["P3D"][:n].astype(F), r["triangulated"][:n].astype(np.uint8)))
    return calls


def pack(calls):
    return dict(head=np.array([c[:3] for c in calls], np.int32), model=np.array([c[3] for c in calls], F),
                points=np.concatenate([c[4].reshape(-1, 3) for c in calls]), triangulated=np.concatenate([c[5] for c in calls]))


def parse_output(blob):
    calls, p = [], 0
    while p < len(blob):
        head = np.frombuffer(blob[p:p + 12], np.int32)
        model = np.frombuffer(blob[p + 12:p + 60], F)
        n = int(head[2])
        pts = np.frombuffer(blob[p + 60:p + 60 + 12 * n], F).reshape(n, 3)
        tri = np.frombuffer(blob[p + 60 + 12 * n:p + 60 + 13 * n], np.uint8)
        calls.append((int(head[0]), int(head[1]), n, model, pts, tri))
        p += 60 + 13 * n
    return calls


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **pack(replay()))
    print(GOLDEN, os.path.getsize(GOLDEN))

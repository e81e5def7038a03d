"""orbfe_compute_f12 and orbfe_tri_search_scratch_bytes: the host entry points of the batched SearchForTriangulation that need
no device.  ComputeF12 (src/LocalMapping.cc:848-867) against tests/f12_oracle.py as bit patterns, and the epipolar constraint it
must satisfy on planted correspondences within a bound derived here."""
import numpy as np

import f12_oracle as FO
import proj_cases as PC

f32 = np.float32
K = (535.4, 539.2, 320.1, 247.6)
EPS = float(np.finfo(f32).eps)


def _cam():
    from orb_slam2_ssd_semantic_amd import mapping
    return mapping.camera(*K, 40.0, 0.0, 640.0, 0.0, 480.0)


def _pose(R=None, t=(0, 0, 0)):
    T = np.zeros((3, 4), f32)
    T[:, :3] = np.eye(3) if R is None else R
    T[:, 3] = t
    return T


def _poses():
    out = [(_pose(), _pose())]
    for ax in range(3):
        for s in (0.3, -0.3):
            t = [0.0, 0.0, 0.0]
            t[ax] = s
            out.append((_pose(), _pose(t=t)))
    for seed in range(200):
        rng = np.random.default_rng(4200 + seed)
        T1 = PC._pose(rng, 3.0, rng.normal(0, 0.1, 3)).astype(f32)[:3]
        T2 = T1.copy()
        T2[:3, :3] = (PC._rot(rng, 4.0) @ T1[:3, :3].astype(np.float64)).astype(f32)
        T2[:3, 3] = T1[:3, 3] + rng.normal(0, 0.3, 3).astype(f32)
        out.append((T1, T2))
    return out


def test_compute_f12_equals_oracle_bitwise():
    from orb_slam2_ssd_semantic_amd import compute_f12
    cam = _cam()
    nonzero = 0
    for T1, T2 in _poses():
        got = compute_f12(T1, T2, cam).reshape(9)
        want = FO.f12_compute(T1.reshape(12), T2.reshape(12), *K)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (T1, T2)
        nonzero += bool(np.any(want != 0))
    # identity against identity has t12 = 0 and so F12 = 0; every other pose pair gives a matrix
    assert nonzero == len(_poses()) - 1


def _error_matrix(T1, T2):
    """|F12 - exact| entry by entry, from float epsilon and the magnitudes that enter each sum.  Every rounding of f12_compute is a
    relative error of at most eps on a value whose magnitude the matrices of absolute values bound: the two inverses (1 each), R12
    (the double sum stored as float: 1), t12 (a three-term float sum, its scaling and the store: 4 -- relative to
    |R12| |t2| + |t1|, not to |t12|, which may cancel), and three products of three terms (3 + the store = 4 each): 19, taken as
    20.  So |dF| <= 20 eps * |K1^-T| skew(|R12| |t2| + |t1|) |R12| |K2^-1|, all entries non-negative."""
    fx, fy, cx, cy = K
    R1, t1, R2, t2 = [a.astype(np.float64) for a in (T1[:, :3], T1[:, 3], T2[:, :3], T2[:, 3])]
    R12 = np.abs(R1 @ R2.T)
    ta = R12 @ np.abs(t2) + np.abs(t1)
    S = np.array([[0, ta[2], ta[1]], [ta[2], 0, ta[0]], [ta[1], ta[0], 0]])
    K1ti = np.abs(np.linalg.inv(np.array([[fx, 0, 0], [0, fy, 0], [cx, cy, 1.0]])))
    K2i = np.abs(np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])))
    return 20 * EPS * (K1ti @ S @ R12 @ K2i)


def test_f12_satisfies_the_epipolar_constraint():
    """x1' F12 x2 = 0 for the two images of one world point (the form CheckDistEpipolarLine uses: the line of kp1 in image 2 is
    kp1' F12).  The points are made in double from the float poses, so the exact F gives a residual at double rounding and
    |x1' F12 x2| <= sum_ij |x1_i| |dF_ij| |x2_j| with dF of _error_matrix: each term with the pixel magnitudes it really meets.
    The bound is tight enough to tell a fundamental matrix from a near miss: the transpose (the other convention) and 1 % noise on the
    entries exceed it for every pose pair, one entry scaled by 1.5 for nearly all."""
    from orb_slam2_ssd_semantic_amd import compute_f12
    cam = _cam()
    fx, fy, cx, cy = K
    checked, scaled_caught, poses = 0, 0, _poses()[7:60]
    for T1, T2 in poses:
        rng = np.random.default_rng(7)
        F = compute_f12(T1, T2, cam).astype(np.float64)
        R1, t1, R2, t2 = [a.astype(np.float64) for a in (T1[:, :3], T1[:, 3], T2[:, :3], T2[:, 3])]
        z = rng.uniform(1.0, 8.0, 20)
        p1 = np.stack([rng.uniform(20, 620, 20), rng.uniform(20, 460, 20)], 1)
        Xc1 = np.stack([(p1[:, 0] - cx) / fx * z, (p1[:, 1] - cy) / fy * z, z], 1)
        Xw = (Xc1 - t1) @ R1
        Xc2 = Xw @ R2.T + t2
        ok = Xc2[:, 2] > 0.1
        p2 = np.stack([fx * Xc2[:, 0] / Xc2[:, 2] + cx, fy * Xc2[:, 1] / Xc2[:, 2] + cy], 1)
        ok &= (np.abs(p2) < 800).all(1)
        x1 = np.concatenate([p1, np.ones((20, 1))], 1)[ok]
        x2 = np.concatenate([p2, np.ones((20, 1))], 1)[ok]
        bound = np.einsum("ni,ij,nj->n", np.abs(x1), _error_matrix(T1, T2), np.abs(x2))

        def resid(G):
            return np.abs(np.einsum("ni,ij,nj->n", x1, G, x2))
        assert (resid(F) <= bound).all(), (resid(F) / bound).max()
        assert (resid(F.T) > bound).any(), "the transposed matrix passes"
        assert (resid(F * (1 + 0.01 * np.random.default_rng(1).normal(size=(3, 3)))) > bound).any(), "1 % noise passes"
        assert (resid(np.zeros((3, 3))) <= bound).all()   # zero satisfies any such bound: F12 != 0 is test_compute_f12_equals_oracle_bitwise's
        G = F.copy()
        G[0, 0] *= 1.5
        scaled_caught += bool((resid(G) > bound).any())
        checked += int(ok.sum())
    assert checked > 500 and scaled_caught >= len(poses) - 3, scaled_caught


def test_epipole_oracle_equals_the_pinned_arithmetic():
    """tests/f12_oracle.py::f12_epipole is the arithmetic tests/proj_cases.py::tri_core_inputs states (which the compiled
    reference pins in tests/test_ref_pin.py)"""
    for seed in range(20):
        k1, k2, _ = PC.triangulation_case(np.random.default_rng(seed), 5, 5, 2)
        _, _, ex, ey = PC.tri_core_inputs(k1, k2, False)
        T2 = np.concatenate([k2["Rcw"], k2["tcw"][:, None]], 1).astype(f32)
        gx, gy = FO.f12_epipole(T2.reshape(12), k1["Ow"], *k2["K"][:4])
        assert (f32(gx).view(np.uint32), f32(gy).view(np.uint32)) == (f32(ex).view(np.uint32), f32(ey).view(np.uint32))


def test_tri_search_scratch_bytes_limits():
    from orb_slam2_ssd_semantic_amd import _ffi, mapping
    L = _ffi.lib()
    info = mapping.tri_search_info()
    assert info["max_cap"] == 8192 and info["lanes"] * info["queries_per_pass"] == 256 and info["tile"] >= info["lanes"]
    assert L.orbfe_tri_search_info(99) == -1
    prev = 0
    for P, cap in ((0, 1), (1, 1), (1, 100), (2, 100), (2, 2000), (20, 2000), (256, 2000), (256, 8192), (4095, 8192)):
        n = L.orbfe_tri_search_scratch_bytes(P, cap)
        assert n >= prev and n >= 0, (P, cap, n, prev)
        prev = n
    assert L.orbfe_tri_search_scratch_bytes(1, 8192) > 0 and L.orbfe_tri_search_scratch_bytes(1, 8193) == -1
    assert L.orbfe_tri_search_scratch_bytes(1, 0) == -1 and L.orbfe_tri_search_scratch_bytes(-1, 10) == -1
    assert L.orbfe_tri_search_scratch_bytes(4096, 8192) == -1          # npairs * cap == 2^25
    assert L.orbfe_tri_search_scratch_bytes((1 << 25) - 1, 1) > 0 and L.orbfe_tri_search_scratch_bytes(1 << 25, 1) == -1
    try:
        mapping.tri_search_scratch_bytes(1, 9000)
    except ValueError:
        pass
    else:
        raise AssertionError("cap 9000 accepted")

"""The geometry of the device-resident tracker on the CPU: tests/track_oracle.py against the compiled reference
(PredictScale), against the literal UpdateLastFrame loop (selection), against its own case table (every isInFrustum gate has a
point that it alone rejects), and the product's host entry points orbfe_frustum_points / orbfe_track_scratch_bytes against the
oracle.  No GPU; comparisons are exact."""
import numpy as np
import pytest

import proj_cases as PC
import track_oracle as TO

F = np.float32


@pytest.fixture(scope="module")
def sweep():
    mx, ds = TO.predict_sweep()
    mx.setflags(write=False)
    ds.setflags(write=False)
    return mx, ds


def test_predict_scale_equals_the_compiled_reference(sweep):
    """ceil((float)log(ratio) / mfLogScaleFactor) on the +-6 float neighbours of 1.2^k, k = -2 .. 9, and 10^5 random ratios"""
    from oracle import ref_ffi as R
    mx, ds = sweep
    assert len(mx) == 100156
    want = np.array([R.predict_scale(float(m), float(d), float(TO.LOG_SF), TO.NLEVELS) for m, d in zip(mx, ds)])
    got = np.array([TO.predict_scale(m, d) for m, d in zip(mx, ds)])
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], mx[got != want][:8], ds[got != want][:8])
    assert set(want.tolist()) == set(range(8))   # every level, both clamps


def test_selection_equals_the_literal_loop():
    """the closed form min(n_pos, max(c, 100) + 1) against the sort-visit-break loop: counts around 100, thresholds below all,
    above all and on a depth, ties in z, non-positive and NaN depths"""
    rng = np.random.default_rng(5)
    for it in range(600):
        n = int(rng.choice([0, 1, 50, 99, 100, 101, 102, 150, 400]))
        z = rng.uniform(0.3, 12.0, n).astype(F)
        if n > 4:
            z[rng.integers(0, n, n // 4)] = z[rng.integers(0, n, n // 4)]     # ties
            z[rng.integers(0, n, n // 10 + 1)] = rng.choice([0.0, -1.0, np.nan])
        pos = z[z > 0]
        th = [0.1, 100.0, float(rng.uniform(0.3, 12.0))] + ([float(rng.choice(pos))] if len(pos) else [])
        for t in th:
            a, b = TO.select_literal(z, t), TO.select_closed(z, t)
            assert np.array_equal(a, b), (it, n, t)
            assert not a[~(z > 0)].any()


def test_frustum_case_table_has_a_point_for_every_gate():
    """every gate of isInFrustum rejects one point of the table ALONE (the point passes with that gate left out, and the gate is
    the one the oracle names) next to a neighbour that passes; the cosine and level pairs land on either side of their edge"""
    cases = TO.frustum_cases()
    seen_gates = set()
    for name, (rej, ok) in cases.items():
        r_ok, g_ok = TO.run_case_point(ok)
        assert r_ok is not None and g_ok is None, (name, g_ok)
        if rej["gate"] is None:
            r, g = TO.run_case_point(rej)
            assert r is not None, (name, g)
            continue
        r, g = TO.run_case_point(rej)
        assert r is None and g == rej["gate"], (name, g)
        r2, g2 = TO.run_case_point(rej, off=(rej["gate"],))
        assert r2 is not None, (name, "also rejected by", g2)
        seen_gates.add(g)
    assert seen_gates == set(TO.GATES)
    # viewCos just under 0.5 and at it
    lo, hi = cases["view_cos_just_under_0.5"]
    assert TO.run_case_point(lo, off=("view_cos",))[0]["view_cos"] == TO.dn(0.5) and TO.run_case_point(hi)[0]["view_cos"] == F(0.5)
    # either side of 0.998: the radius of RadiusByViewingCos
    sf = PC.scale_factors()
    for c in cases["view_cos_0.998"]:
        r = TO.run_case_point(c)[0]
        proj, inv = TO.frustum(c["T"], TO.K0, TO.BOUNDS0, [c["P"]], [c["Pn"]], [c["min_dist"]], [c["max_dist"]])
        q, _ = TO.queries_local_map(proj, inv, [1], 1.0, sf)
        assert q["r"][0] == F(c["want"]["radius"] * sf[r["level"]]), c["want"]
    assert cases["view_cos_0.998"][0]["Pn"][2] == TO.dn(F(0.998)) and cases["view_cos_0.998"][1]["Pn"][2] == F(0.998)
    # the level clamps
    for key in ("level_0", "level_7"):
        for c in cases[key]:
            r = TO.run_case_point(c)[0]
            assert r["level"] == c["want"]["level"], (key, r)
            if "unclamped" in c["want"]:
                assert r["unclamped"] == c["want"]["unclamped"], (key, r)


def _random_frustum_points(rng, T, n):
    pts = [TO._point_at(T, float(rng.uniform(-60, 700)), float(rng.uniform(-60, 540)), float(rng.choice([-1, 1, 1, 1, 1]) * rng.uniform(0.4, 9)),
                        cos=float(rng.uniform(0.3, 1.0)), ratio=float(rng.uniform(0.8, 4.5))) for _ in range(n)]
    for p in pts:
        p["seen"], p["bad"] = int(rng.random() < 0.1), int(rng.random() < 0.05)
        if rng.random() < 0.1:
            p["min_dist"] = F(float(p["max_dist"]) * 0.9)
    return pts


def _arrays(pts):
    return (np.stack([p["P"] for p in pts]), np.stack([p["Pn"] for p in pts]), np.array([p["min_dist"] for p in pts], F),
            np.array([p["max_dist"] for p in pts], F), np.array([p["seen"] for p in pts], np.uint8), np.array([p["bad"] for p in pts], np.uint8))


def test_host_frustum_points_equals_the_oracle(sweep):
    """orbfe_frustum_points == the numpy oracle: the case table, 3 000 random points under a posed camera, and PredictScale on
    the sweep (identity pose, P = (0, 0, dist), max_dist = ratio * dist: ratios below 1 are past max_dist and out of view)"""
    from orb_slam2_ssd_semantic_amd import tracking
    cam = tracking.camera(*TO.K0, *TO.BOUNDS0)
    rng = np.random.default_rng(77)
    sets = []
    for name, pair in TO.frustum_cases().items():
        for c in pair:
            sets.append((c["T"], [c]))
    T = TO._posed()
    sets.append((T, _random_frustum_points(rng, T, 3000)))
    nin = 0
    for T, pts in sets:
        P, Pn, mn, mx, seen, bad = _arrays(pts)
        want, win = TO.frustum(T, TO.K0, TO.BOUNDS0, P, Pn, mn, mx, seen=seen, bad=bad)
        got, gin = tracking.frustum_points(T, cam, TO.LOG_SF, TO.NLEVELS, P, Pn, mn, mx, seen, bad)
        assert np.array_equal(gin, win) and got.tobytes() == want.tobytes(), (np.flatnonzero(gin != win)[:8],)
        nin += int(win.sum())
    assert 500 < nin < 2800
    mx, ds = sweep
    P = np.zeros((len(mx), 3), F)
    P[:, 2] = ds
    Pn = np.tile(np.array([0, 0, 1], F), (len(mx), 1))
    got, gin = tracking.frustum_points(TO.IDENTITY, cam, TO.LOG_SF, TO.NLEVELS, P, Pn, np.zeros(len(mx), F), mx)
    want = np.array([TO.predict_scale(m, d) if d <= m else -1 for m, d in zip(mx, ds)])
    assert np.array_equal(got["level"], want) and np.array_equal(gin, (want >= 0).astype(np.uint8))
    assert (want >= 0).sum() > 70000


def test_unproject_oracle_inverts_the_projection():
    """a sanity check of the restatement itself: UnprojectStereo under pose T, projected back with T, returns the keypoint"""
    rng = np.random.default_rng(3)
    T = TO._posed()
    xy = np.stack([rng.uniform(0, 640, 200), rng.uniform(0, 480, 200)], 1).astype(F)
    z = rng.uniform(0.5, 8, 200).astype(F)
    z[::7] = 0
    wp, created = TO.unproject_select(xy, z, T, TO.K0, 3.0)
    T3 = TO.T34(T)
    for i in np.flatnonzero(z > 0):
        pc = TO.to_camera(T3, wp[i])
        u, v = TO.K0[0] * pc[0] / pc[2] + TO.K0[2], TO.K0[1] * pc[1] / pc[2] + TO.K0[3]
        assert abs(u - xy[i, 0]) < 1e-2 and abs(v - xy[i, 1]) < 1e-2 and abs(pc[2] - z[i]) < 1e-4
    assert not wp[z <= 0].any() and not created[z <= 0].any()
    assert np.array_equal(created.astype(bool), TO.select_closed(z, 3.0))


def test_scratch_bytes():
    """orbfe_track_scratch_bytes: counts (4 B), per-lane counts (64 x 2 B), offsets (4 B, one more) per query slot and 4 B per
    entry, each block rounded up to 256 bytes; -1 outside the limits"""
    from orb_slam2_ssd_semantic_amd import _ffi, tracking

    def al(x):
        return (x + 255) // 256 * 256
    for nf, qcap, ent in ((1, 1, 0), (1, 1000, 65536), (16, 1024, 1 << 20), (256, 1024, 25_000_000), (3, 77, 12345)):
        ng = nf * qcap
        assert tracking.scratch_bytes(nf, qcap, ent) == al(ng * 4) + al(ng * 128) + al((ng + 1) * 4) + al(max(ent, 1) * 4), (nf, qcap, ent)
    assert tracking.scratch_bytes(0, 5, 0) == 256 * 4
    L = _ffi.lib()
    for bad in ((-1, 1, 0), (1, 0, 0), (1, 1, -1), (1 << 13, 1 << 12, 0), (1, 1, 1 << 32)):
        assert L.orbfe_track_scratch_bytes(*bad) == -1, bad
        with pytest.raises(ValueError):
            tracking.scratch_bytes(*bad)

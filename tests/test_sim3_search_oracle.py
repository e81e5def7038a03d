"""The batched SearchBySim3 / SearchByProjection(pKF, Scw, ...) without a GPU: the numpy oracle (tests/sim3_search_oracle.py), fed the
poses of orbfe_sim3_pair_pose, against the compiled reference (ref_search_by_sim3 / ref_search_by_projection_kf_sim3) where oracle/_ref
is built; the host pose and the host gate orbfe_sim3_gate_points (trk_sim3_pair_pose / trk_gate_sim3, the functions the kernels run)
against the oracle as bit patterns, on seeds and on a hand-made table of edges; the hand-made scenarios' own expectations."""
import numpy as np
import pytest

import proj_cases as PC
import sim3_search_cases as SC
import sim3_search_oracle as SO
from oracle import ref_ffi as R

F = np.float32
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built")
SHAPES = ((0, 0), (0, 40), (1, 1), (300, 280))
SEEDS = tuple(range(12))


def _lc():
    from orb_slam2_ssd_semantic_amd import loopclosing
    return loopclosing


def _poses(s12, R12, t12):
    T12, T21 = _lc().sim3_pair_pose(s12, R12, t12)
    return T12.reshape(3, 4), T21.reshape(3, 4)


def _shape(seed):
    return SHAPES[seed % len(SHAPES)] if seed < 8 else SHAPES[3]


@pytest.mark.parametrize("seed", SEEDS)
def test_pair_pose_equals_oracle(seed):
    rng = np.random.default_rng(500 + seed)
    s = F(rng.uniform(0.3, 3.0))
    Rm = PC._rot(rng, 40.0).astype(F)
    t = rng.normal(0, 1.0, 3).astype(F)
    if seed == 0:
        s, Rm, t = F(1), np.eye(3, dtype=F), np.zeros(3, F)
    T12, T21 = _poses(s, Rm, t)
    w12, w21 = SO.pair_pose(s, Rm, t)
    assert np.array_equal(T12.view(np.uint32), w12.view(np.uint32)) and np.array_equal(T21.view(np.uint32), w21.view(np.uint32))


@needs_ref
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_search_by_sim3_equals_reference(seed):
    n1, n2 = _shape(seed)
    k1, k2, s12, R12, t12, m_in = PC.sim3_pair_case(np.random.default_rng(9100 + seed), n1, n2)
    T12, T21 = _poses(s12, R12, t12)
    got, nf, _, _ = SO.search_by_sim3(k1, k2, T12, T21, 7.5, m_in)
    want, rv = R.search_by_sim3(k1, k2, s12, R12, t12, 7.5, m_in)
    assert nf == rv and np.array_equal(got, want[:n1])
    assert n1 < 100 or nf > 20


@needs_ref
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_search_by_projection_kf_sim3_equals_reference(seed):
    nkf, npts = _shape(seed)
    kf, Scw, pts, m_in = PC.kf_sim3_case(np.random.default_rng(9300 + seed), nkf, npts)
    got, nm = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
    want, rv = R.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
    assert nm == rv and np.array_equal(got, want)
    assert nkf < 100 or nm > 10


def _gate_both(T_own, T_to, K, bounds, th, sf, log_sf, wp, mn, mx):
    lc = _lc()
    cam = lc.camera(*[float(v) for v in K[:5]], *[float(b) for b in bounds])
    q, level, ok = lc.sim3_gate_points(np.asarray(T_own, F).reshape(-1), np.asarray(T_to, F).reshape(-1), cam, th, sf, log_sf, wp, mn, mx)
    wq, wlevel, wok = SO.gate_points(T_own, T_to, K, bounds, th, sf, log_sf, wp, mn, mx)
    assert np.array_equal(ok, wok) and np.array_equal(level, wlevel)
    assert np.array_equal(q.view(np.uint32).reshape(-1, 8), wq)
    return q, level, ok


@pytest.mark.parametrize("seed", SEEDS)
def test_gate_equals_oracle_on_seeds(seed):
    n1, n2 = _shape(seed)
    k1, k2, s12, R12, t12, _ = PC.sim3_pair_case(np.random.default_rng(9100 + seed), n1, n2)
    T12, T21 = _poses(s12, R12, t12)
    for ks, ko, T_to in ((k1, k2, T21), (k2, k1, T12)):
        _, _, ok = _gate_both(SO.pose34(ks), T_to, ko["K"], ko["bounds"], 7.5, ko["scale_factors"], ko["log_scale"], ks["world_pos"], ks["min_dist"],
                              ks["max_dist"])
        assert len(ok) < 100 or 0 < ok.sum() < len(ok)


def test_gate_planted_edges():
    """identity poses, so pc' = P exactly and |pc'| = z for a point on the axis"""
    I34 = np.concatenate([np.eye(3, dtype=F), np.zeros((3, 1), F)], 1)
    sf, log_sf = SC.SF, SC.LOG_SF
    up = lambda x: np.nextafter(F(x), F(np.inf))     # noqa: E731
    down = lambda x: np.nextafter(F(x), F(-np.inf))  # noqa: E731
    # the image bounds on a camera with fx = 1, cx = 0 and z = 1: u = x exactly
    K1, bounds = (1.0, 1.0, 0.0, 0.0, 40.0), (0.0, 640.0, 0.0, 480.0)
    wp = np.array([[0, 0, 1], [640, 0, 1], [down(640), 0, 1], [0, 480, 1], [0, down(480), 1], [down(0), 0, 1], [3, 3, 0], [3, 3, down(0)],
                   [0, 0, 0]], F)
    n = len(wp)
    _, _, ok = _gate_both(I34, I34, K1, bounds, 7.5, sf, log_sf, wp, np.full(n, 1e-3, F), np.full(n, 1e4, F))
    assert list(ok) == [1, 0, 1, 0, 1, 0, 0, 0, 0]
    # the distance bounds on the axis of the usual camera: dist3D = z exactly
    K = (SC.FX, SC.FY, SC.CX, SC.CY, SC.BF)
    mn, mx = F(1.7), F(9.3)
    lo, hi = F(F(0.8) * mn), F(F(1.2) * mx)
    z = np.array([lo, down(lo), hi, up(hi)], F)
    wp = np.stack([np.zeros(4, F), np.zeros(4, F), z], 1)
    q, level, ok = _gate_both(I34, I34, K, bounds, 7.5, sf, log_sf, wp, np.full(4, mn, F), np.full(4, mx, F))
    assert list(ok) == [1, 0, 1, 0]
    assert q["u"][0] == F(SC.CX) and q["v"][0] == F(SC.CY) and q["flags"][0] == 0
    # the predicted level clamped at 0 (the point is farther than mfMaxDistance) and at nlevels - 1
    wp = np.array([[0, 0, 2.3], [0, 0, 1.0], [0, 0, 1.0]], F)
    q, level, ok = _gate_both(I34, I34, K, bounds, 7.5, sf, log_sf, wp, np.array([0.1, 0.1, 0.1], F), np.array([2.0, 1000.0, 1.2 ** 6.5], F))
    assert list(ok) == [1, 1, 1] and list(level) == [0, len(sf) - 1, len(sf) - 1]
    assert list(q["min_level"]) == [-1, len(sf) - 2, len(sf) - 2] and q["r"][0] == F(7.5) * sf[0]
    # a real similarity in front of an own pose: the two-stage product, not one fused pose
    rng = np.random.default_rng(3)
    T_own = np.concatenate([PC._rot(rng, 20.0).astype(F), rng.normal(0, 0.3, (3, 1)).astype(F)], 1)
    T12, T21 = _poses(1.3, PC._rot(rng, 10.0), rng.normal(0, 0.2, 3))
    wp = rng.normal(0, 1.5, (200, 3)).astype(F) + np.array([0, 0, 4], F)
    _, _, ok = _gate_both(T_own, T21, K, bounds, 7.5, sf, log_sf, wp, np.full(200, 0.5, F), np.full(200, 30.0, F))
    assert 0 < ok.sum() < 200


def test_hand_made_scenarios_hold_in_the_oracle():
    """what the GPU tests expect of the hand-made cases is what the restated members give"""
    rng = np.random.default_rng(77)
    T12, T21 = _poses(*SC.IDENT)
    k1, k2 = SC.tie_pair(rng)
    _, nf, vn1, vn2 = SO.search_by_sim3(k1, k2, T12, T21, 7.5, np.full(3, -1, np.int32))
    assert vn1[2] == 1 and vn2[2] == 1 and nf == 0
    k1, k2, want = SC.threshold_pair(rng, 100)
    assert np.array_equal(SO.search_by_sim3(k1, k2, T12, T21, 7.5, np.full(6, -1, np.int32))[2], want)
    k1, k2, m_in, (w1, w2, wout, wn) = SC.agreement_pair(rng)
    out, nf, vn1, vn2 = SO.search_by_sim3(k1, k2, T12, T21, 7.5, m_in)
    assert np.array_equal(vn1, w1) and np.array_equal(vn2, w2) and np.array_equal(out, wout) and nf == wn
    kf, Scw, pts, m_in, want, wn = SC.claims_case(rng)
    got, nm = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
    assert np.array_equal(got, want) and nm == wn


@needs_ref
def test_hand_made_scenarios_hold_in_the_reference():
    rng = np.random.default_rng(77)
    k1, k2 = SC.tie_pair(rng)
    SC.threshold_pair(rng, 100)
    SC.agreement_pair(rng)   # its preset index >= N2 cannot be given to the mock: the oracle alone holds that scenario
    kf, Scw, pts, m_in, want, wn = SC.claims_case(rng)
    got, rv = R.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
    assert np.array_equal(got, want) and rv == wn
    out, rv = R.search_by_sim3(k1, k2, *SC.IDENT, 7.5, np.full(3, -1, np.int32))
    assert rv == 0 and (out == -1).all()


def test_limits_and_scratch():
    lc = _lc()
    assert lc.sim3_search_scratch_bytes(0, 1) > 0 and lc.sim3_search_scratch_bytes(256, 2000) > 256 * 2 * 2000 * 44
    from orb_slam2_ssd_semantic_amd import tracking
    assert lc.sim3_search_scratch_bytes(4, 2000, 500, 2000, 100000) > tracking.scratch_bytes(4, 500, 100000)
    for bad in ((1, 15361), (1, 0), (1 << 13, 4096)):
        with pytest.raises(ValueError):
            lc.sim3_search_scratch_bytes(*bad)
    # the qcap >= 1 form: npairs * qcap < 2^25, nentries <= 2^25, ent_cap < 2^32, each on its last good and first bad value
    assert lc.sim3_search_scratch_bytes(1 << 12, 64, (1 << 13) - 1, 0, 0) > 0 and lc.sim3_search_scratch_bytes(1, 64, (1 << 25) - 1, 0, 0) > 0
    assert lc.sim3_search_scratch_bytes(1, 64, 1, 1 << 25, 0) > 1 << 25
    assert lc.sim3_search_scratch_bytes(1, 64, 1, 0, (1 << 32) - 1) > lc.sim3_search_scratch_bytes(1, 64, 1, 0, 0)
    for bad in ((1 << 12, 64, 1 << 13, 0, 0), (1, 64, 1 << 25, 0, 0), (1, 64, 1, (1 << 25) + 1, 0), (1, 64, 1, 0, 1 << 32), (1, 64, -1, 0, 0),
                (1, 64, 1, -1, 0), (1, 64, 1, 0, -1)):
        with pytest.raises(ValueError):
            lc.sim3_search_scratch_bytes(*bad)

"""tests/sim3_search_edge_cases.py checked on the CPU, so that tests/test_gpu_sim3_search_edges.py cannot go blind when someone edits
a case: (a) with SIM3S_BREAK unset the oracle gives, on every input of the older tests, the bits it gave before the trace and the
switch were added (tests/golden/sim3_search_oracle_digests.json); (b) a census of the oracle's trace over the table: every listed
comparison is met with every listed outcome; (c) every rule of SIM3S_RULES, broken alone, changes what the GPU test compares in at
least one case of the table; (d) the planted cases do what their builders say; (e) where oracle/_ref is built, every case the mocks
can express equals the compiled reference.

Run against the older inputs (sim3_search_edge_cases.old_inputs(): the seeded parity cases and sim3_search_cases.py, 58 runs), 14 of
the 30 rules change nothing: z_le, u_min_open, u_max_closed, v_min_open, v_max_closed, d08_le, d12_ge, clamp0, clampN, r_no_sf,
fused_pose, already2_clip, found_live, angle_le (`PYTHONPATH=. python tests/test_sim3_search_edge_cases.py` from the repository's
root prints the list; test_old_inputs_report_and_the_table_misses_none prints the same under `pytest -s`).  The table misses
one, z_le, which no finite input can show: at z == 0 the quotient is infinite or not a number and the image test throws the point
out either way (test_z_equal_zero_is_out_under_either_reading).

Not held against the compiled reference: search_exact_th0 / _th255 and proj_exact_th0 / _th255 (TH_HIGH and TH_LOW are constants
of the reference), dup_point (the mock builds one MapPoint per list entry, so no point can stand in a list twice) and bookkeeping as
it stands (an index >= N2 in vpMatches12 is a pointer the mock cannot make; the same scenario with -2 in its place is held)."""
import hashlib
import json
import os

import numpy as np
import pytest

import proj_cases as PC
import sim3_search_cases as SC
import sim3_search_edge_cases as EC
import sim3_search_oracle as SO
from oracle import ref_ffi as R

F = np.float32
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built")
DIGESTS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_search_oracle_digests.json")))
UNREACHABLE = {"z_le"}


def _digest(out):
    return hashlib.sha256(EC.compared(out)).hexdigest()[:16]


@pytest.fixture(scope="module")
def runs():
    """name -> (compared bytes, trace) of the unbroken oracle for every case of the table, computed once"""
    out = {}
    for name, c in EC.table().items():
        tr = []
        out[name] = (EC.compared(EC.run(c, tr)), tr)
    return out


# ---- (a) the switch unset ----------------------------------------------------------------------------------------------------------
def test_digest_table_names_the_old_inputs():
    assert set(DIGESTS) == set(EC.old_inputs())


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_unbroken_oracle_reproduces_the_old_inputs(name):
    assert SO.SIM3S_BREAK == frozenset()
    c = EC.old_inputs()[name]
    assert _digest(EC.run(c)) == DIGESTS[name]
    assert _digest(EC.run(c, [])) == DIGESTS[name]   # tracing changes nothing


def test_sizes():
    for name, c in EC.table().items():
        if c["kind"] == "sim3":
            assert max(len(c["k1"]["octave"]), len(c["k2"]["octave"])) <= 1000, name
        else:
            assert len(c["kf"]["octave"]) <= 1000 and len(c["pts"]["bad"]) <= 1100, name


# ---- (b) the census ----------------------------------------------------------------------------------------------------------------
def test_census(runs):
    seen = {}
    for name, (_, tr) in runs.items():
        for key, val in tr:
            seen.setdefault(key, {}).setdefault(val, name)
    for key, need in EC.CENSUS.items():
        assert need <= set(seen.get(key, {})), (key, need - set(seen.get(key, {})))
    assert set(seen) == set(EC.CENSUS)   # nothing traced that the census does not ask about


# ---- (c) sensitivity ----------------------------------------------------------------------------------------------------------------
def _noticed_by(rule, cases, base, first_only=False):
    hit = []
    for name, c in cases.items():
        if EC.compared(EC.with_break(rule, lambda: EC.run(c))) != base[name]:
            hit.append(name)
            if first_only:
                break
    return hit


@pytest.mark.parametrize("rule", sorted(SO.SIM3S_RULES))
def test_broken_rule_changes_what_the_gpu_test_compares(runs, rule):
    hit = _noticed_by(rule, EC.table(), {k: v[0] for k, v in runs.items()})
    assert SO.SIM3S_BREAK == frozenset()
    assert bool(hit) != (rule in UNREACHABLE), (rule, hit)


def test_z_equal_zero_is_out_under_either_reading():
    """z < 0 against z <= 0: with finite poses, points and image bounds no input tells them apart.  z == 0 makes invz infinite, x and
    y infinite or not a number, so is u, and `u >= minx && u < maxx` is false for every finite bound."""
    rng = np.random.default_rng(9610)
    I34 = np.concatenate([np.eye(3, dtype=F), np.zeros((3, 1), F)], 1)
    perm = [np.eye(3, dtype=F)[list(p)] for p in ((0, 1, 2), (1, 0, 2), (2, 1, 0), (0, 2, 1))]
    n = 0
    for i in range(400):
        P = rng.choice([0.0, 1e-30, -3.0, 7.5, 1e30], 3).astype(F) * rng.choice([-1, 1], 3).astype(F)
        if i % 3:
            P = rng.normal(0, 5.0, 3).astype(F)
        T_own = np.concatenate([perm[i % 4], np.zeros((3, 1), F)], 1)
        P[int(np.flatnonzero(perm[i % 4][2])[0])] = F(0) if i % 2 else F(-0.0)   # the coordinate that becomes z
        K = (float(rng.choice([1.0, 500.0])), 500.0, float(rng.choice([0.0, 320.0])), 240.0, 40.0)
        bounds = (float(rng.choice([-1e30, 0.0])), float(rng.choice([640.0, 1e30])), float(rng.choice([-1e30, 0.0])), 480.0)
        args = (T_own, I34, K, bounds, 7.5, SC.SF, SC.LOG_SF, P, F(0.0), F(1e30))
        assert SO.affine(I34, SO.affine(T_own, P))[2] == 0
        tr = []
        assert SO.gate_point(*args, trace=tr) is None and ("z", 0) in tr and not any(k == "d08" for k, _ in tr)   # stopped by the image test
        assert EC.with_break("z_le", lambda: SO.gate_point(*args)) is None
        n += 1
    assert n == 400


def test_old_inputs_report_and_the_table_misses_none(runs):
    """which rules the older inputs let a wrong kernel break: a finding (see the module docstring), not a target"""
    old = EC.old_inputs()
    order = sorted(old, key=lambda k: len(old[k].get("k1", old[k].get("kf"))["octave"]))   # the small ones first
    cases = {k: old[k] for k in order}
    base = {k: EC.compared(EC.run(c)) for k, c in cases.items()}
    unnoticed = [rule for rule in SO.SIM3S_RULES if not _noticed_by(rule, cases, base, first_only=True)]
    print(f"\n{len(unnoticed)} of {len(SO.SIM3S_RULES)} rules change nothing on the {len(old)} older inputs: {', '.join(unnoticed)}")
    table_base = {k: v[0] for k, v in runs.items()}
    assert [rule for rule in SO.SIM3S_RULES if not _noticed_by(rule, EC.table(), table_base, first_only=True)] == sorted(UNREACHABLE)
    assert set(UNREACHABLE) <= set(unnoticed)


# ---- (d) the planted cases ----------------------------------------------------------------------------------------------------------
def test_gate_exact_finds_what_it_plants():
    c, want = EC.gate_exact()
    _, nf, vn1, vn2 = EC.run(c)
    assert np.array_equal(vn1, want) and nf == 0 and (vn2 == -1).all() and (want >= 0).sum() >= 10 and (want < 0).sum() >= 8


@pytest.mark.parametrize("th_high", [0, 100, 255])
def test_search_exact_finds_what_it_plants(th_high):
    c, want = EC.search_exact(th_high)
    assert np.array_equal(EC.run(c)[2], want)


def test_bookkeeping():
    out, nf, vn1, vn2 = EC.run(EC.bookkeeping())
    assert list(out) == [0, 1, -1, -2, 9, 5, -1] and nf == 2 and list(vn1) == [0, -1, 1, -1, -1, 5, -1] and list(vn2) == [0, -1, -1, 3, 4, 5]


def test_fused_pose_case_has_points_the_two_products_disagree_on():
    c, differ = EC.fused_pose()
    assert differ >= 3 and len(c["k1"]["octave"]) <= 40


def test_cascade_and_dup_point():
    c, want = EC.cascade()
    got, nm = EC.run(c)
    assert np.array_equal(got, want) and nm == 8 and sorted(got) == list(range(8))   # entry k on its k-th choice, the ninth on none
    got, nm = EC.run(EC.dup_point())
    assert list(got) == [0, 0, 1] and nm == 3


def test_proj_lists_oracle_equals_the_plain_oracle_on_plain_lists():
    import sim3_search_checks as CK
    kf, Scw, pts, m = PC.kf_sim3_case(np.random.default_rng(9502), 70, 90)
    want, wn = SO.search_by_projection_kf_sim3(kf, Scw, pts, m, 10)
    got, nm = CK.proj_lists_oracle(kf, Scw, pts, np.arange(90), m)
    assert np.array_equal(got, want) and nm == wn
    got, nm = CK.proj_lists_oracle(kf, Scw, pts, np.arange(90), m, qcap=90)
    assert np.array_equal(got, want) and nm == wn
    got1, nm1 = CK.proj_lists_oracle(kf, Scw, pts, np.arange(90), m, qcap=1)
    assert nm1 <= 1 < wn


# ---- (e) the compiled reference ----------------------------------------------------------------------------------------------------
def _ref_cases():
    out = {}
    for name, c in EC.table().items():
        if name in ("search_exact_th0", "search_exact_th255", "proj_exact_th0", "proj_exact_th255", "dup_point"):
            continue
        if name == "bookkeeping":
            c = dict(c, m_in=np.where(c["m_in"] >= len(c["k2"]["octave"]), -2, c["m_in"]).astype(np.int32))
        out[name] = c
    return out


@needs_ref
@pytest.mark.parametrize("name", sorted(_ref_cases()))
def test_table_equals_the_compiled_reference(name):
    c = _ref_cases()[name]
    if c["kind"] == "sim3":
        want, rv = R.search_by_sim3(c["k1"], c["k2"], *c["sim"], c["th"], c["m_in"])
        got, nf, _, _ = EC.run(c)
        assert nf == rv and np.array_equal(got, want[:len(got)])
    else:
        want, rv = R.search_by_projection_kf_sim3(c["kf"], c["Scw"], c["pts"], c["m_in"], c["th"])
        got, nm = EC.run(c)
        assert nm == rv and np.array_equal(got, want)


if __name__ == "__main__":   # the before number: the rules the older inputs do not notice
    old = EC.old_inputs()
    base = {k: EC.compared(EC.run(c)) for k, c in old.items()}
    for rule in SO.SIM3S_RULES:
        hit = _noticed_by(rule, old, base)
        print(rule, "noticed by", f"{len(hit)} older inputs, e.g. {hit[:3]}" if hit else "NO older input")

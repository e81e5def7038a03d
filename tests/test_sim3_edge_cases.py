"""tests/sim3_edge_cases.py checked on the CPU, so that tests/test_gpu_sim3_edges.py cannot go blind when someone edits a
case: (a) with SIM3_BREAK unset the oracle reproduces every case of the old table bit for bit (digests recorded before the
trace and the switch were added: tests/golden/ransac_oracle_digests.json); (b) a census of the oracle's trace, entry by
entry, with the case that shows it; (c) the six SIM3_BREAK rules, each of which must change a bit of what the GPU test
compares in a named edge case; (d) libm and canonical oracles agree wherever a decision is made.

Run once against the old table (`python tests/test_sim3_edge_cases.py`): of the six rules, sim3_cases.full_table() does
not notice `return_ge` (no iteration counts exactly min_inliers) and `no_identity_arm` (no model takes it).

The reference's Sim3Solver is not compiled anywhere in this project (it needs OpenCV, which is not available: the oracle is
"unpinned", see its docstring), so there is no compiled reference to tie the new cases to; the shim test of
tests/test_shim_sim3.py runs the library, not the reference."""
import hashlib
import json
import os

import numpy as np
import pytest

import sim3_cases as SC
import sim3_edge_cases as EC
import sim3_oracle as SO

DIGESTS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac_oracle_digests.json")))


def _digest(outs):
    return hashlib.sha256(EC.compared(outs)).hexdigest()[:16]


@pytest.fixture(scope="module")
def runs():
    """name -> the canonical oracle's results of every edge case, computed once"""
    return {name: EC.reference(name)[0] for name in EC.table()}


# ---- (a) the switch unset ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.full_table()))
def test_unbroken_oracle_reproduces_the_old_table(name):
    assert SO.SIM3_BREAK == frozenset()
    assert _digest(SC.reference(name)[0]) == DIGESTS["sim3:" + name]


def test_sizes(runs):
    for name, c in EC.table().items():
        assert len(c["X1"]) <= 600 and all(nit <= 200 for nit, _ in c["calls"]), name
    assert max(len(c["X1"]) for c in EC.table().values()) == 513


def test_cases_sit_on_their_committed_seeds():
    assert {name: c["seed"] for name, c in EC.table().items()} == EC.SEEDS


# ---- (b) the census ----------------------------------------------------------------------------------------------------------------
def _log(runs, name, call=0):
    return runs[name][call]["log"]


def test_census_count_equals_min_inliers(runs):
    c = EC.table()["count_eq_min"]
    o, = runs["count_eq_min"]
    assert o["log"][2]["count"] == c["min_inliers"] and not o["found"] and o["iterations_run"] == 5
    assert o["state"]["best_inliers"] == c["min_inliers"] and o["state"]["best"]["T12"].tobytes() == o["log"][2]["T12"].tobytes()
    b = EC.table()["count_eq_min_minus_1"]
    o, = runs["count_eq_min_minus_1"]
    assert b["min_inliers"] == c["min_inliers"] - 1 and o["found"] and o["iterations_run"] == 3 and o["n_inliers"] == c["min_inliers"]
    assert np.array_equal(b["X1"], c["X1"]) and np.array_equal(b["calls"][0][1], c["calls"][0][1])   # the same data


@pytest.mark.parametrize("name,a,b", [("tie_same_chunk", 3, 7), ("tie_31_32", 31, 32)])
def test_census_positive_ties(runs, name, a, b):
    o, = runs[name]
    lg = o["log"]
    assert lg[a]["count"] == lg[b]["count"] > 0 and lg[a]["T12"].tobytes() != lg[b]["T12"].tobytes()
    assert a // 32 == 0 and b // 32 == (1 if name == "tie_31_32" else 0)   # the chunk of 32 hypotheses each falls into
    assert max(x["count"] for i, x in enumerate(lg) if i not in (a, b)) < lg[a]["count"]
    assert o["state"]["best"]["T12"].tobytes() == lg[b]["T12"].tobytes() and o["state"]["best_inliers"] == lg[b]["count"]
    inl = (lg[b]["err1"] < SO.max_errors(EC.table()[name]["sigma2_1"])) & (lg[b]["err2"] < SO.max_errors(EC.table()[name]["sigma2_2"]))
    assert np.array_equal(o["state"]["best_mask"], inl.astype(np.uint8))


@pytest.mark.parametrize("name,finite", [("zero_tie_nan_first", [False, True]), ("zero_tie_nan_last", [True, False])])
def test_census_zero_ties(runs, name, finite):
    o, = runs[name]
    assert [x["finite"] for x in o["log"]] == finite and [x["count"] for x in o["log"]] == [0, 0]
    assert o["state"]["best_inliers"] == 0 and bool(np.isfinite(o["state"]["best"]["T12"]).all()) == finite[1]   # the later one won


def test_census_one_nan_hypothesis_in_a_chunk(runs):
    o, = runs["one_nan_in_chunk"]
    fin = [x["finite"] for x in o["log"]]
    assert fin.count(False) == 1 and not fin[2] and o["found"] and o["iterations_run"] == 7
    assert np.isnan(o["log"][2]["T12"][:3]).any() and np.isnan(o["log"][2]["err1"]).all() and o["log"][2]["count"] == 0


def test_census_clamp(runs):
    for mi in (32, 33, 64):
        c, (o,) = EC.table()[f"clamp_{mi}"], runs[f"clamp_{mi}"]
        assert c["max_its"] == mi < c["calls"][0][0] and (o["iterations_run"], o["no_more"], o["found"]) == (mi, True, False)
    c, outs = EC.table()["clamp_carried"], runs["clamp_carried"]
    assert c["max_its"] == 32 and [nit for nit, _ in c["calls"]] == [20, 40, 10]
    assert [(o["iterations_run"], o["no_more"]) for o in outs] == [(20, False), (12, True), (0, True)]
    a, b = outs[1]["state"], outs[2]["state"]   # the call after no_more changes nothing
    assert outs[2]["T12"] is None and a["iterations"] == b["iterations"] == 32 and a["best_inliers"] == b["best_inliers"]
    assert np.array_equal(a["best_mask"], b["best_mask"]) and a["best"] is b["best"]


@pytest.mark.parametrize("n", [255, 256, 512, 513])
def test_census_pair_counts(runs, n):
    c, (o,) = EC.table()[f"pairs_{n}"], runs[f"pairs_{n}"]
    assert len(c["X1"]) == n and o["found"]
    for i, want in ((254, 0), (255, 1), (256, 1), (257, 0), (n - 2, 0), (n - 1, 1)):
        if 0 <= i < n and not (want == 0 and i in (255, 256, n - 1)):
            assert o["mask"][i] == want, (n, i)


@pytest.mark.parametrize("s", [0.05, 20])
def test_census_scale(runs, s):
    c, (o,) = EC.table()[f"scale_{s}"], runs[f"scale_{s}"]
    assert not c["fix_scale"] and o["found"] and abs(float(o["state"]["best"]["s"]) / s - 1) < 0.02


def test_census_identity_arm(runs):
    assert "identity_arm" in EC.table(), "the bounded scan of sim3_edge_cases.identity_arm found no pair set"
    o, = runs["identity_arm"]
    lg = o["log"][0]
    assert lg["identity"] and lg["finite"] and np.array_equal(lg["R"], np.eye(3, dtype=np.float32)) and o["found"]
    assert not any(x["identity"] for name in SC.full_table() for r in SC.reference(name)[0] for x in r["log"])   # new to the suite


def test_census_truncated_threshold(runs):
    c, (o,) = EC.table()["truncation"], runs["truncation"]
    t1, t2 = SO.max_errors(c["sigma2_1"]), SO.max_errors(c["sigma2_2"])
    u1, u2 = (9.210 * c["sigma2_1"].astype(np.float64)).astype(np.float32), (9.210 * c["sigma2_2"].astype(np.float64)).astype(np.float32)
    lg = o["log"][2]
    assert (((lg["err1"] >= t1) & (lg["err1"] < u1)) | ((lg["err2"] >= t2) & (lg["err2"] < u2))).any()


# ---- (c) sensitivity ----------------------------------------------------------------------------------------------------------------
SENSITIVE = {"tie_gt": "tie_31_32", "return_ge": "count_eq_min", "clamp_le": "clamp_32", "fix_scale_ignored": "scale_0.05",
             "max_errors_no_trunc": "truncation", "no_identity_arm": "identity_arm"}


def test_every_rule_has_a_case():
    assert set(SENSITIVE) == set(SO.SIM3_RULES)


@pytest.mark.parametrize("rule", sorted(SO.SIM3_RULES))
def test_broken_rule_changes_what_the_gpu_test_compares(runs, rule):
    c = EC.table()[SENSITIVE[rule]]
    broken = EC.with_break(rule, lambda: SC.run(c, "canonical"))[0]
    assert SO.SIM3_BREAK == frozenset()
    assert EC.compared(broken) != EC.compared(runs[SENSITIVE[rule]]), rule


# ---- (d) the two oracles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EC.table()))
def test_libm_and_canonical_oracles_decide_alike(runs, name):
    c = EC.table()[name]
    libm, _ = SC.run(c, "libm")
    assert SC.margin(c, libm) > SC.MARGIN
    for a, b in zip(libm, runs[name]):
        assert (a["found"], a["no_more"], a["n_inliers"], a["iterations_run"]) == (b["found"], b["no_more"], b["n_inliers"], b["iterations_run"])
        assert [x["count"] for x in a["log"]] == [x["count"] for x in b["log"]] and np.array_equal(a["mask"], b["mask"])
        assert np.array_equal(a["state"]["best_mask"], b["state"]["best_mask"])


if __name__ == "__main__":   # the before number: the rules the old table does not notice
    base = {k: EC.compared(SC.reference(k)[0]) for k in SC.full_table()}
    for rule in SO.SIM3_RULES:
        hit = [k for k, c in SC.full_table().items() if EC.compared(EC.with_break(rule, lambda: SC.run(c, "canonical"))[0]) != base[k]]
        print(rule, "noticed by", hit or "NO CASE of sim3_cases.full_table()")

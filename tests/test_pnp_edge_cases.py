"""tests/pnp_edge_cases.py checked on the CPU, so that tests/test_gpu_pnp_edges.py cannot go blind when someone edits a case:
(a) with EPNP_BREAK unset the oracle reproduces every replay of the old tables bit for bit (digests recorded before the
trace and the switch were added: tests/golden/ransac_oracle_digests.json); (b) a census read from the oracle's trace, entry
by entry, with the case that shows it; (c) every EPNP_BREAK rule, the EPnP arithmetic ones in both scopes, must change a bit
of what the GPU test compares in a named edge case.

Run once against the old tables (`python tests/test_pnp_edge_cases.py`; ITERATE_CASES, the three rules replays and
older_replay): every rule is noticed in the scope "all" (by the hypotheses of n10 already), but of the eight EPnP rules in
the scope "refine" -- a fault in the cooperative Refine alone -- only solve_for_sign is; the other seven pass unnoticed.

Not covered (pnp_edge_cases.UNREACHED): arms 4, 6 and 7 of _betas_23 at k = 2 (b[0] < 0 with the given signs of b[2] and
b[1]).  Neither search stage (SEARCH, SEARCH_WIDE: 2 x 4 x 60 x 2 and 3 x 9 x 120 x 2 contaminated scenes) reaches
them on a returning Refine over more than four points; arms 4 and 7 of k = 2 appear only on failing Refines whose
refine_inliers the broken rule leaves alone.  A random check of compute_pose would run the single-lane path and cannot stand
in.  qr_solve's singular branch is reached by no contaminated scene of either stage, and by no Refine of the old tables
either (0 of 50 by this trace); map points on an axis-parallel line reach it (refine_qr_singular).

The reference's PnPsolver is not compiled anywhere in this project (it needs OpenCV, which is not available: the oracle is
"unpinned", see its docstring), so there is no compiled reference to tie the new cases to; tests/test_shim_pnp.py runs the
library, not the reference."""
import hashlib
import json
import os

import numpy as np
import pytest

import pnp_cases as PC
import pnp_edge_cases as EC
import pnp_oracle as PO

DIGESTS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac_oracle_digests.json")))
OLD = {**{name: (lambda name=name: PC.replay(name)[2]) for name in PC.ITERATE_CASES},
       **{"rules_" + w: (lambda w=w: PC.rules_replay(w)[2]) for w in ("tie", "past5", "again")}, "older": lambda: PC.older_replay()[2]}


@pytest.fixture(scope="module")
def tab():
    return EC.table()


# ---- (a) the switch unset ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OLD))
def test_unbroken_oracle_reproduces_the_old_tables(name):
    assert PO.EPNP_BREAK == frozenset() and PO.EPNP_BREAK_SCOPE == "all"
    assert hashlib.sha256(EC.compared(OLD[name]())).hexdigest()[:16] == DIGESTS["pnp:" + name]


def test_trace_argument_does_not_change_compute_pose():
    sc = PC.scene(5, 12, inlier_ratio=0.5)
    P3, P2 = sc["P3Dw"].astype(np.float64)[None], sc["P2D"].astype(np.float64)[None]
    tr = {}
    a, b = PO.compute_pose(P3, P2, PC.K, detail=True), PO.compute_pose(P3, P2, PC.K, detail=True, trace=tr)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert set(tr) == {"n", "betas1_neg", "betas23_arm", "flip", "det_neg", "qr_kept", "N"} and tr["n"] == 12


def test_sizes(tab):
    for name, (sc, prm, runs) in tab.items():
        assert len(sc["P3Dw"]) <= EC.MAX_POINTS and all(r["out"]["iterations_run"] <= EC.MAX_ITERATIONS for r in runs), name


# ---- (b) the census ----------------------------------------------------------------------------------------------------------------
def _refine(tab, name):
    sc, prm, runs = tab[name]
    return EC.refine_trace(runs), runs[0]


REFINE_CENSUS = [
    ("b1 < 0", "refine_b1_neg", lambda tr: tr["betas1_neg"][0]),
    ("b[0] < 0 at k = 2", "refine_k2_b0_neg", lambda tr: tr["betas23_arm"][2][0] >= 4),
    ("b[0] < 0 at k = 3", "refine_k3_b0_neg", lambda tr: tr["betas23_arm"][3][0] >= 4),
    ("b[0] < 0 at k = 3, another sub-arm", "refine_k3_b0_neg#2", lambda tr: tr["betas23_arm"][3][0] >= 4),
    ("det < 0", "refine_det_neg", lambda tr: any(tr["det_neg"][k][0] for k in (1, 2, 3))),
    ("qr_solve singular", "refine_qr_singular", lambda tr: any(tr["qr_kept"][k][0] for k in (1, 2, 3))),
    ("N = 1", "refine_N1", lambda tr: tr["N"][0] == 1),
    ("N = 2", "refine_N2", lambda tr: tr["N"][0] == 2),
    ("N = 3", "refine_N3", lambda tr: tr["N"][0] == 3),
]


@pytest.mark.parametrize("entry,name,reached", REFINE_CENSUS, ids=[c[0] for c in REFINE_CENSUS])
def test_census_refine_branches(tab, entry, name, reached):
    tr, run = _refine(tab, name)
    assert reached(tr), (entry, tr)
    assert tr["m"] > 4 and tr["n"] == tr["m"]                                   # the cooperative path, not a quad
    o = run["out"]
    assert o["Tcw"] is not None and not o["no_more"] and o["n_inliers"] > 4   # this Refine returns: its Tcw is compared


def test_census_k3_sub_arms_and_solve_for_sign(tab):
    a, b = (int(_refine(tab, n)[0]["betas23_arm"][3][0]) for n in ("refine_k3_b0_neg", "refine_k3_b0_neg#2"))
    assert a != b and a >= 4 and b >= 4
    flips = {(k, bool(_refine(tab, n)[0]["flip"][k][0])) for n in tab if n.startswith("refine_") for k in (1, 2, 3)}
    assert flips == {(k, f) for k in (1, 2, 3) for f in (False, True)}            # solve_for_sign both ways at every k


def test_census_unreached_arms_are_reported(tab, capsys):
    """the arms the search did not reach stay uncovered: named here, and not claimed by any case"""
    seen = set()
    for name, (sc, prm, runs) in tab.items():
        for r in runs:
            for t in r["taps"]:
                if t["refined"] and t["refine"]["m"] > 4:
                    seen |= EC.arms_of(t["refine"])
    assert not seen & set(EC.UNREACHED), seen & set(EC.UNREACHED)   # one that shows up has a case now: take it off the list
    assert all(a.startswith(("k2_arm", "k3_arm")) for a in EC.UNREACHED) and "k2_arm5" in seen
    with capsys.disabled():
        print(f"\n  uncovered on the Refine path (searched: {EC.SEARCH}, then {EC.SEARCH_WIDE}): {', '.join(EC.UNREACHED)}")


@pytest.mark.parametrize("m", EC.REFINE_SIZES)
def test_census_refine_sizes(tab, m):
    sc, prm, runs = tab[f"size_{m}"]
    t, o = runs[0]["taps"][0], runs[0]["out"]
    assert int(sc["truth"].sum()) == m == t["n_inliers"] == t["refine"]["m"] and np.array_equal(runs[0]["best_mask"], sc["truth"])
    if m > 4:
        assert o["Tcw"] is not None and not o["no_more"] and o["n_inliers"] == m == t["refine_inliers"]
    else:   # four points fit both poses and nothing else does: Refine lands on min_inliers and fails, the best goes out at the clamp
        assert prm[0] == 4 == t["refine_inliers"] and o["no_more"] and o["Tcw"].tobytes() == runs[0]["best_Tcw"].tobytes()


def test_census_scan_edges(tab):
    for name, it in (("return_at_63", 63), ("return_at_64", 64), ("return_at_130", 130)):
        sc, prm, (r,) = tab[name]
        assert r["out"]["iterations_run"] == it + 1 and r["out"]["Tcw"] is not None and not r["out"]["no_more"], name
        assert [t["refined"] for t in r["taps"]] == [False] * it + [True], name
    sc, prm, (r,) = tab["two_changes"]
    cnt = [t["n_inliers"] for t in r["taps"]]
    assert [t["refined"] for t in r["taps"]] == [False, True, False, True, False, False] and prm[0] <= cnt[1] < cnt[3]
    assert r["taps"][1]["refine_inliers"] <= prm[0] and r["taps"][3]["refine_inliers"] <= prm[0]   # both Refines fail
    assert r["out"]["no_more"] and r["best_inliers"] == cnt[3] and r["out"]["Tcw"].tobytes() == r["best_Tcw"].tobytes()
    sc, prm, (r,) = tab["best_survives_clamp"]
    assert r["out"]["iterations_run"] == 70 and r["out"]["no_more"] and [i for i, t in enumerate(r["taps"]) if t["refined"]] == [5]
    assert r["out"]["Tcw"].tobytes() == PO.tcw_from(r["taps"][5]["R"], r["taps"][5]["t"]).tobytes()
    sc, prm, (r,) = tab["tie_across_chunks"]
    assert r["taps"][63]["n_inliers"] == r["taps"][64]["n_inliers"] == prm[0] and r["taps"][63]["R"].tobytes() != r["taps"][64]["R"].tobytes()
    assert r["best_Tcw"].tobytes() == PO.tcw_from(r["taps"][63]["R"], r["taps"][63]["t"]).tobytes()
    sc, prm, (r,) = tab["older_across_chunks"]
    assert prm[0] <= r["taps"][65]["n_inliers"] < r["taps"][62]["n_inliers"] == r["best_inliers"]
    assert r["taps"][65]["refine_inliers"] == r["taps"][62]["refine_inliers"] and not np.array_equal(r["taps"][65]["mask"], r["best_mask"])


@pytest.mark.parametrize("name,entered,ran", [("carried_1", 1, 65), ("carried_63", 63, 64)])
def test_census_carried_state(tab, name, entered, ran):
    sc, prm, (a, b) = tab[name]
    assert a["iterations"] == entered and a["out"]["Tcw"] is not None and not a["out"]["no_more"]
    assert b["out"]["iterations_run"] == ran == max(b["n_iterations"], prm[2] - entered) and b["out"]["no_more"]
    assert b["best_inliers"] == a["best_inliers"] and b["out"]["Tcw"].tobytes() == a["best_Tcw"].tobytes()   # the carried best goes out
    assert ran % 64 == (1 if name == "carried_1" else 0)   # the last chunk of 64 hypotheses holds 1, and 64


def test_prepare_inputs_hold_every_edge():
    x, y, octave, idx, pos, usable = EC.prepare_inputs()
    n = len(idx)
    for e in (0, 63, 64, 255, 256, n - 1):
        assert not usable[e] and (idx[e] >= EC.N_MAPPOINTS or octave[e] in (-1, EC.N_LEVELS)), e
    assert {int(idx[e]) for e in (0, 64)} == {EC.N_MAPPOINTS, EC.N_MAPPOINTS + 1}
    assert {int(octave[e]) for e in (63, 255, 256, n - 1)} == {-1, EC.N_LEVELS}
    assert all(usable[e] for e in (1, 62, 65, 254, 257, n - 2)) and 256 < usable.sum() < n


# ---- (c) sensitivity ----------------------------------------------------------------------------------------------------------------
SENSITIVE = {
    ("betas1_sign", "all"): "refine_b1_neg", ("betas1_sign", "refine"): "refine_b1_neg",
    ("betas23_b0", "all"): "refine_k2_b0_neg", ("betas23_b0", "refine"): "refine_k2_b0_neg",
    ("betas23_b2", "all"): "refine_k3_b0_neg", ("betas23_b2", "refine"): "refine_k3_b0_neg",
    ("betas23_b1", "all"): "refine_N2", ("betas23_b1", "refine"): "refine_N2",
    ("solve_for_sign", "all"): "refine_det_neg", ("solve_for_sign", "refine"): "refine_det_neg",
    ("det_neg", "all"): "refine_det_neg", ("det_neg", "refine"): "refine_det_neg",
    ("choose_2", "all"): "refine_N2", ("choose_2", "refine"): "refine_N2",
    ("choose_3", "all"): "refine_N3", ("choose_3", "refine"): "refine_N3",
    ("best_tie_replaces", "all"): "tie_across_chunks", ("refine_current_mask", "all"): "older_across_chunks",
    ("refine_return_ge", "all"): "size_4", ("loop_and", "all"): "two_changes",
}


def test_every_rule_has_a_case():
    assert {r for r, _ in SENSITIVE} == set(PO.EPNP_RULES) | set(PO.SCAN_RULES)
    assert {r for r, s in SENSITIVE if s == "refine"} == set(PO.EPNP_RULES)


@pytest.mark.parametrize("rule,scope", sorted(SENSITIVE))
def test_broken_rule_changes_what_the_gpu_test_compares(tab, rule, scope):
    name = SENSITIVE[(rule, scope)]
    args = EC.inputs()[name]   # the case's inputs come from the unbroken oracle; only the replay runs broken
    broken = EC.with_break(rule, scope, lambda: PC.replay_custom(*args))[2]
    assert PO.EPNP_BREAK == frozenset() and PO.EPNP_BREAK_SCOPE == "all"
    assert EC.compared(broken) != EC.compared(tab[name][2]), (rule, scope)
    if scope == "refine":   # a fault in Refine alone leaves every hypothesis as it was
        for rb, r in zip(broken, tab[name][2]):
            assert all(a["R"].tobytes() == b["R"].tobytes() for a, b in zip(rb["taps"], r["taps"]))


if __name__ == "__main__":   # the before number: the rules the old tables do not notice
    fresh = {**{n: (lambda n=n: PC.replay.__wrapped__(n)[2]) for n in PC.ITERATE_CASES},
             **{"rules_" + w: (lambda w=w: PC.rules_replay.__wrapped__(w)[2]) for w in ("tie", "past5", "again")},
             "older": lambda: PC.older_replay.__wrapped__()[2]}
    base = {n: EC.compared(f()) for n, f in fresh.items()}
    for rule in list(PO.EPNP_RULES) + list(PO.SCAN_RULES):
        for scope in (("all", "refine") if rule in PO.EPNP_RULES else ("all",)):
            hit = None
            for n, f in fresh.items():
                try:
                    changed = EC.compared(EC.with_break(rule, scope, f)) != base[n]
                except AssertionError:   # older_replay's own assertions notice
                    changed = True
                if changed:
                    hit = n
                    break
            print(rule, scope, "noticed by", hit or "NO CASE of the old tables")

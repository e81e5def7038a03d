"""tests/initializer_edge_cases.py holds what it claims, on tests/initializer_oracle.py alone (CPU; tests/test_gpu_initializer_edges.py
runs the same cases through csrc/orbfe_initializer.hip).  Each test fails if a planted condition is absent:

 1. PASSES: n1 covers 256, 257, 512, 513, 1025, 2000 with n2 on both sides of n1; the per-256 histogram of matches12 >= 0 is the
    planted recipe: a middle pass with no match between matched ones, a pass with every key matched, a last pass whose only
    match is the frame's last key (of one key and of 208), a first pass with no match, a pass matched in wave 3 only; N >= 8
    and ok = 1, so P3D shows where first[] put every match.
 2. STAGES: N covers 256, 512, 513, 1000, 4096 (n1 = 4096 there); ok = 1, model H for the planar and F for the general scenes,
    the winner's nGood >= 0.9 N; general and planar at N = 1000.
 3. ITERATIONS: 448, 449, 511, 512; iterF = iterH = iterations - 1, strictly, and SH > SF.
 4. PARALLAX, on the rt tap of the winning hypothesis (stage >= RT_FAR, column cosParallax, sorted) and sel_cos[best]: all
    negative; exactly 51 / 50 negative among >= 60 with index 50 the largest negative / the smallest non-negative; a spread
    beyond [-0.9, 0.99]; one bit pattern at the indices 45 .. 55 and no further; a list of two with maxGood = 2 and ok = 0.
 5. NONFINITE: every score of both models NaN and NO_MODEL; at least one non-finite and one positive finite score per model
    with finite winners.
 6. the batches: 33 pairs of three distinct cases; the two empty pairs; 1 and 512 iterations; two orders of one set.

Then the mutations of csrc/orbfe_initializer.hip that tests/test_gpu_initializer_edges.py is there to catch, each restated here
in numpy beside a restatement of the kernel's own lines (compaction, record stride, selection, winner scan, size gate): the
faithful restatement reproduces the oracle on every case, the mutated one does not on the case named -- and does on every case
of tests/initializer_cases.py's table, which is why the earlier suite cannot see it."""
import numpy as np
import pytest

import initializer_cases as IC
import initializer_edge_cases as E
import initializer_oracle as IO

PASS = E.PASS


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_passes_hold_their_layouts():
    n1s, below, above = [], 0, 0
    for name in E.PASSES:
        c, r = E.case("PASSES", name), E.answer("PASSES", name)
        n1, n2 = len(c["keys1"]), len(c["keys2"])
        n1s.append(n1)
        below += n2 < n1
        above += n2 > n1
        hist, waves = E.pass_histogram(c)
        assert len(hist) == len(c["blocks"]) == (n1 + PASS - 1) // PASS
        for b, what in enumerate(c["blocks"]):
            size = min(n1, (b + 1) * PASS) - b * PASS
            want = {"all": size, "wave3": 64, "last": 1}.get(what, what)
            assert hist[b] == want, (name, b, what)
            if what == "wave3":
                assert waves[b].tolist() == [0, 0, 0, 64]
            if what == "last":
                assert c["matches12"][n1 - 1] >= 0 and b == len(hist) - 1
        assert r["n_matches"] == hist.sum() >= 8 and r["ok"] == 1 and r["P3D"][c["matched"]].all(1).all(), name
        assert (c["matches12"][c["matched"]] != np.arange(len(c["matched"]))).any()
    assert n1s == [256, 257, 512, 513, 1025, 2000] and below >= 2 and above >= 2
    H = {n: E.pass_histogram(E.case("PASSES", n))[0].tolist() for n in E.PASSES}
    assert any(0 < i < len(h) - 1 and h[i] == 0 and any(h[:i]) and any(h[i + 1:]) for h in H.values() for i in range(len(h)))   # (a)
    assert any(PASS in h for h in H.values())                                                                                  # (b)
    assert H["p257_last_key"][-1] == 1 and H["p2000_mixed"][-1] == 1 and 2000 - 7 * PASS == 208                              # (c)
    assert H["p512_first_empty"][0] == 0 and H["p512_first_empty"][1] > 0                                                    # (d)
    assert H["p256_wave3"] == [64]                                                                                            # (e)
    # ... and the earlier table never ran more than two passes or an empty pass (its one-key last pass: planar_257, n1 = N = 257)
    for name in IC.TABLE:
        h = E.pass_histogram(IC.case(name))[0]
        assert len(h) <= 2 and h.all()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def test_stages_hold_their_sizes():
    Ns = []
    for name in E.STAGES:
        c, r = E.case("STAGES", name), E.answer("STAGES", name)
        Ns.append(r["n_matches"])
        assert r["ok"] == 1 and r["model"] == (IO.MODEL_H if name.startswith("planar") else IO.MODEL_F), name
        assert r["nGood"][r["best"]] >= 0.9 * r["n_matches"], name
        assert len(c["keys1"]) <= 4096
    assert sorted(Ns) == [256, 512, 513, 1000, 1000, 4096]
    assert len(E.case("STAGES", "general_4096")["keys1"]) == 4096
    assert {E.answer("STAGES", n)["model"] for n in ("general_1000", "planar_1000")} == {IO.MODEL_H, IO.MODEL_F}


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def test_iterations_end_on_their_winner():
    its = []
    for name in E.ITERATIONS:
        c, r = E.case("ITERATIONS", name), E.answer("ITERATIONS", name)
        n = c["iterations"]
        its.append(n)
        sH, sF = r["tap"]["scoreH"], r["tap"]["scoreF"]
        assert r["iterF"] == r["iterH"] == n - 1, name
        assert (sF[:-1] < sF[-1]).all() and (sH[:-1] < sH[-1]).all() and (sF[:-1] > 0).all() and (sH[:-1] > 0).all(), name
        assert r["SH"] > r["SF"], name
        assert 50 <= r["n_matches"] <= 70
    assert its == [448, 449, 511, 512] and E.MAXIT == 512


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def accepted(name):
    """the winner's vCosParallax, sorted, and the oracle's answer"""
    best = E.answer("PARALLAX", name)["best"]
    r = E.answer("PARALLAX", name, 0, best)
    rt = r["tap"]["rt"]
    return np.sort(rt[rt[:, 4] >= IO.RT_FAR, 3]), r


def test_parallax_cases_select_what_they_name():
    a, r = accepted("all_negative")
    assert len(a) == 120 == r["nGood"][r["best"]] and (a < 0).all() and r["ok"] == 1 and r["model"] == IO.MODEL_F
    assert bits(r["sel_cos"][r["best"]]) == bits(a[50]) and r["sel_cos"][r["best"]] < 0
    a, r = accepted("negatives_51")
    assert len(a) >= 60 and (a < 0).sum() == 51 and a[50] < 0 <= a[51] and bits(r["sel_cos"][r["best"]]) == bits(a[50])
    a, r = accepted("negatives_50")
    assert len(a) >= 60 and (a < 0).sum() == 50 and a[49] < 0 <= a[50] and bits(r["sel_cos"][r["best"]]) == bits(a[50])
    a, r = accepted("spread")
    assert a[0] < -0.9 and a[-1] > 0.99 and bits(r["sel_cos"][r["best"]]) == bits(a[50]) and 0 < a[50] < 0.9
    keys = order_key(a)
    tops = {int(k) >> 23 for k in keys}   # sign and exponent: the earlier table's keys all share these nine bits
    assert len(tops) >= 3 and {t >> 8 for t in tops} == {0, 1}, "the selection's rounds differ from the top bit down"
    a, r = accepted("duplicates")
    assert len(set(bits(a[45:56]).tolist())) == 1 and a[44] < a[45] and a[55] < a[56] and bits(r["sel_cos"][r["best"]]) == bits(a[50])
    a, r = accepted("two_entries")
    assert len(a) == 2 and r["n_matches"] == 8 and max(r["nGood"]) == 2 == r["nGood"][r["best"]] and r["ok"] == 0
    assert bits(r["sel_cos"][r["best"]]) == bits(a[1]) and r["n_cos"][:4].tolist() == [2, 2, 2, 2]
    # the earlier table: every selected cosine in [0.99, 1], so all keys share their top bits
    for name in IC.TABLE:
        r = IC.answer(name)
        assert (r["sel_cos"] >= 0).all()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_cases():
    r = E.answer("NONFINITE", "same_x")
    _, T2 = IO.normalize(E.case("NONFINITE", "same_x")["keys2"])
    assert np.isinf(T2[0, 0])
    assert np.isnan(r["tap"]["scoreH"]).all() and np.isnan(r["tap"]["scoreF"]).all()
    assert (r["model"], r["status"], r["iterH"], r["iterF"], r["ok"]) == (IO.MODEL_NONE, IO.STATUS_NO_MODEL, -1, -1, 0)
    r = E.answer("NONFINITE", "partly_finite")
    c = E.case("NONFINITE", "partly_finite")
    assert np.isfinite(c["keys1"]).all() and (np.abs(c["keys1"][:, 0]) > np.finfo(np.float32).tiny).all()
    for s, win in ((r["tap"]["scoreH"], r["iterH"]), (r["tap"]["scoreF"], r["iterF"])):
        assert (~np.isfinite(s)).any() and (np.isfinite(s) & (s > 0)).any()
        assert win >= 0 and np.isfinite(s[win])
    assert r["status"] == IO.STATUS_OK and r["model"] != IO.MODEL_NONE
    for name in IC.TABLE:   # the earlier table holds no non-finite score
        t = IC.answer(name)["tap"]
        assert np.isfinite(t["scoreH"]).all() and np.isfinite(t["scoreF"]).all()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def test_batches():
    keys = E.batch33()
    assert len(keys) == 33 > E.TAP_SETS and len(set(keys)) == 3
    assert all(2 < E.case(*k)["iterations"] and len(E.case(*k)["keys1"]) < 100 and E.answer(*k)["model"] != 0 for k in set(keys))
    keys = E.empties()
    sizes = [(len(E.case(*k)["keys1"]), len(E.case(*k)["keys2"])) for k in keys]
    assert sizes[1][0] == 0 and sizes[3] == (6, 0) and (E.case(*keys[3])["matches12"] == -1).all()
    assert all(E.answer(*keys[i])["model"] != 0 for i in (0, 2, 4))
    assert [E.case(*k)["iterations"] for k in E.iteration_mix()] == [1, 512, 1, 512]
    first, second = E.reorder()
    assert sorted(first) == sorted(second) and all(a != b for a, b in zip(first, second))
    big = lambda k: (E.case(*k)["iterations"], E.answer(*k)["n_matches"])   # noqa: E731
    assert big(first[0])[0] == 512 > big(second[0])[0] and big(first[1])[1] == 1000 > big(second[1])[1]


# ---- the kernel's lines, restated, and their mutations ----------------------------------------------------------------------------------
def compact(matches12, lose_base_after_empty=False):
    """k_init_prepare's loop over passes of 256 keys -> first[]"""
    m = np.asarray(matches12)
    first = np.full(len(m), -1, np.int64)
    base = 0
    for i0 in range(0, len(m), PASS):
        keep = np.nonzero(m[i0:i0 + PASS] >= 0)[0]
        first[base + np.arange(len(keep))] = i0 + keep
        total = len(keep)
        base = 0 if (lose_base_after_empty and total == 0) else base + total
    return first[:int((m >= 0).sum())]


def test_mutation_base_lost_after_an_empty_pass():
    for name in E.PASSES:
        c, r = E.case("PASSES", name), E.answer("PASSES", name)
        assert np.array_equal(compact(c["matches12"]), r["idx1"]), name
    seen = [n for n in E.PASSES if not np.array_equal(compact(E.case("PASSES", n)["matches12"], True), E.answer("PASSES", n)["idx1"])]
    assert "p1025_middle_empty" in seen and "p2000_mixed" in seen
    for name in IC.TABLE:
        assert np.array_equal(compact(IC.case(name)["matches12"], True), IC.answer(name)["idx1"]), name


def order_key(f, negative_branch_returns_b=False):
    b = bits(f).astype(np.uint64)
    neg = (b & 0x80000000) != 0
    return np.where(neg, b if negative_branch_returns_b else (~b & 0xFFFFFFFF), b | 0x80000000).astype(np.uint32)


def radix_select(cos, inverse_keeps_prefix=False, negative_branch_returns_b=False):
    """k_init_reconstruct's selection of vCosParallax[min(50, size - 1)] -> the float"""
    keys = order_key(np.asarray(cos, np.float32), negative_branch_returns_b).astype(np.uint64)
    k = min(50, len(keys) - 1)
    prefix = 0
    for bit in range(31, -1, -1):
        high = 0 if bit == 31 else (0xFFFFFFFF << (bit + 1)) & 0xFFFFFFFF
        zeros = int((((keys & high) == prefix) & ((keys >> bit) & 1 == 0)).sum())
        if k >= zeros:
            k -= zeros
            prefix |= 1 << bit
    if prefix & 0x80000000:
        out = prefix & 0x7FFFFFFF
    else:
        out = prefix if inverse_keeps_prefix else (~prefix & 0xFFFFFFFF)
    return np.array([out], np.uint32).view(np.float32)[0]


def test_mutations_of_the_selection():
    caught_inverse, caught_key = [], []
    for name in E.PARALLAX:
        a, r = accepted(name)
        want = bits(r["sel_cos"][r["best"]])
        assert bits(radix_select(a)) == want, name
        if bits(radix_select(a, inverse_keeps_prefix=True)) != want:
            caught_inverse.append(name)
        if bits(radix_select(a, negative_branch_returns_b=True)) != want:
            caught_key.append(name)
    assert set(caught_inverse) >= {"all_negative", "negatives_51"}
    assert set(caught_key) >= {"all_negative", "negatives_51", "negatives_50", "spread", "duplicates"}
    for name in ("general_65", "planar_257", "sized_51", "noisy_general_200"):   # no negative cosine: neither shows
        r0 = IC.answer(name)
        r = IC.answer(name, 0, r0["best"])
        rt = r["tap"]["rt"]
        a = rt[rt[:, 4] >= IO.RT_FAR, 3]
        for kw in (dict(inverse_keeps_prefix=True), dict(negative_branch_returns_b=True)):
            assert bits(radix_select(a, **kw)) == bits(r["sel_cos"][r["best"]])


def scan(scores, mutated=False):
    """k_init_reconstruct's winner scan; mutated: `!(s <= score)` for `s > score`"""
    best, score = -1, np.float32(0)
    for it, s in enumerate(scores):
        if (not (s <= score)) if mutated else (s > score):
            best, score = it, s
    return best, score


def test_mutation_of_the_winner_scan():
    for name in E.NONFINITE:
        r = E.answer("NONFINITE", name)
        for s, win in ((r["tap"]["scoreH"], r["iterH"]), (r["tap"]["scoreF"], r["iterF"])):
            assert scan(s)[0] == win
            assert scan(s, True)[0] != win, name
    for name in IC.TABLE:
        r = IC.answer(name)
        assert scan(r["tap"]["scoreF"], True)[0] == r["iterF"] and scan(r["tap"]["scoreH"], True)[0] == r["iterH"]


def strided_winners(sH, sF, stride, h_writes_last):
    """the two winner scans over a record array whose (model, iteration) rows lie `stride` apart instead of 512: model H's rows
    from `stride` on are model F's first ones; which of the two workgroups writes last is not defined"""
    n = len(sH)
    rows = np.zeros(max(2 * stride, stride + n) + n, np.float32)
    for model, s in ((1, sF), (0, sH)) if h_writes_last else ((0, sH), (1, sF)):
        rows[model * stride + np.arange(n)] = s
    return scan(rows[:n]), scan(rows[stride:stride + n])


@pytest.mark.parametrize("stride", [200, 256, 448, 511])
def test_mutation_of_the_record_stride(stride):
    caught = 0
    for name in E.ITERATIONS:
        r = E.answer("ITERATIONS", name)
        sH, sF = r["tap"]["scoreH"], r["tap"]["scoreF"]
        assert strided_winners(sH, sF, 512, True) == ((r["iterH"], r["SH"]), (r["iterF"], r["SF"]))
        if len(sH) > stride:   # either writing order changes a winner or its score
            for last in (True, False):
                assert strided_winners(sH, sF, stride, last) != ((r["iterH"], r["SH"]), (r["iterF"], r["SF"])), (name, last)
            caught += 1
    assert caught >= 1
    for name in IC.TABLE:   # at most 200 iterations: no row of one model reaches the other's
        r = IC.answer(name)
        sH, sF = r["tap"]["scoreH"], r["tap"]["scoreF"]
        assert strided_winners(sH, sF, stride, True) == strided_winners(sH, sF, 512, True)


def test_mutation_of_the_size_gate_and_of_tapped():
    keys = E.exact_fit()
    n = [len(E.case(*k)["keys1"]) for k in keys]
    o1, total = int(np.sum(n[:-1])), int(np.sum(n))
    assert not (o1 + n[-1] > total) and (o1 + n[-1] >= total) and (o1 + n[-1] > total - 1)   # `>` runs the pair, `>=` refuses it
    # tests/test_gpu_initializer.py's batch overshoots by ten keys: both comparisons refuse it
    npairs, tap_cap = len(E.batch33()), E.TAP_SETS
    assert [p < min(npairs, tap_cap) for p in (31, 32)] == [True, False] and [p < npairs for p in (31, 32)] == [True, True]

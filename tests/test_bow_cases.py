"""The case builders of tests/bow_cases.py, and the CPU oracle's BoW transform / distinctive descriptors on what they build.
CPU only.

Every planted distance is checked by np.unpackbits counts; the inputs are checked to have the properties the GPU tests
rely on to be SENSITIVE (a sum that depends on its order, a norm that depends on its order: conditions on the inputs, not
measurements of any kernel); the oracle is checked against the Python twins of tests/test_bow.py and
tests/test_distinctive.py on every case that tests/test_gpu_bow_edges.py feeds to the HIP kernels, against the answers the
plantings were made for, and -- where it is built -- against the compiled DBoW2-shaped class on the regular trees."""
import os

import numpy as np
import pytest

import bow_cases as B
from oracle import ref_ffi as R
from test_bow import twin as bow_twin
from test_distinctive import twin as distinctive_twin

_ORACLE = {}


def oracle_transform(oracle, name):
    """the oracle's answer for a transform case, computed once"""
    if name not in _ORACLE:
        c = B.TRANSFORM_CASES[name]
        _ORACLE[name] = oracle.bow_transform(c["voc"], c["desc"], c["levelsup"])
    return _ORACLE[name]


def unpack_dist(a, b):
    return int(np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)).sum())


def u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ builders
def test_case_tables_hold_what_the_gpu_tests_ask_for():
    names = set(B.TRANSFORM_CASES)
    assert {f"widths[{n}]" for n in B.WIDTHS} <= names and B.WIDTHS[-1] == B.BOW_MAX_FEATURES
    assert {"one_word", "three_words", "all_distinct", "shared_order", "ties[tied]", "ties[planted]"} <= names
    assert {f"zero_{k}[{n}]" for k in ("all", "half", "ends") for n in (1024, 1025)} <= names
    assert {f"levels[{s}]" for s in (0, 1, 3, 4, 6)} <= names and {f"ragged[{s}]" for s in (0, 1, 2, 4)} <= names
    for c in B.TRANSFORM_CASES.values():
        assert c["doc"] and c["desc"].dtype == np.uint8 and c["desc"].shape == (len(c["desc"]), 32)
        assert len(c["desc"]) <= B.BOW_MAX_FEATURES
    assert set(B.DISTINCTIVE_CASES) == {"sizes", "cluster_edge", "cross_pass_ties", "equilateral", "extremes"}
    for c in B.DISTINCTIVE_CASES.values():
        assert c["doc"] and int(c["off"][-1]) == len(c["idx"]) and (c["idx"] < len(c["pool"])).all()
        assert np.diff(c["off"].astype(np.int64)).max() <= B.DD_MAX_OBS
    assert [len(B.TRANSFORM_CASES[f"widths[{n}]"]["desc"]) for n in B.WIDTHS] == list(B.WIDTHS)
    for n in (1024, 1025):
        assert len(B.TRANSFORM_CASES[f"zero_all[{n}]"]["desc"]) == n


def test_ragged_tree_shape():
    voc = B.ragged(0)
    co, ci = voc["child_off"], voc["child_idx"]
    lev, leaves = B.levels_of(voc), B.leaves_of(voc)
    assert voc["L"] == 4 and sorted(set(lev[leaves])) == [1, 2, 3, 4]          # leaves at every level
    nch = np.diff(co.astype(np.int64))
    assert (nch == 1).sum() >= 1 and lev[leaves].min() == 1                      # a single child, a level-1 leaf
    root_children = ci[co[0]:co[1]]
    assert any(nch[c] == 0 for c in root_children)
    for p in range(len(nch)):                                                    # ids in creation order
        assert (ci[co[p]:co[p + 1]] > p).all()
    assert np.array_equal(np.sort(ci), np.arange(1, len(nch)))                   # every node but the root has one parent
    assert np.array_equal(voc["word_id"][leaves], np.arange(len(leaves)))
    for p in range(1, len(nch)):
        for c in ci[co[p]:co[p + 1]]:
            assert unpack_dist(voc["node_desc"][p], voc["node_desc"][c]) == 20
    assert (voc["weight"][leaves] == 0).any() and (voc["weight"][leaves] > 0).sum() > len(leaves) // 2


def test_ragged_queries_reach_leaves_of_every_depth(oracle):
    c = B.TRANSFORM_CASES["ragged[0]"]
    voc, t = c["voc"], c["target"]
    leaf, path = B.descend(voc, c["desc"])
    planted = t >= 0
    assert planted.sum() == 250 and np.array_equal(leaf[planted], t[planted])    # a planted query ends on its leaf
    assert set(leaf[planted]) == set(B.leaves_of(voc))
    r = oracle_transform(oracle, "ragged[0]")
    kept = r["word"] >= 0
    lev = B.levels_of(voc)
    deep = kept & (lev[leaf] == 4)
    assert deep.any() and np.array_equal(r["node"][deep], leaf[deep])            # levelsup 0: the node is a level-4 leaf itself
    for ls in (0, 1, 2, 4):                                                       # node at level L - levelsup, 0 if the leaf is above
        rr = oracle_transform(oracle, f"ragged[{ls}]")
        want = np.where(lev[leaf] >= 4 - ls, path[:, 4 - ls], 0)
        assert np.array_equal(rr["node"][kept], want[kept])
        if ls < 4:
            assert (lev[leaf][kept] < 4 - ls).any() and (rr["node"][kept] == 0).any()   # the unset-nid rule is exercised


def test_tied_and_planted_descents(oracle):
    voc = B.tied(5, 3)
    co, ci = voc["child_off"], voc["child_idx"]
    for p in range(len(co) - 1):
        ch = ci[co[p]:co[p + 1]]
        assert all(unpack_dist(voc["node_desc"][ch[0]], voc["node_desc"][x]) == 0 for x in ch)
    r = oracle_transform(oracle, "ties[tied]")
    first_leaf = int(ci[co[ci[co[ci[co[0]]]]]])                                  # first child, three times
    assert set(r["word"]) == {int(voc["word_id"][first_leaf])} and set(r["node"]) == {int(ci[co[ci[co[0]]]])}
    voc, desc, expect = B.planted_ties()
    co, ci, nd = voc["child_off"], voc["child_idx"], voc["node_desc"]
    for j, pair in enumerate([(0, 1), (2, 3), (4, 5), (0, 5)]):
        p = int(ci[co[0] + j])
        d = [unpack_dist(desc[j], nd[x]) for x in ci[co[p]:co[p + 1]]]
        assert unpack_dist(desc[j], nd[p]) == 10 and d[pair[0]] == d[pair[1]] == 30
        assert min(d[i] for i in range(6) if i not in pair) > 30
    p4, p5 = int(ci[co[0] + 4]), int(ci[co[0] + 5])
    assert unpack_dist(desc[4], nd[ci[co[p4] + 2]]) == 0 and unpack_dist(desc[5], nd[ci[co[p5]]]) == 256
    r = oracle_transform(oracle, "ties[planted]")
    assert np.array_equal(r["node"][:6], expect)                                 # the first of the two tied siblings


def test_flat_cases(oracle):
    c = B.TRANSFORM_CASES["all_distinct"]
    r = oracle_transform(oracle, "all_distinct")
    assert len(c["desc"]) == 2048 and np.array_equal(r["word"], np.arange(2047, -1, -1))   # feature i = leaf 2047 - i
    assert len(r["bow_id"]) == len(r["fv_node"]) == 2048 and np.array_equal(r["fv_idx"], np.arange(2047, -1, -1))
    r = oracle_transform(oracle, "one_word")
    assert r["bow_id"].tolist() == [0] and r["bow_val"].tolist() == [1.0] and np.diff(r["fv_off"]).tolist() == [8192]
    r = oracle_transform(oracle, "three_words")
    runs = np.bincount(r["word"], minlength=3)
    assert runs.sum() == 8192 and runs.min() > 2048                              # every run spans hundreds of 8-key chunks
    voc = B.shared_words()
    leaves = B.leaves_of(voc)
    w, wid = voc["weight"][leaves], voc["word_id"][leaves]
    assert len(set(wid)) < len(wid) and (np.diff(wid.astype(np.int64)) < 0).any() and w.min() <= 1e-3 and w.max() >= 1e3
    r = oracle_transform(oracle, "shared_order")
    assert r["bow_id"].tolist() == sorted(set(wid.tolist()))


def test_zero_weight_cases(oracle):
    for n in (1024, 1025):
        r = oracle_transform(oracle, f"zero_all[{n}]")
        assert (r["word"] == -1).all() and (r["node"] == -1).all() and (r["weight"] == 0).all()
        assert len(r["bow_id"]) == len(r["fv_node"]) == len(r["fv_idx"]) == 0 and r["fv_off"].tolist() == [0]
        r = oracle_transform(oracle, f"zero_half[{n}]")
        assert 0.3 * n < (r["word"] < 0).sum() < 0.7 * n
        r = oracle_transform(oracle, f"zero_ends[{n}]")
        assert (r["word"][:5] < 0).all() and (r["word"][-5:] < 0).all() and (r["word"] >= 0).sum() > n // 2


def test_levels_cases(oracle):
    voc = B.TRANSFORM_CASES["levels[0]"]["voc"]
    leaf, path = B.descend(voc, B.TRANSFORM_CASES["levels[0]"]["desc"])
    for ls, lev in ((0, 4), (1, 3), (3, 1), (4, 0), (6, 0)):
        r = oracle_transform(oracle, f"levels[{ls}]")
        kept = r["word"] >= 0
        assert np.array_equal(r["node"][kept], path[kept, lev]) and kept.sum() > 300


# ------------------------------------------------------------------------------------------------ sensitivity preconditions
def _word_weights(r):
    """{word: weights of its features in feature order}"""
    out = {}
    for w, x in zip(r["word"], r["weight"]):
        if w >= 0:
            out.setdefault(int(w), []).append(float(x))
    return out


def _seq(xs):
    v = 0.0
    for x in xs:
        v += x
    return v


def test_three_words_sum_is_not_count_times_weight(oracle):
    ww = _word_weights(oracle_transform(oracle, "three_words"))
    assert any(u64(_seq(xs)) != u64(len(xs) * xs[0]) for xs in ww.values())


def test_shared_order_sum_depends_on_direction(oracle):
    ww = _word_weights(oracle_transform(oracle, "shared_order"))
    assert any(u64(_seq(xs)) != u64(_seq(xs[::-1])) for xs in ww.values())


def test_widths_norm_depends_on_word_order(oracle):
    r = oracle_transform(oracle, "widths[8192]")
    sums = {w: _seq(xs) for w, xs in _word_weights(r).items()}
    first = list(dict.fromkeys(int(w) for w in r["word"] if w >= 0))              # order of first appearance
    assert u64(_seq(sums[w] for w in sorted(sums))) != u64(_seq(sums[w] for w in first))
    # ... and some width's norm differs between ascending and DESCENDING word order (a norm taken backwards would show)
    r = oracle_transform(oracle, "widths[4096]")
    sums = {w: _seq(xs) for w, xs in _word_weights(r).items()}
    assert u64(_seq(sums[w] for w in sorted(sums))) != u64(_seq(sums[w] for w in sorted(sums, reverse=True)))


# ------------------------------------------------------------------------------------------------ oracle against the twins
@pytest.mark.parametrize("name", list(B.TRANSFORM_CASES))
def test_oracle_transform_equals_the_python_twin(oracle, name):
    c = B.TRANSFORM_CASES[name]
    r = oracle_transform(oracle, name)
    ids, vals, fv = bow_twin(c["voc"], c["desc"], c["levelsup"])
    assert r["bow_id"].tolist() == ids
    assert r["bow_val"].tolist() == vals                                         # doubles, same summation order
    assert r["fv_node"].tolist() == sorted(fv)
    for j, nd in enumerate(r["fv_node"]):
        assert r["fv_idx"][r["fv_off"][j]:r["fv_off"][j + 1]].tolist() == fv[int(nd)]
    leaf = B.descend(c["voc"], c["desc"])[0]
    kept = c["voc"]["weight"][leaf] > 0
    assert np.array_equal(r["word"], np.where(kept, c["voc"]["word_id"][leaf].astype(np.int64), -1))
    assert np.array_equal(u64(r["weight"]), u64(np.where(kept, c["voc"]["weight"][leaf], 0.0)))
    assert np.array_equal(r["node"] >= 0, kept)


@pytest.mark.parametrize("name", list(B.DISTINCTIVE_CASES))
def test_oracle_distinctive_equals_the_numpy_twin(oracle, name):
    c = B.DISTINCTIVE_CASES[name]
    b, m = oracle.distinctive(c["pool"], c["off"], c["idx"])
    tb, tm = distinctive_twin(c["pool"], c["off"], c["idx"])
    assert np.array_equal(b, tb) and np.array_equal(m, tm)
    if c["expect"] is not None:
        assert np.array_equal(b, c["expect"][0]) and np.array_equal(m, c["expect"][1])


def test_distinctive_plantings():
    c = B.DISTINCTIVE_CASES["sizes"]
    n = np.diff(c["off"].astype(np.int64))
    assert n.tolist() == list(B.SIZES) and n[0] == n[-1] == n[len(n) // 2 + 1] == 0 and n.max() == B.DD_MAX_OBS
    c = B.DISTINCTIVE_CASES["equilateral"]
    rows = c["pool"][c["idx"]].reshape(-1, 3, 32)
    for t, d in zip(rows, B.EQUILATERAL_D):
        assert [unpack_dist(t[0], t[1]), unpack_dist(t[0], t[2]), unpack_dist(t[1], t[2])] == [d, d, d]
    for t, d in zip(rows[len(B.EQUILATERAL_D):], B.ISOSCELES_D):
        assert [unpack_dist(t[0], t[1]), unpack_dist(t[0], t[2]), unpack_dist(t[1], t[2])] == [d, d, d + 1]
    assert {128} < set(B.EQUILATERAL_D) and min(B.ISOSCELES_D) < 128 < max(B.ISOSCELES_D)
    c = B.DISTINCTIVE_CASES["cross_pass_ties"]
    rows = c["pool"][c["idx"]].reshape(3, 200, 32)
    for p, better in enumerate((None, 64, 199)):
        s = rows[p, 3]
        assert unpack_dist(s, rows[p, 67]) == 0 and unpack_dist(s, rows[p, 131]) == 0
        d = np.array([unpack_dist(s, x) for x in rows[p]])
        want = 10 if better is None else 11
        assert np.sort(d)[99] == want and np.sort(d)[98] <= want < np.sort(d)[100]
        if better is not None:
            assert unpack_dist(s, rows[p, better]) == 1
    c = B.DISTINCTIVE_CASES["cluster_edge"]
    n = np.diff(c["off"].astype(np.int64))
    assert n.tolist() == [10, 10, 11, 11, 64, 64, 65, 65]
    c = B.DISTINCTIVE_CASES["extremes"]
    rows = c["pool"][c["idx"]]
    o = c["off"]
    assert unpack_dist(rows[o[2]], rows[o[2] + 1]) == 256 and unpack_dist(rows[o[3] + 1], rows[o[3] + 2]) == 0
    assert len(set(c["idx"][o[4]:o[5]].tolist())) == 1 and o[5] - o[4] == 3


def test_empty_vocabulary_gives_the_empty_result(oracle):
    """a root without children is DBoW2's empty(): every feature without a word, both vectors empty"""
    voc = dict(child_off=np.zeros(2, np.uint32), child_idx=np.zeros(0, np.uint32), node_desc=np.zeros((1, 32), np.uint8),
               word_id=np.zeros(1, np.uint32), weight=np.ones(1), L=3)
    for n in (0, 1, 300):
        r = oracle.bow_transform(voc, B.random_rows(np.random.default_rng(n), n), 1)
        assert (r["word"] == -1).all() and (r["node"] == -1).all() and (r["weight"] == 0).all() and len(r["word"]) == n
        assert len(r["bow_id"]) == len(r["bow_val"]) == len(r["fv_node"]) == len(r["fv_idx"]) == 0 and r["fv_off"].tolist() == [0]


# ------------------------------------------------------------------------------------------------ compiled DBoW2-shaped twin
@pytest.mark.skipif(not R.twin_available(), reason="the compiled DBoW2-shaped twin is not built")
def test_oracle_equals_the_compiled_twin_on_the_regular_trees(oracle, tmp_path):
    """Trees of full depth only: where a leaf is reached above level L - levelsup DBoW2 leaves `nid` unset, so the ragged
    cases are not put to it (and its text loader holds k <= 20 and word ids in leaf order only)."""
    from test_formats import _write_voc_text
    files = {}
    for name, c in B.TRANSFORM_CASES.items():
        if not c["regular"]:
            continue
        voc = c["voc"]
        if id(voc) not in files:
            k = int(np.diff(voc["child_off"].astype(np.int64)).max())
            path = os.path.join(tmp_path, f"voc{len(files)}.txt")
            _write_voc_text(path, voc, k, voc["L"])
            files[id(voc)] = R.TwinVocabulary(path)
        t = files[id(voc)].transform(c["desc"], c["levelsup"])
        r = oracle_transform(oracle, name)
        for key in ("bow_id", "fv_node", "fv_off", "fv_idx"):
            assert np.array_equal(t[key], r[key]), (name, key)
        assert np.array_equal(u64(t["bow_val"]), u64(r["bow_val"])), name
    assert len(files) >= 4


# ------------------------------------------------------------------------------------------------ argument checks
def test_vocabulary_word_id_limit_cpu():
    """f_word is int32 with -1 for "no word": a leaf's word id of 2^31 or more is refused, before any device is looked for"""
    from orb_slam2_ssd_semantic_amd import _ffi
    import ctypes as C
    L = _ffi.lib()
    voc = B.flat(3)
    for bad in (1 << 31, (1 << 32) - 1):
        wid = voc["word_id"].copy()
        wid[2] = bad
        out = C.c_void_p()
        st = L.orbfe_vocabulary_create(0, len(wid), _ffi.ptr(voc["child_off"]), _ffi.ptr(voc["child_idx"]), _ffi.ptr(voc["node_desc"]),
                                       _ffi.ptr(wid), _ffi.ptr(voc["weight"]), 1, C.byref(out))
        assert st == _ffi.ORBFE_ERR_ARG and not out.value
        assert "word id" in _ffi.last_error()

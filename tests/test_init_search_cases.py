"""The oracle and the planted cases of the device-resident SearchForInitialization, on the CPU: tests/init_search_oracle.py equals
the compiled reference body (src/ORBmatcher.cc:523-651) and orbfe_initialization_resolve; every planted case of
tests/init_search_cases.py sits on the edge it claims; the relaxation model (what csrc/orbfe_init_search.hip runs) equals the
sequential rule, and its two one-word-per-feature variants do not."""
import ctypes as C
import functools

import numpy as np
import pytest

import init_search_cases as IC
import init_search_oracle as IO
from oracle import ref_ffi as R

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built and the reference sources are absent")


@functools.lru_cache(maxsize=None)
def planted(name):
    return IC.PLANTED[name]()


def same(a, b):
    return a[2] == b[2] and np.array_equal(a[0], b[0]) and np.asarray(a[1], np.float32).tobytes() == np.asarray(b[1], np.float32).tobytes()


def all_cases():
    for name in IC.PLANTED:
        yield name, planted(name)
    for i in range(len(IC.CONTENDED)):
        yield "contended_%d" % i, IC.contended_case(i)
    for name, c in IC.batch_edges().items():
        yield "edge_" + name, c


@needs_ref
def test_oracle_equals_the_reference_on_every_table():
    for name, c in all_cases():
        for ori in (c["check_ori"], not c["check_ori"]):
            o = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=ori)
            r = R.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], 0.9, ori)
            assert same(o, r), (name, ori, o[2], r[2])


@needs_ref
def test_oracle_equals_the_reference_on_random_frames():
    total = 0
    for seed in range(60):
        c = IC.random_case(seed)
        o = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=c["check_ori"])
        r = R.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], 0.9, c["check_ori"])
        assert same(o, r), (seed, o[2], r[2])
        o2 = IO.search_for_initialization(c["f1"], c["f2"], o[1], c["window"], check_ori=c["check_ori"])
        r2 = R.search_for_initialization(c["f1"], c["f2"], r[1], c["window"], 0.9, c["check_ori"])
        assert same(o2, r2), (seed, "second call")
        total += o[2]
    assert total > 1000


def test_oracle_equals_initialization_resolve_on_the_lists():
    """the host rule the shim runs today (csrc/orbfe_hostgeom.hip) and the oracle's loop accept the same features"""
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    for name, c in all_cases():
        qsrc, lists = IO.candidate_lists(c["f1"], c["f2"], c["prev"], c["window"])
        off, ent = IO.entries(lists)
        nq, n2 = len(lists), len(c["f2"]["octave"])
        acc, hold = np.full(max(nq, 1), -9, np.int32), np.full(max(n2, 1), -9, np.int32)
        assert L.orbfe_initialization_resolve(_ffi.ptr(off), _ffi.ptr(ent if len(ent) else np.zeros(1, np.uint32)), nq, n2, 50, C.c_float(0.9),
                                              _ffi.ptr(acc), _ffi.ptr(hold)) == 0
        d = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False, details=True)[3]
        assert np.array_equal(acc[:nq], d["accepted"]), name
        m = np.full(len(c["f1"]["octave"]), -1, np.int32)
        for j in range(n2):
            if hold[j] >= 0:
                m[qsrc[hold[j]]] = j
        assert np.array_equal(m, IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False)[0]), name


@pytest.mark.parametrize("name", list(IC.PLANTED))
def test_planted_case_is_what_it_claims(name):
    c = planted(name)
    m, prev, nm, d = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=c["check_ori"], details=True)
    e = c["expect"]
    assert list(m) == list(e["matches12"]) and nm == e["nmatches"] and d["takeovers"] == e["takeovers"], (name, list(m), nm, d["takeovers"])
    st = m >= 0
    assert np.array_equal(prev[st], c["f2"]["xy"][m[st]]) and np.array_equal(prev[~st], c["prev"][~st])


def test_planted_distances_are_exact():
    c = planted("skip_20_12_15")
    _, lists = IO.candidate_lists(c["f1"], c["f2"], c["prev"], c["window"])
    assert [sorted(d.tolist()) for _, d in lists] == [[20], [12], [15, 16]]
    c = planted("takeover_20_15_10")
    _, lists = IO.candidate_lists(c["f1"], c["f2"], c["prev"], c["window"])
    assert [sorted(d.tolist()) for _, d in lists] == [[20], [15, 30], [10]]
    c = planted("chain_40")
    _, lists = IO.candidate_lists(c["f1"], c["f2"], c["prev"], c["window"])
    assert sorted(lists[0][1].tolist()) == [10] and all(sorted(d.tolist()) == [10, 11] for _, d in lists[1:])


def test_skip_changes_the_third_query():
    """skip_20_12_15 without the skip of :566: query 2 would meet A at 15 and B at 16 and fail the ratio"""
    c = planted("skip_20_12_15")
    _, lists = IO.candidate_lists(c["f1"], c["f2"], c["prev"], c["window"])
    d = sorted(lists[2][1].tolist())
    assert not IO._accepts(d[0], d[1], 50, 0.9) and IO._accepts(d[1], IO.INT_MAX, 50, 0.9)


@pytest.mark.parametrize("L", [40, 70])
def test_chain_flips_entirely_without_query0(L):
    a, b = planted("chain_%d" % L), planted("chain_%d_without_query0" % L)
    ma = IO.search_for_initialization(a["f1"], a["f2"], a["prev"], a["window"], check_ori=False)
    mb = IO.search_for_initialization(b["f1"], b["f2"], b["prev"], b["window"], check_ori=False)
    assert ma[2] == L and (ma[0] >= 0).all() and mb[2] == 0 and (mb[0] < 0).all()
    assert np.array_equal(a["f1"]["desc"][1:], b["f1"]["desc"][1:]) and np.array_equal(a["f2"]["desc"], b["f2"]["desc"])
    ra, rb = IO.model(a["f1"], a["f2"], a["prev"], a["window"], check_ori=False), IO.model(b["f1"], b["f2"], b["prev"], b["window"], check_ori=False)
    assert same(ra[:3], ma) and same(rb[:3], mb)
    assert ra[3] >= L + 1 and ra[3] == a["expect"]["min_rounds"] and rb[3] == 1
    assert L <= 64 or ra[3] > 64   # the longer chain crosses the 64 query groups of the resolve workgroup


def test_relaxation_model_equals_the_sequential_rule():
    n = 0
    for name, c in all_cases():
        o = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=c["check_ori"])
        r = IO.model(c["f1"], c["f2"], c["prev"], c["window"], check_ori=c["check_ori"])
        assert same(r[:3], o), name
        n += 1
    for seed in (0, 3, 4, 11, 17, 23):
        c = IC.random_case(seed)
        o = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=c["check_ori"])
        assert same(IO.model(c["f1"], c["f2"], c["prev"], c["window"], check_ori=c["check_ori"])[:3], o), seed
    assert n >= 20


def test_one_word_tables_fail_on_the_three_query_patterns():
    """the smallest claimed distance per feature is wrong on (20, 15, 10), the lowest claiming query on (20, 12, 15); each is
    right on the other pattern, so both patterns are needed"""
    t, s = planted("takeover_20_15_10"), planted("skip_20_12_15")
    for c, wrong, right in ((t, "min_distance", "lowest_query"), (s, "lowest_query", "min_distance")):
        o = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False)
        assert not np.array_equal(IO.model(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False, table=wrong)[0], o[0])
        assert np.array_equal(IO.model(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False, table=right)[0], o[0])


def test_contended_frames_take_matches_over():
    for i in range(len(IC.CONTENDED)):
        c = IC.contended_case(i)
        m, _, nm, d = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False, details=True)
        acc = int((d["accepted"] >= 0).sum())
        assert d["takeovers"] > 0 and acc - d["takeovers"] == nm and d["skipped"] > 0, (i, acc, nm, d["takeovers"], d["skipped"])
        # the skip decides: a query alone against its list (no claims) would accept another feature, or none
        _, lists = IO.candidate_lists(c["f1"], c["f2"], c["prev"], c["window"])
        alone = np.array([_first(cc, dd) for cc, dd in lists])
        assert (alone != d["accepted"]).sum() > 0, i


def _first(cand, dd):
    if len(cand) == 0:
        return -1
    o = np.argsort(dd, kind="stable")
    best, second = int(dd[o[0]]), int(dd[o[1]]) if len(o) > 1 else IO.INT_MAX
    return int(cand[o[0]]) if IO._accepts(best, second, 50, 0.9) else -1


def test_random_cases_never_take_over():
    """why the planted cases exist: on the random generator of the existing tests no match is taken over"""
    for seed in (0, 1, 2, 3, 4, 5, 6, 7):
        c = IC.random_case(seed)
        d = IO.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False, details=True)[3]
        assert d["takeovers"] == 0, seed


def test_scratch_bytes_needs_no_device():
    from orb_slam2_ssd_semantic_amd import tracking
    a, b = tracking.init_search_scratch_bytes(16, 2000, 1 << 22), tracking.scratch_bytes(16, 2000, 1 << 22)
    assert a > b and tracking.init_search_scratch_bytes(1, 1, 0) > 0
    for bad in ((1, 15361, 0), (1 << 13, 1 << 12, 0), (1, 0, 0), (-1, 8, 0), (1, 8, 1 << 33)):
        with pytest.raises(ValueError):
            tracking.init_search_scratch_bytes(*bad)

"""csrc/orbfe_initializer.hip at its pass, stage, iteration, selection and batch edges, bit for bit against
tests/initializer_oracle.py.  The cases come from tests/initializer_edge_cases.py (tests/test_initializer_edge_cases.py shows on
the CPU that every case sits on the edge it names); the comparison helpers are those of tests/test_gpu_initializer.py:

  1. PASSES      k_init_prepare's 256-key compaction passes: empty, full, wave 3 only, the frame's last key alone
  2. STAGES      N = 256 .. 4096 matches over the 256-match LDS stages of k_init_ransac and the strides of k_init_reconstruct
  3. ITERATIONS  448 .. 512 iterations, both winners in the last one, every tap record
  4. PARALLAX    the radix selection on negative, mixed, widely spread and duplicated cosines and on a list of two
  5. NONFINITE   every score NaN, and NaN scores among finite ones
  6. the batch form: a pair past the taps, empty pairs, the exact max_matches boundary, 1 and 512 iterations, two orders

No tolerance.  `parallax` (the device's acosf) stays out of the comparison as in tests/test_gpu_initializer.py; in group 5 alone a
NaN in a tap compares by position (its payload is the processor's, as tests/test_gpu_pnp.py argues), finite tap values and every
result field as bits."""
import numpy as np
import pytest

import initializer_edge_cases as E
from orb_slam2_ssd_semantic_amd import InitializerHandle, OrbfeError, _ffi
from orb_slam2_ssd_semantic_amd import initializer as IN
from test_gpu_initializer import FIELDS, assert_result, bits, same   # noqa: F401  (FIELDS: what assert_result compares)

pytestmark = pytest.mark.gpu

TAP_FIELDS = ("Hn", "Fn", "H21i", "F21i", "scoreH", "scoreF")
SENT_F, SENT_B = np.float32(-7.25e11), np.uint8(0xA5)


@pytest.fixture(scope="module")
def handle():
    with InitializerHandle(4096, 33) as h:   # exactly the largest case: general_4096 has n1 = 4096
        yield h


def run_host(h, c):
    return h.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], c["sigma"], c["iterations"], c["draws"])


def same_nan(a, b):
    """as same(), but a NaN matches a NaN whatever its payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def check_taps(h, r, what, pair=0, eq=same):
    """the iteration records and the match records of `pair` against the oracle's answer r (made with the same tap choice)"""
    t = r["tap"]
    it = h.tap(pair, IN.TAP_ITERATIONS)
    assert len(it) == len(t["sets"]), what
    assert same(it["set"], t["sets"]), f"{what}: mvSets"
    for f in TAP_FIELDS:
        assert eq(it[f], t[f]), f"{what}: tap {f}"
    m = h.tap(pair, IN.TAP_MATCHES)
    assert m.shape == (r["n_matches"], 9), what
    assert eq(m[:, :4], t["chi"]), f"{what}: chiSquare of both models in match order"
    rt = t["rt"] if t["rt"] is not None else np.zeros((r["n_matches"], 5), np.float32)
    assert eq(m[:, 4:], rt), f"{what}: CheckRT records"


def host_case(h, table, name, tap_iteration, eq=same):
    """one host call with the taps on `tap_iteration` and the oracle's best hypothesis; everything compared"""
    c = E.case(table, name)
    hyp = max(E.answer(table, name)["best"], 0)
    r = E.answer(table, name, tap_iteration, hyp)
    h.set_tap_iteration(tap_iteration, hyp)
    res, P3D, tri = run_host(h, c)
    assert_result(res, r, name)
    assert same(P3D, r["P3D"]), f"{name}: P3D by index of keys1"
    assert same(tri, r["triangulated"]), f"{name}: triangulated"
    check_taps(h, r, name, eq=eq)
    return res, r


# ---- 1, 2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.PASSES))
def test_compaction_passes(handle, name):
    res, r = host_case(handle, "PASSES", name, E.case("PASSES", name)["iterations"] // 2)
    assert res["ok"] == 1 and r["P3D"].any()


@pytest.mark.parametrize("name", list(E.STAGES))
def test_stages_and_the_size_ceiling(handle, name):
    res, r = host_case(handle, "STAGES", name, E.case("STAGES", name)["iterations"] // 2)
    assert res["ok"] == 1 and res["n_matches"] == int(name.split("_")[1])


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.ITERATIONS))
def test_iteration_ceiling(handle, name):
    its = E.case("ITERATIONS", name)["iterations"]
    res, r = host_case(handle, "ITERATIONS", name, its - 1)   # check_taps: all `its` records
    assert res["iterF"] == res["iterH"] == its - 1
    assert len(handle.tap(0, IN.TAP_ITERATIONS)) == its


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.PARALLAX))
def test_parallax_selection(handle, name):
    res, r = host_case(handle, "PARALLAX", name, 0)
    for h in range(8):   # every hypothesis, not only the winner (assert_result has compared them already: said again by name)
        assert same(res["sel_cos"][h], np.float32(r["sel_cos"][h])), (name, h, res["sel_cos"][h], r["sel_cos"][h])
        assert res["n_cos"][h] == r["n_cos"][h] and res["nGood"][h] == r["nGood"][h], (name, h)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.NONFINITE))
def test_non_finite_scores(handle, name):
    res, r = host_case(handle, "NONFINITE", name, 3, eq=same_nan)
    it = handle.tap(0, IN.TAP_ITERATIONS)
    for f in ("scoreH", "scoreF"):   # which iterations are finite, said on its own
        assert np.array_equal(np.isfinite(it[f]), np.isfinite(r["tap"][f])), (name, f)
    if name == "same_x":
        assert res["status"] == IN.STATUS_NO_MODEL and res["model"] == 0 and res["iterH"] == res["iterF"] == -1
    else:
        assert res["status"] == IN.STATUS_OK and res["iterH"] >= 0 and res["iterF"] >= 0


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def device_batch(keys):
    """the CSR batch of the cases `keys` (table, name) on the device, outputs pre-filled with sentinels -> (args, outputs, off1)"""
    import torch
    cs = [E.case(*k) for k in keys]
    off1 = np.cumsum([0] + [len(c["keys1"]) for c in cs]).astype(np.int32)
    off2 = np.cumsum([0] + [len(c["keys2"]) for c in cs]).astype(np.int32)
    pairs = np.zeros(len(cs), IN.PAIR_DTYPE)
    doff = 0
    for p, c in zip(pairs, cs):
        p["K"], p["sigma"], p["iterations"], p["draws_offset"] = c["K"], c["sigma"], c["iterations"], doff
        doff += 8 * c["iterations"]
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    n = int(off1[-1])
    args = dict(offsets1=t(off1), offsets2=t(off2), keys1=t(np.concatenate([c["keys1"] for c in cs])),
                keys2=t(np.concatenate([c["keys2"] for c in cs])), matches12=t(np.concatenate([c["matches12"] for c in cs])),
                pairs=t(pairs.view(np.uint8).reshape(len(cs), -1)), draws=t(np.concatenate([c["draws"] for c in cs])))
    outs = dict(result=t(np.full((len(cs), IN.RESULT_DTYPE.itemsize), SENT_B, np.uint8)), P3D=t(np.full((n, 3), SENT_F, np.float32)),
                triangulated=t(np.full(n, SENT_B, np.uint8)))
    return args, outs, off1


def run_batch(h, keys):
    import torch
    args, outs, off1 = device_batch(keys)
    res, P3D, tri = h.initialize_device(**args, **outs)
    torch.cuda.synchronize()
    return res.cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1), P3D.cpu().numpy(), tri.cpu().numpy(), off1


def check_pair(i, key, rec, P3D, tri, off1):
    r = E.answer(*key)
    assert_result(rec[i], r, f"pair {i} {key}")
    assert same(P3D[off1[i]:off1[i + 1]], r["P3D"]), (i, key, "P3D")
    assert same(tri[off1[i]:off1[i + 1]], r["triangulated"]), (i, key, "triangulated")


def untouched(i, P3D, tri, off1):
    return (P3D[off1[i]:off1[i + 1]] == SENT_F).all() and (tri[off1[i]:off1[i + 1]] == SENT_B).all()


def test_batch_pair_past_the_taps():
    keys = E.batch33()
    total = sum(len(E.case(*k)["keys1"]) for k in keys)
    with InitializerHandle(total, 33) as h:
        h.set_tap_iteration(2, 0)
        rec, P3D, tri, off1 = run_batch(h, keys)
        for i, k in enumerate(keys):
            check_pair(i, k, rec, P3D, tri, off1)
        for i in (0, 31):   # the first and the last tapped pair in full
            check_taps(h, E.answer(*keys[i], 2, 0), f"pair {i}", pair=i)
        for stage in (IN.TAP_ITERATIONS, IN.TAP_MATCHES):
            with pytest.raises(OrbfeError) as e:
                h.tap(E.TAP_SETS, stage)
            assert e.value.status == _ffi.ORBFE_ERR_STATE
        check_pair(32, keys[32], rec, P3D, tri, off1)


def test_batch_empty_pairs_between_good_ones():
    keys = E.empties()
    total = sum(len(E.case(*k)["keys1"]) for k in keys)
    with InitializerHandle(total, len(keys)) as h:
        rec, P3D, tri, off1 = run_batch(h, keys)
        assert off1[1] == off1[2] and off1[4] - off1[3] == 6
        for i in (1, 3):
            assert rec[i]["status"] == IN.STATUS_FEW_MATCHES and rec[i]["ok"] == 0 and rec[i]["n_matches"] == 0
            assert rec[i]["iterH"] == rec[i]["iterF"] == rec[i]["best"] == -1
            assert untouched(i, P3D, tri, off1)
        for i in (0, 2, 4):
            check_pair(i, keys[i], rec, P3D, tri, off1)


def test_batch_ending_exactly_at_max_matches():
    keys = E.exact_fit()
    total = sum(len(E.case(*k)["keys1"]) for k in keys)
    with InitializerHandle(total, len(keys)) as h:
        rec, P3D, tri, off1 = run_batch(h, keys)
        assert off1[-1] == total == h.max_matches
        for i, k in enumerate(keys):
            check_pair(i, k, rec, P3D, tri, off1)
    with InitializerHandle(total - 1, len(keys)) as h:   # one key short: the last pair ends one past max_matches
        rec, P3D, tri, off1 = run_batch(h, keys)
        assert rec[2]["status"] == IN.STATUS_BAD_SIZES and rec[2]["ok"] == 0 and untouched(2, P3D, tri, off1)
        for i in (0, 1):
            check_pair(i, keys[i], rec, P3D, tri, off1)


def test_batch_of_1_and_512_iterations():
    keys = E.iteration_mix()
    assert [E.case(*k)["iterations"] for k in keys] == [1, 512, 1, 512]
    total = sum(len(E.case(*k)["keys1"]) for k in keys)
    with InitializerHandle(total, len(keys)) as h:
        h.set_tap_iteration(0, 0)
        rec, P3D, tri, off1 = run_batch(h, keys)
        for i, k in enumerate(keys):
            check_pair(i, k, rec, P3D, tri, off1)
        for i in (0, 3):
            check_taps(h, E.answer(*keys[i], 0, 0), f"pair {i}", pair=i)


def test_batch_twice_in_two_orders_on_one_handle():
    first, second = E.reorder()
    total = sum(len(E.case(*k)["keys1"]) for k in first)
    with InitializerHandle(total, len(first)) as h:
        for keys in (first, second, first):
            rec, P3D, tri, off1 = run_batch(h, keys)
            for i, k in enumerate(keys):
                check_pair(i, k, rec, P3D, tri, off1)

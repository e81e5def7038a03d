"""cv::findHomography on the GPU (csrc/orbfe_homography.hip) at the edges tests/homography_edge_cases.py plants: the
Levenberg-Marquardt state machine of k_homo_refine, the 32-iteration chunk and the 256-lane stride of k_homo_ransac, and the
batched form's set rules (oversized and negative-length sets, min_pairs, taps, two handles on two streams).  Everything is bit
for bit against tests/homography_oracle.py; tests/test_homography_edge_cases.py shows on the CPU that the cases reach and
separate the branches they are named for."""
import numpy as np
import pytest

import homography_cases as HC
import homography_edge_cases as EC
import homography_oracle as HO
from homography_checks import bits, check_case, check_taps
from orb_slam2_ssd_semantic_amd import Homography, OrbfeError, _ffi
from orb_slam2_ssd_semantic_amd import homography as HG

SENTINEL = 0xA5
GUARD = 64
_CASES = EC.table()
_GROUPS = EC.groups(_CASES)


@pytest.fixture(scope="module")
def hg():
    h = Homography(EC.MAX_PAIRS, 64)
    yield h
    h.close()


@pytest.fixture(scope="module")
def want():
    """name -> (H, mask, taps) of the oracle, computed once"""
    return {name: HO.find_homography(s, d, taps=True, **kw) for name, (s, d, kw) in _CASES.items()}


def _oracle(s, d, **kw):
    return HO.find_homography(s, d, taps=True, **kw)


def _upload(hg, off, src, dst):
    """CSR point sets on the handle's device, with sentinel-filled outputs and a guard band behind the mask"""
    import torch
    dev = torch.device("cuda", hg.device)
    nsets = len(off) - 1
    t = dict(H=torch.full((nsets, 3, 3), 7.0, dtype=torch.float64, device=dev),
             ok=torch.full((nsets,), -7, dtype=torch.int32, device=dev),
             mask=torch.full((len(src) + GUARD,), SENTINEL, dtype=torch.uint8, device=dev),
             off=torch.from_numpy(np.asarray(off, np.int32)).to(dev),
             src=torch.from_numpy(np.ascontiguousarray(src, np.float32)).to(dev),
             dst=torch.from_numpy(np.ascontiguousarray(dst, np.float32)).to(dev))
    torch.cuda.synchronize()
    return t


def _launch(hg, t, min_pairs=-1, stream=None, **kw):
    """find_batch on uploaded sets; synchronised unless a stream is given.  Returns the device tensors (H, ok, mask with guard)."""
    import torch
    hg.find_batch(t["off"], t["src"], t["dst"], min_pairs=min_pairs, H=t["H"], ok=t["ok"], mask=t["mask"],
                  stream=None if stream is None else stream.cuda_stream, **kw)
    if stream is None:
        torch.cuda.synchronize()
    return t["H"], t["ok"], t["mask"]


def _device_batch(hg, off, src, dst, min_pairs=-1, **kw):
    return _launch(hg, _upload(hg, off, src, dst), min_pairs, **kw)


def _csr(sets):
    off = np.r_[0, np.cumsum([len(s) for s, _ in sets])].astype(np.int32)
    return off, np.concatenate([s for s, _ in sets]), np.concatenate([d for _, d in sets])


def _all_taps(hg, nsets):
    return [(hg.tap(i, HG.TAP_RANSAC).tobytes(), hg.tap(i, HG.TAP_INFO).tobytes(), hg.tap(i, HG.TAP_REFIT).tobytes())
            for i in range(nsets)]


def _check_set(H, ok, mask, want_set, n, min_pairs, name):
    """one set of a batch against (H or None, mask, taps) of the oracle or of a host call"""
    wH, wmask = want_set[0], want_set[1]
    assert np.array_equal(mask, wmask), name
    if wH is None:
        assert ok == 0 and not H.any(), name
    else:
        assert np.array_equal(bits(H), bits(wH)), (name, H, wH)
        assert ok == int(n > min_pairs), name


# ---- every edge case through the host call -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_edge_case_bit_exact_at_every_tap(hg, want, name):
    s, d, kw = _CASES[name]
    H, t = check_case(hg, s, d, kw, name, oracle=want[name])
    assert H is not None


@pytest.mark.gpu
def test_max_iters_and_threshold_defaults(hg):
    """max_iters <= 0 is 1 and threshold <= 0 is 3: H, mask and taps of the GPU calls are equal byte for byte"""
    def call(name):
        s, d, kw = _CASES[name]
        H, mask = hg.find(s, d, **kw)
        return H.tobytes(), mask.tobytes(), _all_taps(hg, 1)
    one = call("max_iters_1")
    assert call("max_iters_0") == one and call("max_iters_-3") == one
    assert np.frombuffer(one[2][0][1], np.int32).tolist()[:3] == [1, 1, 1]
    three = call("threshold_3.0")
    assert call("threshold_0.0") == three and call("threshold_-1.0") == three


# ---- the batched form ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kw,names", _GROUPS, ids=["-".join(f"{k}={v}" for k, v in kw.items()) or "default" for kw, _ in _GROUPS])
def test_edge_cases_as_one_batch_per_kwargs(hg, want, kw, names):
    sets = [_CASES[n][:2] for n in names]
    off, src, dst = _csr(sets)
    runs = []
    for _ in range(2):
        H, ok, mask = _device_batch(hg, off, src, dst, **kw)
        runs.append((H.cpu().numpy(), ok.cpu().numpy(), mask.cpu().numpy(), _all_taps(hg, len(sets))))
    H, ok, mask, _ = runs[0]
    for i, name in enumerate(names):   # the taps of every set of the batch, before a host call overwrites them
        check_taps(hg, i, want[name][2], name)
    assert (mask[len(src):] == SENTINEL).all()
    for i, name in enumerate(names):
        s, d = sets[i]
        hH, hmask = hg.find(s, d, **kw)
        assert np.array_equal(bits(hH), bits(want[name][0])), name
        _check_set(H[i], ok[i], mask[off[i]:off[i + 1]], (hH, hmask), len(s), -1, name)
    a, b = runs
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3]


@pytest.mark.gpu
def test_oversized_and_negative_sets_beside_ordinary_ones():
    """0, 3 and 4 points, a set of max_pairs + 1 points and two sets whose offsets decrease, between ordinary sets.  The
    negative-length set in the middle steps 7 pairs back into the oversized set's range, whose mask nobody writes; the last
    set steps 20 back from the end."""
    mp = 300
    A = HC.planar(60, 0.7, 31)[:2]
    n3 = HC.planar(3, 1.0, 12)[:2]
    n4 = HC.planar(4, 1.0, 1004)[:2]
    big = HC.planar(mp + 1, 0.8, 32)[:2]
    B = HC.planar(100, 0.6, 33)[:2]
    n5 = HC.planar(5, 1.0, 34)[:2]
    #       n=0  A   n3  n4  big  -7   B    n5   -20
    off = [0, 0, 60, 63, 67, 368, 361, 461, 466, 446]
    names = ["n_0", "A", "n_3", "n_4", "oversized", "negative", "B", "n_5", "negative_last"]
    total = max(off)
    src, dst = np.zeros((total, 2), np.float32), np.zeros((total, 2), np.float32)
    for o, (s, d) in ((0, A), (60, n3), (63, n4), (67, big), (361, B), (461, n5)):   # B overwrites big's last 7 pairs
        src[o:o + len(s)], dst[o:o + len(s)] = s, d
    empty = np.zeros((0, 2), np.float32)
    ordinary = {0: (empty, empty), 1: A, 2: n3, 3: n4, 6: B, 7: n5}
    with Homography(mp, 16) as hg:
        runs = []
        for _ in range(2):
            H, ok, mask = _device_batch(hg, off, src, dst)
            runs.append((H.cpu().numpy(), ok.cpu().numpy(), mask.cpu().numpy(), _all_taps(hg, len(names))))
        H, ok, mask, taps = runs[0]
        assert runs[1][0].tobytes() == H.tobytes() and runs[1][1].tobytes() == ok.tobytes() and runs[1][2].tobytes() == mask.tobytes()
        assert runs[1][3] == taps
        zeros = (np.zeros(9).tobytes(), np.zeros(4, np.int32).tobytes(), np.zeros(9).tobytes())
        for i in (4, 5, 8):   # oversized, negative: no model, nothing of the mask written, taps cleared
            assert ok[i] == 0 and not bits(H[i]).any(), names[i]   # +0.0, bit for bit
            assert taps[i] == zeros, names[i]
        assert (mask[67:361] == SENTINEL).all()     # the oversized set's bytes no other set owns
        assert (mask[total:] == SENTINEL).all() and len(mask) == total + GUARD
        for i, (s, d) in ordinary.items():
            o = _oracle(s, d)
            check_taps(hg, i, o[2], names[i])
            _check_set(H[i], ok[i], mask[off[i]:off[i] + len(s)], o, len(s), -1, names[i])
        assert [int(ok[i]) for i in (0, 2)] == [0, 0] and [int(ok[i]) for i in (1, 3, 6, 7)] == [1, 1, 1, 1]
        for i, (s, d) in ordinary.items():   # and against the host call on the same handle
            hH, hmask = hg.find(s, d)
            _check_set(H[i], ok[i], mask[off[i]:off[i] + len(s)], (hH, hmask), len(s), -1, names[i])
        with pytest.raises(OrbfeError):   # the host call refuses what the batch skips
            hg.find(*big)


@pytest.mark.gpu
@pytest.mark.parametrize("min_pairs,ratio", [(7, 1.0), (120, 0.7)])
def test_min_pairs_either_side(hg, min_pairs, ratio):
    sets = [HC.planar(n, ratio, 40 + n)[:2] for n in (min_pairs, min_pairs + 1, min_pairs - 1, min_pairs + 1)]
    off, src, dst = _csr(sets)
    H, ok, mask = _device_batch(hg, off, src, dst, min_pairs=min_pairs)
    H, ok, mask = H.cpu().numpy(), ok.cpu().numpy(), mask.cpu().numpy()
    assert ok.tolist() == [0, 1, 0, 1]
    for i, (s, d) in enumerate(sets):   # ok gates nothing but itself: H and the mask are the host call's
        o = _oracle(s, d)
        assert o[0] is not None and np.array_equal(bits(H[i]), bits(o[0])), i
        assert np.array_equal(mask[off[i]:off[i + 1]], o[1]), i
        check_taps(hg, i, o[2], i)
    assert (mask[len(src):] == SENTINEL).all()


@pytest.mark.gpu
def test_tap_errors_and_the_sets_the_taps_cover(hg):
    import torch
    L = _ffi.lib()
    sets = [HC.planar(n, 0.8, 50 + n)[:2] for n in (30, 3, 40)]
    off, src, dst = _csr(sets)

    def tap(set_index, stage, cap):
        buf = np.full(80, SENTINEL, np.uint8)
        return L.orbfe_homography_tap(hg.h, set_index, stage, _ffi.ptr(buf), cap), buf

    _device_batch(hg, off, src, dst)
    for i in range(3):
        for stage, need in ((HG.TAP_RANSAC, 72), (HG.TAP_INFO, 16), (HG.TAP_REFIT, 72)):
            st, buf = tap(i, stage, need)
            assert st == _ffi.ORBFE_OK and (buf[need:] == SENTINEL).all(), (i, stage)
            st, buf = tap(i, stage, need - 1)
            assert st == _ffi.ORBFE_ERR_CAP and (buf == SENTINEL).all(), (i, stage)
    for bad_set in (3, -1, 64):
        assert tap(bad_set, HG.TAP_INFO, 16)[0] == _ffi.ORBFE_ERR_STATE, bad_set
    for bad_stage in (-1, 3, 1 << 20):
        st, buf = tap(0, bad_stage, 80)
        assert st == _ffi.ORBFE_ERR_ARG and (buf == SENTINEL).all(), bad_stage
    assert L.orbfe_homography_tap(hg.h, 0, HG.TAP_INFO, None, 16) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_homography_tap(None, 0, HG.TAP_INFO, _ffi.ptr(np.zeros(4, np.int32)), 16) == _ffi.ORBFE_ERR_ARG
    with pytest.raises(OrbfeError) as e:
        hg.tap(3, HG.TAP_INFO)
    assert e.value.status == _ffi.ORBFE_ERR_STATE
    # a host call leaves one set
    hg.find(*sets[0])
    assert tap(0, HG.TAP_INFO, 16)[0] == _ffi.ORBFE_OK and tap(1, HG.TAP_INFO, 16)[0] == _ffi.ORBFE_ERR_STATE
    # an empty batch leaves none
    dev = torch.device("cuda", 0)
    z = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    hg.find_batch(torch.zeros(1, dtype=torch.int32, device=dev), z, z)
    assert tap(0, HG.TAP_INFO, 16)[0] == _ffi.ORBFE_ERR_STATE


@pytest.mark.gpu
def test_two_handles_on_two_streams_interleaved(want):
    import torch
    dev = torch.device("cuda", 0)
    default = next(names for kw, names in _GROUPS if kw == {})
    method0 = next(names for kw, names in _GROUPS if kw == dict(method=0))
    work = {0: [(default[:4], {}), (method0[:4], dict(method=0))],   # handle 0: RANSAC sets, then method 0
            1: [(method0[4:], dict(method=0)), (default[4:], {})]}    # handle 1: the other way round, other sets
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    with Homography(EC.MAX_PAIRS, 16) as h0, Homography(EC.MAX_PAIRS, 16) as h1:
        handles = [h0, h1]
        up = {}
        for k in (0, 1):
            for step in range(2):
                off, src, dst = _csr([_CASES[n][:2] for n in work[k][step][0]])
                up[k, step] = (off, _upload(handles[k], off, src, dst))
        out = {}
        for step in range(2):   # nothing waits between these four launches
            for k in (0, 1):
                out[k, step] = (up[k, step][0],) + _launch(handles[k], up[k, step][1], stream=streams[k], **work[k][step][1])
        for st in streams:
            st.synchronize()
        for k in (0, 1):   # the taps are the last call's
            for i, name in enumerate(work[k][1][0]):
                check_taps(handles[k], i, want[name][2], (k, name))
        for (k, step), (off, H, ok, mask) in out.items():
            names, kw = work[k][step]
            H, ok, mask = H.cpu().numpy(), ok.cpu().numpy(), mask.cpu().numpy()
            for i, name in enumerate(names):
                _check_set(H[i], ok[i], mask[off[i]:off[i + 1]], want[name], len(_CASES[name][0]), -1, (k, step, name))
            assert (mask[off[-1]:] == SENTINEL).all()
            for i, name in enumerate(names):   # and its own host calls (these overwrite the taps)
                hH, hmask = handles[k].find(*_CASES[name][:2], **kw)
                _check_set(H[i], ok[i], mask[off[i]:off[i + 1]], (hH, hmask), len(hmask), -1, (k, step, name))

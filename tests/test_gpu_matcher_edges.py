"""The Hamming matchers at their tie, ratio, threshold, bin and size edges, bit for bit against the CPU oracle.

Inputs come from tests/hamming_cases.py: planted distances instead of random descriptors, so that every case sits on the
boundary it names.  The all-pairs matcher runs through both kernels (k_match_bf on the matrix cores, k_match_popc) and all
four entry points (host buffers, orbfe_match_bf_device, the frames form, the blocks form with distinct query and train
blocks); SearchByBoW through the host form (k_search_by_bow) and the batched device form (k_search_by_bow_rows) with
hand-written feature-vector blocks; HammingCSR through its three entry points.  A nnratio above 1 is used where the
index of a tied best has to reach `match` (with nnratio <= 1 a tie always fails the ratio test)."""
import ctypes as C

import numpy as np
import pytest

import hamming_cases as H
from rotation_cases import ROTATION_CASES, ROTATION_KEPT, _rotation_groups

pytestmark = pytest.mark.gpu

BIG = 1 << 22          # BM_MAX_NT: the largest train set / cap the all-pairs entry points take


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _lib():
    from orb_slam2_ssd_semantic_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def mts():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    out = {}
    for k in (0, 1):
        out[k] = ORBmatcher(0.6, True)
        out[k].set_bf_kernel(k)
    yield out
    for m in out.values():
        m.close()


# ------------------------------------------------------------------------------------------------ all-pairs harness
def _case(q, t, rng=None, qa=None, ta=None):
    rng = rng or np.random.default_rng(len(q) * 7919 + len(t))
    qa = rng.uniform(0, 360, len(q)).astype(np.float32) if qa is None else np.asarray(qa, np.float32)
    ta = rng.uniform(0, 360, len(t)).astype(np.float32) if ta is None else np.asarray(ta, np.float32)
    return np.ascontiguousarray(q, np.uint8).reshape(-1, 32), np.ascontiguousarray(t, np.uint8).reshape(-1, 32), qa, ta


def _host(mt, c, ratio, th, ori):
    q, t, qa, ta = c
    mt.mfNNratio, mt.mbCheckOrientation = ratio, ori
    return mt.MatchBruteForce(q, t, qa, ta, th)


def _device(mt, c, ratio, th, ori):
    import torch
    q, t, qa, ta = c
    nq, nt = len(q), len(t)
    dq, dt = _dev(q if nq else np.zeros((1, 32), np.uint8)), _dev(t if nt else np.zeros((1, 32), np.uint8))
    dqa, dta = _dev(qa if nq else np.zeros(1, np.float32)), _dev(ta if nt else np.zeros(1, np.float32))
    out = [torch.full((max(nq, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    dn = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = _lib().orbfe_match_bf_device(mt.handle, dq.data_ptr(), nq, dt.data_ptr(), nt, dqa.data_ptr(), dta.data_ptr(), ratio, th,
                                      int(ori), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), dn.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy()[:nq] for o in out) + (int(dn[0]),)


def _block(frames, cap):
    """frames: list of (desc, angles) -> desc block [B][cap][32], keypoint block [B][cap][7] (angle at field 3), n [B]"""
    B = len(frames)
    desc = np.zeros((B, cap, 32), np.uint8)
    kps = np.zeros((B, cap, 7), np.float32)
    n = np.zeros(B, np.int32)
    for b, (d, a) in enumerate(frames):
        k = min(len(d), cap)
        desc[b, :k], kps[b, :k, 3], n[b] = d[:k], a[:k], len(d)
    return _dev(desc), _dev(kps), _dev(n)


def _batched(mt, cases, ratio, th, ori, cap, blocks):
    """All cases in one launch.  frames form: one block [q0, t0, q1, t1, ...], pair p = (2p, 2p + 1); blocks form: a query
    block [q0, q1, ...] and a train block holding the train sets in reverse order.  Returns (match [P][cap], nmatches [P])."""
    import torch
    P = len(cases)
    if blocks:
        dqd, dqk, dqn = _block([(c[0], c[2]) for c in cases], cap)
        dtd, dtk, dtn = _block([(c[1], c[3]) for c in cases[::-1]], cap)
        qf, tf = _dev(np.arange(P, dtype=np.int32)), _dev(np.arange(P - 1, -1, -1, dtype=np.int32))
    else:
        dqd, dqk, dqn = _block([x for c in cases for x in ((c[0], c[2]), (c[1], c[3]))], cap)
        dtd, dtk, dtn = dqd, dqk, dqn
        qf, tf = _dev(np.arange(0, 2 * P, 2, dtype=np.int32)), _dev(np.arange(1, 2 * P, 2, dtype=np.int32))
    dm = torch.full((P, cap), -7, dtype=torch.int32, device="cuda")
    dnm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    rc = _lib().orbfe_match_bf_blocks_device(mt.handle, dqk.data_ptr(), dqd.data_ptr(), dqn.data_ptr(), dtk.data_ptr(), dtd.data_ptr(),
                                             dtn.data_ptr(), cap, qf.data_ptr(), tf.data_ptr(), P, ratio, th, int(ori), dm.data_ptr(),
                                             dnm.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return dm.cpu().numpy(), dnm.cpu().numpy()


def check_bf(oracle, mts, cases, ratio, th, ori, cap=None, forms=("host", "device", "frames", "blocks")):
    """Every case through every form of both kernels == oracle.match_bf (match, best, second, nmatches)."""
    refs = [oracle.match_bf(q, t, qa, ta, ratio, th, ori) for q, t, qa, ta in cases]
    cap = cap or max(1, max(max(len(c[0]), len(c[1])) for c in cases) + 3)
    for k, mt in mts.items():
        for i, (c, ref) in enumerate(zip(cases, refs)):
            for form in ("host", "device"):
                if form in forms:
                    got = (_host if form == "host" else _device)(mt, c, ratio, th, ori)
                    for name, g, r in zip(("match", "best", "second"), got[:3], ref[:3]):
                        assert np.array_equal(g, r), (k, form, i, name, np.flatnonzero(g != r)[:8])
                    assert got[3] == ref[3], (k, form, i, got[3], ref[3])
        for form in ("frames", "blocks"):
            if form not in forms:
                continue
            m, n = _batched(mt, cases, ratio, th, ori, cap, form == "blocks")
            for i, (c, ref) in enumerate(zip(cases, refs)):
                nq = len(c[0])
                assert np.array_equal(m[i, :nq], ref[0]), (k, form, i, np.flatnonzero(m[i, :nq] != ref[0])[:8])
                assert (m[i, nq:] == -1).all() and n[i] == ref[3], (k, form, i, n[i], ref[3])
    return refs


# ------------------------------------------------------------------------------------------------ ties
def _tie_cases(rng):
    cases = []
    # one query per tie layout; rows 0-3 / 8-11 / ... sit in lane half 0 of a 32-row tile of k_match_bf, 4-7 / 12-15 in half 1
    layouts = [
        (40, [(4, 7), (9, 7)]),              # half 1 before half 0
        (40, [(3, 7), (5, 7)]),              # half 0 before half 1
        (40, [(12, 9), (16, 9), (20, 9)]),   # three-way, halves 1 / 0 / 1
        (64, [(31, 6), (32, 6)]),            # across the 32-row tile boundary
        (64, [(5, 6), (33, 6)]),             # later tile, smaller in-tile row: the field latch must keep row 5
        (64, [(13, 6), (44, 6), (60, 8)]),
        (200, [(127, 11), (128, 11)]),       # across k_match_popc's 128-row tile
        (200, [(100, 11), (130, 11), (190, 11)]),
        (200, [(0, 15), (199, 15)]),         # first and last row
        (200, [(10, 9), (50, 9), (60, 8)]),  # a strictly better row after a tie
        (129, [(128, 3), (96, 3)]),          # last (partial) tile
        (33, [(32, 2), (0, 2)]),
    ]
    for nt, plants in layouts:
        q, t = H.planted_bf(rng, 1, nt, [(0, r, d) for r, d in plants])
        cases.append(_case(q, t, rng))
    # many queries, a tie planted for every third of them at two rows of a random order
    nq, nt = 300, 260
    rows = rng.permutation(nt)
    plants = []
    for j, i in enumerate(range(0, nq, 3)):
        d = 10 + i % 7
        plants += [(i, int(rows[2 * j]), d), (i, int(rows[2 * j + 1]), d)]
    q, t = H.planted_bf(rng, nq, nt, plants)
    cases.append(_case(q, t, rng))
    return cases


@pytest.mark.parametrize("ratio", [1.5, 0.9])
def test_bf_ties(oracle, mts, ratio):
    cases = _tie_cases(np.random.default_rng(11))
    refs = check_bf(oracle, mts, cases, ratio, 100, False)
    if ratio > 1:   # the intended winners: the earliest of the tied rows
        assert [int(r[0][0]) for r in refs[:12]] == [4, 3, 12, 31, 5, 13, 127, 100, 0, 60, 96, 0]
        assert [int(r[2][0]) for r in refs[:12]] == [7, 7, 9, 6, 6, 6, 11, 11, 15, 9, 3, 2]


# ------------------------------------------------------------------------------------------------ query positions + ratio edges
POSITIONS = (0, 31, 32, 127, 128, 511, 512, 1024)


def _position_case(rng, nq, ratio):
    nt = 700
    edges = H.RATIO_EDGES.get(ratio, [(5, 9), (7, 7), (20, 21)])
    plants, row = [], 0
    for j, p in enumerate(x for x in POSITIONS if x < nq):
        b, s = edges[j % len(edges)]
        plants += [(p, row, b), (p, row + 1, s)]
        row += 2
    for p in range(1, nq, 37):   # more planted queries between the named positions
        if p not in POSITIONS and row + 1 < nt:
            b, s = edges[p % len(edges)]
            plants += [(p, row + 1, b), (p, row, s)]
            row += 2
    perm = rng.permutation(nt)   # spread the planted rows over the tiles
    q, t = H.planted_bf(rng, nq, nt, [(qi, int(perm[r]), d) for qi, r, d in plants])
    return _case(q, t, rng), plants, perm


@pytest.mark.parametrize("ratio", [0.6, 0.8, 1.0, 1.5])
def test_bf_query_positions_and_ratio_edges(oracle, mts, ratio):
    rng = np.random.default_rng(int(ratio * 10))
    built = [_position_case(rng, nq, ratio) for nq in (511, 512, 513, 1025)]
    refs = check_bf(oracle, mts, [b[0] for b in built], ratio, 100, False)
    for (c, plants, perm), ref in zip(built, refs):   # the planted pairs decide these queries
        for qi, r, d in plants[::2]:
            assert ref[1][qi] == d, (qi, ref[1][qi], d)
        if ratio in H.RATIO_EDGES:                       # float rejects what double would accept
            assert (ref[0][[p for p in POSITIONS if p < len(c[0])]] == -1).all()


def test_bf_ratio_edges_accept_just_inside(oracle, mts):
    """(3, 6) at 0.6 and (4, 6) at 0.8 pass: the boundary pairs above fail for the rounding, not for the planting"""
    rng = np.random.default_rng(5)
    for ratio, (b, s) in ((0.6, (3, 6)), (0.8, (4, 6)), (0.6, (3, 5)), (0.8, (4, 5)), (1.0, (9, 10)), (1.0, (9, 9))):
        q, t = H.planted_bf(rng, 1, 50, [(0, 17, b), (0, 40, s)])
        ref = check_bf(oracle, mts, [_case(q, t, rng)], ratio, 100, False)[0]
        assert (ref[1][0], ref[2][0]) == (b, s)
        assert ref[0][0] == (17 if H.ratio_pass(b, s, ratio) else -1)


# ------------------------------------------------------------------------------------------------ distance / threshold extremes
def _extreme_cases(rng):
    base = H.random_rows(rng, 1)[0]
    inv = np.bitwise_not(base)
    Q = base[None]
    far = lambda n: H.far_rows(rng, base, n)   # noqa: E731
    cases = [
        (Q, np.repeat(inv[None], 70, 0)),                              # every row at 256
        (Q, inv[None]),                                                # a single row at 256
        (Q, np.concatenate([far(40), base[None], far(30)])),           # d = 0 as best, second >= 200
        (Q, np.concatenate([far(33), base[None], far(5), base[None]])),  # d = 0 as best and as second
        (Q, np.concatenate([H.at_distance(rng, base, 7)[None], inv[None]])),  # d = 256 as second
        (Q, np.concatenate([inv[None], H.at_distance(rng, base, 7)[None], inv[None]])),
        (Q, np.repeat(H.random_rows(rng, 1), 45, 0)),                  # every row identical
        (H.near_rows(rng, base, 5), np.repeat(base[None], 37, 0)),     # every row identical, d = 0
        (Q, np.concatenate([far(10), H.at_distance(rng, base, 50)[None], far(3)])),   # best == th (50)
        (Q, np.concatenate([far(10), H.at_distance(rng, base, 51)[None], far(3)])),   # best == th + 1
        (Q, np.concatenate([far(10), H.at_distance(rng, base, 200)[None]])),
    ]
    return [_case(q, t, rng) for q, t in cases]


@pytest.mark.parametrize("th,ratio", [(50, 0.9), (0, 0.9), (256, 0.9), (256, 1.5), (255, 1.5), (100, 1.0)])
def test_bf_distance_and_threshold_extremes(oracle, mts, th, ratio):
    cases = _extreme_cases(np.random.default_rng(3))
    refs = check_bf(oracle, mts, cases, ratio, th, False)
    assert (refs[0][1][0], refs[0][2][0], refs[0][0][0]) == (256, 256, -1)   # no row below 256: no best index at all
    assert (refs[2][1][0], refs[3][1][0], refs[3][2][0]) == (0, 0, 0)
    assert refs[8][1][0] == 50 and refs[9][1][0] == 51
    if th == 50 and ratio < 1:
        assert refs[8][0][0] == 10 and refs[9][0][0] == -1


# ------------------------------------------------------------------------------------------------ rotation histogram
def _rotation_bf_case(name):
    qa, ta = _rotation_groups(ROTATION_CASES[name])
    n = len(qa)
    rng = np.random.default_rng(n)
    q = H.random_rows(rng, n)
    t = np.stack([H.at_distance(rng, q[i], 5) for i in range(n)])   # query i -> train row i at 5, all others ~128
    return _case(q, t, rng, qa, ta)


def test_rotation_prune_bf(oracle, mts):
    """k_rot_prune (host, device, frames and blocks forms): more than 256 matches per pair, exact half-bin rotations and wraps
    through +360, the 0.1 * max1 boundary, equal-count maxima."""
    cases = [_rotation_bf_case(n) for n in ROTATION_CASES]
    refs = check_bf(oracle, mts, cases, 0.6, 100, True)
    kept = {n: r[3] for n, r in zip(ROTATION_CASES, refs)}
    assert kept == ROTATION_KEPT, kept
    assert min(len(c[0]) for c in cases) >= 109 and max(len(c[0]) for c in cases) > 256


# ------------------------------------------------------------------------------------------------ batched forms
@pytest.mark.parametrize("cap", [300, 777, 1100])
def test_bf_batched_counts(oracle, mts, cap):
    """frames / blocks forms: counts 0, counts above cap (clamped), a frame against itself, cap not a multiple of 256 or 512;
    slots past a pair's query count stay -1."""
    import torch
    rng = np.random.default_rng(cap)
    sizes = [0, 1, cap + 9, cap, cap - 1, 200, 37]
    descs = [H.random_rows(rng, min(s, cap)) for s in sizes]
    for i in range(1, len(descs)):   # correlate neighbours so that pairs have matches
        k = min(len(descs[i]), len(descs[i - 1]))
        descs[i][:k] = np.stack([H.at_distance(rng, descs[i - 1][j], 3 + j % 20) for j in range(k)]) if k else descs[i][:k]
    angs = [rng.uniform(0, 360, len(d)).astype(np.float32) for d in descs]
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (4, 4), (2, 2), (3, 4), (5, 6), (6, 5), (0, 0), (2, 5)]
    B, P = len(sizes), len(pairs)
    desc = np.zeros((B, cap, 32), np.uint8)
    kps = np.zeros((B, cap, 7), np.float32)
    for b, (d, a) in enumerate(zip(descs, angs)):
        desc[b, :len(d)], kps[b, :len(d), 3] = d, a
    dd, dk, dn = _dev(desc), _dev(kps), _dev(np.asarray(sizes, np.int32))
    qf, tf = _dev(np.asarray([p[0] for p in pairs], np.int32)), _dev(np.asarray([p[1] for p in pairs], np.int32))
    for k, mt in mts.items():
        for ori in (True, False):
            dm = torch.full((P, cap), -7, dtype=torch.int32, device="cuda")
            dnm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
            rc = _lib().orbfe_match_bf_frames_device(mt.handle, dk.data_ptr(), dd.data_ptr(), dn.data_ptr(), cap, qf.data_ptr(),
                                                     tf.data_ptr(), P, 0.8, 60, int(ori), dm.data_ptr(), dnm.data_ptr(), None)
            assert rc == 0
            torch.cuda.synchronize()
            m, n = dm.cpu().numpy(), dnm.cpu().numpy()
            for p, (a, b) in enumerate(pairs):
                ref = oracle.match_bf(descs[a], descs[b], angs[a], angs[b], 0.8, 60, ori)
                na = len(descs[a])
                assert np.array_equal(m[p, :na], ref[0]) and (m[p, na:] == -1).all() and n[p] == ref[3], (k, ori, p)
    # the generic harness on the same shapes, distinct query / train blocks
    cases = [_case(descs[a], descs[b], rng, angs[a], angs[b]) for a, b in pairs]
    check_bf(oracle, mts, cases, 0.8, 60, True, cap=cap, forms=("blocks",))


# ------------------------------------------------------------------------------------------------ train-set limit
def _big_case(nt):
    """8 queries against a train set of nt rows: one filler row repeated, planted rows in the last tile, at and past 2^21.
    Returns (q, t, keep): the oracle on t[keep] -- the planted rows plus the first two filler rows -- gives the expected
    result once its indices are mapped back through keep."""
    rng = np.random.default_rng(22)
    q = H.random_rows(rng, 8)
    filler = H.random_rows(rng, 1)[0]
    plants = [(0, BIG - 1, 9), (1, BIG // 2, 11), (1, BIG // 2 + 1, 11), (2, BIG // 2 + 5, 3), (2, BIG - 2, 5),
              (3, BIG - 31, 20), (4, BIG // 2 + BIG // 4 + 7, 0), (4, 5, 4), (5, 0, 12), (5, BIG - 3, 12), (6, BIG // 2 - 1, 30),
              (6, BIG // 2 - 3, 31)]
    rows = {}
    for qi, r, d in plants:
        if r < nt:
            rows[r] = H.at_distance(rng, q[qi], d)
    t = np.empty((nt, 32), np.uint8)
    t[:] = filler
    for r, v in rows.items():
        t[r] = v
    fillers = [i for i in range(8) if i not in rows][:2]   # two copies: a filler best or second keeps its multiplicity
    keep = sorted(list(rows) + fillers)
    return q, t, keep


def test_bf_train_set_limit(oracle, mts):
    """nt = 2^22 (BM_MAX_NT: k_match_popc keeps the row in 22 key bits) and 2^22 - 3 (a partial last tile), host and
    device forms; nt or cap = 2^22 + 1 is refused by every all-pairs entry point."""
    import torch
    for nt in (BIG, BIG - 3):
        q, t, keep = _big_case(nt)
        small = t[keep]
        mref, bref, sref, _ = oracle.match_bf(q, small, None, None, 1.5, 200, False)
        mref = np.where(mref >= 0, np.asarray(keep)[np.maximum(mref, 0)], -1)
        assert bref.tolist()[1:6] == [11, 3, 20, 0, 12] and (bref[0] == 9) == (nt == BIG)
        assert mref[1] == BIG // 2 and mref[5] == 0 and mref[4] == BIG // 2 + BIG // 4 + 7
        dq, dt = _dev(q), torch.from_numpy(t).cuda()
        for k, mt in mts.items():
            got = _host(mt, (q, t, None, None), 1.5, 200, False)
            assert np.array_equal(got[0], mref) and np.array_equal(got[1], bref) and np.array_equal(got[2], sref), (k, nt, got)
            out = [torch.full((8,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
            rc = _lib().orbfe_match_bf_device(mt.handle, dq.data_ptr(), 8, dt.data_ptr(), nt, None, None, 1.5, 200, 0,
                                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None)
            assert rc == 0
            torch.cuda.synchronize()
            for o, r in zip(out[:3], (mref, bref, sref)):
                assert np.array_equal(o.cpu().numpy(), r), (k, nt)
            assert int(out[3][0]) == int((mref >= 0).sum())
        del dt
    # one row past the limit: refused before anything is read or written (the buffers are big enough anyway)
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _lib()
    over = BIG + 1
    ht = np.zeros((over, 32), np.uint8)
    hq = np.zeros((4, 32), np.uint8)
    m4, b4, s4, n1 = (np.zeros(4, np.int32) for _ in range(4))
    dt = torch.zeros((over, 32), dtype=torch.uint8, device="cuda")
    dq = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
    dm = torch.zeros(over, dtype=torch.int32, device="cuda")
    dkp = torch.zeros((1, 7), dtype=torch.float32, device="cuda")
    dn = torch.tensor([4], dtype=torch.int32, device="cuda")
    zf = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k, mt in mts.items():
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        assert L.orbfe_match_bf(mt.handle, p(hq), 4, p(ht), over, None, None, 0.9, 100, 0, p(m4), p(b4), p(s4), p(n1)) == _ffi.ORBFE_ERR_ARG
        assert L.orbfe_match_bf_device(mt.handle, dq.data_ptr(), 4, dt.data_ptr(), over, None, None, 0.9, 100, 0, dm.data_ptr(),
                                       dm.data_ptr(), dm.data_ptr(), dm.data_ptr(), None) == _ffi.ORBFE_ERR_ARG
        assert L.orbfe_match_bf_frames_device(mt.handle, dkp.data_ptr(), dt.data_ptr(), dn.data_ptr(), over, zf.data_ptr(), zf.data_ptr(),
                                              1, 0.9, 100, 0, dm.data_ptr(), dm.data_ptr(), None) == _ffi.ORBFE_ERR_ARG
        assert L.orbfe_match_bf_blocks_device(mt.handle, dkp.data_ptr(), dt.data_ptr(), dn.data_ptr(), dkp.data_ptr(), dt.data_ptr(),
                                              dn.data_ptr(), over, zf.data_ptr(), zf.data_ptr(), 1, 0.9, 100, 0, dm.data_ptr(),
                                              dm.data_ptr(), None) == _ffi.ORBFE_ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ SearchByBoW
def _bow_host(mt, kf, f, ratio, th_low, kf_kf, ori):
    dK, vK, aK, fvK = kf
    dF, vF, aF, fvF = f
    mt.mfNNratio, mt.mbCheckOrientation = ratio, ori
    return mt.SearchByBoW(dK, vK, aK, fvK, dF, vF if kf_kf else None, aF, fvF, strict_lt=kf_kf, th_low=th_low)


def _bow_batched(mt, pairs, ratio, th_low, kf_kf, ori):
    """pairs: list of (kf side, f side), each (desc, valid, angles, (node, off, idx)); frames are packed into one block
    [kf0, f0, kf1, f1, ...] with hand-written feature-vector CSR blocks.  Returns (match [P][cap], nmatches [P])."""
    import torch
    frames = [s for p in pairs for s in p]
    cap = max(1, max(len(s[0]) for s in frames))
    B, P = len(frames), len(pairs)
    desc = np.zeros((B, cap, 32), np.uint8)
    kps = np.zeros((B, cap, 7), np.float32)
    valid = np.zeros((B, cap), np.uint8)
    node = np.zeros((B, cap), np.uint32)
    off = np.zeros((B, cap + 1), np.uint32)
    idx = np.zeros((B, cap), np.uint32)
    counts = np.zeros((B, 4), np.int32)
    for b, (d, v, a, (nd, of, ix)) in enumerate(frames):
        n = len(d)
        desc[b, :n], kps[b, :n, 3] = d, a
        valid[b, :n] = 1 if v is None else v
        node[b, :len(nd)], off[b, :len(of)], idx[b, :len(ix)] = nd, of, ix
        counts[b] = (len(nd), len(nd), len(ix), 0)
    dd, dk, dv, dno, dof, dix, dc = (_dev(x) for x in (desc, kps, valid, node, off, idx, counts))
    kf_i, f_i = _dev(np.arange(0, 2 * P, 2, dtype=np.int32)), _dev(np.arange(1, 2 * P, 2, dtype=np.int32))
    dm = torch.full((P, cap), -7, dtype=torch.int32, device="cuda")
    dn = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    mt.mfNNratio, mt.mbCheckOrientation = ratio, ori
    mt.SearchByBoW_batch_device(dk.data_ptr(), dd.data_ptr(), cap, dv.data_ptr(), dno.data_ptr(), dof.data_ptr(), dix.data_ptr(),
                                dc.data_ptr(), kf_i.data_ptr(), f_i.data_ptr(), P, dm.data_ptr(), dn.data_ptr(), kf_kf=kf_kf,
                                th_low=th_low)
    torch.cuda.synchronize()
    return dm.cpu().numpy(), dn.cpu().numpy()


def check_bow(oracle, mt, pairs, ratio, th_low, kf_kf, ori):
    """host and batched SearchByBoW == oracle.search_by_bow for every pair; returns the oracle's results"""
    refs = []
    for kf, f in pairs:
        refs.append(oracle.search_by_bow(kf[0], kf[1], kf[2], kf[3], f[0], f[1] if kf_kf else None, f[2], f[3], ratio, th_low,
                                         kf_kf, ori))
        got = _bow_host(mt, kf, f, ratio, th_low, kf_kf, ori)
        assert np.array_equal(got[0], refs[-1][0]) and got[1] == refs[-1][1], ("host", len(refs) - 1, got[1], refs[-1][1])
    m, n = _bow_batched(mt, pairs, ratio, th_low, kf_kf, ori)
    for p, ((kf, f), ref) in enumerate(zip(pairs, refs)):
        nf = len(f[0])
        assert np.array_equal(m[p, :nf], ref[0]), ("batched", p, np.flatnonzero(m[p, :nf] != ref[0])[:8])
        assert (m[p, nf:] == -1).all() and n[p] == ref[1], ("batched", p, n[p], ref[1])
    return refs


def _side(desc, fv, rng, valid=None, ang=None):
    n = len(desc)
    v = np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8)
    a = rng.uniform(0, 360, n).astype(np.float32) if ang is None else np.asarray(ang, np.float32)
    return desc, v, a, fv


def _pair(rng, nodes, vK=None, vF=None):
    (dK, fvK), (dF, fvF) = H.bow_frame_pair(nodes)
    return _side(dK, fvK, rng, vK), _side(dF, fvF, rng, vF)


def _chunk_tie_pairs(rng):
    """F lists of 15 / 16 / 17 / 33 features, ties at the 16-feature chunk edges, KF lists longer than 16 (LDS restaging)"""
    pairs = []
    for nF, ties in ((15, [(0, 14), (13, 14)]), (16, [(7, 15), (14, 15)]), (17, [(15, 16), (0, 16)]),
                     (33, [(16, 32), (3, 31), (15, 16), (31, 32)])):
        plants = []
        for k, (a, b) in enumerate(ties):
            plants += [(k, a, 9 + k), (k, b, 9 + k)]
        nodes = [H.bow_node(rng, 10 + j, 4, nF, plants) for j in range(3)]
        pairs.append(_pair(rng, nodes))
    for nK in (17, 33, 40):   # every KF feature planted on its own F feature, plus ties inside later chunks of the KF list
        nF = 48
        plants = [(k, (5 * k) % nF, 8 + k % 6) for k in range(nK)]
        plants += [(k, (5 * k + 17) % nF, 8 + k % 6) for k in range(16, nK, 3)]
        pairs.append(_pair(rng, [H.bow_node(rng, 3, nK, nF, plants), H.bow_node(rng, 900, nK, 20, plants[:4])]))
    return pairs


def _claim_pairs(rng):
    """a tied best whose earlier feature is already claimed by an earlier KF feature (in chunk 0 and in chunk 1)"""
    plants = [
        ("K", 0, 3, 4),      # KF 0 -> F 3 at 4: claims F 3
        ("K", 1, 3, 6), (1, 20, 6),   # KF 1: F 3 and F 20 at 6, F 3 taken -> F 20
        ("K", 2, 18, 4),     # KF 2 claims F 18 (chunk 1)
        ("K", 3, 18, 7), (3, 35, 7),  # KF 3: F 18 taken -> F 35
        ("K", 4, 5, 10), (4, 6, 10),  # KF 4: plain tie in chunk 0
    ]
    pairs = [_pair(rng, [H.bow_node(rng, 7, 6, 40, plants, shuffle=False)]),
             _pair(rng, [H.bow_node(rng, 7, 6, 40, plants), H.bow_node(rng, 8, 5, 24, plants[:3])])]
    return pairs


def _th_ratio_pairs(rng, ratio):
    """best at TH_LOW - 1 / TH_LOW / TH_LOW + 1 with a far second; ratio edge pairs (best, second) planted in list order"""
    edges = H.RATIO_EDGES.get(ratio, [(5, 9), (7, 7)])
    plants = [(0, 0, 49), (1, 1, 50), (2, 2, 51)]
    for k, (b, s) in enumerate(edges + [(3, 6), (2, 4)]):
        plants += [(3 + k, 3 + 2 * k, s), (3 + k, 4 + 2 * k, b)]
    nK = 3 + len(edges) + 2
    return [_pair(rng, [H.bow_node(rng, 40, nK, 30, plants)]),
            _pair(rng, [H.bow_node(rng, 40, nK, 30, plants, shuffle=False), H.bow_node(rng, 41, 3, 3, [(0, 0, 50)])])]


def _invalid_pairs(rng):
    """the best F feature / the KF feature marked invalid (no good MapPoint) on either side"""
    plants = [(0, 0, 5), (0, 1, 9), (1, 2, 5), (1, 3, 20), (2, 4, 6), (2, 5, 30)]
    kf, f = _pair(rng, [H.bow_node(rng, 2, 3, 8, plants, shuffle=False)])
    vK = np.array([1, 0, 1], np.uint8)
    vF = np.array([0, 1, 1, 1, 0, 1, 1, 1], np.uint8)
    return [((kf[0], vK, kf[2], kf[3]), (f[0], vF, f[2], f[3]))]


@pytest.mark.parametrize("ratio,kf_kf", [(0.6, False), (0.8, True), (0.6, True), (0.8, False), (1.5, False), (1.5, True)])
def test_search_by_bow_edges(oracle, mts, ratio, kf_kf):
    rng = np.random.default_rng(int(ratio * 10) + kf_kf)
    mt = mts[0]
    pairs = _chunk_tie_pairs(rng) + _claim_pairs(rng) + _th_ratio_pairs(rng, ratio) + _invalid_pairs(rng)
    for ori in (False, True):
        refs = check_bow(oracle, mt, pairs, ratio, 50, kf_kf, ori)
    assert sum(r[1] for r in refs) > 20


def _many_nodes_pair(rng, nnodes, groups=None):
    """nnodes nodes, one KF and one F feature each at distance 5 (every node matches), rotations from `groups`"""
    nodes = [H.bow_node(rng, 3 * i + 1, 1, 1, [(0, 0, 5)], shuffle=False) for i in range(nnodes)]
    kf, f = _pair(rng, nodes)
    f = (f[0], f[1], kf[2].copy(), f[3])   # KF feature i <-> F feature i: rotation 0
    if groups is not None:
        aK, aF = _rotation_groups(groups)
        kf = (kf[0], kf[1], aK[:nnodes], kf[3])
        f = (f[0], f[1], aF[:nnodes], f[3])
    return kf, f


def test_search_by_bow_many_nodes_and_rotation_prune(oracle, mts):
    """more than 128 and more than 1000 KF nodes (k_search_by_bow_rows' grid-stride loop over 8 blocks x 16 rows), a KF
    node list that only partly overlaps the F one, and the two SearchByBoW prune kernels on the half-bin, 0.1 * max1 and
    equal-count histograms (more than 256 matches: several strides per thread)"""
    rng = np.random.default_rng(8)
    pairs = [_many_nodes_pair(rng, 129), _many_nodes_pair(rng, 1500)]
    for name in ROTATION_CASES:
        n = sum(c for c, _, _ in ROTATION_CASES[name])
        pairs.append(_many_nodes_pair(rng, n, ROTATION_CASES[name]))
    kf, f = pairs[1]   # drop every third F node: KF nodes without a partner
    nodeF, offF, idxF = f[3]
    keepn = np.arange(len(nodeF)) % 3 != 1
    lists = {int(nodeF[i]): list(idxF[offF[i]:offF[i + 1]]) for i in np.flatnonzero(keepn)}
    pairs.append((kf, (f[0], f[1], f[2], H.csr(lists))))
    for kf_kf in (False, True):
        refs = check_bow(oracle, mts[1], pairs, 0.6, 50, kf_kf, True)
        assert refs[0][1] == 129 and refs[1][1] == 1500 and refs[-1][1] == 1000
        assert [r[1] for r in refs[2:-1]] == list(ROTATION_KEPT.values())
    refs = check_bow(oracle, mts[1], pairs[:2], 0.6, 50, False, False)


def _ref_pin_bow_cases():
    """the first cases of test_ref_pin's SearchByBoW generator (proven equal to the compiled reference there), drawn in the
    same order: 40 + 20 (KeyFrame, Frame) cases of seeds 100 / 101, 20 (KeyFrame, KeyFrame) cases of seed 200"""
    from test_ref_pin import _bow_case
    out = []
    for seed, count, kf_kf in ((100, 40, False), (101, 20, False), (200, 20, True)):
        rng = np.random.default_rng(seed)
        for it in range(count):
            n1, n2 = int(rng.choice([0, 1, 7, 150, 1000])), int(rng.choice([0, 1, 9, 180, 1000]))
            (d1, v1, a1, fv1), (d2, v2, a2, fv2) = _bow_case(rng, n1, n2, int(rng.choice([1, 4, 30, 120])), 0.7 if kf_kf else 0.8,
                                                            it % 2)
            ratio = float(rng.choice([0.6, 0.75, 0.8, 0.9] if kf_kf else [0.6, 0.7, 0.75, 0.9, 1.0]))
            out.append(((d1, (v1 == 1).astype(np.uint8), a1, fv1), (d2, (v2 == 1).astype(np.uint8), a2, fv2), ratio, bool(it % 3), kf_kf))
    return out


def test_search_by_bow_ref_pin_cases(oracle, mts):
    total = 0
    for i, (kf, f, ratio, ori, kf_kf) in enumerate(_ref_pin_bow_cases()):
        refs = check_bow(oracle, mts[i % 2], [(kf, f)], ratio, 50, kf_kf, ori)
        total += refs[0][1]
    assert total > 500


# ------------------------------------------------------------------------------------------------ HammingCSR
def test_hamming_csr_lists(oracle, mts):
    """repeated candidates, ties whose runner-up owner (second_idx) depends on list order, empty lists at the start, in the
    middle and at the end; HammingCSR, HammingCSR2 (orbfe_hamming_csr_ex) and orbfe_hamming_csr_device"""
    import torch
    rng = np.random.default_rng(31)
    nq, nt = 300, 400
    q, t = H.random_rows(rng, nq), H.random_rows(rng, nt)
    free = iter(rng.permutation(nt))   # rows planted for one query are not rewritten for another
    lists = []
    for i in range(nq):
        kind = i % 8
        if kind in (1, 2, 3):
            a, b, c = next(free), next(free), next(free)
            t[a] = H.at_distance(rng, q[i], 5 + i % 9)
            t[b] = H.at_distance(rng, q[i], 5 + i % 9)
            t[c] = H.at_distance(rng, q[i], 7 + i % 9)
        else:
            a, b, c = (int(x) for x in rng.choice(nt, 3, replace=False))
        lists.append({0: [], 1: [a, b, c], 2: [b, a, c], 3: [c, b, a, b], 4: [a, a, a], 5: [a], 6: [c, a, c, b, c],
                      7: []}[kind] if i not in (0, nq - 1) else [])
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    cand = np.asarray([c for x in lists for c in x], np.uint32)
    ref = oracle.hamming_csr2(q, t, off, cand)
    assert ref[0][0] == -1 and ref[1][0] == 256 and ref[3][0] == -1
    for k, mt in mts.items():
        got = mt.HammingCSR(q, t, off, cand)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref[:3])), k
        got = mt.HammingCSR2(q, t, off, cand)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref)), k
        dq, dt, do, dc = _dev(q), _dev(t), _dev(off), _dev(cand)
        outs = [torch.full((nq,), -9, dtype=torch.int32, device="cuda") for _ in range(4)]
        rc = _lib().orbfe_hamming_csr_device(mt.handle, dq.data_ptr(), nq, dt.data_ptr(), do.data_ptr(), dc.data_ptr(),
                                             outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r), k
    # the order-dependent runner-up owners the lists were built for
    assert (ref[0][1], ref[3][1]) == tuple(lists[1][:2]) and (ref[0][2], ref[3][2]) == tuple(lists[2][:2])
    assert ref[1][4] == ref[2][4] and ref[3][4] == lists[4][0]

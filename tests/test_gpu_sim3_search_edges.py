"""The batched SearchBySim3 and the loop's SearchByProjection (csrc/orbfe_sim3_search.hip) at the edges its parity tests do not
reach: the second turn of the search's stride loop and the clamp of its grid, the 256-thread chunks of both compactions, qcap below
the live count, the member set at its smallest tables with planted probe chains, the three glue calls on their own, inputs the
host cannot reject, thresholds 0 and 255, scratch reuse and two handles on two streams, the largest block -- and every case of
tests/sim3_search_edge_cases.py, which tests/test_sim3_search_edge_cases.py shows to notice each rule of the oracle.  Bit for bit
against tests/sim3_search_oracle.py (and the compiled reference where it is built and the case can be given to it) or against a
few lines of numpy; every output starts as a sentinel with a guard band behind it."""
import numpy as np
import pytest

import fuse_oracle as FO
import proj_cases as PC
import sim3_search_checks as CK
import sim3_search_edge_cases as EC
import sim3_search_oracle as SO

pytestmark = pytest.mark.gpu

F = np.float32
rng_of = np.random.default_rng


@pytest.fixture(scope="module")
def mt():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m = ORBmatcher(0.9, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lc(mt):
    from orb_slam2_ssd_semantic_amd import LoopCloser
    return LoopCloser(mt)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _live(ks, ko, T_to, already, th=7.5):
    """the slots of ks that leave k_s3_gate as queries, in slot order"""
    T_own = SO.pose34(ks)
    wp = np.asarray(ks["world_pos"], F).reshape(-1, 3)
    return np.array([i for i in range(len(ks["octave"])) if ks["state"][i] == 1 and not already[i] and
                     SO.gate_point(T_own, T_to, ko["K"], ko["bounds"], th, ko["scale_factors"], ko["log_scale"], wp[i], ks["min_dist"][i],
                                   ks["max_dist"][i]) is not None], np.int64)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", sorted(EC.table()))
def test_table_case(lc, name):
    c = EC.table()[name]
    if c["kind"] == "sim3":
        n2 = len(c["k2"]["octave"])
        CK.check_sim3_single(lc, c["k1"], c["k2"], c["sim"], c["m_in"], cap=max(len(c["k1"]["octave"]), n2) + 3, th=c["th"], th_high=c["th_high"],
                             ref=not (c["m_in"] >= n2).any())
    elif c["ids"] is None:
        for how in ("device", "host"):
            CK.check_proj(lc, c["kf"], c["Scw"], c["pts"], c["m_in"], cap=len(c["kf"]["octave"]) + 3, th=c["th"], th_low=c["th_low"], list_skip=how)
    else:   # a point twice in a list: the list names the first entry's row of the table for both
        cap = len(c["kf"]["octave"]) + 3
        got, nm, status = CK.proj_raw(lc, [c["kf"]], [c["Scw"]], c["pts"], [c["ids"]], [c["m_in"]], cap, c["th"], c["th_low"])()
        want, wn = EC.run(c)
        assert status[0] == 0 and nm[0] == wn and np.array_equal(got[0], CK.pad(want, cap))


# ------------------------------------------------------------------------------------------------ the stride loop of k_s3_search
def test_stride_loop_takes_a_second_turn(lc):
    """cap = 1000 gives 128 workgroups = 512 waves per (pair, direction); more than 512 live queries in direction 0"""
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9500), 1000, 900)
    T12, T21 = CK.poses(s, R, t)
    live = _live(k1, k2, T21, m_in != -1)
    _, _, v1, _ = CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in)
    assert len(v1) == 1000 and len(live) > 512
    late = live[512:]
    assert (v1[late] >= 0).sum() >= 20   # accepted vnMatch1 entries whose query the second turn searched


@pytest.mark.parametrize("cap", [508, 512, 516])
def test_search_grid_around_its_clamp(lc, cap):
    """(cap + 3) / 4 = 127, 128, 129 -> 127, 128 and the clamped 128 workgroups"""
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9510), 40, 37)
    _, nf, _, _ = CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=cap)
    assert nf > 2


# ------------------------------------------------------------------------------------------------ the chunks of k_s3_gate
@pytest.mark.parametrize("shape", [(255, 257), (256, 513), (257, 512), (512, 256), (513, 255)])
def test_feature_counts_on_the_chunk_edges(lc, shape):
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9520 + shape[0]), *shape)
    _, nf, _, _ = CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=max(shape) + (0 if shape[0] == 512 else 3))
    assert nf > 20


@pytest.mark.parametrize("how", ["null", "bad", "preset"])
def test_a_middle_chunk_without_a_live_slot(lc, how):
    """slots 256 .. 511 of both keyframes hold no query: the compaction's base passes an empty chunk between two live ones"""
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9530), 700, 640)
    k1, k2, m_in = dict(k1), dict(k2), m_in.copy()
    for k in (k1, k2):
        k["state"] = k["state"].copy()
    if how == "preset":   # feature i of keyframe 1 is matched to feature i of keyframe 2: neither asks
        m_in[256:512] = np.arange(256, 512)
        k2["state"][256:512] = 1   # a preset match is a point keyframe 2 really has
    else:
        k1["state"][256:512] = k2["state"][256:512] = 0 if how == "null" else 2
        m_in[(m_in >= 256) & (m_in < 512)] = -1
    T12, T21 = CK.poses(s, R, t)
    a2 = np.zeros(640, bool)
    a2[m_in[(m_in >= 0) & (m_in < 640)]] = True
    l1, l2 = _live(k1, k2, T21, m_in != -1), _live(k2, k1, T12, a2)
    for lv in (l1, l2):
        assert (lv < 256).any() and (lv >= 512).any() and not ((lv >= 256) & (lv < 512)).any()
    _, nf, _, _ = CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=703)
    assert nf > 20


def test_a_first_chunk_that_is_entirely_live(lc):
    """all of slots 0 .. 255 of keyframe 1 pass the gate: trk_compact_pos returns tot == 256"""
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9540), 520, 400)
    T12, T21 = CK.poses(s, R, t)
    k1, m_in = dict(k1), m_in.copy()
    for key in ("state", "world_pos", "min_dist", "max_dist"):
        k1[key] = np.array(k1[key]).copy()
    k1["state"][:256], m_in[:256] = 1, -1
    ok = _live(k1, k2, T21, np.zeros(520, bool))
    donors = ok[ok >= 256]
    for n, i in enumerate(np.setdiff1d(np.arange(256), ok)):   # a slot the gate stops takes the point of one it lets through
        for key in ("world_pos", "min_dist", "max_dist"):
            k1[key][i] = k1[key][donors[n]]
    live = _live(k1, k2, T21, m_in != -1)
    assert np.array_equal(live[:256], np.arange(256)) and len(live) > 300
    CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=523)


def test_bit_table_words_and_last_bit(lc):
    """vbAlreadyMatched2 as bits in LDS: presets on bits 31 and 32 of word 0 / 1, 63 / 64, the last bit below n2, and n2 itself"""
    n1, n2 = 120, 97
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9550), n1, n2)
    k2, m_in = dict(k2), np.full(n1, -1, np.int32)
    k2["state"] = k2["state"].copy()
    marks = [31, 32, 63, 64, n2 - 1, n2]
    k2["state"][marks[:-1]] = 1
    k2["state"][[30, 33, 62, 65, n2 - 2]] = 1   # their neighbours stay live
    m_in[np.arange(len(marks)) * 7 + 3] = marks
    T12, T21 = CK.poses(s, R, t)
    a2 = np.zeros(n2, bool)
    a2[marks[:-1]] = True
    live2 = _live(k2, k1, T12, a2)
    assert not np.isin(marks[:-1], live2).any() and np.isin([30, 33, 62, 65], live2).sum() >= 3
    CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=n1 + 8, ref=False)   # an index >= N2 is not the mock's to take
    m_in[m_in == n2] = -2
    CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=n1 + 8)


# ------------------------------------------------------------------------------------------------ the chunks of k_ps3_gate, qcap
LIST_LENGTHS = (0, 1, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def list_cases():
    return [PC.kf_sim3_case(rng_of(9560 + n), 200, n) for n in LIST_LENGTHS]


@pytest.mark.parametrize("k", range(len(LIST_LENGTHS)))
def test_list_lengths_on_the_chunk_edges(lc, list_cases, k):
    _, nm = CK.check_proj(lc, *list_cases[k], cap=203)
    assert nm > 10 or LIST_LENGTHS[k] < 255


def test_list_lengths_mixed_in_one_batch(lc, list_cases):
    order = [5, 0, 2, 1, 4, 3]
    cases = [list_cases[k] for k in order]
    out, status = lc.search_by_projection_sim3_pairs_device(cases, 10, cap=203)
    assert status[0] == 0
    for (kf, Scw, pts, m_in), (got, nm) in zip(cases, out):
        want, wn = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
        assert np.array_equal(got, want) and nm == wn


def test_entry_buffer_protocol_on_the_longest_list(lc, list_cases):
    kf, Scw, pts, m_in = list_cases[5]
    want, wn = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
    out, status = lc.search_by_projection_sim3_pairs_device([list_cases[5]], 10, ent_cap=0)
    need = int(status[0])
    assert need > 0 and out[0][1] == 0 and np.array_equal(out[0][0], m_in)
    out, status = lc.search_by_projection_sim3_pairs_device([list_cases[5]], 10, ent_cap=need - 1)
    assert status[0] == need and out[0][1] == 0 and np.array_equal(out[0][0], m_in)
    out, status = lc.search_by_projection_sim3_pairs_device([list_cases[5]], 10, ent_cap=need)
    assert status[0] == 0 and out[0][1] == wn and np.array_equal(out[0][0], want)


def test_qcap_below_the_live_count_drops_the_later_queries(lc):
    kf, Scw, pts, m_in = PC.kf_sim3_case(rng_of(9570), 300, 400)
    T, Ow = FO.decompose_sim3(Scw)
    found = set(int(v) for v in m_in if v >= 0)
    nlive = sum(1 for i in range(400) if not pts["bad"][i] and i not in found and
                FO.gate_point(T, Ow, kf["K"], kf["bounds"], 10, kf["scale_factors"], kf["log_scale"], pts["world_pos"][i], pts["normal"][i],
                              pts["min_dist"][i], pts["max_dist"][i], False) is not None)
    assert nlive > 257   # the cut falls in the second chunk
    full, nfull = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
    seen = []
    for qcap in (nlive, nlive - 1, 256, 1):
        want, wn = CK.proj_lists_oracle(kf, Scw, pts, np.arange(400), m_in, qcap=qcap)
        out, status = lc.search_by_projection_sim3_pairs_device([(kf, Scw, pts, m_in)], 10, cap=303, qcap=qcap)
        assert status[0] == 0 and out[0][1] == wn and np.array_equal(out[0][0], want), qcap
        seen.append(wn)
    assert seen[0] == nfull and np.array_equal(CK.proj_lists_oracle(kf, Scw, pts, np.arange(400), m_in, qcap=nlive)[0], full)
    assert seen[3] <= 1 and seen[2] < seen[0]


# ------------------------------------------------------------------------------------------------ the member set
HASH_MUL = 2654435761


def _member_hash(v, lg):
    return ((int(v) * HASH_MUL) & 0xFFFFFFFF) >> (32 - lg)


def _member_lg(cap):
    lg = 6
    while (1 << lg) < 2 * cap:
        lg += 1
    return lg


def _planted_row(cap, rng, dup=True):
    """a row of `cap` entries and the values to look up: three values whose home is the last place (the probe wraps to 0 and 1), one
    of them twice in a row, the value 0 (home 0, inside that chain), non-members whose home is the last place and place 0"""
    lg = _member_lg(cap)
    H = 1 << lg
    last = [v for v in range(1, 400000) if _member_hash(v, lg) == H - 1]
    first = [v for v in range(1, 400000) if _member_hash(v, lg) == 0]
    members = last[:3] + ([last[2]] if dup else []) + [0] if cap >= 5 else last[:cap]
    pool = [int(v) for v in rng.permutation(1 << 20)[:cap + 8] + 1 if v not in last[:8] and v not in first[:8]]
    row = np.array((members + pool)[:cap], np.int32)
    if cap == 33:
        row[20:] = -1   # a row that is mostly empty
    row[5:] = rng.permutation(row[5:])
    # the wrap, shown before anything goes to the device: insert in row order as the kernel's loop would on one thread
    table = [-1] * H
    for v in row[row >= 0]:
        h = _member_hash(v, lg)
        while table[h] not in (-1, int(v)):
            h = (h + 1) & (H - 1)
        table[h] = int(v)
    if cap >= 3:
        assert table[H - 1] in last[:3] and table[0] in last[:3] + [0] and table[1] in last[:3] + [0]
        assert sum(1 for v in table[:4] if v in last[:3]) == 2   # two of the three were pushed past the end
    else:
        assert table[H - 1] == last[0]
    assert sum(1 for v in table if v != -1) <= H // 2
    strangers = last[3:6] + first[:3] + [pool[-1], 1 << 30]
    assert not np.isin(strangers, row).any()
    return row, np.array(list(row[row >= 0][:40]) + strangers + [0, -1, -2], np.int32), table


@pytest.mark.parametrize("cap", [1, 31, 32, 33, 15360])
def test_member_set_tables_and_probe_chains(lc, cap):
    import torch
    rng = rng_of(9580 + cap)
    row0, look, table = _planted_row(cap, rng, dup=cap != 32)
    if cap == 32:   # 32 distinct values in 64 places: the table half full, the documented worst case
        assert len(set(row0)) == 32 and (row0 >= 0).all() and sum(1 for v in table if v != -1) == 32 and len(table) == 64
    elif cap > 1:
        assert len(set(row0[row0 >= 0])) == (row0 >= 0).sum() - 1
    rows = np.stack([row0, np.full(cap, -1, np.int32)])
    rows[1, :1] = look[0]
    lists = [look, np.zeros(0, np.int32), look[::-1].copy(), look[:7], look[:5]]
    pair_row = np.array([0, 1, 0, 1, 2], np.int32)                          # the last pair names a row that is not there
    ne = sum(len(x) for x in lists)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    off[-1] += 100                                                          # runs past nentries: clamped
    idx = np.concatenate(lists).astype(np.int32)
    d_rows, d_pr, d_off, d_idx = _dev(rows), _dev(pair_row), _dev(off.view(np.int32)), _dev(idx)
    d_skip = torch.full((ne + 256,), 9, dtype=torch.uint8, device="cuda")
    lc.mark_list_members_device(d_rows.data_ptr(), 2, cap, d_pr.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), ne, len(lists), d_skip.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_skip.cpu().numpy()
    want = np.concatenate([np.isin(x, rows[r][rows[r] >= 0]) & (np.asarray(x) >= 0) if r < 2 else np.zeros(len(x), bool)
                           for x, r in zip(lists, pair_row)]).astype(np.uint8)
    assert np.array_equal(got[:ne], want) and (got[ne:] == 9).all()
    n_in = int((row0[row0 >= 0][:40] >= 0).sum())
    assert want[:n_in].all() and not want[n_in:n_in + 8].any() and want[len(look) + len(look) - 1] == 1


# ------------------------------------------------------------------------------------------------ the glue calls, one by one
def test_invert_matches_alone(lc):
    import torch
    rng = rng_of(9590)
    cap, nkf = 300, 3
    d_n = np.array([280, -5, 400], np.int32)
    kf2 = np.array([0, 1, 2, 7, -1, 0], np.int32)
    P = len(kf2)
    bow = rng.integers(-2, cap + 40, (P, cap)).astype(np.int32)
    bow[rng.random((P, cap)) < 0.5] = -1
    bow[0, :6] = [-1, -2, cap, cap + 1, 290, 299]          # none, another, >= cap, >= n1 but < cap (kept: the row is cap wide)
    bow[0, 6:][np.isin(bow[0, 6:], [290, 299])] = -1
    bow[5] = -1
    bow[5, [3, 200, 279, 280, 299]] = [17, 17, 4, 5, 6]    # one keyframe-1 feature from two sides: the later wins; i >= n2 is not read
    want = np.full((P, cap), -1, np.int32)
    for p in range(P):
        if 0 <= kf2[p] < nkf:
            for i in range(min(max(int(d_n[kf2[p]]), 0), cap)):
                j = bow[p, i]
                if 0 <= j < cap:
                    want[p, j] = max(want[p, j], i)
    d_out = torch.full((P * cap + 64,), -77, dtype=torch.int32, device="cuda")
    t = [_dev(bow), _dev(kf2), _dev(d_n)]
    lc.InvertMatches_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), nkf, cap, P, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:P * cap].reshape(P, cap), want) and (got[P * cap:] == -77).all()
    assert (want[1] == -1).all() and (want[3] == -1).all() and (want[4] == -1).all() and want[5, 17] == 200 and (want[5] >= 0).sum() == 2
    assert (want[2] >= 0).sum() > 100 and want[0, 299] == 5 and want[0, 290] == 4


def _to_camera(T, W):
    """orbfe_sim3_prepare_device's arithmetic: ((r0 * x + r1 * y) + r2 * z) + t in float, as the chain test restates it"""
    T = np.asarray(T, F).reshape(3, 4)
    W = np.asarray(W, F).reshape(-1, 3)
    return np.stack([((T[c, 0] * W[:, 0] + T[c, 1] * W[:, 1]) + T[c, 2] * W[:, 2]) + T[c, 3] for c in range(3)], 1).astype(F)


def test_correspondences_alone(lc, mt):
    import torch
    from orb_slam2_ssd_semantic_amd import OrbfeError, _ffi, loopclosing, tracking
    rng = rng_of(9591)
    cap, nkf, nlevels, npts = 300, 4, 8, 1000
    ns = np.array([300, 290, 300, 260], np.int32)
    kfs = [dict(xy=rng.uniform(0, 600, (n, 2)).astype(F), octave=rng.integers(0, nlevels, n).astype(np.int32), desc=np.zeros((n, 32), np.uint8))
           for n in ns]
    kfs[3]["octave"][::9] = -1
    kfs[3]["octave"][4::9] = nlevels
    blk, desc, _, _ = loopclosing._keyframe_block(kfs, cap)
    slot = np.full((nkf, cap), -1, np.int32)
    for r in range(nkf):
        slot[r, :ns[r]] = rng.permutation(npts)[:ns[r]]
    slot[3, 1::7], slot[3, 2::7], slot[2, 5::11] = -1, npts, npts + 3
    bad = (rng.random(npts) < 0.05).astype(np.uint8)
    bad[slot[0, :300]] = 0
    bad[slot[1, :290]] = 0
    wp = rng.normal(0, 3, (npts, 3)).astype(F)
    Tcw = np.stack([np.concatenate([PC._rot(rng, 20.0), rng.normal(0, 1, (3, 1))], 1).reshape(12) for _ in range(nkf)]).astype(F)
    sigma2 = (PC.scale_factors() ** 2).astype(F)
    pairs = np.array([(0, 1), (1, 0), (0, 1), (0, 1), (2, 3), (3, 2), (0, 9), (-1, 1), (2, 2)], np.int32)
    P = len(pairs)
    m12 = np.full((P, cap), -1, np.int32)
    m12[0, rng.permutation(290)[:255]] = 7                                  # 255 correspondences, all to feature 7
    for p, cnt in ((2, 256), (3, 257)):                                     # pair 1 has none: the offsets repeat
        sel = np.sort(rng.permutation(290)[:cnt])
        m12[p, sel] = rng.permutation(290)[:cnt]
    for p in (4, 5, 6, 7, 8):
        m12[p] = rng.integers(-2, 310, cap)
    m12[4, :4] = [260, 299, 259, 0]                                         # >= n2, >= n2, the last one below it, the first
    idx1, X1, X2, s1, s2, offs = [], [], [], [], [], [0]
    for p, (a, b) in enumerate(pairs):
        if 0 <= a < nkf and 0 <= b < nkf:
            for i1 in range(ns[a]):
                j = m12[p, i1]
                if not 0 <= j < ns[b]:
                    continue
                mp1, mp2, o1, o2 = slot[a, i1], slot[b, j], kfs[a]["octave"][i1], kfs[b]["octave"][j]
                if not (0 <= mp1 < npts and 0 <= mp2 < npts and 0 <= o1 < nlevels and 0 <= o2 < nlevels) or bad[mp1] or bad[mp2]:
                    continue
                idx1.append(i1)
                X1.append(_to_camera(Tcw[a], wp[mp1])[0])
                X2.append(_to_camera(Tcw[b], wp[mp2])[0])
                s1.append(sigma2[o1])
                s2.append(sigma2[o2])
        offs.append(len(idx1))
    counts = np.diff(offs)
    assert list(counts[:4]) == [255, 0, 256, 257] and 0 < counts[4] < 200 and 0 < counts[5] and counts[6] == counts[7] == 0 and counts[8] > 0
    n = offs[-1]
    corr_cap = P * cap
    st = torch.cuda.current_stream().cuda_stream
    d = dict(kps=_dev(blk.view(np.uint8).reshape(nkf, cap, -1)), desc=_dev(desc), n=_dev(ns), slot=_dev(slot), Tcw=_dev(Tcw), wp=_dev(wp), bad=_dev(bad),
             k1=_dev(pairs[:, 0].copy()), k2=_dev(pairs[:, 1].copy()), m12=_dev(m12), dummy=torch.zeros((nkf, 64 * 48 + 1), dtype=torch.int32, device="cuda"))
    frames = tracking.frames_struct(d["kps"], d["desc"], d["n"], cap, d["dummy"], d["dummy"], 0.0, 0.0, 0.1, 0.1)
    tmap = _ffi.TrackMap(d["wp"].data_ptr(), None, None, None, d["bad"].data_ptr(), None, None, npts)

    def outputs():
        f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
        return dict(off=torch.full((P + 1 + 64,), -77, **i32), X1=torch.full((corr_cap * 3 + 64,), -7.0, **f32), X2=torch.full((corr_cap * 3 + 64,), -7.0, **f32),
                    s1=torch.full((corr_cap + 64,), -7.0, **f32), s2=torch.full((corr_cap + 64,), -7.0, **f32), idx1=torch.full((corr_cap + 64,), -77, **i32))

    def call(o, npairs, cc):
        lc.Sim3Correspondences_device(frames, nkf, d["Tcw"].data_ptr(), d["slot"].data_ptr(), tmap, d["k1"].data_ptr(), d["k2"].data_ptr(), npairs,
                                      d["m12"].data_ptr(), sigma2, cc, o["off"].data_ptr(), o["X1"].data_ptr(), o["X2"].data_ptr(), o["s1"].data_ptr(),
                                      o["s2"].data_ptr(), o["idx1"].data_ptr(), st)
    o = outputs()
    with pytest.raises(OrbfeError) as e:     # corr_cap one short of npairs * cap: refused before any launch
        call(o, P, corr_cap - 1)
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == (-7.0 if v.dtype == torch.float32 else -77)).all() for v in o.values())
    call(o, P, corr_cap)                     # the handle is usable afterwards
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in o.items()}
    assert np.array_equal(g["off"][:P + 1], np.array(offs, np.int32)) and (g["off"][P + 1:] == -77).all()
    assert np.array_equal(g["idx1"][:n], np.array(idx1, np.int32)) and (g["idx1"][n:] == -77).all()
    assert np.array_equal(g["X1"][:3 * n].view(np.uint32), np.array(X1, F).reshape(-1).view(np.uint32)) and (g["X1"][3 * n:] == -7).all()
    assert np.array_equal(g["X2"][:3 * n].view(np.uint32), np.array(X2, F).reshape(-1).view(np.uint32)) and (g["X2"][3 * n:] == -7).all()
    assert np.array_equal(g["s1"][:n], np.array(s1, F)) and (g["s1"][n:] == -7).all()
    assert np.array_equal(g["s2"][:n], np.array(s2, F)) and (g["s2"][n:] == -7).all()
    o = outputs()
    call(o, 0, 0)                            # no pair: offsets[0] = 0 and nothing else
    torch.cuda.synchronize()
    off = o["off"].cpu().numpy()
    assert off[0] == 0 and (off[1:] == -77).all() and (o["idx1"].cpu().numpy() == -77).all()


@pytest.mark.parametrize("npairs,cap", [(1, 255), (1, 256), (1, 257), (3, 85), (5, 103)])
def test_keep_inliers_alone(lc, npairs, cap):
    import torch
    rng = rng_of(9592 + cap)
    n = npairs * cap
    m12 = rng.integers(-2, cap, n + 64).astype(np.int32)
    mask = (rng.random(n + 64) < 0.5).astype(np.uint8)
    mask[0], mask[n - 1], mask[n:] = 0, 1, 0
    m12[[0, n - 1]] = 5
    d_m, d_k = _dev(m12), _dev(mask)
    lc.KeepInliers_device(d_k.data_ptr(), cap, npairs, d_m.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_m.cpu().numpy()
    assert np.array_equal(got[:n], np.where(mask[:n] != 0, m12[:n], -1)) and np.array_equal(got[n:], m12[n:])   # the band behind keeps its values
    assert got[0] == -1 and got[n - 1] == 5


# ------------------------------------------------------------------------------------------------ inputs the host cannot reject
def test_sim3_rows_slots_and_counts_out_of_range(lc):
    """each is range-checked in the kernels (s3_pair_ok, s3_count, mp >= 0 && mp < npoints): nothing found, the row untouched"""
    rng = rng_of(9593)
    A, B, s, R, t, mAB = PC.sim3_pair_case(rng, 130, 150)
    C, _, _, _, _, _ = PC.sim3_pair_case(rng, 90, 5)
    cap = 153
    sim = (s, R, t)
    kfs = [A, B, C, A]
    pairs = [(0, 1), (0, 4), (-1, 1), (2, 1), (3, 1), (0, 1), (0, 1)]
    skip = np.array([0, 0, 0, 0, 0, 1, 0], np.uint8)
    rows = [mAB, mAB, mAB, np.full(90, -1, np.int32), mAB, mAB, np.full(cap, -2, np.int32)]
    gone = np.flatnonzero(A["state"] == 1)[[0, 3, 17, 40, 60]]

    def slot_edit(slot, base):
        npts = int(base[-1])
        slot[3, gone] = [npts, npts + 5, -3, 2 ** 31 - 1, -2 ** 31]
    # keyframe 2 is told a negative count, keyframe 1 (B) one above cap; pair 5 is skipped AND has all-zero poses
    n_device = np.array([130, cap + 50, -4, 130], np.int32)
    mo, nf, v1, v2 = CK.sim3_raw(lc, kfs, pairs, [sim] * 7, rows, cap, slot_edit=slot_edit, n_device=n_device, pair_skip=skip, T_zero=(5,))()
    wo, wn, w1, w2 = CK.oracle_sim3(A, B, sim, 7.5, mAB)
    assert wn > 5
    assert nf[0] == wn and np.array_equal(mo[0], CK.pad(wo, cap)) and np.array_equal(v1[0], CK.pad(w1, cap)) and np.array_equal(v2[0], CK.pad(w2, cap))
    for p in (1, 2, 3, 5):   # a row past the block, a negative row, a keyframe with a negative count, a skipped pair
        assert nf[p] == 0 and np.array_equal(mo[p], CK.pad(rows[p], cap)) and (v1[p] == -1).all() and (v2[p] == -1).all(), p
    A2 = dict(A, state=A["state"].copy())
    A2["state"][gone] = 0    # a slot whose map index is outside the map is an empty slot
    wo, wn, w1, w2 = CK.oracle_sim3(A2, B, sim, 7.5, mAB)
    assert nf[4] == wn and np.array_equal(mo[4], CK.pad(wo, cap)) and np.array_equal(v1[4], CK.pad(w1, cap)) and np.array_equal(v2[4], CK.pad(w2, cap))
    assert nf[6] == 0 and (mo[6] == -2).all() and (v1[6] == -1).all()   # every feature of keyframe 1 already matched, to nothing in keyframe 2


def test_projection_list_indices_out_of_range(lc):
    """k_ps3_gate tests idx against [0, npoints) before it reads the map; the member set takes any non-negative value"""
    kf, Scw, pts, m_in = PC.kf_sim3_case(rng_of(9594), 150, 200)
    lst = np.arange(200, dtype=np.int64)
    lst = np.insert(lst, [0, 50, 50, 120, 200], [-1, 200, 2 ** 31 - 1, -2 ** 31, 205])
    lst = np.concatenate([lst, lst[60:70]])   # ten points a second time
    cap = 153
    got, nm, status = CK.proj_raw(lc, [kf], [Scw], pts, [lst], [m_in], cap)()
    want, wn = CK.proj_lists_oracle(kf, Scw, pts, lst, m_in)
    assert status[0] == 0 and nm[0] == wn and np.array_equal(got[0], CK.pad(want, cap)) and wn > 10


# ------------------------------------------------------------------------------------------------ state and streams
def test_scratch_grows_and_shrinks_without_leaking(lc):
    big = PC.sim3_pair_case(rng_of(9595), 600, 520)
    small = PC.sim3_pair_case(rng_of(9596), 30, 41)
    pbig, psmall = PC.kf_sim3_case(rng_of(9597), 300, 513), PC.kf_sim3_case(rng_of(9598), 20, 30)
    want = {}
    for name, c in (("big", big), ("small", small)):
        want[name] = CK.oracle_sim3(c[0], c[1], c[2:5], 7.5, c[5])
    for name, c in (("pbig", pbig), ("psmall", psmall)):
        want[name] = SO.search_by_projection_kf_sim3(*c, 10)

    def s3(name, c, cap):
        mo, nf, v1, v2 = lc.search_by_sim3_pairs_device([c[0], c[1]], [(0, 1)], [c[2:5]], 7.5, [c[5]], cap=cap)[0]
        wo, wn, w1, w2 = want[name]
        assert nf == wn and np.array_equal(mo, wo) and np.array_equal(v1, CK.pad(w1, cap)) and np.array_equal(v2, CK.pad(w2, cap)), name

    def pj(name, c, cap):
        got, nm = lc.search_by_projection_sim3_device(*c, 10, cap=cap)
        assert nm == want[name][1] and np.array_equal(got, want[name][0]), name
    s3("small", small, 45)
    s3("big", big, 603)
    s3("small", small, 45)      # fewer live queries than the scratch still holds
    pj("pbig", pbig, 303)
    pj("psmall", psmall, 45)
    s3("big", big, 603)
    s3("big", big, 603)         # the same batch twice
    pj("pbig", pbig, 303)
    pj("pbig", pbig, 303)
    s3("small", small, 700)     # a small pair in a block wider than the big one's
    assert want["big"][1] > 20 and want["pbig"][1] > 10


def test_two_handles_on_two_streams(lc):
    """SearchBySim3 and the projection call back to back on each of two streams, each stream with a matcher of its own, one
    synchronize: each result equals its single run"""
    import torch
    from orb_slam2_ssd_semantic_amd import LoopCloser, ORBmatcher
    mt2 = ORBmatcher(0.9, True)
    lc2 = LoopCloser(mt2)
    try:
        sa, sb = PC.sim3_pair_case(rng_of(9599), 260, 300), PC.sim3_pair_case(rng_of(9600), 300, 257)
        pa, pb = PC.kf_sim3_case(rng_of(9601), 200, 300), PC.kf_sim3_case(rng_of(9602), 256, 257)

        def enqueue(h, s, p, stream):
            return (CK.sim3_raw(h, [s[0], s[1]], [(0, 1)], [s[2:5]], [s[5]], 303, stream=stream),
                    CK.proj_raw(h, [p[0]], [p[1]], p[2], [np.arange(len(p[2]["bad"]))], [p[3]], 259, stream=stream))
        st1, st2 = torch.cuda.Stream(), torch.cuda.Stream()
        f = enqueue(lc, sa, pa, st1) + enqueue(lc2, sb, pb, st2)
        both = [g() for g in f]   # the first fetch synchronizes the device, the others find it idle
        alone = [g() for h, s, p in ((lc, sa, pa), (lc2, sb, pb)) for g in enqueue(h, s, p, None)]
        for x, y in zip(both, alone):
            assert all(np.array_equal(a, b) for a, b in zip(x, y))
        for (mo, nf, v1, v2), s in ((both[0], sa), (both[2], sb)):
            wo, wn, w1, w2 = CK.oracle_sim3(s[0], s[1], s[2:5], 7.5, s[5])
            assert nf[0] == wn > 20 and np.array_equal(mo[0], CK.pad(wo, 303)) and np.array_equal(v1[0], CK.pad(w1, 303)) and np.array_equal(v2[0], CK.pad(w2, 303))
        for (got, nm, status), p in ((both[1], pa), (both[3], pb)):
            want, wn = SO.search_by_projection_kf_sim3(*p, 10)
            assert status[0] == 0 and nm[0] == wn > 10 and np.array_equal(got[0], CK.pad(want, 259))
    finally:
        mt2.close()


# ------------------------------------------------------------------------------------------------ the largest block
def test_largest_block(lc):
    """cap = 15360: vn's initialisation, s_matched at its full size, the scratch at its widest row"""
    k1, k2, s, R, t, m_in = PC.sim3_pair_case(rng_of(9603), 300, 280)
    _, nf, v1, v2 = CK.check_sim3_single(lc, k1, k2, (s, R, t), m_in, cap=15360)
    assert nf > 20 and len(v1) == 15360 and (v1[300:] == -1).all() and (v2[280:] == -1).all()

"""Planted inputs for the device-resident tracker (csrc/orbfe_track.hip) at its frustum, pose, chunk and replay edges, with the
expected outputs from the oracles alone (tests/track_oracle.py, tests/proj_cases.py, oracle_ffi).  numpy only: no torch, no
GPU.  tests/test_track_edge_cases.py shows on the CPU that every table holds what it claims, tests/test_gpu_track_edges.py
feeds the tables to the kernels through tracking.Tracker.  Test support only.

The tables (the sizes 64 and 256 are the wave and the workgroup of the gating / replay kernels, 1024 the workgroup of the
unproject kernel):
  frustum_table()         every entry of track_oracle.frustum_cases() as three frames of one map-gate call (posed | empty | identity)
  map_gate_case()         nine frames with nine poses over one map of 600 points, lists of 0 .. 513 entries back to back
  qcap_last_case() ...    more queries than qcap, octaves outside [0, nlevels), counts outside [0, cap]
  unproject_stride_case() n = 1023 .. 2049 and 15360 with depth ties across index 1024 and on the selection boundary
  replay_case()           hand-built match / qsrc / nq rows: rotation histograms by chosen angles, twice-matched slots
  core_pool_case()        the search core's two pool layouts, rows shared between frames and rows outside the pool"""
import functools

import numpy as np

import proj_cases as PC
import proj_edge_cases as E
import track_oracle as TO
from oracle import oracle_ffi as O

F = np.float32
SF = PC.scale_factors()
WAVE, CHUNK = 64, 256


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ------------------------------------------------------------------------------------------------ the map gate's expectation
def gate_map_expect(poses, m, list_off, list_idx, seen, th, nentries=None, use_seen=True):
    """what orbfe_gate_local_map_batch_device leaves per frame, from TO.frustum with THAT frame's pose on the gathered points:
    dict(e0, e1, proj, in_view, q, src = positions in the list, qsrc = map point indices).  The list is cut at nentries; an
    index outside [0, npoints) makes no query and leaves level -1 / zeros, like a seen entry."""
    npts = len(m["bad"])
    ne = len(list_idx) if nentries is None else int(nentries)
    out = []
    for f, T in enumerate(poses):
        e1 = min(int(list_off[f + 1]), ne)
        e0 = min(int(list_off[f]), e1)
        idx = np.asarray(list_idx[e0:e1], np.int64)
        ok = (idx >= 0) & (idx < npts)
        g = np.where(ok, idx, 0)
        sn = np.zeros(e1 - e0, bool) if (seen is None or not use_seen) else np.asarray(seen[e0:e1]).astype(bool)
        proj, inv = TO.frustum(T, TO.K0, TO.BOUNDS0, m["world_pos"][g], m["normal"][g], m["min_dist"][g], m["max_dist"][g],
                               seen=(sn | ~ok).astype(np.uint8), bad=m["bad"][g])
        q, src = TO.queries_local_map(proj, inv, m["obs_gt0"][g], th, SF)
        out.append(dict(e0=e0, e1=e1, proj=proj, in_view=inv, q=q, src=src, qsrc=idx[src].astype(np.int32)))
    return out


# ------------------------------------------------------------------------------------------------ 1. the frustum table
THIRD_POSE = PC._pose(np.random.default_rng(77), 5.0, (-0.25, 0.1, 0.4))


@functools.lru_cache(maxsize=None)
def frustum_table():
    """TO.frustum_cases(), both members of every pair, as the points of one map (in the table's order) and three lists: the
    posed entries under TO._posed(), an empty list under a third pose, the identity entries under the identity.  th = 1, so a
    query's radius is RadiusByViewingCos * scale_factors[level] unscaled."""
    entries = [(name, k, c) for name, pair in TO.frustum_cases().items() for k, c in enumerate(pair)]
    ident = [i for i, (_, _, c) in enumerate(entries) if np.array_equal(c["T"], TO.IDENTITY)]
    posed = [i for i, (_, _, c) in enumerate(entries) if np.array_equal(c["T"], TO._posed())]
    assert len(ident) + len(posed) == len(entries) and ident and posed
    n = len(entries)
    m = dict(world_pos=np.stack([c["P"] for _, _, c in entries]).astype(F), normal=np.stack([c["Pn"] for _, _, c in entries]).astype(F),
             min_dist=np.array([c["min_dist"] for _, _, c in entries], F), max_dist=np.array([c["max_dist"] for _, _, c in entries], F),
             bad=np.array([c["bad"] for _, _, c in entries], np.uint8), obs_gt0=(np.arange(n) % 3 != 0).astype(np.uint8))
    list_idx = np.array(posed + ident, np.int32)
    list_off = np.array([0, len(posed), len(posed), n], np.uint32)
    seen = np.array([entries[i][2]["seen"] for i in list_idx], np.uint8)
    poses = [TO._posed(), THIRD_POSE, TO.IDENTITY.copy()]
    t = dict(entries=entries, poses=poses, map=m, list_off=list_off, list_idx=list_idx, seen=seen, th=1.0)
    t["want"] = gate_map_expect(poses, m, list_off, list_idx, seen, 1.0)
    return t


# ------------------------------------------------------------------------------------------------ 2. the map gate's lists
MAP_N = 600
GATE_LENGTHS = (1, 0, 65, 63, 257, 64, 255, 513, 256)        # in this order only the first list starts on a multiple of 64
GATE_RATES = (1.0, 0.0, 0.5, 0.5, 0.5, 1.0, 0.0, 0.5, 1.0)   # in view: about none, about all, about half
GATE_TH, GATE_QCAP = 3.0, 520
REJECT_KINDS = ("index -1", "index npoints", "seen", "out of view")


def _edge_map(rng, T, n):
    """n map points around pose T: every second one meant to be in view (inside the image, in range, seen head-on), the others
    with one reason to be rejected; a few bad"""
    pts = []
    for i in range(n):
        kw = dict(px=float(rng.uniform(60, 580)), py=float(rng.uniform(60, 420)), z=float(rng.uniform(0.6, 8.0)),
                  cos=float(rng.choice([0.7, 0.9, 0.9985, 1.0])), ratio=float(rng.uniform(1.1, 4.2)))
        if i % 2:
            why = int(rng.integers(0, 5))
            if why == 0:
                kw["z"] = -kw["z"]
            elif why == 1:
                kw["px"] += float(rng.choice([-1, 1])) * 900
            elif why == 2:
                kw["py"] += float(rng.choice([-1, 1])) * 700
            elif why == 3:
                kw["cos"] = float(rng.uniform(0.1, 0.4))
            else:
                kw["ratio"] = float(rng.uniform(0.5, 0.9))
        pts.append(TO._point_at(T, **kw))
    return dict(world_pos=np.stack([p["P"] for p in pts]).astype(F), normal=np.stack([p["Pn"] for p in pts]).astype(F),
                min_dist=np.array([p["min_dist"] for p in pts], F), max_dist=np.array([p["max_dist"] for p in pts], F),
                bad=(rng.random(n) < 0.04).astype(np.uint8), obs_gt0=(rng.random(n) < 0.8).astype(np.uint8))


def gate_boundaries(n):
    """the multiples of 64 (every fourth one a multiple of 256) that a list of n entries crosses: entries on both sides"""
    return list(range(WAVE, n, WAVE))


@functools.lru_cache(maxsize=None)
def map_gate_case():
    """one map, nine frames, nine poses.  Every list is a shuffled draw from the map (points repeat across frames and inside a
    list when the pool is short), laid out back to back.  Around every boundary b a list crosses, entries b - 2 and b + 1 are
    rejected (index -1, index npoints, seen, out of view in turn) and b - 1 and b accepted; `planted` records them."""
    rng = np.random.default_rng(4242)
    m = _edge_map(rng, TO._posed(), MAP_N)
    poses = [PC._pose(np.random.default_rng(200 + f), 4.0, (0.3 + 0.05 * f, -0.2 - 0.03 * f, 0.15 + 0.02 * f)) for f in range(len(GATE_LENGTHS))]
    idx_all, seen_all, planted, kind = [], [], [], 0
    for f, (n, rate) in enumerate(zip(GATE_LENGTHS, GATE_RATES)):
        _, inv = TO.frustum(poses[f], TO.K0, TO.BOUNDS0, m["world_pos"], m["normal"], m["min_dist"], m["max_dist"], bad=m["bad"])
        pin, pout = np.flatnonzero(inv), np.flatnonzero(inv == 0)
        assert len(pin) > 100 and len(pout) > 100, (f, len(pin), len(pout))
        nin = int(round(n * rate))
        pick = np.concatenate([rng.choice(pin, nin, replace=nin > len(pin)), rng.choice(pout, n - nin, replace=n - nin > len(pout))]).astype(np.int32)
        rng.shuffle(pick)
        sn = np.zeros(n, np.uint8)
        if rate > 0:
            sn[rng.random(n) < 0.04] = 1
            for b in gate_boundaries(n):
                for e, accept in ((b - 2, False), (b - 1, True), (b, True), (b + 1, False)):
                    if e >= n:
                        continue
                    sn[e] = 0
                    if accept:
                        pick[e] = rng.choice(pin)
                        continue
                    what = REJECT_KINDS[kind % len(REJECT_KINDS)]
                    kind += 1
                    pick[e] = {"index -1": -1, "index npoints": MAP_N, "seen": rng.choice(pin), "out of view": rng.choice(pout)}[what]
                    sn[e] = what == "seen"
                    planted.append((f, e, what))
        else:
            for e, v in ((0, -1), (n - 1, MAP_N)):
                if n > 1:
                    pick[e] = v
                    planted.append((f, e, "index -1" if v < 0 else "index npoints"))
        idx_all.append(pick)
        seen_all.append(sn)
    list_idx = np.concatenate(idx_all).astype(np.int32)
    list_off = np.concatenate([[0], np.cumsum(GATE_LENGTHS)]).astype(np.uint32)
    c = dict(poses=poses, map=m, list_off=list_off, list_idx=list_idx, seen=np.concatenate(seen_all), th=GATE_TH, qcap=GATE_QCAP, planted=planted)
    c["cut"] = int(list_off[7]) + 200   # nentries of the cut call: inside frame 7's list, before frame 8's
    _frozen(list_idx, list_off, c["seen"], *m.values())
    return c


@functools.lru_cache(maxsize=None)
def map_gate_want(variant):
    """the expectation of one run: 'full', 'no-seen' (d_seen = NULL) or 'cut' (nentries below the last offsets)"""
    c = map_gate_case()
    return gate_map_expect(c["poses"], c["map"], c["list_off"], c["list_idx"], c["seen"], c["th"],
                           nentries=c["cut"] if variant == "cut" else None, use_seen=variant != "no-seen")


# ------------------------------------------------------------------------------------------------ 3. qcap, octaves
QCAPS = (1, 64, 255, 256)
LAST_TH = 15.0


def gate_last_expect(pairs, th=LAST_TH, mono=False, n_eff=None, octave_key="octave"):
    """per frame (queries, sources) of the last-frame gate from orc_proj_queries_last_frame on the first n_eff[f] features"""
    out = []
    for f, (cur, la) in enumerate(pairs):
        n = len(la["octave"]) if n_eff is None else n_eff[f]
        wq, wv = O.proj_queries_last_frame(cur["Tcw"], la["Tcw"], cur["K"], cur["bounds"], cur["scale_factors"], la["has_mp"][:n], la["outlier"][:n],
                                           la["world_pos"][:n], la[octave_key][:n], la["obs_gt0"][:n], th, mono)
        sel = np.flatnonzero(wv)
        out.append((wq[sel], sel.astype(np.int32)))
    return out


def _all_valid(last, rate=1):
    n = len(last["octave"])
    last["has_mp"], last["outlier"] = np.full(n, rate, np.uint8), np.zeros(n, np.uint8)
    return last


@functools.lru_cache(maxsize=None)
def qcap_last_case():
    """four (cur, last) pairs: about 294 queries, about 38, none, about 294 -- above every qcap of QCAPS, below 64 / 255 / 256,
    below 1; the last frame's overflow would land in the guard band, the first one's in the second frame's row"""
    rng = np.random.default_rng(808)
    pairs = []
    for nL, motion, rate in ((300, "small", 1), (40, "forward", 1), (20, "small", 0), (300, "backward", 1)):
        cur, last = PC.last_frame_case(rng, 64, nL, motion)
        pairs.append((cur, _all_valid(last, rate)))
    return pairs, gate_last_expect(pairs)


@functools.lru_cache(maxsize=None)
def qcap_map_case():
    """one list of 400 entries, 330 of them in view under the frame's pose"""
    c = map_gate_case()
    rng = np.random.default_rng(909)
    T, m = c["poses"][8], c["map"]
    _, inv = TO.frustum(T, TO.K0, TO.BOUNDS0, m["world_pos"], m["normal"], m["min_dist"], m["max_dist"], bad=m["bad"])
    pick = np.concatenate([rng.choice(np.flatnonzero(inv), 330, replace=True), rng.choice(np.flatnonzero(inv == 0), 70, replace=True)]).astype(np.int32)
    rng.shuffle(pick)
    off = np.array([0, len(pick)], np.uint32)
    return dict(poses=[T], map=m, list_off=off, list_idx=pick, th=GATE_TH, want=gate_map_expect([T], m, off, pick, None, GATE_TH))


OCT_RANKS = (0, 9, 10, 30, 55, 56, -1)   # which of frame 0's query-making features get an octave outside [0, nlevels)


@functools.lru_cache(maxsize=None)
def octave_case():
    """(device pairs, oracle pairs, planted): two pairs of 80 valid features.  On the device side frame 0 carries octave -1
    and nlevels = 8 in turn on `planted` features, which make queries under their own octave; the oracle side keeps the
    octave and marks those features invalid instead."""
    rng = np.random.default_rng(1001)
    dev = [(cur, _all_valid(last)) for cur, last in (PC.last_frame_case(rng, 64, 80, "small") for _ in range(2))]
    own = gate_last_expect(dev)[0][1]
    planted = {int(own[r]): (-1 if k % 2 == 0 else TO.NLEVELS) for k, r in enumerate(OCT_RANKS)}
    cur0, la0 = dev[0]
    ora0, dev0 = dict(la0, has_mp=la0["has_mp"].copy()), dict(la0, octave=la0["octave"].copy())
    for i, o in planted.items():
        dev0["octave"][i] = o
        ora0["has_mp"][i] = 0
    ora = [(cur0, ora0), dev[1]]
    return [(cur0, dev0), dev[1]], ora, planted, gate_last_expect(ora)


# ------------------------------------------------------------------------------------------------ 4. counts outside [0, cap]
COUNT_CAP_LAST, COUNT_CAP_UNPROJ = 90, 150


def count_ns(cap):
    """(d_n as the device reads it, the rows it must use)"""
    return np.array([-3, cap + 7, cap - 30], np.int32), [0, cap, cap - 30]


@functools.lru_cache(maxsize=None)
def count_last_case():
    """three pairs with cap live features each; last->d_n = -3, cap + 7, cap - 30"""
    rng = np.random.default_rng(1102)
    pairs = []
    for motion in ("small", "forward", "backward"):
        cur, last = PC.last_frame_case(rng, 64, COUNT_CAP_LAST, motion)
        pairs.append((cur, _all_valid(last)))
    n_dev, n_eff = count_ns(COUNT_CAP_LAST)
    return pairs, n_dev, gate_last_expect(pairs, n_eff=n_eff), gate_last_expect(pairs)


def _depth_frame(rng, n):
    xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(F)
    z = np.where(rng.random(n) < 0.25, rng.choice([0.0, -1.0], n), rng.uniform(0.4, 9.0, n)).astype(F)
    return xy, z, (rng.random(n) < 0.3).astype(np.uint8)


def unproject_expect(frames, poses, th_depth, n_eff=None, keeps=True):
    """per frame (world_pos[cap][3], created[cap]): TO.unproject_select on the first n_eff rows, zeros behind them"""
    out = []
    for f, (xy, z, kp) in enumerate(frames):
        n = len(z) if n_eff is None else n_eff[f]
        wp, cr = np.zeros((len(z), 3), F), np.zeros(len(z), np.uint8)
        wp[:n], cr[:n] = TO.unproject_select(xy[:n], z[:n], poses[f], TO.K0, th_depth, kp[:n] if keeps else None)
        out.append((wp, cr))
    return out


@functools.lru_cache(maxsize=None)
def count_unproject_case():
    """three frames of cap live rows; d_n = -3, cap + 7, cap - 30"""
    rng = np.random.default_rng(1203)
    frames = [_depth_frame(rng, COUNT_CAP_UNPROJ) for _ in range(3)]
    poses = [PC._pose(np.random.default_rng(400 + f), 6.0, (0.1 * f, -0.2, 0.3)) for f in range(3)]
    n_dev, n_eff = count_ns(COUNT_CAP_UNPROJ)
    return dict(frames=frames, poses=poses, th_depth=3.0, n_dev=n_dev, want=unproject_expect(frames, poses, 3.0, n_eff))


# ------------------------------------------------------------------------------------------------ 5. unproject past one stride
STRIDE = 1024
STRIDE_NS = (1023, 1024, 1025, 2049)
STRIDE_TH = 3.0
TIE_Z = F(3.25)   # the smallest depth above the threshold, twice: ranks nsel - 1 and nsel
TIE_LO = 700


def _stride_frame(rng, n):
    """depths with equal pairs mirrored about index 1024 (1023 - k and 1024 + k), nothing in (th, TIE_Z] but the two entries
    TIE_LO and n - 1, which then rank nsel - 1 and nsel: the lower index is selected, the last entry of the frame is not"""
    xy, z, kp = _depth_frame(rng, n)
    for k in range(1, 7):
        if STRIDE + k < n - 1:
            z[STRIDE + k] = z[STRIDE - 1 - k] = F(1.5 + 0.25 * k)
    z[(z > F(STRIDE_TH)) & (z <= F(3.3))] += F(0.5)
    z[TIE_LO] = z[n - 1] = TIE_Z
    kp[TIE_LO] = kp[n - 1] = 0
    return xy, z, kp


def boundary_tie(z, th_depth):
    """(nsel, the two (z, i) entries ranked nsel - 1 and nsel) of one frame's depths"""
    order = sorted((float(v), i) for i, v in enumerate(z) if v > 0)
    nsel = int(TO.select_closed(z, th_depth).sum())
    return nsel, order[nsel - 1], order[nsel] if nsel < len(order) else None


@functools.lru_cache(maxsize=None)
def unproject_stride_case():
    """(small, big): four frames of n = 1023 .. 2049 under four poses in one call (cap 2052; `want_no_keeps` for the run with
    d_keeps = NULL), and one frame of cap = n = 15360 under a fifth pose in a call of its own"""
    rng = np.random.default_rng(1304)
    frames = [_stride_frame(rng, n) for n in STRIDE_NS]
    poses = [PC._pose(np.random.default_rng(500 + f), 6.0, (0.2 - 0.1 * f, 0.05 * f, 0.1)) for f in range(len(STRIDE_NS) + 1)]
    small = dict(frames=frames, poses=poses[:-1], th_depth=STRIDE_TH, cap=max(STRIDE_NS) + 3, want=unproject_expect(frames, poses, STRIDE_TH),
                 want_no_keeps=unproject_expect(frames, poses, STRIDE_TH, keeps=False))
    bigf = [_stride_frame(rng, E.PJ_MAX_NF)]
    big = dict(frames=bigf, poses=poses[-1:], th_depth=STRIDE_TH, cap=E.PJ_MAX_NF, want=unproject_expect(bigf, poses[-1:], STRIDE_TH))
    return small, big


# ------------------------------------------------------------------------------------------------ 6. the replay
REPLAY_QCAP, REPLAY_CAP_LAST = 603, 800
REPLAY_NQ = (0, 1, 255, 256, 257, 600)


def _replay_frame(seed, nF, nq, plan, dense=0.0, beyond=()):
    """one frame of the replay table.  plan = [(position, slot, bin)]: query `position` matched slot `slot`, the angle of its
    source chosen so that the pair falls in rotation bin `bin`.  beyond = raw match values >= nF, put on unmatched positions.
    The rows are REPLAY_QCAP long: positions from nq on hold live-looking values (a slot, a source)."""
    rng = np.random.default_rng(seed)
    qsrc = np.sort(rng.choice(REPLAY_CAP_LAST, REPLAY_QCAP, replace=False)).astype(np.int32)
    cur_angle = (rng.integers(0, 720, nF) / 2).astype(F)
    last_angle = (rng.integers(0, 720, REPLAY_CAP_LAST) / 2).astype(F)
    match = np.full(REPLAY_QCAP, -1, np.int32)
    if nF:
        match[nq:] = np.arange(REPLAY_QCAP - nq) % nF
    if dense:
        hit = rng.random(nq) < dense
        match[:nq][hit] = rng.integers(0, nF, int(hit.sum()))
    for pos, slot, b in plan:
        assert pos < nq and slot < nF and match[pos] == -1
        match[pos] = slot
        last_angle[qsrc[pos]] = F((float(cur_angle[slot]) + 30.0 * b + 3.0) % 360.0)
    free = [p for p in range(5, nq) if match[p] == -1]
    for pos, v in zip(free, beyond):
        assert v >= nF
        match[pos] = v
    clean = match[:nq].copy()
    clean[clean >= nF] = -1
    cur = dict(desc=np.full((nF, 32), 0x11, np.uint8), xy=np.stack([rng.uniform(0, 640, nF), rng.uniform(0, 480, nF)], 1).astype(F),
               octave=np.zeros(nF, np.int32), angle=cur_angle, state=(np.arange(nF) % 3).astype(np.uint8), uRight=None)
    return dict(cur=cur, last=dict(angle=last_angle), nq=nq, qsrc=qsrc, match=match, clean=clean, plan=list(plan), nF=nF)


def _spread(rng, nq, count, must=()):
    """`count` distinct positions below nq, `must` among them, ascending"""
    rest = np.setdiff1d(np.arange(nq), np.array(must, np.int64))
    return sorted(set(must) | set(rng.choice(rest, count - len(must), replace=False).tolist()))


def _plan(rng, nq, bins, must=(), first_slot=0):
    """matches on distinct slots first_slot, first_slot + 1, ...: bins = [(bin, count)], shuffled over the positions"""
    labels = [b for b, c in bins for _ in range(c)]
    rng.shuffle(labels)
    pos = _spread(rng, nq, len(labels), must)
    return [(p, first_slot + k, b) for k, (p, b) in enumerate(zip(pos, labels))]


@functools.lru_cache(maxsize=None)
def replay_case():
    """name -> frame, in batch order.  Slot states cycle 0, 1, 2 (slot k holds state k % 3)."""
    rng = np.random.default_rng(1405)
    t = {}
    t["none"] = _replay_frame(1, 12, 0, [])
    t["one"] = _replay_frame(2, 9, 1, [(0, 4, 4)])                                   # slot 4 holds state 1 and takes the source
    t["10:1:1"] = _replay_frame(3, 40, 255, _plan(rng, 255, [(2, 10), (5, 1), (9, 1)], must=(0, 63, 64, 254)), beyond=[40])
    t["11:1:1"] = _replay_frame(4, 40, 256, _plan(rng, 256, [(2, 11), (5, 1), (9, 1)], must=(0, 127, 128, 255)), beyond=[41])
    # 20 : 5 : 1 and a slot matched twice: the single match of bin 10 (dropped) sits EARLIER than a bin-1 match (kept) to the same slot
    # (slot 1, which held a MapPoint without observations: it ends NULL, not -2)
    plan = _plan(rng, 257, [(1, 19), (6, 5)], must=(3, 255, 256), first_slot=2)
    free = [p for p in range(20, 250) if p not in {q for q, _, _ in plan}]
    plan += [(free[0], 1, 10), (free[-1], 1, 1)]
    t["20:5:1"] = _replay_frame(5, 60, 257, sorted(plan))
    # 40 : 40 : 30 : 30 -- two equal fullest bins and a tie for the third place; slot 150 matched twice in two kept bins
    plan = _plan(rng, 600, [(1, 39), (3, 39), (5, 30), (7, 30)], must=(0, 255, 256, 511, 512, 599))
    free = [p for p in range(100, 500) if p not in {q for q, _, _ in plan}]
    plan += [(free[0], 150, 1), (free[-1], 150, 3)]
    t["40:40:30:30"] = _replay_frame(6, 200, 600, sorted(plan), beyond=[200, 202])
    t["dense"] = _replay_frame(7, 200, 600, [], dense=0.7)
    t["one-bin"] = _replay_frame(8, 40, 255, _plan(rng, 255, [(7, 30)], must=(254,)))
    return t


def replay_want(kind, check_ori):
    t = list(replay_case().values())
    return TO.replay_batch(kind, [fr["cur"] for fr in t], [fr["qsrc"][:fr["nq"]] for fr in t], [fr["clean"] for fr in t],
                           lasts=[fr["last"] for fr in t], check_ori=check_ori)


def replay_bins(fr):
    """the 30 bin counts of a frame's matches, by the oracle's rot_bin"""
    counts = [0] * 30
    for i, mt in enumerate(fr["clean"]):
        if mt >= 0:
            counts[O.rot_bin(float(fr["last"]["angle"][fr["qsrc"][i]]), float(fr["cur"]["angle"][mt]))] += 1
    return counts


# ------------------------------------------------------------------------------------------------ 7. the core's pools
POOL_MEMBERS = ("queries_65", "queries_64", "queries_5")
POOL_ROWS, POOL_STRIDE = 66, 70   # rows a query may address; rows between two frames' pools


def _pool_calls():
    calls = [E.SLAB_CASES[k]()["calls"][0] for k in POOL_MEMBERS]
    assert len({(tuple(float(v) for v in c["ci"]["bounds"]), c["th"], float(c["nnratio"]), c["rule"]) for c in calls}) == 1 and all(c["is2"] is None for c in calls)
    return calls


def _core_want(c, qd, keep=None):
    """the oracle on the call with descriptors qd; keep = the queries that stay (the others are REMOVED, so the claims of the
    kept ones chain as if the others had never been there) -> (match, best, second) over all queries, -1 / 256 / 256 on the removed"""
    nq = len(c["q"])
    keep = np.ones(nq, bool) if keep is None else keep
    m, b, s = E.run_core(O.search_by_projection, dict(c, q=c["q"][keep], qd=qd[keep]))
    out = [np.full(nq, -1, np.int32), np.full(nq, 256, np.int32), np.full(nq, 256, np.int32)]
    for o, v in zip(out, (m, b, s)):
        o[keep] = v
    need = sum(len(E.oracle_area(c, i)) for i in np.flatnonzero(keep))
    return out, need


@functools.lru_cache(maxsize=None)
def core_pool_case():
    """(shared, per_frame).  shared: ONE pool of the three calls' descriptors, shuffled (134 rows, pool_frame_rows = 0); most
    queries point at their own descriptor, every seventh at a row that belongs to ANOTHER frame's query, and two frames'
    queries share rows.  per_frame: pools of POOL_STRIDE rows per frame of which POOL_ROWS may be addressed; sources -1 and
    POOL_ROWS planted on `off_pool` queries (the rows behind POOL_ROWS hold the descriptor that query would match)."""
    calls = _pool_calls()
    rng = np.random.default_rng(1506)
    qds = [c["qd"] for c in calls]
    base = np.concatenate([[0], np.cumsum([len(q) for q in qds])])
    perm = rng.permutation(int(base[-1]))
    pool = np.zeros((int(base[-1]), 32), np.uint8)
    pool[perm] = np.concatenate(qds)
    srcs, foreign = [], []
    for f, c in enumerate(calls):
        own = perm[base[f]:base[f + 1]].astype(np.int32)
        oth = perm[base[(f + 1) % 3]:base[(f + 1) % 3 + 1]]
        src = own.copy()
        src[::7] = oth[np.arange(len(src[::7])) % len(oth)]
        srcs.append(src)
        foreign.append(np.arange(len(src))[::7])
    shared = dict(calls=calls, pool=pool, srcs=srcs, foreign=foreign, want=[_core_want(c, pool[s]) for c, s in zip(calls, srcs)])
    pf_srcs, pools, off_pool, want = [], [], [], []
    for f, c in enumerate(calls):
        nq = len(c["q"])
        perm = rng.permutation(nq).astype(np.int32)
        p = np.full((POOL_STRIDE, 32), 0x3C, np.uint8)
        p[perm] = c["qd"]
        src = perm.copy()
        out = np.arange(nq)[1::4][:6]
        p[POOL_ROWS] = c["qd"][out[0]]
        src[out[0::2]], src[out[1::2]] = POOL_ROWS, -1
        keep = np.ones(nq, bool)
        keep[out] = False
        pf_srcs.append(src)
        pools.append(p)
        off_pool.append(out)
        want.append(_core_want(c, c["qd"], keep))
    per_frame = dict(calls=calls, pools=np.stack(pools), srcs=pf_srcs, off_pool=off_pool, want=want, full=[_core_want(c, c["qd"]) for c in calls])
    return shared, per_frame


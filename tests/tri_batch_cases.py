"""Cases for the batched, device-resident SearchForTriangulation (csrc/orbfe_tri_search.hip): planted edges of the per-candidate
test, FeatureVector shapes at the ends of the node lookup, node-list lengths at the kernel's lane-group and tile sizes,
rotation-histogram shapes, batches, and keyframes with more nodes than the search has workgroups.  numpy + the CPU oracle only;
tests/test_tri_batch_cases.py checks that every case reaches its edge, tests/test_gpu_tri_search.py and
tests/test_gpu_tri_search_edges.py feed them to the HIP kernels.  Test support only.

A keyframe is dict(desc [n][32], xy [n][2], octave, angle, uRight (stereo: >= 0), has_mp, fv=(node, off, idx)), optionally `dead`
[n]: features the device must ignore without an error (octave outside the levels, index >= the keyframe's count).  A pair case is
dict(k1, k2, F12 [9], ex, ey) plus `want` (the planted match of keyframe-1 feature 0) where one is planted.  A batch is
dict(frames=[keyframe], pairs=[(i1, i2, F12, ex, ey)]).  th_low, only_stereo and check_ori belong to a call."""
import functools

import numpy as np

import hamming_cases as H
import proj_cases as PC
import proj_edge_cases as E
from oracle import oracle_ffi as O

F = np.float32
SF = PC.scale_factors()
S2 = (SF * SF).astype(F)
NLEVELS = len(SF)


# ------------------------------------------------------------------------------------------------ keyframes and the expected result
def keyframe(desc, xy, octave, angle, uRight, has_mp, fv, dead=None):
    n = len(desc)
    return dict(desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32), xy=np.ascontiguousarray(xy, F).reshape(n, 2),
                octave=np.ascontiguousarray(octave, np.int32), angle=np.ascontiguousarray(angle, F), uRight=np.ascontiguousarray(uRight, F),
                has_mp=np.ascontiguousarray(has_mp, np.uint8), fv=tuple(np.ascontiguousarray(a, np.uint32) for a in fv),
                dead=np.zeros(n, bool) if dead is None else np.asarray(dead, bool))


def from_scene(k):
    """a keyframe of proj_cases.triangulation_case"""
    return keyframe(k["desc"], k["xy"], k["octave"], k["angle"], k["uRight"], k["has_mp"], k["fv"])


def from_core(c, octave=None):
    """a side of a proj_edge_cases triangulation call (elig / stereo flags) as a keyframe; only_stereo = False reproduces it"""
    n = len(c["desc"])
    return keyframe(c["desc"], c["xy"], c.get("octave", np.zeros(n, np.int32)) if octave is None else octave, np.full(n, 10.0, F),
                    np.where(np.asarray(c["stereo"]) != 0, 5.0, -1.0), 1 - np.asarray(c["elig"], np.uint8), c["fv"])


def core_side(k, only_stereo):
    """what the shim hands orbfe_search_for_triangulation for one keyframe (proj_cases.tri_core_inputs' prep), with the features
    the device must ignore made ineligible"""
    st = (k["uRight"] >= 0).astype(np.uint8)
    el = ((k["has_mp"] == 0) & ((st == 1) | (not only_stereo)) & ~k["dead"]).astype(np.uint8)
    node, off, idx = k["fv"]
    idx = np.where(idx < len(st), idx, 0).astype(np.uint32) if len(st) else idx    # a dead index is never looked at: elig is 0 ...
    return dict(desc=k["desc"], xy=k["xy"], elig=el, stereo=st, fv=(node, off, idx), octave=np.clip(k["octave"], 0, NLEVELS - 1),
                scale_factors=SF, level_sigma2=S2)


def core_match(c, th_low=50, only_stereo=False, fn=None):
    """match12 of the matching core: the oracle's, or fn's (the HIP host-buffer call, the compiled reference's core)"""
    return (fn or O.search_for_triangulation)(core_side(c["k1"], only_stereo), core_side(c["k2"], only_stereo), c["F12"], c["ex"], c["ey"], th_low)


def expected(c, th_low=50, only_stereo=False, check_ori=True, fn=None):
    """(match12 [n1] after the rotation check, nmatches, pairs [k][2]) = core + proj_cases.replay_triangulation"""
    m = np.array(core_match(c, th_low, only_stereo, fn), np.int32)
    n1 = len(c["k1"]["desc"])
    if n1 and c["k1"]["dead"].any():
        m[c["k1"]["dead"]] = -1
    pairs, nm = PC.replay_triangulation(c["k1"], c["k2"], m, check_ori)
    out = np.full(n1, -1, np.int32)
    out[pairs[:, 0]] = pairs[:, 1]
    return out, nm, pairs


def pair_case(k1, k2, F12, ex, ey, want=None, pose=None):
    return dict(k1=k1, k2=k2, F12=np.asarray(F12, F).reshape(9), ex=F(ex), ey=F(ey), want=want, pose=pose)


def ref_keyframes(c):
    """the two mock KeyFrames oracle.ref_ffi.search_for_triangulation takes.  The compiled reference computes the epipole itself
    from keyframe 1's centre and keyframe 2's pose and intrinsics; a case without a pose gets K = (1, 1, 0, 0), Rcw = I, tcw = 0
    and Ow = (ex, ey, 1), whose epipole is (ex, ey) exactly (1 * ex * (1 / 1) + 0)."""
    pose = c["pose"] or dict(Ow=np.array([c["ex"], c["ey"], 1], F), Rcw=np.eye(3, dtype=F), tcw=np.zeros(3, F), K=(1.0, 1.0, 0.0, 0.0, 40.0))
    extra = dict(K=pose["K"], bounds=(0.0, 640.0, 0.0, 480.0), gw_inv=F(PC.GRID_COLS) / F(640), gh_inv=F(PC.GRID_ROWS) / F(480), scale_factors=SF,
                 inv_sigma2=(1.0 / S2).astype(F), level_sigma2=S2, log_scale=F(np.log(F(1.2))))
    k1, k2 = dict(c["k1"], **extra), dict(c["k2"], **extra)
    k1["Ow"], k2["Rcw"], k2["tcw"] = pose["Ow"], pose["Rcw"], pose["tcw"]
    return k1, k2


def has_dead(c):
    return bool(c["k1"]["dead"].any() or c["k2"]["dead"].any())


def scene(seed, n1, n2, nnodes):
    rng = np.random.default_rng(seed)
    k1, k2, F12 = PC.triangulation_case(rng, n1, n2, nnodes)
    _, _, ex, ey = PC.tri_core_inputs(k1, k2, False)
    return pair_case(from_scene(k1), from_scene(k2), F12, ex, ey, pose=dict(Ow=k1["Ow"], Rcw=k2["Rcw"], tcw=k2["tcw"], K=k2["K"])), (k1, k2)


def nodes_of(k):
    """node id per feature, -1 = in no node"""
    out = np.full(len(k["desc"]), -1, np.int64)
    node, off, idx = k["fv"]
    for a in range(len(node)):
        out[idx[off[a]:off[a + 1]]] = node[a]
    return out


def with_nodes(k, nodes):
    k = dict(k)
    k["fv"] = tuple(np.ascontiguousarray(a, np.uint32) for a in PC._fv_csr([int(v) for v in nodes], [v >= 0 for v in nodes]))
    return k


def permuted(k, perm):
    """the keyframe with its features in another order (new feature i = old feature perm[i])"""
    out = {f: (k[f][perm] if f != "fv" else None) for f in k}
    return with_nodes(out, nodes_of(k)[perm])


# ------------------------------------------------------------------------------------------------ planted: one candidate decides
def _from_call(call):
    return pair_case(from_core(call["k1"]), from_core(call["k2"], call["k2"]["octave"]), call["F12"], call["ex"], call["ey"], call["want"][0]), call["th_low"]


def x_gate_fail_closer():
    """a CLOSER candidate that fails the epipolar gate, before and after a farther one that passes: it must not win (its distance
    never becomes bestDist) and must not block (the farther one still takes over)"""
    return dict(calls=[E._tri_call([E._on(300, d=10, y=140.0), E._on(340, d=20)], 1), E._tri_call([E._on(300, d=20), E._on(340, d=10, y=140.0)], 0, seed=1),
                       E._tri_call([E._on(300, d=10), E._on(340, d=20)], 0, seed=2)], differ=[])


def x_epipole_levels():
    """the epipole gate just inside and just outside 100 * scale[octave] on levels 0 and 7, and bypassed when either side is stereo"""
    calls, differ = [], []
    for o in (0, 7):
        lim = F(F(100) * SF[o])

        def d2(x):
            dx = F(E.TRI_EX - F(x))
            return F(F(dx * dx) + F(0))
        x_in, x_out = E.adjacent(E.TRI_EX - F(np.sqrt(float(lim))), lambda x: d2(x) < lim)
        k = len(calls)
        calls += [E._tri_call([E._on(x_in, o=o)], 0, seed=k), E._tri_call([E._on(x_out, o=o)], -1, seed=k + 1),
                  E._tri_call([E._on(x_out, o=o)], 0, stereo1=1, seed=k + 2), E._tri_call([E._on(x_out, o=o, st=1)], 0, seed=k + 3)]
        differ += [(k, k + 1), (k + 1, k + 2), (k + 1, k + 3)]
    return dict(calls=calls, differ=differ)


def x_three_tied():
    """three passing candidates at one distance: the last in list order wins; with the last one bit worse, the second"""
    return dict(calls=[E._tri_call([E._on(300), E._on(340), E._on(380)], 2), E._tri_call([E._on(300), E._on(340), E._on(380, d=21)], 1, seed=1)],
                differ=[(0, 1)])


PLANTED_TABLES = dict(E.TRI_CASES, gate_fail_closer=x_gate_fail_closer, epipole_levels=x_epipole_levels, three_tied=x_three_tied)
PLANTED_NAMES = ("threshold", "tie", "three_tied", "gate_fail_closer", "epipole", "epipole_levels", "epipolar_line", "zero_f", "eligibility", "nodes")


@functools.lru_cache(maxsize=None)
def planted():
    """[(name, call index, pair case, th_low)] of every planted call with th_low >= 0 (a negative threshold is the host call's)"""
    out = []
    for name in PLANTED_NAMES:
        for k, call in enumerate(PLANTED_TABLES[name]()["calls"]):
            c, th = _from_call(call)
            if th >= 0:
                out.append((name, k, c, th))
    return out


# ------------------------------------------------------------------------------------------------ FeatureVector shapes
def fv_shapes():
    """{name: pair case}: the node lookup at its ends.  The scene has nodes 0, 1, 2 on both sides; they are renamed per side."""
    out = {}
    base, _ = scene(31, 60, 60, 3)

    def renamed(m1, m2):
        n1, n2 = nodes_of(base["k1"]), nodes_of(base["k2"])
        return dict(base, k1=with_nodes(base["k1"], [m1.get(int(v), -1) for v in n1]), k2=with_nodes(base["k2"], [m2.get(int(v), -1) for v in n2]))
    out["all_below"] = renamed({0: 1, 1: 2, 2: 3}, {0: 10, 1: 11, 2: 12})
    out["all_above"] = renamed({0: 10, 1: 11, 2: 12}, {0: 1, 1: 2, 2: 3})
    out["common_first"] = renamed({0: 5, 1: 100, 2: 101}, {0: 5, 1: 6, 2: 7})
    out["common_last"] = renamed({0: 1, 1: 2, 2: 9}, {0: 7, 1: 8, 2: 9})
    out["interleaved"] = renamed({0: 2, 1: 4, 2: 6}, {0: 1, 1: 4, 2: 7})
    out["empty_fv1"] = dict(base, k1=with_nodes(base["k1"], [-1] * 60))
    out["empty_fv2"] = dict(base, k2=with_nodes(base["k2"], [-1] * 60))
    e, _ = scene(32, 0, 40, 3)
    out["n1_zero"] = e
    e, _ = scene(33, 40, 0, 3)
    out["n2_zero"] = e
    return out


def one_node(seed, n1, n2):
    """every feature of both keyframes in ONE node (id 3): node lists of exactly n1 and n2 entries"""
    c, _ = scene(seed, n1, n2, 1)
    return dict(c, k1=with_nodes(c["k1"], [3] * n1), k2=with_nodes(c["k2"], [3] * n2))


def list_lengths(info):
    """{name: pair case} at the lengths where k_tri_search changes path, from the kernel's own constants (orbfe_tri_search_info)"""
    L, T, Q = info["lanes"], info["tile"], info["queries_per_pass"]
    out = {}
    for n2 in sorted({1, L - 1, L, L + 1, T - 1, T, T + 1, 3 * T + 1}):
        out["n2_%d" % n2] = one_node(500 + n2, 40, n2)
    for n1 in sorted({1, Q - 1, Q, Q + 1}):
        out["n1_%d" % n1] = one_node(700 + n1, n1, T + 5)       # more than one pass over a list of more than one tile
        out["n1_%d_short" % n1] = one_node(800 + n1, n1, T - 3)   # ... and over a list that is staged once
    out["both_600"] = one_node(600, 600, 600)
    return out


# ------------------------------------------------------------------------------------------------ more nodes than workgroups
def node_walk(c, only_stereo=False, check_ori=True):
    """what k_tri_search meets at every keyframe-1 node, by position in keyframe 1's node list: dict(n1 = the node's keyframe-1
    entries, n2 = the entries of the same node in keyframe 2 (0 = the node is absent there), elig = the keyframe-1 entries that are
    queries, matches = the standing matches (after the rotation check) whose keyframe-1 feature sits in the node)"""
    k1, k2 = c["k1"], c["k2"]
    node1, off1, idx1 = k1["fv"]
    len2 = {int(v): int(k2["fv"][1][a + 1]) - int(k2["fv"][1][a]) for a, v in enumerate(k2["fv"][0])}
    el = core_side(k1, only_stereo)["elig"]
    stands = expected(c, 50, only_stereo, check_ori)[0] >= 0
    n = len(node1)
    out = dict(n1=np.zeros(n, np.int64), n2=np.zeros(n, np.int64), elig=np.zeros(n, np.int64), matches=np.zeros(n, np.int64))
    for a in range(n):
        f = idx1[off1[a]:off1[a + 1]]
        out["n1"][a], out["n2"][a] = len(f), len2.get(int(node1[a]), 0)
        out["elig"][a], out["matches"][a] = el[f].sum(), stands[f].sum()
    return out


def workgroup_sequences(nfv1, W):
    """the keyframe-1 node positions each of k_tri_search's min(cap, W) workgroups of a pair takes, in its order (cap >= W)"""
    return [list(range(y, nfv1, W)) for y in range(min(W, nfv1))]


MANY_NODES_MERGES = ((0, 44), (44, 60), (324, 368))   # node ids [lo, hi) that become node lo


def many_nodes(info):
    """One pair of 1500 x 1500 features in ~290 nodes, for a kernel whose workgroups take the keyframe-1 nodes round robin, W =
    info["node_workgroups"] (128) at a time, so that every workgroup walks two or three nodes: scene 901 has ~390 nodes of ~4
    features; the ids below 44 become one heavy node at position 0 (150 x 140: three tiles, four passes), 44 .. 59 a node of one
    tile and two passes at position 1, 324 .. 367 a second heavy node at position 2 W, so that workgroup 0 goes heavy, ordinary,
    heavy.  Two gaps are planted in the first workgroups that have three nodes whose first and third match: the middle node of
    one loses its keyframe-2 side (its keyframe-2 features leave the FeatureVector), every keyframe-1 feature of the other's
    middle node gets a MapPoint.  Chosen on the CPU;
    tests/test_tri_batch_cases.py asserts every property from `info`, so a kernel with other sizes fails there, not silently.
    -> (pair case, dict(absent = the workgroup with the absent middle node, taken = the one with the ineligible middle node))"""
    W = info["node_workgroups"]
    c, _ = scene(901, 1500, 1500, 400)

    def merged(v):
        v = v.copy()
        for lo, hi in MANY_NODES_MERGES:
            v[(v >= lo) & (v < hi)] = lo
        return v
    n1, n2 = merged(nodes_of(c["k1"])), merged(nodes_of(c["k2"]))
    c = dict(c, k1=with_nodes(c["k1"], n1), k2=with_nodes(c["k2"], n2))
    walk = node_walk(c)
    node1 = c["k1"]["fv"][0]
    # the workgroups whose three nodes are ordinary (one tile, one pass) and match at both ends and in the middle
    full = [y for y in range(max(len(node1) - 2 * W, 0))
            if all(walk["matches"][y + k * W] > 0 and walk["n2"][y + k * W] < info["tile"] for k in range(3))]
    assert len(full) >= 2, "scene 901 no longer has two workgroups with three matching nodes"
    absent, taken = full[0], full[1]
    n2 = np.where(n2 == int(node1[absent + W]), -1, n2)
    mp = c["k1"]["has_mp"].copy()
    mp[n1 == int(node1[taken + W])] = 1
    return dict(c, k1=dict(c["k1"], has_mp=mp), k2=with_nodes(c["k2"], n2)), dict(absent=absent, taken=taken)


NODES_AT_SEED = {128: 690, 129: 695, 256: 817, 257: 818}   # the first seeds from 560 + n whose LAST node of `back` keeps a match


def nodes_at(n, seed=None):
    """n nodes of ONE feature each on one keyframe, every feature of the other keyframe in its partner's node (or in none), as
    test_counts_above_cap_are_clamped builds them -> (fwd, back): fwd has the n-node keyframe as keyframe 2; back is the pair the
    other way round (F21 = F12', its epipole far away), where keyframe 1 has exactly n nodes: with W workgroups, n = W + 1 is the
    case where exactly one of them takes a second node, and that node is the last: its match is the one a workgroup that stops
    after its first node loses."""
    one = one_node(NODES_AT_SEED.get(n, 560 + n) if seed is None else seed, n, n)
    m = core_match(one)
    full = with_nodes(one["k2"], np.arange(n))                                    # n nodes of one feature each
    part = with_nodes(one["k1"], [m[i] if m[i] >= 0 else -1 for i in range(n)])   # every feature in its partner's node
    Ft = np.ascontiguousarray(one["F12"].reshape(3, 3).T).reshape(9)
    return dict(one, k1=part, k2=full), dict(one, k1=full, k2=part, F12=Ft, ex=F(-1e6), ey=F(-1e6), pose=None)


# ------------------------------------------------------------------------------------------------ rotation histogram
HISTOGRAMS = {
    # name: ([(keyframe-1 angle, matches)], the bins that stay); every keyframe-2 angle is 10, bin = round((a1 - 10 [+ 360]) / 30)
    "one_bin": ([(100.0, 40)], (3,)),
    "tie_earlier_wins": ([(70.0, 6), (160.0, 6), (220.0, 6), (280.0, 6)], (2, 5, 7)),
    "others_under_a_tenth": ([(40.0, 30), (130.0, 2), (190.0, 2)], (1,)),
    "third_under_a_tenth": ([(40.0, 30), (130.0, 5), (190.0, 2)], (1, 4)),
    # 910 - 10 = 900 -> bin 30 -> 0, next to five honest members of bin 0; left in a bin of their own, bin 0 falls behind bin 3
    "bin_30_wraps_to_0": ([(910.0, 3), (10.0, 5), (190.0, 20), (100.0, 6), (130.0, 7)], (6, 0, 4)),
    # 5 - 10 and 1 - 10 are negative: + 360 -> bin 12.  Without the + 360 they would fall into bin 0 and lift it over bin 6
    "negative_difference": ([(5.0, 4), (100.0, 10), (1.0, 3), (190.0, 2), (10.0, 2), (250.0, 1)], (3, 12, 0)),
}


@functools.lru_cache(maxsize=None)
def histogram_case(name):
    """a scene whose core matches get the planted angles; keyframe-1 features that match beyond the plan are taken out (has_mp)"""
    plan, _ = HISTOGRAMS[name]
    c, _ = scene(900, 400, 400, 10)
    k1, k2 = dict(c["k1"]), dict(c["k2"])
    k2["angle"] = np.full(len(k2["angle"]), 10.0, F)
    matched = np.nonzero(core_match(c) >= 0)[0]
    need = sum(n for _, n in plan)
    assert len(matched) >= need, (len(matched), need)
    a1, mp = k1["angle"].copy(), k1["has_mp"].copy()
    at = 0
    for ang, n in plan:
        a1[matched[at:at + n]] = F(ang)
        at += n
    mp[matched[at:]] = 1
    k1["angle"], k1["has_mp"] = a1, mp
    return dict(c, k1=k1, k2=k2)


# ------------------------------------------------------------------------------------------------ batches
def as_batch(cases):
    """every pair case as two keyframes of one block"""
    frames, pairs = [], []
    for c in cases:
        pairs.append((len(frames), len(frames) + 1, c["F12"], c["ex"], c["ey"]))
        frames += [c["k1"], c["k2"]]
    return dict(frames=frames, pairs=pairs)


def pair_of(batch, p):
    i1, i2, F12, ex, ey = batch["pairs"][p]
    return pair_case(batch["frames"][i1], batch["frames"][i2], F12, ex, ey, pose=batch.get("pose"))


@functools.lru_cache(maxsize=None)
def neighbours(nn=20, n=150):
    """one keyframe 1 (frame 0) against nn neighbours: the scene's second keyframe with its features in nn different orders, F12
    scaled per neighbour (a scale changes no decision in exact arithmetic and the roundings of some), plus the pair (0, 0)"""
    c, _ = scene(77, n, n, 12)
    rng = np.random.default_rng(78)
    frames = [c["k1"]] + [permuted(c["k2"], rng.permutation(n)) for _ in range(nn)]
    pairs = [(0, 1 + j, (c["F12"] * F(1 + j / 8)).astype(F), c["ex"], c["ey"]) for j in range(nn)]
    pairs.append((0, 0, c["F12"], c["ex"], c["ey"]))
    return dict(frames=frames, pairs=pairs, pose=c["pose"])


def ignored_inputs():
    """{name: pair case with `dead` features}: what the device cannot reject and must ignore.  The arrays hold the bad values;
    `dead` tells the expected result to leave those features out."""
    out = {}
    c, _ = scene(41, 80, 80, 4)
    k2 = dict(c["k2"])
    oc = k2["octave"].copy()
    oc[::7], oc[3::11] = NLEVELS, -1
    k2["octave"], k2["dead"] = oc, (oc < 0) | (oc >= NLEVELS)
    out["octave_out_of_range"] = dict(c, k2=k2)
    return out


def big():
    return scene(8192, 8192, 8192, 10)[0]

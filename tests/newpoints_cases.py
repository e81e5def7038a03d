"""Cases for CreateNewMapPoints' triangulation (csrc/orbfe_newpoints.h / .hip): synthetic multi-view scenes with known poses, whose
matches stay clear of every gate's threshold in both trig modes, and planted matches that sit exactly on a representable edge.
numpy + tests/newpoints_oracle.py (an UNPINNED restatement: nothing compiled pins LocalMapping.cc); tests/test_newpoints_oracle.py
checks them on the CPU, tests/test_gpu_newpoints.py feeds them to the kernels.  Test support only.

A frame is a tri_batch_cases keyframe (desc, xy = mvKeysUn, octave, angle, uRight, has_mp, fv) plus Tcw [12], Ow [3], depth [n]
and mp_xyz [n][3]."""
import functools

import numpy as np

import f12_oracle as FO
import newpoints_oracle as NO
import proj_cases as PC
import tri_batch_cases as TC

f32 = np.float32
CAM = NO.camera(535.4, 539.2, 320.1, 247.6, 40.0)
MB = f32(f32(40.0) / f32(535.4))
SF, S2, SCALE_FACTOR = TC.SF, TC.S2, f32(1.2)
MARGIN = 1e-4
SEEDS = (1, 2, 3, 4)        # chosen on the CPU: every scene below passes clear_of_thresholds() (test_newpoints_oracle checks it again)


# ------------------------------------------------------------------------------------------------ scenes
def _frame_pose(rng, centre, rot_deg):
    R = PC._rot(rng, rot_deg)
    t = -R @ np.asarray(centre, np.float64)
    T = np.concatenate([R, t[:, None]], 1).astype(f32)
    Ow = (-(T[:, :3].astype(np.float64).T @ T[:, 3].astype(np.float64))).astype(f32)
    return T.reshape(12), Ow


def scene(seed, nkf=2, npts=120, nnodes=6, p_stereo=0.5, p_has_mp=0.0, centres=None, rot_deg=2.0):
    """nkf keyframes around the origin that all see the same npts landmarks, each in its own feature order"""
    rng = np.random.default_rng(seed)
    # near landmarks with degrees of parallax and far ones with next to none: nothing near the 0.9998 cut or the stereo cosines
    far = rng.random(npts) < 0.25
    z = np.where(far, rng.uniform(250.0, 500.0, npts), rng.uniform(1.5, 5.0, npts))
    Xw = np.stack([rng.uniform(-0.45, 0.45, npts) * z, rng.uniform(-0.35, 0.35, npts) * z, z], 1)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    pnode = rng.integers(0, nnodes, npts)
    fx, fy, cx, cy, bf = (float(CAM[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    frames = []
    for b in range(nkf):
        c = centres[b] if centres is not None else (0.35 * b + rng.normal(0, 0.03), rng.normal(0, 0.05), rng.normal(0, 0.05))
        T, Ow = _frame_pose(rng, c, rot_deg)
        perm = rng.permutation(npts)
        Xc = Xw[perm] @ T.reshape(3, 4)[:, :3].astype(np.float64).T + T.reshape(3, 4)[:, 3]
        n = npts
        noise = np.where((rng.random(n) < 0.8)[:, None] | far[perm][:, None], rng.normal(0, 0.4, (n, 2)), rng.normal(0, 5.0, (n, 2)))
        xy = (np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1) + noise).astype(f32)
        dist = np.linalg.norm(Xc, axis=1)
        octave = np.clip(np.round(np.log(dist / 1.5) / np.log(1.2) / 2.5) + rng.choice([0, 0, 0, 0, -3, 3], n), 0, 7).astype(np.int32)
        stereo = (rng.random(n) < p_stereo) & (Xc[:, 2] < 40)
        uR = np.where(stereo, xy[:, 0] - bf / Xc[:, 2] + rng.normal(0, 0.3, n), -1.0).astype(f32)
        uR = np.where(stereo & (uR < 0), f32(0.5), uR).astype(f32)
        with np.errstate(divide="ignore"):
            depth = np.where(uR >= 0, f32(bf) / (xy[:, 0] - uR), f32(-1)).astype(f32)
        k = TC.keyframe(PC.noisy_copy(rng, base[perm], 30), xy, octave, (10.0 + rng.normal(0, 4, n)).astype(f32) % f32(360), uR,
                        (rng.random(n) < p_has_mp).astype(np.uint8), PC._fv_csr(pnode[perm], np.ones(n, bool)))
        k.update(Tcw=T, Ow=Ow, depth=depth, mp_xyz=Xw[perm].astype(f32), landmark=perm)
        frames.append(k)
    return frames


def true_and_false_matches(frames, i1, i2, n, seed, p_false=0.25):
    """n (idx1, idx2): mostly the same landmark in both keyframes, some wrong pairings"""
    rng = np.random.default_rng(seed)
    f1, f2 = frames[i1], frames[i2]
    where2 = np.argsort(f2["landmark"])
    idx1 = rng.permutation(len(f1["desc"]))[:n] if n <= len(f1["desc"]) else rng.integers(0, len(f1["desc"]), n)
    idx2 = where2[f1["landmark"][idx1]]
    wrong = rng.random(n) < p_false
    idx2 = np.where(wrong, rng.integers(0, len(f2["desc"]), n), idx2)
    return np.stack([idx1, idx2], 1).astype(np.int32)


def match_args(frames, i1, i2, a, b):
    f1, f2 = frames[i1], frames[i2]
    return (f1["Tcw"], f1["Ow"], f2["Tcw"], f2["Ow"], CAM, MB, NO.frame_key(f1, a), NO.frame_key(f2, b), SF, S2, SCALE_FACTOR)


@functools.lru_cache(maxsize=None)
def scene_matches(seed, n=150):
    """(frames, pairs [n][2], [(verdict, x3D)] canonical, [..] host, names of the comparisons nearer than MARGIN to their threshold,
    {(comparison, lhs < rhs)} the canonical run met)"""
    frames = scene(seed, 2, 160, rot_deg=2.0 if seed % 2 == 0 else 25.0)   # odd seeds: cameras that look apart, for z2 <= 0 < z1
    pairs = true_and_false_matches(frames, 0, 1, n, seed + 1000)
    can, host, near, sides = [], [], [], set()
    for a, b in pairs:
        for mode, out in (("canonical", can), ("host", host)):
            tr = []
            out.append(NO.triangulate_match(*match_args(frames, 0, 1, a, b), trig=mode, trace=tr))
            near += NO.near_threshold(tr, MARGIN)
            if mode == "canonical":
                sides |= {(name, bool(a < b)) for name, a, b in tr}
    return frames, pairs, can, host, near, sides


def search(k1, k2, cam, th_low=50, check_ori=True):
    """the oracle's SearchForTriangulation between two frames on their poses -> pairs [k][2]"""
    F12 = FO.f12_compute(k1["Tcw"], k2["Tcw"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ex, ey = FO.f12_epipole(k2["Tcw"], k1["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    return TC.expected(TC.pair_case(k1, k2, F12, ex, ey), th_low, False, check_ori)[2]


def loop_kw(mono=False, trig="canonical"):
    return dict(cam=CAM, mb=MB, mono=mono, search=search, sf=SF, s2=S2, scale_factor=SCALE_FACTOR, trig=trig)


# ------------------------------------------------------------------------------------------------ more new points than a claim block
WIDE_SEED, WIDE_CAP, WIDE_PAIRS = 341, 904, ((0, 1), (0, 2))


@functools.lru_cache(maxsize=None)
def wide_loop():
    """keyframe 0 against two neighbours, 900 features each in ~280 nodes, cap = 904 (no multiple of the claim kernels' 256): the
    first pair creates more than 256 points, so k_np_claim runs several blocks per pair, with feature indices up to 899; both
    pairs in ONE round claim some keyframe-0 slots twice, from different blocks.  The oracle's serial loop (= the planned rounds,
    one pair each) and its one-round loop, computed once: dict(frames, cap, pairs, serial, s_serial, static, s_static)."""
    frames, cap, pairs = scene(WIDE_SEED, 3, 900, nnodes=300), WIDE_CAP, list(WIDE_PAIRS)
    s_serial, s_static = NO.new_state(frames, cap), NO.new_state(frames, cap)
    serial = NO.serial_loop(frames, pairs, s_serial, cap, **loop_kw())
    static = NO.round_loop(frames, pairs, [0, len(pairs)], s_static, cap, **loop_kw())
    return dict(frames=frames, cap=cap, pairs=pairs, serial=serial, s_serial=s_serial, static=static, s_static=s_static)


def median_edge_frames(cap=300):
    """frames for the scene median depth at the workgroup's 256 slots and at the ends of the rank: (Tcw [B][12], has_mp [B][cap],
    mp_xyz [B][cap][3], n [B], names): 255, 256 and 257 occupied slots, and a frame whose 100 depths are all equal"""
    rng = np.random.default_rng(97)
    occ, names = [255, 256, 257, 100], ["255", "256", "257", "all_equal"]
    B = len(occ)
    T = np.stack([_frame_pose(rng, rng.normal(0, 1, 3), 20.0)[0] for _ in range(B)])
    xyz = rng.normal(0, 6, (B, cap, 3)).astype(f32)
    xyz[3] = xyz[3, 0]
    has = np.zeros((B, cap), np.uint8)
    for b, k in enumerate(occ):
        has[b, rng.permutation(cap)[:k]] = 1
    return T, has, xyz, np.full(B, cap, np.int32), names


# ------------------------------------------------------------------------------------------------ planted
P_CAM = NO.camera(1.0, 1.0, 0.0, 0.0, 0.08)
P_MB = f32(0.08)
P_SF = np.array([1, 1.5, 2.25, 3.375, 5.0625, 7.59375, 8, 8], f32)
P_S2 = np.array([1, 1, 1, 1, 1, 1, 0, 1], f32)      # level 6: sigma2 = 0, the error gate's threshold is 0
P_SCALE_FACTOR = f32(2.0)                              # ratioFactor = 3


def _T(t=(0, 0, 0), R=None):
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1).astype(f32).reshape(12)


def _uright(u, z):
    """u - bf * invz as the gate computes it, for an exactly zero right error"""
    return f32(f32(u) - f32(P_CAM["bf"] * f32(1.0 / float(f32(z)))))


def _adjacent_x(cut=0.9998):
    """keyframe-2 abscissae whose cosParallaxRays are the two floats around the double 0.9998 (rays (0, 0, 1) and (x, 0, 1))"""
    T = _T()
    k1 = NO.key(0, 0, 0)

    def cos_of(x):
        return NO.cos_parallax_rays(T, T, P_CAM, k1, NO.key(x, 0, 0))[0]
    lo_f = np.nextafter(f32(cut), f32(0)) if float(f32(cut)) >= cut else f32(cut)   # the largest float below the double
    hi_f = np.nextafter(lo_f, f32(2))
    found = {}
    x = f32(np.sqrt(1 / cut ** 2 - 1))
    for step in range(-20000, 20000, 50):
        v = f32(x + f32(step) * f32(1e-9))
        c = cos_of(v)
        if c == lo_f:
            found.setdefault("below", v)
        elif c == hi_f:
            found.setdefault("above", v)
        if len(found) == 2:
            break
    assert len(found) == 2, found
    assert float(cos_of(found["below"])) < cut <= float(cos_of(found["above"]))
    return found["below"], found["above"]


@functools.lru_cache(maxsize=None)
def planted():
    """[dict(name, args = triangulate_match's positional arguments, want = verdict or None (whatever the oracle says, but not
    `never`))], all on P_CAM / P_MB / P_SF / P_S2 / P_SCALE_FACTOR so that one batch call takes them all"""
    V = NO
    out = []

    def add(name, T1, O1, T2, O2, k1, k2, want, never=None):
        out.append(dict(name=name, args=(T1, np.asarray(O1, f32), T2, np.asarray(O2, f32), P_CAM, P_MB, k1, k2, P_SF, P_S2, P_SCALE_FACTOR),
                        want=want, never=never))
    near = (_T((-0.001, 0, 0)), (0.001, 0, 0))   # a second camera a millimetre to the side: rays all but parallel
    side = (_T((-0.3, 0, 0)), (0.3, 0, 0))
    k_near = NO.key(f32(f32(1 - 0.001) / f32(4)), 0, 0)   # (1, 0, 4) seen from there
    # vt.row(3) = (0, 0, 1, 0): A's third column is zero (keyframe 2's rows 0 and 1 have no z), its rays still 37 degrees apart
    add("w_zero", _T(), (0, 0, 0), _T((-0.3, 0, 0), [[1, 0, 0], [0, 1, 0], [0.6, 0, 0.8]]), (0.3, 0, 0), V.key(0, 0, 0), V.key(0, 0, 0), V.W_ZERO)
    # UnprojectStereo(idx1) = (0, 0, 0.04); tcw1z = -0.04
    add("z1_zero", _T((0, 0, -0.04)), (0, 0, 0), *side, V.key(0, 0, 0, 0.04, 0.0), V.key(0.5, 0, 0), V.DEPTH1)
    add("z2_zero", _T(), (0, 0, 0), _T((-0.3, 0, -0.04)), (0.3, 0, 0), V.key(0, 0, 0, 0.04, 0.0), V.key(0.5, 0, 0), V.DEPTH2)
    # (1, 2, 4) from keyframe 1's stereo keypoint reprojects onto it exactly; level 6 has sigma2 = 0: 0 > 0 is false
    add("err_equal", _T(), (0, 0, 0), *near, V.key(0.25, 0.5, 6, 4.0, _uright(0.25, 4)), NO.key(k_near["ux"], 0.5, 7), V.OK)
    add("err_above", _T(), (0, 0, 0), *near, V.key(0.25, 0.5, 6, 4.0, np.nextafter(_uright(0.25, 4), f32(1))), NO.key(k_near["ux"], 0.5, 7), V.ERR1)
    # keyframe 2's stereo keypoint unprojects to exactly (3, 0, 4), 5 from its centre; keyframe 1's ray is parallel, so the point is
    # not triangulated; its centre is planted (the centres and the poses are independent inputs)
    k1m, k2s = V.key(0.75, 0, 1), V.key(0.75, 0, 0, 4.0, _uright(0.75, 4))
    add("dist1_zero", _T(), (3, 0, 4), _T(), (0, 0, 0), k1m, k2s, V.DIST_ZERO)
    # dist1 = 10, dist2 = 5: ratioDist * ratioFactor = 1.5 = scale[1] / scale[0]
    add("scale_equal", _T(), (3, 0, -6), _T(), (0, 0, 0), k1m, k2s, V.OK)
    add("scale_below", _T(), (3, 0, -6.000002), _T(), (0, 0, 0), k1m, k2s, V.SCALE)
    quarter = _T(R=[[0, 0, -1], [0, 1, 0], [1, 0, 0]])   # keyframe 2's optical axis is the world's x: the rays are orthogonal
    add("cos_rays_zero", _T(), (0, 0, 0), quarter, (0, 0, 0), V.key(0, 0, 0), V.key(0, 0, 0), V.LOW_PARALLAX)
    below, above = _adjacent_x()
    left = (_T((0.3, 0, 0)), (-0.3, 0, 0))   # the rays converge
    add("cut_below", _T(), (0, 0, 0), *left, V.key(0, 0, 0), V.key(below, 0, 0), None, never=V.LOW_PARALLAX)
    add("cut_above", _T(), (0, 0, 0), *left, V.key(0, 0, 0), V.key(above, 0, 0), V.LOW_PARALLAX)
    # (0.5, 0.2, 4) seen by two cameras 0.3 apart
    u1, u2 = (0.125, 0.05), (f32(0.2 / 4), 0.05)
    add("stereo_both", _T(), (0, 0, 0), *side, V.key(*u1, 0, 4.0, _uright(u1[0], 4)), V.key(*u2, 0, 4.0, _uright(u2[0], 4)), V.OK)
    add("stereo1_only", _T(), (0, 0, 0), *side, V.key(*u1, 0, 4.0, _uright(u1[0], 4)), V.key(*u2, 0), V.OK)
    add("stereo2_only", _T(), (0, 0, 0), *side, V.key(*u1, 0), V.key(*u2, 0, 4.0, _uright(u2[0], 4)), V.OK)
    # orthogonal rays and a stereo keypoint so far away that its cosine is 1: 1 == 0 + 1
    add("stereo_equal", _T(), (0, 0, 0), quarter, (0, 0, 0), V.key(0, 0, 0, 1e6, 0.0), V.key(0, 0, 0), V.LOW_PARALLAX)
    add("depth_zero_stereo1", _T(), (0, 0, 0), *side, V.key(0, 0, 0, 0.0, 0.0), V.key(0.5, 0, 0), V.DEPTH1)
    add("depth_zero_stereo2", _T(), (0, 0, 0), *side, V.key(0, 0, 0), V.key(0.5, 0, 0, 0.0, 0.0), V.DEPTH2)
    add("depth_negative", _T(), (0, 0, 0), *side, V.key(0, 0, 0, -1.0, 0.0), V.key(0.5, 0, 0), None)
    return out


def planted_frames():
    """the planted matches as a block: match j is feature 0 of frames 2j and 2j + 1 -> (frames, pairs [(2j, 2j + 1)])"""
    frames = []
    for c in planted():
        T1, O1, T2, O2, _, _, k1, k2 = c["args"][:8]
        for T, O, k in ((T1, O1, k1), (T2, O2, k2)):
            f = TC.keyframe(np.zeros((1, 32), np.uint8), [[k["ux"], k["uy"]]], [k["octave"]], [0.0], [k["uright"]], [0], PC._fv_csr([0], [True]))
            f.update(Tcw=np.asarray(T, f32), Ow=np.asarray(O, f32), depth=np.array([k["depth"]], f32), mp_xyz=np.zeros((1, 3), f32))
            frames.append(f)
    return frames, [(2 * j, 2 * j + 1) for j in range(len(planted()))]

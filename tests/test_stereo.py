"""Frame::ComputeStereoMatches (reference src/Frame.cc:642-846).

GPU: extractor + stereo matcher through the C-ABI against the oracle chain on the same synthetic stereo pair:
mvuRight / mvDepth bit-exact (float results of identical operation sequences)."""
import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame


def stereo_pair(seed, w=640, h=480):
    """left = S(seed); right = left seen with a disparity that grows towards the bottom, plus mild noise."""
    rng = np.random.default_rng(seed)
    left = synth_frame(seed, h, w)
    right = np.empty_like(left)
    for y in range(h):
        d = 4 + (20 * y) // h
        right[y] = np.roll(left[y], -d)
    noise = rng.integers(-3, 4, left.shape)
    right = np.clip(right.astype(np.int32) + noise, 0, 255).astype(np.uint8)
    return left, right



def disparity_field(kind, w, h, d=8, dmax=120, steps=(6, 40, 14, 90)):
    """integer disparity per pixel: "const" (d everywhere), "ramp" (0 at the left edge up to dmax at the right, so the
    true disparity outgrows maxD somewhere) or "steps" (len(steps) vertical bands; each jump leaves an occluded band)"""
    xx = np.broadcast_to(np.arange(w), (h, w))
    if kind == "const":
        return np.full((h, w), d, np.int64)
    if kind == "ramp":
        return (dmax * xx) // max(w - 1, 1)
    if kind == "steps":
        return np.asarray(steps, np.int64)[(len(steps) * xx) // w]
    raise ValueError(kind)


def stereo_pair_field(seed, w=640, h=480, kind="const", noise=3, offset=0, **field):
    """left = S(seed); right(y, x - D(y, x)) = left(y, x) for the disparity field D of disparity_field(kind, ...), written
    left to right, so where D jumps up the nearer (later) pixel wins and where it drops the right image keeps a fill of
    its own (the band the left view cannot see); plus uniform noise in [-noise, noise] and a brightness offset on the right image (the
    SAD subtracts each window's centre pixel, so a uniform offset away from the clip range does not change a match)."""
    rng = np.random.default_rng(1000 + seed)
    left = synth_frame(seed, h, w)
    D = disparity_field(kind, w, h, **field)
    right = synth_frame(seed + 7919, h, w).astype(np.int32)   # what no left pixel lands on (occluded in the left view)
    ys, xs = np.mgrid[0:h, 0:w]
    xr = xs - D
    ok = xr >= 0
    right[ys[ok], xr[ok]] = left[ok]
    if noise:
        right += rng.integers(-noise, noise + 1, right.shape)
    right = np.clip(right + offset, 0, 255).astype(np.uint8)
    return left, right


# ---- hand-placed keypoints --------------------------------------------------------------------------------------------------
# orbfe_stereo_matches and the oracle take the caller's keypoint lists, so after both sides have extracted the pair (which
# builds the pyramids the SAD reads), the same hand-built lists go to both.  Each hand case is the real extraction's lists
# with hand-placed keypoints appended; every appended left keypoint has a descriptor of its own, shared only with the right
# keypoints placed for it, so it meets no other candidate (random descriptors are ~128 bits apart, the search keeps < 100).
HAND_CASES = ("band", "edge", "zero", "maxd")


def _f32(v):
    return np.float32(v)


def _roundf(v):
    """roundf of a float32 >= 0 (half away from zero)"""
    return int(np.floor(np.float64(np.float32(v)) + 0.5))


def _kps(rows):
    from oracle.oracle_ffi import KP_DTYPE
    k = np.zeros(len(rows), KP_DTYPE)
    for i, (x, y, o) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
        k[i]["size"], k[i]["response"] = 31.0, 1.0
    return k


def _mirror_patch(left, right, c, y0, half_w=12, half_h=7):
    """left mirror-symmetric about column c in rows y0 +- half_h, and right = left there"""
    for k in range(1, half_w + 1):
        left[y0 - half_h:y0 + half_h + 1, c + k] = left[y0 - half_h:y0 + half_h + 1, c - k]
    right[y0 - half_h:y0 + half_h + 1, c - half_w:c + half_w + 1] = left[y0 - half_h:y0 + half_h + 1, c - half_w:c + half_w + 1]


def _level0_refined(left, right, c, y):
    """bestuR of the SAD search (:752-815) for a level-0 left keypoint at column c, row y whose partner rounds to c too, or
    None unless the minimum is at shift 0 (then bestuR = c + deltaR, and a left keypoint at x = bestuR has disparity 0)"""
    f = np.float32
    IL = left[y - 5:y + 6, c - 5:c + 6].astype(np.int64) - int(left[y, c])
    dists = [int(np.abs(IL - (right[y - 5:y + 6, c + i - 5:c + i + 6].astype(np.int64) - int(right[y, c + i]))).sum())
             for i in range(-5, 6)]
    if int(np.argmin(dists)) != 5:
        return None
    d1, d2, d3 = f(dists[4]), f(dists[5]), f(dists[6])
    deltaR = f(f(d1 - d3) / f(f(2.0) * f(f(d1 + d3) - f(f(2.0) * d2))))
    uR = f(f(1.0) * f(f(c) + deltaR))
    return uR if _roundf(uR) == c and deltaR != 0 else None

def hand_case(name, oracle):
    """-> dict(left, right, ext (nfeatures, scale factor, nlevels), mbf, mb, kL, dL, kR, dR, nreal (left, right), expect)
    expect: label -> (left index, True if the oracle must keep a match there, False if it must have none)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    w, h, ext, mbf, mb = 640, 480, (1000, 1.2, 8), 40.0, 0.08
    if name == "edge":
        left, right = stereo_pair_field(31, w, h, kind="const", d=3, noise=2)
    elif name == "maxd":
        left, right = stereo_pair_field(32, w, h, kind="const", d=8, noise=2)
        mbf, mb = 7.5, 1.0   # maxD = 7.5 < the true disparity
    else:
        left, right = stereo_pair_field(30 if name == "band" else 33, w, h, kind="const", d=8, noise=2)
    L, R = [], []   # appended left (x, y, octave, label, expect) / right (x, y, octave, partner label)
    if name == "band":
        # the row band [floor(y - r), ceil(y + r)] of a right keypoint, r = 2 * scale[octave]: its two edges, one row outside each
        for j, (dy, o, inside) in enumerate([(3.0, 1, True), (3.5, 1, False), (-3.0, 1, True), (-3.5, 1, False),
                                             (2.0, 0, True), (2.5, 0, True), (3.0, 0, False), (-2.0, 0, True),
                                             (-2.75, 0, True), (-3.0, 0, False)]):
            Y, X = 60 + 36 * j, 120.0
            L.append((X, float(Y), 0, f"band{j}", inside))
            R.append([(X - 8, Y + dy, o, f"band{j}")])
        # the octave band levelL +- 1: left keypoints on level 2 (and 0), one right partner each on another octave
        for j, (lo, ro) in enumerate([(2, 0), (2, 1), (2, 2), (2, 3), (2, 4), (0, 0), (0, 1), (0, 2)]):
            Y, X = 70 + 44 * j, 300.0
            L.append((X, float(Y), lo, f"oct{lo}_{ro}", abs(lo - ro) <= 1))
            R.append([(X - 8, float(Y), ro, f"oct{lo}_{ro}")])
        # the SAD minimum at the search's ends: the partner 5 (rejected) or 4 (kept) pixels right of the true match
        for j, (sh, keep) in enumerate([(5, False), (-5, False), (4, True), (-4, True)]):
            Y, X = 90 + 50 * j, 450.0
            L.append((X, float(Y), 0, f"inc{sh}", keep))
            R.append([(X - 8 + sh, float(Y), 0, f"inc{sh}")])
        # equal Hamming distances: copies of one descriptor at several right indices across the wave's lanes and strides;
        # the lowest index holds the true match; the others sit 5+ pixels off it, where the SAD search rejects them
        L.append((540.0, 300.0, 0, "tie_low", True))
        R.append([(532.0, 300.0, 0, "tie_low")] + [(532.0 + dx, 300.0, 0, "tie_low") for dx in (5, -5, 7)])
        L.append((540.0, 360.0, 0, "tie_dist", True))   # distance 1 at a lower index than distance 0 (the true match)
        R.append([(537.0, 360.0, 0, "tie_dist~1"), (532.0, 360.0, 0, "tie_dist")])
    elif name == "edge":
        # endu = scaleduR0 + 11 against the level width: w - 1 (kept) and w (rejected), on levels 0 and 1
        for j, lev in enumerate((0, 1)):
            s = ext[1] ** lev
            wl = int(oracle.OracleExtractor(*ext).level_sizes(w, h)[0][lev])
            inv = oracle.OracleExtractor(*ext).scales()[1][lev]
            for k, (col, keep) in enumerate(((wl - 12, True), (wl - 11, False))):
                uR0 = _f32(col * s)
                while _roundf(_f32(uR0 * inv)) > col:
                    uR0 = np.nextafter(uR0, _f32(0))
                while _roundf(_f32(uR0 * inv)) < col:
                    uR0 = np.nextafter(uR0, _f32(1e9))
                Y = 100 + 120 * j + 50 * k
                L.append((float(uR0 + 3), float(Y), lev, f"endu{lev}_{'w-1' if keep else 'w'}", keep))
                R.append([(float(uR0), float(Y), lev, f"endu{lev}_{'w-1' if keep else 'w'}")])
    elif name == "zero":
        # disparity exactly 0: left mirror-symmetric about column c, right = left around it, both keypoints at x = c
        for j in range(3):
            c, y0 = 100 + 80 * j, 80 + 60 * j
            _mirror_patch(left, right, c, y0)
            L.append((float(c), float(y0), 0, f"zero{j}", True))
            R.append([(float(c), float(y0), 0, f"zero{j}")])
        # ... and with uL fractional: right = left around c (no mirror), uL = the refined bestuR = c + deltaR itself.  (For
        # every float uL >= 1, float((double)uL - 0.01) has the same bits as uL - 0.01f: no value here can tell them apart.)
        j, c, y0 = 3, 340, 260
        while j < 6:
            c += 1
            right[y0 - 7:y0 + 8, c - 12:c + 13] = left[y0 - 7:y0 + 8, c - 12:c + 13]
            uL = _level0_refined(left, right, c, y0)
            if uL is not None:
                L.append((float(uL), float(y0), 0, f"zero{j}", True))
                R.append([(float(uL), float(y0), 0, f"zero{j}")])
                j, c, y0 = j + 1, c + 30, y0 + 40
    elif name == "maxd":
        # the partner one pixel inside maxD of the search range; the SAD moves it to the true disparity 8 >= maxD
        for j in range(4):
            X, Y = 150.0 + 100 * j, 100.0 + 70 * j
            L.append((X, Y, 0, f"maxd{j}", False))
            R.append([(X - 7, Y, 0, f"maxd{j}")])
    exL, exR = oracle.OracleExtractor(*ext, 20, 7), oracle.OracleExtractor(*ext, 20, 7)
    kL, dL = exL(left)
    kR, dR = exR(right)
    nl0, nr0 = len(kL), len(kR)
    # right list: the real keypoints, then filler up to a few waves of lanes, then the partners at spread indices
    desc = {}
    for x, y, o, lab, _ in L:
        desc[lab] = rng.integers(0, 256, 32, dtype=np.uint8)
    if name == "band":
        desc["tie_dist~1"] = desc["tie_dist"].copy()
        desc["tie_dist~1"][0] ^= 1
    nfill = 300
    rk = [(float(rng.integers(60, w - 60)), float(rng.integers(40, h - 40)), int(rng.integers(0, 3)), None) for _ in range(nfill)]
    slots = iter(rng.permutation(np.arange(5, nfill)))
    fixed = {"tie_low": [70, 135, 199, 260], "tie_dist~1": [20], "tie_dist": [150]}   # lanes 6 / 7 / 7 / 4 of strides 1..4
    taken = set(a for v in fixed.values() for a in v)
    slots = iter(a for a in slots if a not in taken)
    dR_extra = rng.integers(0, 256, (nfill, 32), dtype=np.uint8)
    for group in R:
        for x, y, o, lab in group:
            at = fixed[lab].pop(0) if lab in fixed else int(next(slots))
            rk[at] = (x, y, o, lab)
            dR_extra[at] = desc[lab]
    kL = np.concatenate([kL, _kps([(x, y, o) for x, y, o, _, _ in L])])
    dL = np.concatenate([dL, np.stack([desc[lab] for *_, lab, _ in L])])
    kR = np.concatenate([kR, _kps([(x, y, o) for x, y, o, _ in rk])])
    dR = np.concatenate([dR, dR_extra])
    expect = {lab: (nl0 + i, keep) for i, (*_, lab, keep) in enumerate(L)}
    hand_domain_ok(oracle, exL, kL[nl0:], kR[nr0:], w, h)
    return dict(left=left, right=right, ext=ext, mbf=mbf, mb=mb, kL=kL, dL=dL, kR=kR, dR=dR, nreal=(nl0, nr0), expect=expect,
                exL=exL, exR=exR)


def hand_domain_ok(oracle, ex, kL, kR, w, h):
    """the reference's defined domain: every left keypoint's 11 x 11 window at its level inside the level (so the SAD rows
    are too), every right keypoint's row band inside the image rows, every right keypoint's scaled column - 10 >= 0 on the
    levels it can be matched from (so colRange never asserts)"""
    ext_sc, ext_inv = ex.scales()[0], ex.scales()[1]
    lw, lh = ex.level_sizes(w, h)
    for k in kL:
        lev, inv = int(k["octave"]), ext_inv[int(k["octave"])]
        cu, cv = _roundf(_f32(k["x"] * inv)), _roundf(_f32(k["y"] * inv))
        assert 5 <= cu < lw[lev] - 5 and 5 <= cv < lh[lev] - 5, (k, lev)
        assert 0 <= int(k["y"]) < h
    for k in kR:
        o = int(k["octave"])
        r = _f32(_f32(2.0) * ext_sc[o])
        assert np.floor(_f32(k["y"] - r)) >= 0 and np.ceil(_f32(k["y"] + r)) < h, k
        for lev in range(max(0, o - 1), min(len(lw), o + 2)):
            assert _roundf(_f32(k["x"] * ext_inv[lev])) - 10 >= 0, (k, lev)

def test_oracle_stereo_sane(oracle):
    left, right = stereo_pair(5)
    exL, exR = oracle.OracleExtractor(), oracle.OracleExtractor()
    kL, dL = exL(left)
    kR, dR = exR(right)
    u, dep, sad = oracle.stereo_matches(exL, exR, kL, dL, kR, dR, 40.0, 0.08)
    ok = u >= 0
    assert ok.sum() > 100
    disp = kL["x"][ok] - u[ok]
    expect = 4 + (20 * kL["y"][ok].astype(np.int64)) // 480
    assert np.median(np.abs(disp - expect)) < 1.0  # recovers the synthetic disparity
    assert np.allclose(dep[ok], np.float32(40.0) / disp.astype(np.float32), rtol=1e-6)
    assert np.all(dep[~ok] == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,mbf,mb", [(5, 40.0, 0.08), (6, 386.1448, 0.537), (7, 40.0, 4.0)])
def test_gpu_stereo_parity(oracle, seed, mbf, mb):
    from orb_slam2_ssd_semantic_amd import ORBextractor, ORBmatcher
    left, right = stereo_pair(seed)
    exL, exR = oracle.OracleExtractor(), oracle.OracleExtractor()
    kL, dL = exL(left)
    kR, dR = exR(right)
    ru, rd, _ = oracle.stereo_matches(exL, exR, kL, dL, kR, dR, mbf, mb)
    gl = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    gr = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    gkL, gdL = gl(left)
    gkR, gdR = gr(right)
    assert np.array_equal(gdL, dL) and np.array_equal(gdR, dR)
    mt = ORBmatcher(0.9, True)
    u, d = mt.ComputeStereoMatches(gl, gr, gkL, gdL, gkR, gdR, mbf, mb)
    assert (ru >= 0).sum() > 50
    assert np.array_equal(u.view(np.uint32), ru.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32))


@pytest.mark.gpu
def test_gpu_stereo_no_matches(oracle):
    from orb_slam2_ssd_semantic_amd import ORBextractor, ORBmatcher
    left = synth_frame(8, 480, 640)
    right = synth_frame(9, 480, 640)  # unrelated image: few or no accepted matches
    gl = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    gr = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
    kL, dL = gl(left)
    kR, dR = gr(right)
    exL, exR = oracle.OracleExtractor(), oracle.OracleExtractor()
    okL, odL = exL(left)
    okR, odR = exR(right)
    ru, rd, _ = oracle.stereo_matches(exL, exR, okL, odL, okR, odR, 40.0, 0.08)
    u, d = ORBmatcher(0.9, True).ComputeStereoMatches(gl, gr, kL, dL, kR, dR, 40.0, 0.08)
    assert np.array_equal(u.view(np.uint32), ru.view(np.uint32)) and np.array_equal(d.view(np.uint32), rd.view(np.uint32))


@pytest.mark.gpu
def test_gpu_stereo_batch_device_chain(oracle):
    """Device-resident chain: two batched extractor calls (left / right images of 10 stereo pairs, one of them an unrelated
    pair) and orbfe_stereo_matches_batch_device on their output blocks, on one stream, no host buffer in between; every
    frame pair against the oracle chain (mvuRight / mvDepth bit patterns)."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor, ORBmatcher
    w, h, B = 640, 480, 10
    pairs = [stereo_pair(20 + i) for i in range(B)]
    pairs[4] = (synth_frame(8, h, w), synth_frame(9, h, w))
    L = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    R = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    gl = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    gr = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = gl.capacity()
    out = {}
    st = torch.cuda.current_stream().cuda_stream
    for name, e, img in (("L", gl, L), ("R", gr, R)):
        dk = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        dd = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        dn = torch.zeros(B, dtype=torch.int32, device="cuda")
        e.extract_batch_device(img.data_ptr(), B, w, h, w, w * h, dk.data_ptr(), dd.data_ptr(), cap, dn.data_ptr(), st)
        out[name] = (dk, dd, dn)
    du = torch.full((B, cap), 7.0, dtype=torch.float32, device="cuda")
    dz = torch.full((B, cap), 7.0, dtype=torch.float32, device="cuda")
    mbf, mb = 40.0, 0.08
    ORBmatcher(0.9, True).ComputeStereoMatches_batch_device(gl, gr, out["L"][0].data_ptr(), out["L"][1].data_ptr(), out["L"][2].data_ptr(),
                                                            out["R"][0].data_ptr(), out["R"][1].data_ptr(), out["R"][2].data_ptr(), cap, B,
                                                            mbf, mb, du.data_ptr(), dz.data_ptr(), st)
    torch.cuda.synchronize()
    nL = out["L"][2].cpu().numpy()
    u, z = du.cpu().numpy(), dz.cpu().numpy()
    total = 0
    for i, (left, right) in enumerate(pairs):
        exL, exR = oracle.OracleExtractor(), oracle.OracleExtractor()
        kL, dL = exL(left)
        kR, dR = exR(right)
        assert nL[i] == len(kL)
        assert np.array_equal(out["L"][0][i, :nL[i]].cpu().numpy().copy().view(KP_DTYPE).reshape(-1).view(np.uint8), kL.view(np.uint8))
        ru, rd, _ = oracle.stereo_matches(exL, exR, kL, dL, kR, dR, mbf, mb)
        assert np.array_equal(u[i, :nL[i]].view(np.uint32), ru.view(np.uint32)), i
        assert np.array_equal(z[i, :nL[i]].view(np.uint32), rd.view(np.uint32)), i
        assert np.all(u[i, nL[i]:] == 7.0) and np.all(z[i, nL[i]:] == 7.0)   # slots past the count are not touched
        total += int((ru >= 0).sum())
    assert total > 1000

"""Randomised parity sweeps and the sequence-scale check (BASELINE config 2), HIP path vs the CPU oracle.  GPU only.

Fixed seeds, bounded counts: 100 extractor + 100 matcher + 30 caller (grid / distinctive / BoW / stereo) + 30
device-API cases, then one batched device call over 200 frames S(seed) and 96 frames S_tum(seed) in BOTH FAST
variants.  Integer / bit-pattern work: everything must be identical.  ORBFE_FUZZ_SCALE scales the counts
(tools/fuzz_parity.py runs this file with a larger scale)."""
import os

import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame, synth_tum_like

pytestmark = pytest.mark.gpu
SCALE = float(os.environ.get("ORBFE_FUZZ_SCALE", "1"))


def _n(base):
    return max(1, int(round(base * SCALE)))


def _same(gk, gd, ok, od):
    return (len(gk) == len(ok) and np.array_equal(gd, od)
            and all(np.array_equal(gk[f].view(np.uint32), ok[f].view(np.uint32)) for f in ok.dtype.names))


def test_fuzz_extractor(oracle):
    from orb_slam2_ssd_semantic_amd import ORBextractor, OrbfeError
    rng = np.random.default_rng(1)
    ran = 0
    for c in range(_n(100)):
        w, h = int(rng.integers(180, 1000)), int(rng.integers(160, 760))
        sf = float(np.float32(rng.choice([1.1, 1.2, 1.25, 1.3, 1.4, 1.5, 1.7])))
        # most cases keep the smallest level large enough for one FAST cell; one in five may not (rejection path)
        fit = int(np.floor(np.log(min(w, h) / 66.0) / np.log(sf))) + 1
        nlev = int(rng.integers(1, 9)) if rng.random() < 0.2 else int(rng.integers(1, max(2, min(8, fit) + 1)))
        nf = int(rng.integers(50, 3000))
        ini = int(rng.integers(8, 40))
        mn = int(rng.integers(1, ini + 1))
        kind = int(rng.integers(0, 3))
        seed = int(rng.integers(0, 1 << 30))
        img = synth_tum_like(seed, h, w) if kind == 2 else synth_frame(seed, h, w, sparse=bool(kind))
        if rng.random() < 0.2:  # flat regions: empty cells exercise the minTh fallback and tiny trees
            y0, x0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
            img[y0:y0 + h // 3, x0:x0 + w // 3] = 128
        br = (c >> 1) & 1   # GaussianBlur column rounding: 0 = half-up, 1 = the SSE2 kernel's half-to-even
        tag = f"case {c}: {w}x{h} nf={nf} nlev={nlev} sf={sf:.2f} th={ini}/{mn} kind={kind} blur_rounding={br}"
        try:
            e = ORBextractor(nf, sf, nlev, ini, mn, max_width=w, max_height=h, blur_rounding=br)
            e.set_fast_mode(c & 3)   # dense / sparse shortcuts / lane-compacting / auto
            gk, gd = e(img)
        except OrbfeError:
            continue  # sizes the boundary rejects (level too small for one cell, > 4 quadtree roots, per-level cap)
        oe = oracle.OracleExtractor(nf, sf, nlev, ini, mn)
        oe.set_blur_mode(br)
        ok, od = oe(img, cap=nf + 16 * nlev + 256)
        assert _same(gk, gd, ok, od), tag
        for l in range(nlev):
            if len(oe.selected(l)):   # the reference blurs only the levels that hold keypoints (:1090)
                assert np.array_equal(e.blurred_level(l), oe.blurred(l)), (tag, l)
        assert e.overflow() == 0, tag
        ran += 1
    assert ran >= 0.6 * _n(100), ran


def test_fuzz_matcher(oracle):
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    rng = np.random.default_rng(2)
    for c in range(_n(100)):
        nq, nt = int(rng.integers(0, 2500)), int(rng.integers(0, 2500))
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        if nt and nq:
            q = t[rng.integers(0, nt, nq)].copy()
            flips = int(rng.integers(0, 70))
            if flips:
                bits = rng.integers(0, 256, (nq, flips))
                for j in range(flips):
                    q[np.arange(nq), bits[:, j] >> 3] ^= (1 << (bits[:, j] & 7)).astype(np.uint8)
            if rng.random() < 0.5:  # duplicate train rows: first index must win, second == best
                t[rng.integers(0, nt, nt // 4)] = t[rng.integers(0, nt, nt // 4)]
        qa = rng.uniform(0, 360, nq).astype(np.float32)
        ta = rng.uniform(0, 360, nt).astype(np.float32)
        ratio, th, ori = float(rng.choice([0.6, 0.75, 0.9])), int(rng.choice([50, 100])), bool(rng.integers(0, 2))
        got = ORBmatcher(ratio, ori).MatchBruteForce(q, t, qa, ta, th)
        ref = oracle.match_bf(q, t, qa, ta, ratio, th, ori)
        assert all(np.array_equal(g, r) for g, r in zip(got[:3], ref[:3])) and got[3] == ref[3], (c, nq, nt)


def test_fuzz_callers(oracle):
    """The callers either side of the path: generators of the unit tests, fresh seeds."""
    from test_bow import make_voc
    from test_distinctive import make_case
    from test_grid import grid_case, queries
    from test_stereo import stereo_pair
    from orb_slam2_ssd_semantic_amd import FrameGrid, ORBextractor, ORBmatcher, ORBVocabulary
    rng = np.random.default_rng(4)
    mt = ORBmatcher(0.9, True)
    for c in range(_n(30)):
        sd = int(rng.integers(0, 1 << 20))
        xy, octave, minx, miny, gwi, ghi = grid_case(sd, int(rng.integers(0, 3000)))
        g = FrameGrid(mt, xy, octave, minx, miny, gwi, ghi)
        off, idx = oracle.assign_grid(xy, minx, miny, gwi, ghi)
        assert np.array_equal(g.cell_off, off) and np.array_equal(g.cell_idx, idx), (c, sd)
        q, lv = queries(sd, int(rng.integers(0, 400)))
        qoff, cand = g.query(q, lv)
        for i in range(len(q)):
            ref = oracle.features_in_area(xy, octave, off, idx, minx, miny, gwi, ghi, float(q[i, 0]), float(q[i, 1]),
                                          float(q[i, 2]), int(lv[i, 0]), int(lv[i, 1]))
            assert np.array_equal(cand[qoff[i]:qoff[i + 1]], ref), (c, sd, i)
        pool, doff, didx = make_case(sd, int(rng.integers(0, 400)), int(rng.integers(1, 90)))
        b, m = mt.ComputeDistinctiveDescriptors(pool, doff, didx)
        rb, rm = oracle.distinctive(pool, doff, didx)
        assert np.array_equal(b, rb) and np.array_equal(m, rm), (c, sd)
        voc = make_voc(sd, int(rng.integers(2, 11)), int(rng.integers(1, 5)))
        desc = rng.integers(0, 256, (int(rng.integers(0, 3000)), 32), dtype=np.uint8)
        lu = int(rng.integers(0, 5))
        r = oracle.bow_transform(voc, desc, lu)
        (bid, bval), (fvn, fvo, fvi) = ORBVocabulary(mt, **voc).transform(desc, lu)
        assert np.array_equal(bid, r["bow_id"]) and np.array_equal(bval.view(np.uint64), r["bow_val"].view(np.uint64))
        assert np.array_equal(fvn, r["fv_node"]) and np.array_equal(fvo, r["fv_off"]) and np.array_equal(fvi, r["fv_idx"])
        if c < 3:
            left, right = stereo_pair(sd % 1000)
            exL, exR = oracle.OracleExtractor(), oracle.OracleExtractor()
            kL, dL = exL(left)
            kR, dR = exR(right)
            mbf, mb = float(rng.uniform(20, 400)), float(rng.uniform(0.05, 2.0))
            ru, rd, _ = oracle.stereo_matches(exL, exR, kL, dL, kR, dR, mbf, mb)
            gl = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
            gr = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480)
            gkL, gdL = gl(left)
            gkR, gdR = gr(right)
            u, d = mt.ComputeStereoMatches(gl, gr, gkL, gdL, gkR, gdR, mbf, mb)
            assert np.array_equal(u.view(np.uint32), ru.view(np.uint32)), (c, sd)
            assert np.array_equal(d.view(np.uint32), rd.view(np.uint32)), (c, sd)


def _device_batch(e, buf, B, w, h, stride, fstride):
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    cap = e.capacity()
    d_gray = torch.from_numpy(buf).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_gray.data_ptr(), B, w, h, stride, fstride, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                           d_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy()
    desc = d_desc.cpu().numpy()
    assert e.overflow() == 0
    return [(kps[i, :n[i]].copy().view(KP_DTYPE).reshape(-1), desc[i, :n[i]]) for i in range(B)], (kps, desc, n)


def test_fuzz_device_api(oracle):
    """Odd widths, row strides, frame strides, batch sizes, exactly sized input buffers."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    rng = np.random.default_rng(3)
    ran = 0
    for c in range(_n(30)):
        w, h = int(rng.integers(200, 900)), int(rng.integers(180, 700))
        B = int(rng.choice([1, 2, 3, 5, 8, 9, 16, 24]))
        nf = int(rng.integers(100, 1500))
        stride = w + int(rng.choice([0, 0, 1, 3, 4, 7, 64]))
        fstride = stride * (h - 1) + w + int(rng.choice([0, 0, 1, 5, 64, 4096]))
        buf = np.zeros(fstride * (B - 1) + stride * (h - 1) + w, np.uint8)  # exactly sized: not one byte of slack
        imgs = []
        for i in range(B):
            img = synth_frame(int(rng.integers(0, 1 << 30)), h, w, sparse=bool(rng.integers(0, 2)))
            imgs.append(img)
            rows = np.lib.stride_tricks.as_strided(buf[i * fstride:], (h, w), (stride, 1))
            rows[...] = img
        try:
            e = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
        except Exception:
            continue
        e.set_fast_mode(c & 3)
        res, _ = _device_batch(e, buf, B, w, h, stride, fstride)
        oe = oracle.OracleExtractor(nf, 1.2, 8, 20, 7)
        for i in sorted(set([0, B - 1, int(rng.integers(0, B))])):
            ok, od = oe(imgs[i], cap=e.capacity() + 64)
            assert _same(res[i][0], res[i][1], ok, od), (c, w, h, stride, fstride, B, nf, i)
        ran += 1
    assert ran >= 0.6 * _n(30)


@pytest.mark.gpu
def test_auto_fast_mode_is_the_default_small_batches_stay_dense(oracle):
    """orbfe_set_fast_mode 3 is what a fresh handle runs: calls that do not fill the GPU (8 VGA frames here) take the dense form (no probe: the counters
    stay zero); a larger batch of camera-like frames runs the lane-compacting form and leaves the pass rate of a sample of its
    waves behind; results equal the oracle's either way."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    w, h = 640, 480
    B = 40
    frames = np.stack([synth_tum_like(900 + s, h, w) for s in range(B)])
    oe = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)   # no set_fast_mode: the default
    res, _ = _device_batch(e, frames[:8].reshape(-1), 8, w, h, w, w * h)
    for i in (0, 7):
        ok, od = oe(frames[i])
        assert _same(res[i][0], res[i][1], ok, od)
    assert e.fast_stats(reset=False)["row_steps"] == 0          # small call: dense, nothing probed
    for _ in range(2):                                          # the first large call probes, the second reads the probe
        res, _ = _device_batch(e, frames.reshape(-1), B, w, h, w, w * h)
    for i in (0, 17, B - 1):
        ok, od = oe(frames[i])
        assert _same(res[i][0], res[i][1], ok, od)
    st = e.fast_stats(reset=False)
    assert st["row_steps"] > 0 and 0.05 < st["parked_pairs"] / (128.0 * st["row_steps"]) < 0.45, st
    e.close()


@pytest.mark.parametrize("gen,nframes", [("S", 200), ("S_tum", 96)])
def test_sequence_batched_device_call(oracle, gen, nframes):
    """BASELINE config 2 on the synthetic stand-in for the TUM sequence: N frames through ONE batched device call, every
    frame's count, keypoint bit patterns, descriptor bytes and order against the oracle -- in every FAST variant (dense, sparse
    shortcuts, lane-compacting, auto), whose padded output buffers must also be identical byte for byte; the compacting kernel's
    pass-rate statistics separate the two workloads (S: most pixel pairs pass the necessary test, S_tum: under half)."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    B = _n(nframes)
    w, h = 640, 480
    make = synth_frame if gen == "S" else synth_tum_like
    frames = np.stack([make(s, h, w) for s in range(B)])
    e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    oe = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    expect = [oe(f) for f in frames]
    raws = []
    rate = None
    for it, mode in enumerate((0, 1, 2, 3, 3)):   # dense, sparse shortcuts, lane-compacting, auto (the first call probes, the second follows the probe)
        if it < 4:
            e.set_fast_mode(mode, collect_stats=True)
        res, raw = _device_batch(e, frames.reshape(-1), B, w, h, w, w * h)
        for i in range(B):
            assert _same(res[i][0], res[i][1], expect[i][0], expect[i][1]), (gen, mode, i)
        raws.append(raw)
        st = e.fast_stats()
        if mode == 1:
            assert st["row_steps"] > 0
        if mode == 2:   # {row steps, batches, parked pairs} of the sampled waves: the share of pixel pairs passing the necessary test
            assert st["row_steps"] > 0 and st["arc_skips"] > 0
            rate = st["nms_skips"] / (128.0 * st["row_steps"])
            assert (rate > 0.6) if gen == "S" else (0.05 < rate < 0.45), rate   # S ~0.85, S_tum ~0.19
    for r in raws[1:]:
        for a, b in zip(raws[0], r):
            assert np.array_equal(a, b)
    st = e.fast_stats()   # auto mode: the last probe that completed
    assert st["row_steps"] > 0 and abs(st["nms_skips"] / (128.0 * st["row_steps"]) - rate) < 0.05
    ncand = [sum(len(oe.candidates(l)) for l in range(8))]
    assert (ncand[0] > 20000) if gen == "S" else (1000 < ncand[0] < 12000)


def test_tum_sequence(oracle, tmp_path):
    """BASELINE config 2 on the real sequence when it is present ($TUM_FR3_WALKING_XYZ); elsewhere on a miniature sequence in
    the same layout (rgb/<timestamp>.png + associate.txt) made of the committed 640x480 photographs of tests/golden/real/vga.
    Every associated frame goes through the caller's gray conversion and batched device calls, compared per frame with the
    oracle."""
    import shutil
    from orb_slam2_ssd_semantic_amd import ORBextractor, photos, tum
    seq = tum.sequence_dir()
    if seq is None:
        seq = str(tmp_path)
        os.makedirs(os.path.join(seq, "rgb"))
        names = sorted(f for f in os.listdir(os.path.join(photos.ROOT, "vga")) if f.endswith(".png"))
        with open(os.path.join(seq, "associate.txt"), "w") as f:
            for i, name in enumerate(names):
                t = 1341846313.5 + i * 0.03
                shutil.copy(os.path.join(photos.ROOT, "vga", name), os.path.join(seq, "rgb", f"{t:.6f}.png"))
                f.write(f"{t:.6f} rgb/{t:.6f}.png {t + 0.01:.6f} depth/{t + 0.01:.6f}.png\n")
    frames = tum.load_gray_frames(seq)
    N, h, w = frames.shape
    e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=128)
    oe = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    for lo in range(0, N, 128):
        blk = np.ascontiguousarray(frames[lo:lo + 128])
        res, _ = _device_batch(e, blk.reshape(-1), len(blk), w, h, w, w * h)
        for i, (gk, gd) in enumerate(res):
            ok, od = oe(blk[i])
            assert _same(gk, gd, ok, od), lo + i

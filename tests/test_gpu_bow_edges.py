"""k_bow_descend / k_bow_aggregate (orbfe_bow_transform, orbfe_bow_transform_batch_device) and k_distinctive
(orbfe_distinctive_descriptors, ..._device) against the CPU oracle on the edge cases of tests/bow_cases.py, bit for bit:
ids, CSR arrays and counts by array_equal, doubles through their uint64 patterns.  No tolerance anywhere.

What the cases are for is written next to each of them in bow_cases.py (`doc`); tests/test_bow_cases.py checks, on the CPU,
that they hold the plantings and the order-sensitive sums that make a reordered sum, a wrong tie rule or a wrong median
index show here."""
import ctypes as C
import os

import numpy as np
import pytest

import bow_cases as B
from test_bow_cases import oracle_transform, u64

pytestmark = pytest.mark.gpu

CAPS = (1, 1000, 1024, 8192)
OUT = (("f_word", 4, np.int32), ("f_node", 4, np.int32), ("f_weight", 8, np.float64), ("bow_id", 4, np.uint32),
       ("bow_val", 8, np.float64), ("fv_node", 4, np.uint32), ("fv_off", 4, np.uint32), ("fv_idx", 4, np.uint32),
       ("counts", 4, np.int32))


@pytest.fixture(scope="module")
def mt():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    return ORBmatcher(0.7, True)


_VOCS = {}


def device_voc(mt, voc):
    """one device vocabulary per case vocabulary (and matcher), kept for the module"""
    from orb_slam2_ssd_semantic_amd import ORBVocabulary
    key = (id(mt), id(voc))
    if key not in _VOCS:
        _VOCS[key] = (ORBVocabulary(mt, **voc), voc)
    return _VOCS[key][0]


def assert_host_form(got, r):
    (bid, bval), (fvn, fvo, fvi), (fw, fn, fwt) = got
    assert np.array_equal(fw, r["word"]) and np.array_equal(fn, r["node"]) and np.array_equal(u64(fwt), u64(r["weight"]))
    assert np.array_equal(bid, r["bow_id"]) and np.array_equal(u64(bval), u64(r["bow_val"]))
    assert np.array_equal(fvn, r["fv_node"]) and np.array_equal(fvo, r["fv_off"]) and np.array_equal(fvi, r["fv_idx"])


class Block:
    """The nine output blocks of orbfe_bow_transform_batch_device for B frames of `cap` slots, every byte prefilled with
    0x5A, and the input block; run() enqueues the transform on `stream` (the current one by default)."""

    def __init__(self, frames, cap):
        import torch
        self.B, self.cap, self.frames = len(frames), cap, frames
        B_ = self.B
        desc = np.zeros((B_, cap, 32), np.uint8)
        for b, (d, _) in enumerate(frames):
            desc[b, :len(d)] = d
        self.d_desc = torch.from_numpy(desc).cuda()
        self.d_n = torch.tensor([n for _, n in frames], dtype=torch.int32, device="cuda")
        self.slots = dict(fv_off=cap + 1, counts=4)
        self.t = {k: torch.full((B_ * self.slots.get(k, cap) * sz,), 0x5A, dtype=torch.uint8, device="cuda") for k, sz, _ in OUT}

    def run(self, V, levelsup, stream=None):
        import torch
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        V.transform_batch_device(self.d_desc.data_ptr(), self.d_n.data_ptr(), self.B, self.cap, levelsup,
                                 *[self.t[k].data_ptr() for k, _, _ in OUT], st)
        return self

    def host(self):
        return {k: self.t[k].cpu().numpy().view(dt).reshape(self.B, self.slots.get(k, self.cap)) for k, _, dt in OUT}

    def check(self, oracle, voc, levelsup, refs=None):
        """every documented extent of every frame equals the oracle's transform of the frame's first min(d_n, cap) rows"""
        h = self.host()
        for b, (d, dn) in enumerate(self.frames):
            n = min(dn, self.cap)
            r = refs[b] if refs and refs[b] is not None else oracle.bow_transform(voc, d[:n], levelsup)
            nb, nfv, nidx = (int(x) for x in h["counts"][b, :3])
            assert (nb, nfv, nidx) == (len(r["bow_id"]), len(r["fv_node"]), len(r["fv_idx"])), b
            assert np.array_equal(h["bow_id"][b, :nb], r["bow_id"]) and np.array_equal(u64(h["bow_val"][b, :nb]), u64(r["bow_val"])), b
            assert np.array_equal(h["fv_node"][b, :nfv], r["fv_node"]) and np.array_equal(h["fv_off"][b, :nfv + 1], r["fv_off"]), b
            assert np.array_equal(h["fv_idx"][b, :nidx], r["fv_idx"]), b
            assert np.array_equal(h["f_word"][b, :n], r["word"]) and np.array_equal(h["f_node"][b, :n], r["node"]), b
            assert np.array_equal(u64(h["f_weight"][b, :n]), u64(r["weight"])), b
            assert (h["f_word"][b, n:] == -1).all() and (h["f_node"][b, n:] == -1).all(), b      # padding slots: "no word"
            assert np.array_equal(u64(h["f_weight"][b, n:]), np.zeros(self.cap - n, np.uint64)), b
        return h


def fill(desc, cap, shift):
    """cap rows made of the case's rows, backwards and rotated"""
    return np.roll(np.resize(desc[::-1], (cap, 32)), shift, axis=0)


# ------------------------------------------------------------------------------------------------ transform, host form
@pytest.mark.parametrize("name", list(B.TRANSFORM_CASES))
def test_transform_host_form(oracle, mt, name):
    c = B.TRANSFORM_CASES[name]
    assert_host_form(device_voc(mt, c["voc"]).transform(c["desc"], c["levelsup"], per_feature=True), oracle_transform(oracle, name))


# ------------------------------------------------------------------------------------------------ transform, batched form
@pytest.mark.parametrize("name", list(B.TRANSFORM_CASES))
def test_transform_batched_form(oracle, mt, name):
    """the case as frame 0 of five; the others hold 0, 1, cap and cap + 7 (= cap) features"""
    import torch
    c = B.TRANSFORM_CASES[name]
    d, n = c["desc"], len(c["desc"])
    cap = min(x for x in CAPS if x >= n)
    frames = [(d, n), (d[:0], 0), (d[-1:], 1), (fill(d, cap, 3), cap), (fill(d, cap, 11), cap + 7)]
    blk = Block(frames, cap).run(device_voc(mt, c["voc"]), c["levelsup"])
    torch.cuda.synchronize()
    blk.check(oracle, c["voc"], c["levelsup"], refs=[oracle_transform(oracle, name)] + [None] * 4)


@pytest.mark.parametrize("name,cap,dn", [("widths[1]", 1, 1), ("widths[1]", 1, 8), ("widths[3]", 1, 0), ("widths[1023]", 1000, 1007),
                                         ("widths[1024]", 1024, 1024), ("widths[1025]", 1024, 1031), ("widths[8192]", 8192, 8199),
                                         ("widths[255]", 8192, 255), ("three_words", 8192, 8192)])
def test_transform_batched_form_single_frame(oracle, mt, name, cap, dn):
    import torch
    c = B.TRANSFORM_CASES[name]
    blk = Block([(c["desc"][:cap], dn)], cap).run(device_voc(mt, c["voc"]), c["levelsup"])
    torch.cuda.synchronize()
    blk.check(oracle, c["voc"], c["levelsup"])


def test_word_id_just_below_the_limit(oracle, mt):
    from orb_slam2_ssd_semantic_amd import ORBVocabulary
    voc = B.flat(3, [0.5, 1.5, 2.5], [(1 << 31) - 1, 5, 0])
    desc = B.random_rows(np.random.default_rng(1), 100)
    r = oracle.bow_transform(voc, desc, 0)
    assert r["bow_id"].tolist() == [0, 5, (1 << 31) - 1]
    assert_host_form(ORBVocabulary(mt, **voc).transform(desc, 0, per_feature=True), r)


# ------------------------------------------------------------------------------------------------ 0-feature frame -> SearchByBoW
def test_zero_feature_frame_through_search_by_bow(oracle, mt):
    import torch
    c = B.TRANSFORM_CASES["levels[1]"]
    d, n, cap = c["desc"], len(c["desc"]), 1000
    blk = Block([(d, n), (d[:0], 0)], cap).run(device_voc(mt, c["voc"]), c["levelsup"])
    d_kps = torch.zeros((2, cap, 7), dtype=torch.int32, device="cuda")
    pairs = [(0, 1), (1, 0), (1, 1), (0, 0)]
    d_kf = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
    d_f = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
    d_match = torch.full((len(pairs), cap), 77, dtype=torch.int32, device="cuda")
    d_nm = torch.full((len(pairs),), 77, dtype=torch.int32, device="cuda")
    mt.SearchByBoW_batch_device(d_kps.data_ptr(), blk.d_desc.data_ptr(), cap, None, blk.t["fv_node"].data_ptr(),
                                blk.t["fv_off"].data_ptr(), blk.t["fv_idx"].data_ptr(), blk.t["counts"].data_ptr(), d_kf.data_ptr(),
                                d_f.data_ptr(), len(pairs), d_match.data_ptr(), d_nm.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = blk.check(oracle, c["voc"], c["levelsup"])
    assert h["counts"][1, :3].tolist() == [0, 0, 0] and h["fv_off"][1, 0] == 0
    match, nm = d_match.cpu().numpy(), d_nm.cpu().numpy()
    for p in range(3):                       # the empty frame as F, as KF, on both sides: no match, a row of -1
        assert nm[p] == 0 and (match[p] == -1).all()
    r = oracle_transform(oracle, "levels[1]")
    fv = (r["fv_node"], r["fv_off"], r["fv_idx"])
    ang = np.zeros(n, np.float32)
    om, on = oracle.search_by_bow(d, None, ang, fv, d, None, ang, fv, mt.mfNNratio, 50, False, True)
    assert np.array_equal(match[3, :n], om) and (match[3, n:] == -1).all() and nm[3] == on and on > 100


# ------------------------------------------------------------------------------------------------ limits
def test_limits_are_refused_and_the_handle_goes_on(oracle, mt):
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi
    c = B.TRANSFORM_CASES["widths[257]"]
    V = device_voc(mt, c["voc"])
    with pytest.raises(_ffi.OrbfeError) as e:
        V.transform(B.random_rows(np.random.default_rng(0), B.BOW_MAX_FEATURES + 1), 1)
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    assert_host_form(V.transform(c["desc"], c["levelsup"], per_feature=True), oracle_transform(oracle, "widths[257]"))
    cap = B.BOW_MAX_FEATURES + 1
    blk = Block([(c["desc"], 257)], cap)
    with pytest.raises(_ffi.OrbfeError) as e:
        blk.run(V, 1)
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0x5A).all() for t in blk.t.values())          # nothing was launched
    blk = Block([(c["desc"], 257)], 1000).run(V, 1)
    torch.cuda.synchronize()
    blk.check(oracle, c["voc"], 1, refs=[oracle_transform(oracle, "widths[257]")])


# ------------------------------------------------------------------------------------------------ empty vocabulary
def _empty_by_arrays(mt, tmp_path):
    from orb_slam2_ssd_semantic_amd import ORBVocabulary
    return ORBVocabulary(mt, child_off=np.zeros(2, np.uint32), child_idx=np.zeros(0, np.uint32), node_desc=np.full((1, 32), 0xA5, np.uint8),
                         word_id=np.array([3], np.uint32), weight=np.array([2.5]), L=3)


def _header_only_file(tmp_path):
    from orb_slam2_ssd_semantic_amd import VocabularyFile
    path = os.path.join(tmp_path, "ORBvoc.txt")
    with open(path, "w") as f:
        f.write("10 6 0 0\n")
    vf = VocabularyFile(path)
    assert (vf.nnodes, vf.nwords) == (1, 0)
    return vf


def _empty_by_file(mt, tmp_path):
    return _header_only_file(tmp_path).to_device(mt)


def _empty_by_create_from_file(mt, tmp_path):
    from orb_slam2_ssd_semantic_amd import ORBVocabulary, _ffi
    vf = _header_only_file(tmp_path)
    V = ORBVocabulary.__new__(ORBVocabulary)
    V._mt, V._L, V._v = mt, _ffi.lib(), C.c_void_p()
    _ffi.check(V._L.orbfe_vocabulary_create_from_file(0, vf.handle, C.byref(V._v)), "orbfe_vocabulary_create_from_file")
    return V


@pytest.mark.parametrize("make", [_empty_by_arrays, _empty_by_file, _empty_by_create_from_file])
def test_empty_vocabulary(oracle, mt, tmp_path, make):
    """a root without children: every feature without a word, both vectors empty, in the host and the batched form; the
    matcher then serves another vocabulary as before"""
    import torch
    V = make(mt, tmp_path)
    desc = B.random_rows(np.random.default_rng(5), 1030)
    for n in (0, 1, 300, 1030):
        (bid, bval), (fvn, fvo, fvi), (fw, fn, fwt) = V.transform(desc[:n], 1, per_feature=True)
        assert len(bid) == len(bval) == len(fvn) == len(fvi) == 0 and fvo.tolist() == [0]
        assert len(fw) == n and (fw == -1).all() and (fn == -1).all() and np.array_equal(u64(fwt), np.zeros(n, np.uint64))
    for cap, dns in ((1000, (300, 0, 1, 1000, 1007)), (1, (1,))):
        blk = Block([(desc[:min(dn, cap)], dn) for dn in dns], cap).run(V, 1)
        torch.cuda.synchronize()
        h = blk.host()
        assert (h["counts"][:, :3] == 0).all() and (h["fv_off"][:, 0] == 0).all()
        assert (h["f_word"] == -1).all() and (h["f_node"] == -1).all() and (h["f_weight"].view(np.uint64) == 0).all()
    c = B.TRANSFORM_CASES["widths[1025]"]
    assert_host_form(device_voc(mt, c["voc"]).transform(c["desc"], c["levelsup"], per_feature=True), oracle_transform(oracle, "widths[1025]"))


# ------------------------------------------------------------------------------------------------ distinctive descriptors
_DREF = {}


def oracle_distinctive(oracle, name):
    if name not in _DREF:
        c = B.DISTINCTIVE_CASES[name]
        _DREF[name] = oracle.distinctive(c["pool"], c["off"], c["idx"])
        if c["expect"] is not None:
            assert np.array_equal(_DREF[name][0], c["expect"][0]) and np.array_equal(_DREF[name][1], c["expect"][1])
    return _DREF[name]


@pytest.mark.parametrize("name", list(B.DISTINCTIVE_CASES))
def test_distinctive_host_form(oracle, mt, name):
    c = B.DISTINCTIVE_CASES[name]
    b, m = mt.ComputeDistinctiveDescriptors(c["pool"], c["off"], c["idx"])
    rb, rm = oracle_distinctive(oracle, name)
    assert np.array_equal(b, rb) and np.array_equal(m, rm)


def distinctive_device(mt, c, max_obs):
    import torch
    npts = len(c["off"]) - 1
    dp = torch.from_numpy(c["pool"]).cuda()
    do = torch.from_numpy(c["off"].astype(np.int32)).cuda()
    di = torch.from_numpy(c["idx"].astype(np.int32)).cuda()
    db = torch.full((npts,), 99, dtype=torch.int32, device="cuda")
    dm = torch.full((npts,), 99, dtype=torch.int32, device="cuda")
    mt.ComputeDistinctiveDescriptors_device(dp.data_ptr(), do.data_ptr(), di.data_ptr(), npts, max_obs, db.data_ptr(), dm.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return db.cpu().numpy(), dm.cpu().numpy()


@pytest.mark.parametrize("name", list(B.DISTINCTIVE_CASES))
def test_distinctive_device_form(oracle, mt, name):
    c = B.DISTINCTIVE_CASES[name]
    b, m = distinctive_device(mt, c, int(np.diff(c["off"].astype(np.int64)).max()))
    rb, rm = oracle_distinctive(oracle, name)
    assert np.array_equal(b, rb) and np.array_equal(m, rm)


def test_distinctive_limits(oracle, mt):
    from orb_slam2_ssd_semantic_amd import _ffi
    c = B.DISTINCTIVE_CASES["sizes"]
    nobs = np.diff(c["off"].astype(np.int64))
    b, m = distinctive_device(mt, c, B.DD_MAX_OBS - 1)        # LDS sized for 1023: exactly the 1024-observation point is marked
    rb, rm = oracle_distinctive(oracle, "sizes")
    big = nobs == B.DD_MAX_OBS
    assert big.sum() == 1 and (b[big] == -2).all() and (m[big] == -2).all()
    assert np.array_equal(b[~big], rb[~big]) and np.array_equal(m[~big], rm[~big])
    pool = B.random_rows(np.random.default_rng(3), B.DD_MAX_OBS + 1)
    with pytest.raises(_ffi.OrbfeError) as e:
        mt.ComputeDistinctiveDescriptors(pool, np.array([0, B.DD_MAX_OBS + 1], np.uint32), np.arange(B.DD_MAX_OBS + 1, dtype=np.uint32))
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    c = B.DISTINCTIVE_CASES["equilateral"]
    b, m = mt.ComputeDistinctiveDescriptors(c["pool"], c["off"], c["idx"])
    assert np.array_equal(b, c["expect"][0]) and np.array_equal(m, c["expect"][1])


# ------------------------------------------------------------------------------------------------ two matchers, two streams
def test_two_matchers_on_two_streams(oracle):
    """The dynamic-LDS limit of k_bow_aggregate is a process-wide attribute of the kernel: a small sort of one matcher must
    not lower it under a 128 KiB sort of another.  Host form back to back, then the batched form enqueued on two streams
    without a host synchronisation in between."""
    import torch
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m1, m2 = ORBmatcher(0.7, True), ORBmatcher(0.7, True)
    voc = B.WIDTHS_VOC
    V1, V2 = device_voc(m1, voc), device_voc(m2, voc)
    w300 = B.widths(300)
    r300 = oracle.bow_transform(voc, w300["desc"], 1)
    for V, name in ((V1, "widths[4097]"), (V2, "widths[8192]")):
        assert_host_form(V.transform(B.TRANSFORM_CASES[name]["desc"], 1, per_feature=True), oracle_transform(oracle, name))
    assert_host_form(V1.transform(w300["desc"], 1, per_feature=True), r300)
    assert_host_form(V2.transform(B.TRANSFORM_CASES["widths[8192]"]["desc"], 1, per_feature=True), oracle_transform(oracle, "widths[8192]"))
    d4097, d8192 = B.TRANSFORM_CASES["widths[4097]"]["desc"], B.TRANSFORM_CASES["widths[8192]"]["desc"]
    blocks = [(Block([(d8192, 8192), (d4097, 4097)], 8192), V1, 0), (Block([(d4097, 4097)], 8192), V2, 1),
              (Block([(w300["desc"], 300)], 1000), V1, 0), (Block([(d8192, 8192)], 8192), V2, 1), (Block([(w300["desc"], 300)], 1000), V2, 1)]
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()               # the blocks were filled on the default stream
    for blk, V, si in blocks:
        blk.run(V, 1, stream=s[si].cuda_stream)
    torch.cuda.synchronize()
    refs = {8192: oracle_transform(oracle, "widths[8192]"), 4097: oracle_transform(oracle, "widths[4097]"), 300: r300}
    for blk, _, _ in blocks:
        blk.check(oracle, voc, 1, refs=[refs[dn] for _, dn in blk.frames])

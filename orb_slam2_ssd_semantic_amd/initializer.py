"""The reference's monocular Initializer (src/Initializer.cc) on the GPU: the H / F RANSAC over sets of eight matches, the model
choice, ReconstructH / ReconstructF with CheckRT and Triangulate, through the C-ABI of csrc/orbfe_initializer.hip.  The random
draws are an input (raw values in [0, 2^31 - 1], eight per iteration), so a run can be replayed.  No CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi, _ransac
from ._ffi import stream_arg, tensor_ptr

ABI, dtype = _ffi.ABI, _ffi.dtype
RESULT_DTYPE = dtype("orbfe_initializer_result", H21=(3, 3), F21=(3, 3), R21=(3, 3))
PAIR_DTYPE = dtype("orbfe_initializer_pair", K=(3, 3))
ITER_DTYPE = dtype("orbfe_initializer_iter", Hn=(3, 3), Fn=(3, 3), H21i=(3, 3), F21i=(3, 3))
MAX_ITERATIONS = ABI.ORBFE_INIT_MAX_ITERATIONS
STATUS_OK, STATUS_FEW_MATCHES, STATUS_BAD_INDEX, STATUS_NO_MODEL, STATUS_BAD_SIZES = (
    ABI.ORBFE_INIT_OK, ABI.ORBFE_INIT_FEW_MATCHES, ABI.ORBFE_INIT_BAD_INDEX, ABI.ORBFE_INIT_NO_MODEL, ABI.ORBFE_INIT_BAD_SIZES)
MODEL_NONE, MODEL_H, MODEL_F = range(3)   # orbfe_initializer_result.model; the header names no constants for it
TAP_ITERATIONS, TAP_MATCHES = ABI.ORBFE_INIT_TAP_ITERATIONS, ABI.ORBFE_INIT_TAP_MATCHES
(KAT_SVD16X9, KAT_SVD8X9, KAT_SVD3, KAT_SVD4, KAT_INV3, KAT_H21, KAT_F21, KAT_TRIANGULATE, KAT_PARALLAX) = (
    ABI.constants["ORBFE_INIT_KAT_" + k] for k in ("SVD16X9", "SVD8X9", "SVD3", "SVD4", "INV3", "H21", "F21", "TRIANGULATE", "PARALLAX"))
_KAT_IO = {KAT_SVD16X9: (144, 346), KAT_SVD8X9: (72, 153), KAT_SVD3: (9, 21), KAT_SVD4: (16, 36), KAT_INV3: (9, 9), KAT_H21: (32, 9),
           KAT_F21: (32, 9), KAT_TRIANGULATE: (28, 3), KAT_PARALLAX: (1, 1)}


class InitializerHandle(_ransac.RansacHandle):
    """Device scratch for Initialize calls over at most max_matches keys of the first frames (all pairs of a batch together) and
    batches of at most max_pairs pairs.  The match tap is float32 [N, 9]: the chiSquare pairs of H and F of the tapped iteration,
    then p3dC1, cosParallax and the CheckRT stage of the tapped hypothesis."""

    _PREFIX, ITER_DTYPE, _ERR_SHAPE = "orbfe_initializer", ITER_DTYPE, (9,)

    def __init__(self, max_matches=4096, max_pairs=1, device=0):
        super().__init__(max_matches, max_pairs, device)
        self.max_matches = max_matches

    def set_tap_iteration(self, iteration, hypothesis=0):
        self._call("set_tap_iteration", self.h, int(iteration), int(hypothesis))

    def initialize(self, keys1, keys2, matches12, K, sigma, iterations, draws):
        """One Initialize on host arrays: keys float32 [n, 2], matches12 int32 [n1], K [3, 3], draws int32 [iterations * 8].
        -> (result RESULT_DTYPE record, P3D float32 [n1, 3], triangulated uint8 [n1])"""
        k1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        if len(m) != len(k1):
            raise ValueError("matches12 must hold one entry per key of the first frame")
        d = np.ascontiguousarray(draws, np.int32).reshape(-1)
        if len(d) < 8 * int(iterations):
            raise ValueError("eight draws per iteration are needed")
        k = np.ascontiguousarray(K, np.float32).reshape(9)
        res = np.zeros(1, RESULT_DTYPE)
        P3D = np.zeros((len(k1), 3), np.float32)
        tri = np.zeros(len(k1), np.uint8)
        one = np.zeros(1, np.float32)   # a valid address for an empty array
        self._call("initialize", self.h, _ffi.ptr(k1 if len(k1) else one), len(k1), _ffi.ptr(k2 if len(k2) else one), len(k2),
                   _ffi.ptr(m if len(m) else one), _ffi.ptr(k), float(sigma), int(iterations), _ffi.ptr(d if len(d) else one),
                   _ffi.ptr(res), _ffi.ptr(P3D if len(k1) else one), _ffi.ptr(tri if len(k1) else one))
        return res[0], P3D, tri

    def initialize_device(self, offsets1, offsets2, keys1, keys2, matches12, pairs, draws, result=None, P3D=None, triangulated=None,
                          stream=None):
        """The batched form on torch device tensors: offsets1 / offsets2 int32 [npairs + 1] (CSR over the pairs' keys), keys1 /
        keys2 float32 [., 2], matches12 int32 following offsets1, pairs uint8 [npairs, 64] (PAIR_DTYPE bytes), draws int32.
        Returns (result uint8 [npairs, 288] of RESULT_DTYPE bytes, P3D float32 [., 3], triangulated uint8 [.]) on the device.
        Enqueued on `stream` (default: torch's current stream), no synchronisation."""
        import torch
        npairs = offsets1.numel() - 1
        dev = offsets1.device
        _ransac.check_tensors((offsets1, torch.int32, "offsets1"), (offsets2, torch.int32, "offsets2"), (keys1, torch.float32, "keys1"),
                              (keys2, torch.float32, "keys2"), (matches12, torch.int32, "matches12"), (pairs, torch.uint8, "pairs"),
                              (draws, torch.int32, "draws"))
        if offsets2.numel() != npairs + 1 or pairs.numel() != npairs * PAIR_DTYPE.itemsize:
            raise ValueError("offsets2 / pairs must hold one entry per pair")
        n = matches12.numel()
        if keys1.numel() != 2 * n:
            raise ValueError("keys1 and matches12 must hold one entry per key of the first frames")
        if result is None:
            result = torch.zeros((npairs, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if P3D is None:
            P3D = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
        if triangulated is None:
            triangulated = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        self._call("initialize_device", self.h, tensor_ptr(offsets1), tensor_ptr(offsets2), tensor_ptr(keys1), tensor_ptr(keys2),
                   tensor_ptr(matches12), tensor_ptr(pairs), tensor_ptr(draws), npairs, tensor_ptr(result), tensor_ptr(P3D),
                   tensor_ptr(triangulated), stream_arg(dev, stream))
        return result, P3D[:n], triangulated[:n]


_default = {}


def _handle(device, n):
    return _ransac.default_handle(_default, InitializerHandle, "max_matches", device, n)


def initialize_device(handle, offsets1, offsets2, keys1, keys2, matches12, pairs, draws, **kw):
    """InitializerHandle.initialize_device as a function: every pair of a batch in one launch sequence"""
    return handle.initialize_device(offsets1, offsets2, keys1, keys2, matches12, pairs, draws, **kw)


def monocular_initialization_device(tracker, handle, first, second, pairs, draws, window=100, d_prev_in=None, th_low=50, nnratio=0.9,
                                    check_ori=True, min_matches=100, ent_cap=None):
    """Tracking::MonocularInitialization's device work for a batch of frame pairs on torch's current stream, nothing read in between:
    SearchForInitialization (tracking.Tracker.SearchForInitialization_batch_device) -> Initializer::Initialize (handle.initialize_device).
    first = dict(kps, desc, n) of torch tensors [npairs, cap1, 7] float32 / [npairs, cap1, 32] uint8 / [npairs] int32; second =
    (tensors kept alive by the caller, orbfe_track_frames from tracking.frames_struct) or the struct alone; pairs uint8
    [npairs, 64] (PAIR_DTYPE bytes), draws int32.  A pair under min_matches (Tracking: 100) reaches the Initializer without
    matches and comes back STATUS_FEW_MATCHES.  Returns a dict of device tensors: matches12 [npairs, cap1], nmatches [npairs],
    prev [npairs, cap1, 2], status [2] (status[0] != 0: the entry buffer was short, no pair has matches; call again with ent_cap
    = status[0]), offsets1 / offsets2 [npairs + 1] (the pairs packed by their counts: Initialize normalises over ALL keys of a
    frame, so nothing is padded), and result, P3D, triangulated following offsets1.  No synchronisation."""
    import torch
    from . import tracking
    frames = second[1] if isinstance(second, tuple) else second
    kps1 = first["kps"]
    dev = kps1.device
    npairs, cap1, cap2 = int(first["n"].numel()), int(kps1.shape[1]), int(frames.cap)
    if handle.max_matches < npairs * cap1:
        raise ValueError("the Initializer handle holds %d keys of the first frames, the batch may have %d" % (handle.max_matches, npairs * cap1))
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    t = dict(matches12=torch.empty((npairs, cap1), **i32), nmatches=torch.empty((npairs,), **i32), status=torch.zeros((2,), **i32),
             prev=torch.empty((npairs, cap1, 2), **f32), offsets1=torch.zeros((npairs + 1,), **i32), offsets2=torch.zeros((npairs + 1,), **i32),
             matches12_csr=torch.full((npairs * cap1,), -1, **i32), keys1=torch.zeros((npairs * cap1, 2), **f32),
             keys2=torch.zeros((max(npairs * cap2, 1), 2), **f32))
    st = stream_arg(dev, None)
    f, o = tracking.init_search_structs(kps1, first["desc"], first["n"], cap1, t["matches12"], t["nmatches"], t["status"], t["prev"],
                                        t["offsets1"], t["offsets2"], t["matches12_csr"], t["keys1"], t["keys2"])
    tracker.SearchForInitialization_batch_device(f, frames, npairs, d_prev_in, window, o, th_low=th_low, nnratio=nnratio, check_ori=check_ori,
                                                 min_matches=min_matches, ent_cap=ent_cap, stream=st)
    t["result"], t["P3D"], t["triangulated"] = handle.initialize_device(t["offsets1"], t["offsets2"], t["keys1"], t["keys2"], t["matches12_csr"],
                                                                        pairs, draws, stream=st.value)
    return t


class Initializer:
    """Mirrors the reference's class: constructed on the reference frame's undistorted keypoints keys1 [n1, 2] and K [3, 3];
    initialize(keys2, matches12) is Initialize on the current frame.  Draws come from `draws` of each call, or from `rand` (a
    callable returning k raw values in [0, 2^31 - 1]; default: a numpy generator seeded with 0, as the reference seeds rand()
    with 0 once), iterations * 8 per call."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, device=0, handle=None, rand=None):
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        self.K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self.sigma, self.iterations = float(sigma), int(iterations)
        self._h = handle if handle is not None else _handle(device, len(self.keys1))
        if rand is None:
            rng = np.random.default_rng(0)
            rand = lambda k: rng.integers(0, 2 ** 31, k)   # noqa: E731
        self._rand = rand
        self.result = None

    def initialize(self, keys2, matches12, draws=None):
        """-> (ok, R21 float32 [3, 3], t21 float32 [3], P3D float32 [n1, 3], triangulated bool [n1]); self.result keeps the
        whole RESULT_DTYPE record"""
        if draws is None:
            draws = self._rand(8 * self.iterations)
        res, P3D, tri = self._h.initialize(self.keys1, keys2, matches12, self.K, self.sigma, self.iterations, draws)
        self.result = res
        return bool(res["ok"]), res["R21"].copy(), res["t21"].copy(), P3D, tri.astype(bool)


def kat(what, data):
    """Runs a device primitive on host data (orbfe_initializer_kat), float32, n items: data [n, in] -> [n, out] with KAT_SVD16X9:
    144 -> w 9, u 256, vt 81; KAT_SVD8X9: 72 -> w 8, u 64, vt 81; KAT_SVD3: 9 -> 3, 9, 9; KAT_SVD4: 16 -> 4, 16, 16; KAT_INV3:
    9 -> 9; KAT_H21 / KAT_F21: vP1 16, vP2 16 -> 9; KAT_TRIANGULATE: kp1 2, kp2 2, P1 12, P2 12 -> 3; KAT_PARALLAX: cos -> 0 / 1."""
    i, o = _KAT_IO[what]
    x = np.ascontiguousarray(data, np.float32).reshape(-1, i)
    out = np.zeros((len(x), o), np.float32)
    if len(x):
        _ffi.check(_ffi.lib().orbfe_initializer_kat(int(what), len(x), _ffi.ptr(x), _ffi.ptr(out)), "orbfe_initializer_kat")
    return out

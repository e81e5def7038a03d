"""The reference's PnPsolver (src/PnPsolver.cc) on the GPU: EPnP on four correspondences inside the RANSAC loop of `iterate`,
Refine's EPnP over the best inliers, through the C-ABI of csrc/orbfe_pnp.hip.  The random draws are an input (raw values in
[0, 2^31 - 1], four per iteration), so a run can be replayed.  No CPU fallback."""
import numpy as np

from . import _ffi, _ransac
from ._ffi import stream_arg, tensor_ptr
from ._ransac import TAP_ERRORS, TAP_ITERATIONS, TAP_ITERS, TAP_SETS  # noqa: F401

ABI, dtype = _ffi.ABI, _ffi.dtype
PARAMS_DTYPE = dtype("orbfe_pnp_params")
STATE_DTYPE = dtype("orbfe_pnp_state", best_Tcw=(4, 4))
RESULT_DTYPE = dtype("orbfe_pnp_result", Tcw=(4, 4))
SET_DTYPE = dtype("orbfe_pnp_set")
ITER_DTYPE = dtype("orbfe_pnp_iter", R=(3, 3))
(KAT_SVD3, KAT_SVD12, KAT_SVD6X3, KAT_SVD6X4, KAT_SVD6X5, KAT_SOLVE6X3, KAT_SOLVE6X4, KAT_SOLVE6X5, KAT_INVERT3, KAT_QR_SOLVE,
 KAT_COMPUTE_POSE) = (ABI.constants["ORBFE_PNP_KAT_" + k] for k in (
     "SVD3", "SVD12", "SVD6X3", "SVD6X4", "SVD6X5", "SOLVE6X3", "SOLVE6X4", "SOLVE6X5", "INVERT3", "QR_SOLVE", "COMPUTE_POSE"))
_KAT_SHAPE = {KAT_SVD3: (3, 3), KAT_SVD12: (12, 12), KAT_SVD6X3: (6, 3), KAT_SVD6X4: (6, 4), KAT_SVD6X5: (6, 5), KAT_SOLVE6X3: (6, 3),
              KAT_SOLVE6X4: (6, 4), KAT_SOLVE6X5: (6, 5), KAT_INVERT3: (3, 3), KAT_QR_SOLVE: (6, 4)}


def ransac_params(probability=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4, n=0, th2=5.991):
    """SetRansacParameters (host only) -> PARAMS_DTYPE [1]: the adjusted min inliers, the iteration clamp, epsilon; th2 as given"""
    out = np.zeros(1, PARAMS_DTYPE)
    _ffi.check(_ffi.lib().orbfe_pnp_ransac_params(float(probability), int(min_inliers), int(max_its), int(min_set), float(epsilon), int(n),
                                                  _ffi.ptr(out)), "orbfe_pnp_ransac_params")
    out["th2"] = np.float32(th2)
    return out


def iterations(state, params, n_iterations):
    """iterations one iterate(n_iterations) call can run (four draws each): max(n_iterations, max_its - state.iterations)"""
    return int(_ffi.lib().orbfe_pnp_iterations(_ffi.ptr(state), _ffi.ptr(params), int(n_iterations)))


class PnP(_ransac.RansacHandle):
    """Device scratch for PnP solvers of at most max_points correspondences (host form; in the device form, of all sets of a
    batch together) and batches of at most max_sets solvers.  The error tap is float32 [n]: error2."""

    _PREFIX, ITER_DTYPE = "orbfe_pnp", ITER_DTYPE

    def __init__(self, max_points=4096, max_sets=64, device=0):
        super().__init__(max_points, max_sets, device)
        self.max_points = max_points

    def iterate(self, P3Dw, P2D, sigma2, K, params, n_iterations, draws, state, best_mask):
        """One solver's iterate(n_iterations) on host arrays.  state (STATE_DTYPE [1]) and best_mask (uint8 [n]) are updated in
        place.  -> (result RESULT_DTYPE record, mask uint8 [n])"""
        P3 = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        P2 = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        sg = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        n = len(P3)
        if len(P2) != n or len(sg) != n or len(best_mask) != n:
            raise ValueError("P3Dw, P2D, sigma2 and best_mask must hold one entry per correspondence")
        if state.dtype != STATE_DTYPE or params.dtype != PARAMS_DTYPE or best_mask.dtype != np.uint8 or not best_mask.flags.c_contiguous:
            raise ValueError("state must be a STATE_DTYPE array, params a PARAMS_DTYPE array, best_mask a contiguous uint8 array")
        d = np.ascontiguousarray(draws, np.int32).reshape(-1)
        runs = n >= int(params["min_inliers"][0]) and n >= 4
        if runs and len(d) < 4 * iterations(state, params, n_iterations):
            raise ValueError("four draws per iteration are needed: 4 * iterations(state, params, n_iterations)")
        k = np.ascontiguousarray(K, np.float32).reshape(4)
        res = np.zeros(1, RESULT_DTYPE)
        mask = np.zeros(n, np.uint8)
        self._call("iterate", self.h, _ffi.ptr(P3), _ffi.ptr(P2), _ffi.ptr(sg), n, _ffi.ptr(k), _ffi.ptr(params), int(n_iterations),
                   _ffi.ptr(d) if len(d) else None, _ffi.ptr(state), _ffi.ptr(best_mask) if n else None, _ffi.ptr(res),
                   _ffi.ptr(mask) if n else None)
        return res[0], mask

    def iterate_device(self, offsets, P3Dw, P2D, sigma2, sets, draws, state, best_mask, result=None, mask=None, keypoint_index=None,
                       key_mask=None, stream=None):
        """The batched form on torch device tensors: offsets int32 [nsets + 1] (CSR), P3Dw float32 [N, 3], P2D float32 [N, 2],
        sigma2 float32 [N], sets uint8 [nsets, 48] (SET_DTYPE bytes), draws int32, state uint8 [nsets, 80] (STATE_DTYPE bytes, in
        / out), best_mask uint8 [N] (in / out).  Returns (result uint8 [nsets, 96] of RESULT_DTYPE bytes, mask uint8 [N]) on the
        device.  keypoint_index int32 [N] with key_mask uint8: the per-frame scatter.  Enqueued on `stream` (default: torch's
        current stream), no synchronisation."""
        import torch
        nsets = offsets.numel() - 1
        dev = offsets.device
        _ransac.check_tensors((offsets, torch.int32, "offsets"), (P3Dw, torch.float32, "P3Dw"), (P2D, torch.float32, "P2D"),
                              (sigma2, torch.float32, "sigma2"), (sets, torch.uint8, "sets"), (draws, torch.int32, "draws"),
                              (state, torch.uint8, "state"), (best_mask, torch.uint8, "best_mask"))
        if sets.numel() != nsets * SET_DTYPE.itemsize or state.numel() != nsets * STATE_DTYPE.itemsize:
            raise ValueError("sets / state must hold one record per set")
        if P3Dw.shape[0] > self.max_points:
            raise ValueError("more correspondences than the handle's max_points")
        if result is None:
            result = torch.zeros((nsets, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if mask is None:
            mask = torch.zeros(max(P3Dw.shape[0], 1), dtype=torch.uint8, device=dev)
        self._call("iterate_device", self.h, tensor_ptr(offsets), tensor_ptr(P3Dw), tensor_ptr(P2D), tensor_ptr(sigma2), tensor_ptr(sets),
                   tensor_ptr(draws), nsets, tensor_ptr(state), tensor_ptr(best_mask), tensor_ptr(result), tensor_ptr(mask),
                   tensor_ptr(keypoint_index) if keypoint_index is not None else None,
                   tensor_ptr(key_mask) if key_mask is not None else None, stream_arg(dev, stream))
        return result, mask[:P3Dw.shape[0]]

    def prepare_device(self, keys, level_sigma2, mappoint_index, mappoint_pos, stream=None):
        """The constructor on torch device tensors: keys uint8 [n_keys, 28] (KP_DTYPE bytes of mvKeysUn), level_sigma2 float32
        [n_levels], mappoint_index int32 [n_keys] (-1 = none or bad), mappoint_pos float32 [n_mappoints, 3].  -> (P2D [n_keys, 2],
        sigma2 [n_keys], P3Dw [n_keys, 3], keypoint_index int32 [n_keys], count int32 [1]) on the device; the first `count`
        rows are the solver's vectors, in keypoint order.  No synchronisation."""
        import torch
        _ransac.check_tensors((keys, torch.uint8, "keys"), (level_sigma2, torch.float32, "level_sigma2"),
                              (mappoint_index, torch.int32, "mappoint_index"), (mappoint_pos, torch.float32, "mappoint_pos"))
        n = mappoint_index.numel()
        if keys.numel() != n * _ffi.KP_DTYPE.itemsize:
            raise ValueError("keys must hold one 28-byte record per entry of mappoint_index")
        dev = keys.device
        P2D = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        sigma2 = torch.zeros(n, dtype=torch.float32, device=dev)
        P3Dw = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        kp = torch.zeros(n, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._call("prepare_device", self.h, tensor_ptr(keys), n, tensor_ptr(level_sigma2), level_sigma2.numel(), tensor_ptr(mappoint_index),
                   tensor_ptr(mappoint_pos), mappoint_pos.shape[0], tensor_ptr(P2D), tensor_ptr(sigma2), tensor_ptr(P3Dw), tensor_ptr(kp),
                   tensor_ptr(count), n, stream_arg(dev, stream))
        return P2D, sigma2, P3Dw, kp, count


_default = {}


def _handle(device, n):
    return _ransac.default_handle(_default, PnP, "max_points", device, n)


def pnp_iterate_device(handle, offsets, P3Dw, P2D, sigma2, sets, draws, state, best_mask, **kw):
    """PnP.iterate_device as a function: every solver of one Relocalization round in one launch"""
    return handle.iterate_device(offsets, P3Dw, P2D, sigma2, sets, draws, state, best_mask, **kw)


def pnp_prepare_device(handle, keys, level_sigma2, mappoint_index, mappoint_pos, **kw):
    """PnP.prepare_device as a function: the solver's constructor on device data"""
    return handle.prepare_device(keys, level_sigma2, mappoint_index, mappoint_pos, **kw)


class PnPSolver(_ransac.RansacSolver):
    """Mirrors the reference's class on flattened inputs: P3Dw [n, 3] positions of the matched map points, P2D [n, 2] their
    undistorted keypoints, sigma2 [n] the level sigma^2 of each, K = (fx, fy, cx, cy).  keypoint_index / n_keys (mvKeyPointIndices /
    the size of vpMapPointMatches) make iterate's mask a per-keypoint one.  Draws come from `draws` of each call, or from `rand` (a
    callable returning k raw values in [0, 2^31 - 1]; default: a numpy generator seeded with `seed`)."""

    DRAWS = 4

    def __init__(self, P3Dw, P2D, sigma2, K, keypoint_index=None, n_keys=None, device=0, handle=None, rand=None, seed=0):
        self.P3Dw = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        self.P2D = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.N = len(self.P3Dw)
        self.K = K
        self._setup(handle if handle is not None else _handle(device, self.N), STATE_DTYPE, keypoint_index, n_keys, rand, seed)
        self.keypoint_index, self.n_keys = self._index, self._n_out
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        self.params = ransac_params(probability, min_inliers, max_iterations, min_set, epsilon, self.N, th2)

    def iterations(self, n_iterations):
        return iterations(self.state, self.params, n_iterations)

    def iterate(self, n_iterations, draws=None):
        """-> (Tcw float32 [4, 4] or None, no_more, inlier mask bool [n_keys], n_inliers).  Four draws per iteration that can run
        are read (self.iterations(n_iterations) of them); self.iterations_run tells how many ran."""
        n_iterations = int(n_iterations)
        draws = self._draws(draws, self.iterations(n_iterations))
        res, mask = self._h.iterate(self.P3Dw, self.P2D, self.sigma2, self.K, self.params, n_iterations, draws, self.state, self.best_mask)
        self.iterations_run = int(res["iterations_run"])
        self.result = res
        Tcw = res["Tcw"].copy() if res["found"] else None
        return Tcw, bool(res["no_more"]), self._scatter(mask), int(res["n_inliers"])

    def find(self, draws=None):
        Tcw, _, inl, n = self.iterate(int(self.params["max_its"][0]), draws)
        return Tcw, inl, n


def kat(what, data, b=None):
    """Runs a device primitive on host data (orbfe_pnp_kat), float64.  KAT_SVD*: A [n, m, k] -> (w [n, k], Ut [n, k, m], Vt [n, k,
    k]); KAT_SOLVE* / KAT_QR_SOLVE: A [n, 6, k], b [n, 6] -> x [n, k]; KAT_INVERT3: A [n, 3, 3] -> [n, 3, 3]; KAT_COMPUTE_POSE:
    data = (K of 4, P3Dw [n, 3], P2D [n, 2]) -> (R [3, 3], t [3], error, N, rep_errors [3])."""
    L = _ffi.lib()
    if what == KAT_COMPUTE_POSE:
        K, P3, P2 = data
        P3 = np.asarray(P3, np.float64).reshape(-1, 3)
        P2 = np.asarray(P2, np.float64).reshape(-1, 2)
        n = len(P3)
        inp = np.concatenate([np.asarray(K, np.float64).reshape(4), np.concatenate([P3, P2], 1).reshape(-1)])
        out = np.zeros(17)
        _ffi.check(L.orbfe_pnp_kat(what, n, _ffi.ptr(inp), _ffi.ptr(out)), "orbfe_pnp_kat")
        return out[:9].reshape(3, 3).copy(), out[9:12].copy(), float(out[12]), int(out[13]), out[14:17].copy()
    m, k = _KAT_SHAPE[what]
    A = np.ascontiguousarray(data, np.float64).reshape(-1, m, k)
    n = len(A)
    if what in (KAT_SOLVE6X3, KAT_SOLVE6X4, KAT_SOLVE6X5, KAT_QR_SOLVE):
        inp = np.ascontiguousarray(np.concatenate([A.reshape(n, -1), np.asarray(b, np.float64).reshape(n, m)], 1))
        out = np.zeros((n, k))
    elif what == KAT_INVERT3:
        inp, out = A, np.zeros((n, 9))
    else:
        inp, out = A, np.zeros((n, k + k * m + k * k))
    _ffi.check(L.orbfe_pnp_kat(what, n, _ffi.ptr(inp), _ffi.ptr(out)), "orbfe_pnp_kat")
    if what == KAT_INVERT3:
        return out.reshape(n, 3, 3)
    if what <= KAT_SVD6X5:
        return out[:, :k].copy(), out[:, k:k + k * m].reshape(n, k, m).copy(), out[:, k + k * m:].reshape(n, k, k).copy()
    return out

"""The reference's Sim3Solver (src/Sim3Solver.cc) on the GPU: Horn's closed form on three correspondences inside the RANSAC loop
of `iterate`, through the C-ABI of csrc/orbfe_sim3.hip.  The random draws are an input (raw values in [0, 2^31 - 1], three per
iteration), so a run can be replayed.  No CPU fallback."""
import numpy as np

from . import _ffi, _ransac
from ._ffi import stream_arg, tensor_ptr
from ._ransac import TAP_ERRORS, TAP_ITERATIONS, TAP_ITERS, TAP_SETS  # noqa: F401

ABI, dtype = _ffi.ABI, _ffi.dtype
MODEL_DTYPE = dtype("orbfe_sim3_model", T12=(4, 4), R=(3, 3))
STATE_DTYPE = dtype("orbfe_sim3_state", best=MODEL_DTYPE)
RESULT_DTYPE = dtype("orbfe_sim3_result", model=MODEL_DTYPE)
SET_DTYPE = dtype("orbfe_sim3_set")
ITER_DTYPE = dtype("orbfe_sim3_iter", T12=(4, 4))
KAT_JACOBI4, KAT_ATAN2, KAT_SIN, KAT_COS, KAT_ROTATION = (ABI.ORBFE_SIM3_KAT_JACOBI4, ABI.ORBFE_SIM3_KAT_ATAN2, ABI.ORBFE_SIM3_KAT_SIN,
                                                          ABI.ORBFE_SIM3_KAT_COS, ABI.ORBFE_SIM3_KAT_ROTATION)


def ransac_iterations(probability, min_inliers, max_its, n):
    """SetRansacParameters' clamp of the iteration count (host only)"""
    return int(_ffi.lib().orbfe_sim3_ransac_iterations(float(probability), int(min_inliers), int(max_its), int(n)))


class Sim3(_ransac.RansacHandle):
    """Device scratch for Sim3 solvers of at most max_pairs correspondences (host form) and batches of at most max_sets
    solvers (device form).  The error tap is float32 [n, 2]: (err1, err2)."""

    _PREFIX, ITER_DTYPE, _ERR_SHAPE = "orbfe_sim3", ITER_DTYPE, (2,)

    def __init__(self, max_pairs=4096, max_sets=64, device=0):
        super().__init__(max_pairs, max_sets, device)
        self.max_pairs = max_pairs

    def iterate(self, X1, X2, sigma2_1, sigma2_2, K1, K2, fix_scale, min_inliers, max_its, n_iterations, draws, state, best_mask):
        """One solver's iterate(n_iterations) on host arrays.  state (STATE_DTYPE [1]) and best_mask (uint8 [n]) are updated in
        place.  -> (result RESULT_DTYPE record, mask uint8 [n])"""
        X1 = np.ascontiguousarray(X1, np.float32).reshape(-1, 3)
        X2 = np.ascontiguousarray(X2, np.float32).reshape(-1, 3)
        n = len(X1)
        s1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        s2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        if len(X2) != n or len(s1) != n or len(s2) != n or len(best_mask) != n:
            raise ValueError("X1, X2, sigma2_1, sigma2_2 and best_mask must hold one entry per correspondence")
        d = np.ascontiguousarray(draws, np.int32).reshape(-1)
        if len(d) < 3 * int(n_iterations):
            raise ValueError("three draws per iteration are needed")
        k1 = np.ascontiguousarray(K1, np.float32).reshape(4)
        k2 = np.ascontiguousarray(K2, np.float32).reshape(4)
        if state.dtype != STATE_DTYPE or best_mask.dtype != np.uint8 or not best_mask.flags.c_contiguous:
            raise ValueError("state must be a STATE_DTYPE array, best_mask a contiguous uint8 array")
        res = np.zeros(1, RESULT_DTYPE)
        mask = np.zeros(n, np.uint8)
        self._call("iterate", self.h, _ffi.ptr(X1), _ffi.ptr(X2), _ffi.ptr(s1), _ffi.ptr(s2), n, _ffi.ptr(k1), _ffi.ptr(k2),
                   int(bool(fix_scale)), int(min_inliers), int(max_its), int(n_iterations), _ffi.ptr(d) if len(d) else None, _ffi.ptr(state),
                   _ffi.ptr(best_mask) if n else None, _ffi.ptr(res), _ffi.ptr(mask) if n else None)
        return res[0], mask

    def prepare_device(self, world1, world2, Rcw1, tcw1, Rcw2, tcw2, stream=None):
        """The constructor's camera-frame points on torch device tensors: world1 / world2 float32 [n, 3] -> (X1, X2)"""
        import torch
        _ransac.check_tensors((world1, torch.float32, "world1", "float32 tensor"), (world2, torch.float32, "world2", "float32 tensor"))
        n = world1.shape[0]
        X1, X2 = torch.empty_like(world1), torch.empty_like(world2)
        pose = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (Rcw1, tcw1, Rcw2, tcw2)]
        self._call("prepare_device", self.h, tensor_ptr(world1), tensor_ptr(world2), n, *[_ffi.ptr(p) for p in pose], tensor_ptr(X1),
                   tensor_ptr(X2), stream_arg(world1.device, stream))
        return X1, X2

    def iterate_device(self, offsets, X1, X2, sigma2_1, sigma2_2, sets, draws, state, best_mask, result=None, mask=None, idx1=None,
                       key_mask=None, stream=None):
        """The batched form on torch device tensors: offsets int32 [nsets + 1] (CSR), X1 / X2 float32 [N, 3], sigma2_* float32
        [N], sets uint8 [nsets, 64] (SET_DTYPE bytes), draws int32, state uint8 [nsets, 144] (STATE_DTYPE bytes, in / out),
        best_mask uint8 [N] (in / out).  Returns (result uint8 [nsets, 144] of RESULT_DTYPE bytes, mask uint8 [N]) on the device.
        idx1 int32 [N] with key_mask uint8: the per-keyframe scatter.  Enqueued on `stream` (default: torch's current stream),
        no synchronisation."""
        import torch
        nsets = offsets.numel() - 1
        dev = offsets.device
        _ransac.check_tensors((offsets, torch.int32, "offsets"), (X1, torch.float32, "X1"), (X2, torch.float32, "X2"),
                              (sigma2_1, torch.float32, "sigma2_1"), (sigma2_2, torch.float32, "sigma2_2"), (sets, torch.uint8, "sets"),
                              (draws, torch.int32, "draws"), (state, torch.uint8, "state"), (best_mask, torch.uint8, "best_mask"))
        if sets.numel() != nsets * SET_DTYPE.itemsize or state.numel() != nsets * STATE_DTYPE.itemsize:
            raise ValueError("sets / state must hold one record per set")
        if result is None:
            result = torch.zeros((nsets, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if mask is None:
            mask = torch.zeros(max(X1.shape[0], 1), dtype=torch.uint8, device=dev)
        self._call("iterate_device", self.h, tensor_ptr(offsets), tensor_ptr(X1), tensor_ptr(X2), tensor_ptr(sigma2_1), tensor_ptr(sigma2_2),
                   tensor_ptr(sets), tensor_ptr(draws), nsets, tensor_ptr(state), tensor_ptr(best_mask), tensor_ptr(result), tensor_ptr(mask),
                   tensor_ptr(idx1) if idx1 is not None else None, tensor_ptr(key_mask) if key_mask is not None else None,
                   stream_arg(dev, stream))
        return result, mask[:X1.shape[0]]


_default = {}


def _handle(device, n):
    return _ransac.default_handle(_default, Sim3, "max_pairs", device, n)


def sim3_iterate_device(handle, offsets, X1, X2, sigma2_1, sigma2_2, sets, draws, state, best_mask, **kw):
    """Sim3.iterate_device as a function: every solver of one ComputeSim3 round in one launch"""
    return handle.iterate_device(offsets, X1, X2, sigma2_1, sigma2_2, sets, draws, state, best_mask, **kw)


class Sim3Solver(_ransac.RansacSolver):
    """Mirrors the reference's class on flattened inputs: X1 / X2 [n, 3] camera-frame points of the matched map points (or world
    positions with the two poses, see from_world), their level sigma^2 values, K = (fx, fy, cx, cy) of each keyframe.  idx1 /
    n1 (mvnIndices1 / mN1) make iterate's mask a per-keypoint one.  Draws come from `draws` of each call, or from `rand` (a
    callable returning k raw values in [0, 2^31 - 1]; default: a numpy generator seeded with `seed`)."""

    DRAWS = 3

    def __init__(self, X1, X2, sigma2_1, sigma2_2, K1, K2, fix_scale=True, idx1=None, n1=None, device=0, handle=None, rand=None, seed=0):
        self.X1 = np.ascontiguousarray(X1, np.float32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X2, np.float32).reshape(-1, 3)
        self.N = len(self.X1)
        self.sigma2_1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        self.sigma2_2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        self.K1, self.K2 = K1, K2
        self.fix_scale = bool(fix_scale)
        self._setup(handle if handle is not None else _handle(device, self.N), STATE_DTYPE, idx1, n1, rand, seed)
        self.idx1, self.n1 = self._index, self._n_out
        self.set_ransac_parameters()

    @classmethod
    def from_world(cls, world1, Rcw1, tcw1, world2, Rcw2, tcw2, *args, **kw):
        """the constructor's mvX3Dc: Rcw * Xw + tcw in float, left to right"""
        def cam(W, R, t):
            W = np.asarray(W, np.float32).reshape(-1, 3)
            R = np.asarray(R, np.float32).reshape(3, 3)
            t = np.asarray(t, np.float32).reshape(3)
            return np.stack([((R[k, 0] * W[:, 0] + R[k, 1] * W[:, 1]) + R[k, 2] * W[:, 2]) + t[k] for k in range(3)], 1)
        return cls(cam(world1, Rcw1, tcw1), cam(world2, Rcw2, tcw2), *args, **kw)

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.min_inliers = int(min_inliers)
        self.max_its = ransac_iterations(probability, min_inliers, max_iterations, self.N)
        self.state["iterations"] = 0

    def iterate(self, n_iterations, draws=None):
        """-> (T12 float32 [4, 4] or None, no_more, inlier mask bool [n1], n_inliers).  Three draws per iteration run are
        consumed; self.iterations_run tells how many ran."""
        n_iterations = int(n_iterations)
        res, mask = self._h.iterate(self.X1, self.X2, self.sigma2_1, self.sigma2_2, self.K1, self.K2, self.fix_scale, self.min_inliers,
                                    self.max_its, n_iterations, self._draws(draws, n_iterations), self.state, self.best_mask)
        self.iterations_run = int(res["iterations_run"])
        T12 = res["model"]["T12"].copy() if res["found"] else None
        return T12, bool(res["no_more"]), self._scatter(mask), int(res["n_inliers"])

    def find(self, draws=None):
        T12, _, inl, n = self.iterate(self.max_its, draws)
        return T12, inl, n

    def get_estimated_rotation(self):
        return self.state["best"]["R"][0].copy()

    def get_estimated_translation(self):
        return self.state["best"]["t"][0].copy()

    def get_estimated_scale(self):
        return float(self.state["best"]["s"][0])


def kat(what, data):
    """Runs a device primitive on host data (orbfe_sim3_kat): KAT_JACOBI4 (float32 [n, 4, 4]) -> (W float32 [n, 4], V float32
    [n, 4, 4]); KAT_ATAN2 (float64 [n, 2] of y, x) / KAT_SIN / KAT_COS (float64 [n]) -> float64 [n]; KAT_ROTATION (float32
    [n, 4, 4]) -> float32 [n, 3, 3]."""
    L = _ffi.lib()
    if what in (KAT_JACOBI4, KAT_ROTATION):
        inp = np.ascontiguousarray(data, np.float32).reshape(-1, 4, 4).copy()
        n = len(inp)
        out = np.zeros((n, 20 if what == KAT_JACOBI4 else 9), np.float32)
    else:
        inp = np.ascontiguousarray(data, np.float64).reshape(-1, 2) if what == KAT_ATAN2 else np.ascontiguousarray(data, np.float64).reshape(-1)
        n = len(inp)
        out = np.zeros(n, np.float64)
    _ffi.check(L.orbfe_sim3_kat(what, n, _ffi.ptr(inp), _ffi.ptr(out)), "orbfe_sim3_kat")
    if what == KAT_JACOBI4:
        return out[:, :4].copy(), out[:, 4:].reshape(n, 4, 4).copy()
    if what == KAT_ROTATION:
        return out.reshape(n, 3, 3)
    return out

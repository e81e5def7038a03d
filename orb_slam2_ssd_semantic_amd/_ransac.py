"""What the wrappers of the estimator handles share (the Python side of csrc/orbfe_ransac.h and csrc/orbfe_host.h): the check of a
torch device tensor, the per-device default handle, the base of the Sim3 / PnP handles (create, stream, taps) and the base of
the two solver classes that mirror the reference's (default rand, draw hand-over, the scatter of the mask by index)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import Handle

ABI = _ffi.ABI
# include/orbfe.h names the tap stages and sizes once per handle type, with one set of values: the handles share these
TAP_ITERATIONS, TAP_ERRORS = ABI.ORBFE_SIM3_TAP_ITERATIONS, ABI.ORBFE_SIM3_TAP_ERRORS
TAP_SETS, TAP_ITERS = ABI.ORBFE_SIM3_TAP_SETS, ABI.ORBFE_SIM3_TAP_ITERS
assert ABI.ORBFE_PNP_TAP_ERRORS == TAP_ERRORS and all(
    ABI.constants[f"ORBFE_{p}_TAP_{k}"] == v for p in ("PNP", "INIT")
    for k, v in (("ITERATIONS", TAP_ITERATIONS), ("SETS", TAP_SETS), ("ITERS", TAP_ITERS)))


def check_tensor(t, dtype, name, kind=None, shape=None):
    """raises unless t is a contiguous torch tensor of `dtype` (and `shape`) on the device; kind: how the message names the type"""
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
        raise ValueError(f"{name} must be a contiguous torch {kind or f'{dtype} tensor'} on the device")


def check_tensors(*specs):
    for spec in specs:
        check_tensor(*spec)


def default_handle(cache, cls, size, device, n):
    """the handle of `cache` for `device`, replaced by a larger one when its `size` attribute is below n"""
    h = cache.get(device)
    if h is None or getattr(h, size) < n:
        h = cache[device] = cls(max(n, 4096), 1, device)
    return h


class RansacHandle(Handle):
    """One orbfe_sim3 / orbfe_pnp handle.  A subclass names its C symbols' prefix, its iteration record and the shape of one
    point's entry in the error tap."""

    _HANDLE = "h"
    _PREFIX = None
    ITER_DTYPE = None
    _ERR_SHAPE = ()
    _DESTROY = property(lambda self: self._PREFIX + "_destroy")

    def __init__(self, max_points, max_sets, device):
        self._L = _ffi.lib()
        self.h = C.c_void_p()
        self._call("create", device, max_points, max_sets, C.byref(self.h))
        self.device = device
        self._max_points = max_points
        self.max_sets = max_sets

    def _call(self, entry, *args):
        name = f"{self._PREFIX}_{entry}"
        _ffi.check(getattr(self._L, name)(*args), name)

    @property
    def stream(self):
        return getattr(self._L, self._PREFIX + "_get_stream")(self.h)

    def set_tap_iteration(self, iteration):
        self._call("set_tap_iteration", self.h, int(iteration))

    def tap(self, set_index, stage):
        """A stage of the last call: TAP_ITERATIONS -> ITER_DTYPE [iterations run]; TAP_ERRORS -> float32 [n] + the solver's
        error shape, of the iteration chosen with set_tap_iteration before the call."""
        cnt = C.c_int32()
        out = np.zeros(TAP_ITERS, self.ITER_DTYPE) if stage == TAP_ITERATIONS else np.zeros((self._max_points,) + self._ERR_SHAPE, np.float32)
        self._call("tap", self.h, set_index, stage, _ffi.ptr(out), out.nbytes, C.byref(cnt))
        return out[:cnt.value].copy()


class RansacSolver:
    """The state both solver classes keep between iterate calls, and how they take draws and give the mask back."""

    DRAWS = 0   # raw draws per iteration

    def _setup(self, handle, state_dtype, index, n_out, rand, seed):
        self._h = handle
        self._index = None if index is None else np.asarray(index, np.int64)
        self._n_out = self.N if n_out is None else int(n_out)
        if rand is None:
            rng = np.random.default_rng(seed)
            rand = lambda k: rng.integers(0, 2 ** 31, k)   # noqa: E731
        self._rand = rand
        self.state = np.zeros(1, state_dtype)
        self.best_mask = np.zeros(self.N, np.uint8)

    def _draws(self, draws, iterations):
        return self._rand(self.DRAWS * max(iterations, 0)) if draws is None else draws

    def _scatter(self, mask):
        inl = np.zeros(self._n_out, bool)
        if self._index is None:
            inl[:self.N] = mask.astype(bool)
        else:
            inl[self._index[mask.astype(bool)]] = True
        return inl

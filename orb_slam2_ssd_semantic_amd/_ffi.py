"""ctypes binding of liborbfe.so (the C-ABI declared in include/orbfe.h).

The library is HIP-only: loading works anywhere hipcc's runtime is present, but creating an
extractor / matcher without a GPU fails loudly with ORBFE_ERR_NODEVICE -- there is no fallback.
"""
import ctypes as C
import os

from . import _build, _header

# The structs of include/orbfe.h that the package instantiates and passes with byref: a parameter that points to one of them is
# POINTER of its class, every other pointer c_void_p.
BYREF = ("orbfe_params", "orbfe_camera", "orbfe_track_camera", "orbfe_track_frames", "orbfe_track_last", "orbfe_track_map",
         "orbfe_track_out", "orbfe_init_search_first", "orbfe_init_search_out", "orbfe_tri_keyframes", "orbfe_tri_out", "orbfe_newpt_geom",
         "orbfe_newpt_out", "orbfe_newpt_state", "orbfe_fuse_lists", "orbfe_fuse_out")
with open(_build.HEADERS[-1]) as _f:
    ABI = _header.Header(_f.read(), BYREF)   # include/orbfe.h, parsed once per process: ABI.ORBFE_<NAME>, ABI.structs, ABI.prototypes
dtype = ABI.dtype   # dtype("orbfe_sim3_model", T12=(4, 4)): the numpy record of a header struct
(OrbfeParams, OrbfeCamera, TrackCamera, TrackFrames, TrackLast, TrackMap, TrackOut, InitSearchFirst, InitSearchOut, TriKeyframes, TriOut,
 NewptGeom, NewptOut, NewptState, FuseLists, FuseOut) = (ABI.structs[name] for name in BYREF)
KP_DTYPE, PROJ_QUERY_DTYPE, TRACK_PROJ_DTYPE = dtype("orbfe_keypoint"), dtype("orbfe_proj_query"), dtype("orbfe_track_proj")
NEWPT_KEY_DTYPE = dtype("orbfe_newpt_key")

ORBFE_OK, ORBFE_ERR_ARG, ORBFE_ERR_SIZE, ORBFE_ERR_CAP = ABI.ORBFE_OK, ABI.ORBFE_ERR_ARG, ABI.ORBFE_ERR_SIZE, ABI.ORBFE_ERR_CAP
ORBFE_ERR_HIP, ORBFE_ERR_NOMEM, ORBFE_ERR_NODEVICE, ORBFE_ERR_STATE = (ABI.ORBFE_ERR_HIP, ABI.ORBFE_ERR_NOMEM, ABI.ORBFE_ERR_NODEVICE,
                                                                       ABI.ORBFE_ERR_STATE)
# orbfe_get_stage_ms: a name per ORBFE_T_* slot, in the header's order ("describe" is the public name of ORBFE_T_DESC)
STAGES = ("pyramid", "fast", "octree", "blur", "describe", "total")
assert len(STAGES) == ABI.ORBFE_T_COUNT and STAGES.index("total") == ABI.ORBFE_T_TOTAL
SYMBOLS = tuple(ABI.prototypes)   # every extern "C" symbol include/orbfe.h declares (tests check the .so exports each of them)
# orbfe_set_option: ORBFE_OPT_<NAME> by its lower-case name
OPTIONS = {k[len("ORBFE_OPT_"):].lower(): v for k, v in ABI.constants.items() if k.startswith("ORBFE_OPT_")}
PIPE_CONTINUE, PIPE_NO_JOIN = ABI.ORBFE_PIPE_CONTINUE, ABI.ORBFE_PIPE_NO_JOIN
PROJ_CLAIMS, PROJ_RIGHT_GATE = ABI.ORBFE_PROJ_CLAIMS, ABI.ORBFE_PROJ_RIGHT_GATE
DEPTH_U16, DEPTH_F32 = ABI.ORBFE_DEPTH_U16, ABI.ORBFE_DEPTH_F32


def tensor_ptr(t):
    """the device (or host) address of a torch tensor's first element"""
    return C.c_void_p(t.data_ptr())


def stream_arg(device, stream):
    """the `void *stream` argument of a *_device entry point: `stream` (a raw hipStream_t value), or torch's current stream on `device`"""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(device).cuda_stream
    return C.c_void_p(stream)


class Handle:
    """Base of the wrappers that own one C handle.  A subclass names the attribute that holds the handle (they differ for
    historical reasons and are part of what callers reach into), the attribute that holds the library and the destroy entry
    point; close(), __del__ and the context manager come from here.  `_owned = False` marks a handle someone else destroys."""
    _HANDLE = "_h"
    _LIB = "_L"
    _DESTROY = None
    _owned = True

    def close(self):
        h = getattr(self, self._HANDLE, None)
        if h:
            if self._owned:
                getattr(getattr(self, self._LIB), self._DESTROY)(h)
            setattr(self, self._HANDLE, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class OrbfeError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__(f"{what}: status {status}")


_lib = None


def lib():
    """Load (building if needed) liborbfe.so.  torch is imported first when available so that both
    share ONE HIP runtime (same libamdhip64 SONAME) and device pointers can be exchanged."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (plumbing only: device memory, streams, torch.distributed)
    except Exception:  # pragma: no cover
        pass
    # $ORBFE_LIB: a prebuilt VARIANT of the library (developer A/B runs: kernels compiled with other -D flags, built on the
    # build machine with _build.build_variant so that the GPU box does not spend its minutes compiling)
    path = os.environ.get("ORBFE_LIB") or _build.build()
    _lib = _configure(C.CDLL(path))
    return _lib


def load_variant(path):
    """A second, separately built liborbfe (e.g. ab/liborbfe_dev.so, the -DORBFE_DEVELOPER build) next to the default one in
    the same process: ORBextractor(..., lib=load_variant(path)).  Tests of the developer build use it."""
    lib()   # torch / HIP runtime first, as for the default library
    return _configure(C.CDLL(path))


def _configure(L):
    for name, (restype, argtypes) in ABI.prototypes.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    return L


def library_path():
    return _build.LIB


def last_error():
    return lib().orbfe_last_error().decode("utf-8", "replace")


def check(status, what):
    if status != ORBFE_OK:
        raise OrbfeError(status, f"{what}: {lib().orbfe_strerror(status).decode()} ({last_error()})")


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)

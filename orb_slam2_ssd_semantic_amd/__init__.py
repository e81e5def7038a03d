"""MI355X-native ORB front-end (ORBextractor + ORBmatcher Hamming core) behind a C-ABI.

Product path: liborbfe.so (hand-written HIP for gfx950), bound through ctypes.  Nothing in this
package imports the CPU oracle under oracle/ -- that is test infrastructure.
"""
from .extractor import ORBextractor  # noqa: F401
from .matcher import FrameGrid, ORBVocabulary, ORBmatcher, feature_vector_to_csr  # noqa: F401
from ._ffi import KP_DTYPE, OrbfeError  # noqa: F401
from . import mapio  # noqa: F401
from .mapio import VocabularyFile  # noqa: F401
from .pipeline import FramePipeline  # noqa: F401
from .flow import Flow  # noqa: F401
from . import geometry  # noqa: F401
from .geometry import Geometry  # noqa: F401
from .homography import Homography, find_homography  # noqa: F401
from .camera import Camera  # noqa: F401
from .sim3 import Sim3, Sim3Solver, sim3_iterate_device  # noqa: F401
from .pnp import PnP, PnPSolver, pnp_iterate_device, pnp_prepare_device  # noqa: F401
from .initializer import InitializerHandle, Initializer, initialize_device  # noqa: F401
from . import tracking  # noqa: F401
from .tracking import Tracker  # noqa: F401
from . import mapping  # noqa: F401
from .mapping import LocalMapper, compute_f12, plan_rounds, tri_search_scratch_bytes, triangulate_match  # noqa: F401
from . import loopclosing  # noqa: F401
from .loopclosing import LoopCloser  # noqa: F401
from .cloud import ObjectDatabase, PointCloudMap, generate_point_cloud, paint_boxes, pose_matrix, statistical_outlier_removal, voxel_grid  # noqa: F401

__all__ = ["ORBextractor", "ORBmatcher", "FramePipeline", "Flow", "Geometry", "geometry", "Homography", "find_homography", "Camera", "Sim3", "Sim3Solver", "sim3_iterate_device", "PnP", "PnPSolver", "pnp_iterate_device", "pnp_prepare_device", "InitializerHandle", "Initializer", "initialize_device", "PointCloudMap", "ObjectDatabase", "statistical_outlier_removal", "generate_point_cloud", "voxel_grid", "paint_boxes", "pose_matrix", "FrameGrid", "ORBVocabulary", "VocabularyFile", "mapio", "feature_vector_to_csr",
           "KP_DTYPE", "OrbfeError", "Tracker", "tracking", "LocalMapper", "mapping", "compute_f12", "tri_search_scratch_bytes", "plan_rounds", "triangulate_match", "LoopCloser", "loopclosing"]

"""The comparison every GPU test of DynaSLAM::Geometry makes: the library against tests/geometry_oracle.py over one scene of
tests/geometry_cases.py, masks byte for byte and every tap bit for bit."""
import numpy as np

import geometry_cases as GC
from orb_slam2_ssd_semantic_amd import Geometry
from orb_slam2_ssd_semantic_amd import geometry as GE


def load(scene, nkf=None, max_seeds=8, max_keypoints=None):
    """a handle sized for the scene, with its key frames inserted"""
    h, w = scene["cur_depth"].shape
    frames = scene["key_frames"][:nkf]
    g = Geometry(w, h, max_keypoints or max(1, max(len(f["keys"]) for f in frames)), max_seeds)
    for f in frames:
        g.update_db(f["Tcw"], f["depth"], f["keys"], f["keys_un"])
    return g


def check_taps(g, taps, shape, frame=0):
    """the taps of the last call against the oracle's"""
    counts = g.counts(frame)
    assert counts == taps["counts"], (counts, taps["counts"])
    assert np.array_equal(g.tap(GE.TAP_DYN, frame), taps["dyn"])
    assert np.array_equal(g.tap(GE.TAP_SEEDS, frame), taps["accepted"])
    assert np.array_equal(g.tap(GE.TAP_UNION, frame, shape=shape), taps["union"])
    return counts


def check_scene(scene, nkf=None, max_seeds=8):
    """library against oracle on one scene: (handle, the oracle's taps)"""
    want, done, taps = GC.oracle_run(scene, nkf)
    g = load(scene, nkf, max_seeds)
    mask, computed = g.correct(scene["cur_depth"], scene["cur_T"], *scene["K"])
    assert computed == done
    assert np.array_equal(mask, want)
    if done:
        check_taps(g, taps, want.shape)
    return g, taps

"""Shared by the optical-flow GPU tests: the stage-by-stage comparison of a Flow handle's taps with the oracle's, and the oracle's
result for a frame pair computed once per (case, threshold).  Test support only."""
import numpy as np

import flow_oracle as FO
from orb_slam2_ssd_semantic_amd import flow as FL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_stages(fl, of, a_shape, label):
    """every tap of the GPU's last call (frame 0) against the oracle Flow's taps"""
    h, w = a_shape
    assert np.array_equal(fl.tap(0, FL.TAP_HALF), of.taps["half"]), label + ": half"
    for lv, ofl in enumerate(of.taps["flow_levels"][::-1]):
        got = fl.tap(0, FL.TAP_FLOW, lv)
        assert got.shape == ofl.shape, (label, lv)
        bad = np.count_nonzero(_bits(got) != _bits(ofl))
        assert bad == 0, f"{label}: flow level {lv}: {bad} of {ofl.size} words differ"
    assert np.array_equal(_bits(fl.tap(0, FL.TAP_FLOW2)), _bits(of.taps["flow2"])), label + ": flow2"
    assert np.array_equal(fl.tap(0, FL.TAP_PRE), of.taps["mask_pre"]), label + ": pre-morphology mask"
    assert np.array_equal(fl.tap(0, FL.TAP_MASK), of.taps["mask"]), label + ": mask"


_PAIRS = {}


def oracle_pair(key, make, th):
    """the oracle Flow after frames a, b = make() at threshold th, computed once per (key, th) and shared: read only"""
    k = (key, repr(float(th)))
    if k not in _PAIRS:
        a, b = make()
        of = FO.Flow()
        of.compute_mask(a, th)
        of.compute_mask(b, th)
        _PAIRS[k] = of
    return _PAIRS[k]

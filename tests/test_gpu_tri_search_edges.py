"""k_tri_search where a workgroup takes a second and a third keyframe-1 node (csrc/orbfe_tri_search.hip): a pair gets
min(cap, node_workgroups) workgroups that take the nodes round robin, and every case of tests/test_gpu_tri_search.py has fewer nodes
than workgroups.  Here keyframe 1 has more than two laps of nodes, so the LDS tile is re-staged for a new node after a multi-tile
and after a single-tile one, and nodes that are absent from keyframe 2 or have no query lie between nodes that match; and node
counts one either side of one and two laps.  Bit for bit against the oracle (and the compiled reference where it is built), with
both search kernels; tests/test_tri_batch_cases.py shows on the CPU that every case reaches its edge."""
import numpy as np
import pytest

import tri_batch_cases as TC
from test_gpu_tri_search import Block, check, expected, lm, mt  # noqa: F401  (lm, mt: fixtures)

pytestmark = pytest.mark.gpu

MODES = [(False, True), (False, False), (True, True), (True, False)]   # (only_stereo, check_ori)


def _info():
    from orb_slam2_ssd_semantic_amd import mapping
    return mapping.tri_search_info()


@pytest.fixture(scope="module")
def many():
    """the case and its block on the device: the 3-node pair `interleaved` of fv_shapes() before and after the many-node pair"""
    c, _ = TC.many_nodes(_info())
    small = TC.fv_shapes()["interleaved"]
    b = TC.as_batch([small, c, small])
    return c, small, b, Block(b["frames"])


@pytest.mark.parametrize("only_stereo, check_ori", MODES)
def test_many_nodes(lm, many, only_stereo, check_ori):
    """~290 keyframe-1 nodes over 128 workgroups: heavy, ordinary, heavy in workgroup 0; one tile and two passes, then a new node;
    an absent node and a node without queries between two that match"""
    c, small, b, blk = many
    kw = dict(only_stereo=only_stereo, check_ori=check_ori)
    assert len(c["k1"]["fv"][0]) > 2 * _info()["node_workgroups"] and blk.cap > _info()["node_workgroups"]
    got, raw = blk.run(lm, b["pairs"][1:2], **kw)
    check(got[0], c, what="alone", **kw)
    assert got[0][1] >= 60
    assert blk.run(lm, b["pairs"][1:2], **kw)[1] == raw, "a second run differs"


def test_many_nodes_between_two_small_pairs(lm, many):
    """the same pair behind and in front of a 3-node pair in one batch: its bytes are those of running it alone"""
    c, small, b, blk = many
    alone, _ = blk.run(lm, b["pairs"][1:2])
    got, raw = blk.run(lm, b["pairs"])
    for g, cc, name in zip(got, (small, c, small), ("before", "many", "after")):
        check(g, cc, what=name)
    assert expected(small)[1] > 0
    for a, g in zip(alone[0], got[1]):
        assert np.asarray(a).tobytes() == np.asarray(g).tobytes()
    assert blk.run(lm, b["pairs"])[1] == raw, "a second run differs"


@pytest.mark.parametrize("lap, extra", [(1, 0), (1, 1), (2, 0), (2, 1)], ids=["W", "W+1", "2W", "2W+1"])
def test_node_counts_at_the_workgroup_count(lm, lap, extra):
    """W, W + 1, 2 W, 2 W + 1 nodes of one feature each as keyframe 2 and as keyframe 1 (cap > n: W workgroups); at W + 1 exactly one
    workgroup takes a second node, and that node matches"""
    n = lap * _info()["node_workgroups"] + extra
    fwd, back = TC.nodes_at(n)
    blk = Block([fwd["k1"], fwd["k2"]])
    assert blk.cap > n == len(back["k1"]["fv"][0])
    pairs = [(0, 1, fwd["F12"], fwd["ex"], fwd["ey"]), (1, 0, back["F12"], back["ex"], back["ey"])]
    for only_stereo, check_ori in MODES:
        kw = dict(only_stereo=only_stereo, check_ori=check_ori)
        got, raw = blk.run(lm, pairs, **kw)
        check(got[0], fwd, what=("keyframe 2", n), **kw)
        check(got[1], back, what=("keyframe 1", n), **kw)
        if not only_stereo:
            assert got[1][0][n - 1] >= 0, "the last node's match"
        assert blk.run(lm, pairs, **kw)[1] == raw, "a second run differs"

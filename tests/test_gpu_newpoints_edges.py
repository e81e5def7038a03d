"""CreateNewMapPoints device-resident (csrc/orbfe_newpoints.hip) where a pair fills more than one 256-block of the claim kernels,
where ids do not start at 0, where a second call goes on with the state of the first, and the scene median depth at the
workgroup's 256 slots and at the ends of its rank.  Bit for bit against tests/newpoints_oracle.py, with both search kernels inside
the loop; tests/test_newpoints_oracle.py shows on the CPU that every case reaches its edge."""
import numpy as np
import pytest

import newpoints_cases as NC
import newpoints_oracle as NO
from test_gpu_newpoints import NBlock, _bits, _loop, _median, _same_outputs, _same_state, lm, lm0, mt, neighbours  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ more than one claim block
def test_wide_loop(lm):
    """900 features in ~280 nodes, cap = 904, 506 new points in the first pair: the claim kernels run four blocks per pair and
    the search's workgroups three nodes each.  Planned rounds = the oracle's serial loop; one round of both pairs = its round
    loop, where keyframe-0 slots are claimed from different blocks of the two pairs and the later pair's point stays."""
    w = NC.wide_loop()
    frames, cap, pairs = w["frames"], w["cap"], w["pairs"]
    blk = NBlock(frames, cap=cap)
    got, r, raw = _loop(lm, blk, pairs)
    assert list(r["round_off"]) == [0, 1, 2] and len(got[0]["new_idx"]) > 256
    _same_outputs(got, w["serial"], "rounds")
    _same_state(blk, w["s_serial"], "rounds")
    blk.reset()
    got, _, _ = _loop(lm, blk, pairs, round_off=[0, 2])
    assert len(got[1]["new_idx"]) > 256
    _same_outputs(got, w["static"], "one round")
    _same_state(blk, w["s_static"], "one round")


# ------------------------------------------------------------------------------------------------ id_base
def test_id_base(lm, neighbours):
    """id_base = 1000 moves every id by 1000 and nothing else; the largest id_base the call takes gives the oracle's (positive)
    ids; one more is ORBFE_ERR_SIZE, a negative one ORBFE_ERR_ARG, and neither touches the state or the handle"""
    from orb_slam2_ssd_semantic_amd import OrbfeError, _ffi
    frames, cap, pairs, (serial, s_serial), _ = neighbours
    blk = NBlock(frames, cap=cap)
    got, _, _ = _loop(lm, blk, pairs, id_base=1000)
    _same_outputs(got, serial, "id_base 1000")
    _same_state(blk, (s_serial[0], s_serial[1], np.where(s_serial[2] >= 0, s_serial[2] + 1000, -1).astype(np.int32)), "id_base 1000")
    assert (s_serial[2] >= 0).sum() > 20
    top = 0x7FFFFFFF - len(pairs) * cap
    blk.reset()
    before = blk.state()
    for bad, status in ((top + 1, _ffi.ORBFE_ERR_SIZE), (-1, _ffi.ORBFE_ERR_ARG)):
        with pytest.raises(OrbfeError) as ei:
            _loop(lm, blk, pairs, id_base=bad)
        assert ei.value.status == status, bad
        assert all(np.array_equal(a, b) for a, b in zip(before, blk.state())), bad
    want = NO.new_state(frames, cap)
    w_out = NO.serial_loop(frames, pairs, want, cap, id_base=top, **NC.loop_kw())
    got, _, _ = _loop(lm, blk, pairs, id_base=top)
    _same_outputs(got, w_out, "largest id_base")
    _same_state(blk, want, "largest id_base")
    ids = blk.state()[2]
    assert (ids[ids != -1] >= top).all() and ids.max() < 0x7FFFFFFF


def test_second_call_on_carried_state(lm, neighbours):
    """pair (0, 1) with id_base 0, then the other two pairs on the state it left with id_base = cap: slots, points and ids are,
    byte for byte, those of one call of three pairs"""
    frames, cap, pairs, (serial, s_serial), _ = neighbours
    blk = NBlock(frames, cap=cap)
    _loop(lm, blk, pairs)
    one_call = blk.state()
    _same_state(blk, s_serial, "one call")
    blk.reset()
    a, _, _ = _loop(lm, blk, pairs[:1])
    b, _, _ = _loop(lm, blk, pairs[1:], id_base=cap)
    _same_outputs(a + b, serial, "two calls")
    for x, y, name in zip(blk.state(), one_call, ("has_mp", "mp_xyz", "mp_id")):
        assert x.tobytes() == y.tobytes(), name


# ------------------------------------------------------------------------------------------------ the scene median depth
def test_scene_median_depth_edges(lm0):
    """255, 256 and 257 occupied slots and a frame of equal depths; q = 1 is the largest depth, q above the count the smallest"""
    T, has, xyz, n, names = NC.median_edge_frames()
    cap = has.shape[1]
    for q in (1, 2, 3, 1000):
        got = _median(lm0, T, has, xyz, n, cap, q)
        want = [NO.scene_median_depth(T[b], has[b], xyz[b], n[b], q) for b in range(len(n))]
        assert _bits(got).tolist() == _bits(want).tolist(), q

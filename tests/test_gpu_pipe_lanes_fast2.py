"""Lane placement 2 of the sequence pipeline on the GPU (csrc/orbfe_pipe_plan.h): the FAST launches of even sub-batches on kernel
stream 1, of odd ones on the side stream; the clear of FAST's survivor counts and cell flags on the pyramid's stream (every lane
placement); the brute-force matcher of a lane call with 1, 2 or 4 query tiles per wave.  Shapes and helpers are those of
tests/test_gpu_pipe_lanes.py: sub-batches of 2 frames, 5 pipes on 4 queues, calls of 11 frames.

Case 1: three continuing calls into the same output blocks, joined and NO_JOIN, with 3, 4 and 5 buffer sets (an odd number of sets
        alternates a set between the two FAST streams) and each tile count.
Case 2: an extract-only call, then a matching one, then a CONTINUE call.
Case 3: a call of corner-rich frames, then on the same buffer sets a call of constant-grey frames: no keypoint, no match -- survivor
        counts or cell flags that were not cleared would show as keypoints.
All results: byte-identical to one extractor handle plus brute-force match calls (test_gpu_pipe_queues._reference)."""
import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame
from test_gpu_pipe_lanes import _three_calls
from test_gpu_pipe_queues import H, NF, W, _blocks, _reference, _same

PLACE = 2


@pytest.fixture(scope="module")
def short_sequence():
    frames = np.stack([synth_frame(7500 + i, H, W, sparse=(i % 5 == 3 or i == 10)) for i in range(33)])
    return _reference(frames)


def _pipeline(place=PLACE, sets=0, tiles=0):
    from orb_slam2_ssd_semantic_amd import FramePipeline
    pl = FramePipeline(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, sub_batch=2, npipes=5, _queues=4, _lanes=1, _lane_place=place,
                       _lane_sets=sets, _lane_tiles=tiles)
    assert pl.streams() == (3, 3, 1)   # no stream beyond the four
    return pl


@pytest.mark.gpu
@pytest.mark.parametrize("sets,tiles", [(3, 0), (4, 2), (5, 1), (0, 4)])
def test_fast2_continuing_calls_into_the_same_blocks_equal_single_handle_calls(short_sequence, sets, tiles):
    dg, cap, ref = short_sequence
    pl = _pipeline(sets=sets, tiles=tiles)
    assert pl.capacity() == cap
    _three_calls(pl, dg, cap, ref, f"place 2 sets {sets} tiles {tiles}")
    pl.close()


@pytest.mark.gpu
def test_fast2_extract_only_call_then_a_matching_call(short_sequence):
    import torch
    dg, cap, ref = short_sequence
    pl = _pipeline(tiles=2)
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(11, cap)
    m.fill_(-7)
    pl.extract_match_device(dg[0].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), None, None,
                            flags=pl.NO_JOIN, stream=st)
    pl.extract_match_device(dg[11].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                            nm.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert pl.overflow() == 0
    assert int(nm[0]) == 0 and bool((m[0] == -1).all())   # without CONTINUE frame 11 has no predecessor
    _same(tuple(t[1:] for t in out), ref, 12, 22, "matching call behind an extract-only call")
    assert torch.equal(n[:1], ref[0][11:12])
    pl.extract_match_device(dg[22].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                            nm.data_ptr(), flags=pl.CONTINUE, stream=st)
    torch.cuda.synchronize()
    _same(out, ref, 22, 33, "CONTINUE call")
    pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("place", (0, 1, 2))
def test_lanes_grey_frames_behind_corner_rich_frames_on_the_same_sets_have_no_keypoints(short_sequence, place):
    """3 buffer sets, calls of 6 frames = 3 sub-batches: the second call uses every set the first one filled, and nothing but FAST's
    own clear stands between the first call's survivor counts and cell flags and the second call's quadtree"""
    import torch
    dg, cap, ref = short_sequence
    grey = torch.full((6, H, W), 128, dtype=torch.uint8, device="cuda")
    pl = _pipeline(place=place, sets=3)
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(6, cap)
    for no_join in (0, pl.NO_JOIN):
        pl.reset_sequence()
        pl.extract_match_device(dg[0].data_ptr(), 6, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(), nm.data_ptr(),
                                flags=no_join, stream=st)
        if not no_join:
            torch.cuda.synchronize()
            _same(out, ref, 0, 6, f"place {place}: corner-rich call")
            assert int(n.max()) > 100
        pl.extract_match_device(grey.data_ptr(), 6, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(), nm.data_ptr(),
                                flags=no_join | pl.CONTINUE, stream=st)
        pl.synchronize()
        torch.cuda.synchronize()
        assert n.tolist() == [0] * 6, (place, no_join)
        assert nm.tolist() == [0] * 6 and bool((m == -1).all()), (place, no_join)
        assert pl.overflow() == 0
    pl.close()

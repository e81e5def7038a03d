"""The sequence pipeline in lanes (csrc/orbfe_pipe_plan.h orb_pipe_lanes; run_device in csrc/orbfe_pipeline.hip): 5 pipes on 4
hardware queues -- 3 kernel streams + the side stream --, the four streams dealt by stage (pyramid | FAST | quadtree + descriptor |
matcher, the blur on the first or the last of them) instead of by sub-batch, forced on through `_lanes=1` whatever the library
would choose itself.

Case 1: calls of 11 frames in sub-batches of 2 (6 sub-batches on min(5 pipes, 8) = 5 buffer sets: sets are re-used inside a call, the last
        sub-batch is short), two CONTINUE calls behind the first one, every call into the SAME output blocks; joined (every call checked) and
        with NO_JOIN + synchronize (the last call's blocks checked); both placements of blur and matcher, 3, 4 and 5 buffer sets;
        and the same calls in chains (`_lanes=0`) give the same bytes.
Case 2: 4 x 128 frames, sub-batch 128: the size from which a chain's blur leaves the main stream.
Case 3: an extract-only call, then a matching call without CONTINUE: the carry slot is written twice with no frame-0 match between.
Case 4: a call of one sub-batch on a lanes pipeline runs as a chain, between two lane calls.
Case 5: `_lanes=1` where the plan has no 3 kernel streams + side stream short of its pipes is the library's argument error.
All results: byte-identical to orbfe_extract_batch_device on ONE handle plus brute-force match calls (test_gpu_pipe_queues._reference,
computed once per sequence)."""
import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame
from test_gpu_pipe_queues import H, NF, W, _blocks, _reference, _same

PLACES_SETS = [(0, 0), (1, 0), (0, 3), (1, 4)]


@pytest.fixture(scope="module")
def short_sequence():
    frames = np.stack([synth_frame(7500 + i, H, W, sparse=(i % 5 == 3 or i == 10)) for i in range(33)])
    return _reference(frames)


@pytest.fixture(scope="module")
def long_sequence():
    base = [synth_frame(7600 + i, H, W, sparse=(i % 5 == 3)) for i in range(8)]
    frames = np.empty((512, H, W), np.uint8)
    for i in range(512):   # lossless rolls: every frame another image
        r = i // 8
        frames[i] = np.roll(base[i % 8], ((37 * r) % H, (101 * r) % W), axis=(0, 1)) if r else base[i % 8]
    return _reference(frames)


def _pipeline(sub, lanes=1, place=-1, sets=0, queues=4, pipes=5):
    from orb_slam2_ssd_semantic_amd import FramePipeline
    pl = FramePipeline(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, sub_batch=sub, npipes=pipes, _queues=queues, _lanes=lanes,
                       _lane_place=place, _lane_sets=sets)
    if queues == 4 and pipes == 5:
        assert pl.streams() == (3, 3, 1)   # the plan and its streams are the chains'
    return pl


def _three_calls(pl, dg, cap, ref, label):
    """case 1 on `pl`; returns the blocks of the third unjoined call"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(11, cap)
    for no_join in (0, pl.NO_JOIN):
        pl.reset_sequence()
        for t in out:
            t.zero_()
        for c in range(3):
            lo = 11 * c
            pl.extract_match_device(dg[lo].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                                    nm.data_ptr(), flags=no_join | (pl.CONTINUE if c else 0), stream=st)
            if not no_join:
                torch.cuda.synchronize()
                if c == 0:
                    assert int(nm[0]) == 0 and bool((m[0] == -1).all())
                _same(out, ref, lo, lo + 11, f"{label}: joined call {c}")
        if no_join:
            pl.synchronize()
            torch.cuda.synchronize()
            _same(out, ref, 22, 33, f"{label}: third unjoined call")
        assert pl.overflow() == 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("place,sets", PLACES_SETS)
def test_lanes_continuing_calls_into_the_same_blocks_equal_single_handle_calls(short_sequence, place, sets):
    import torch
    dg, cap, ref = short_sequence
    counts = ref[0]
    assert int(counts.min()) < int(counts.max())   # sparse frames among the dense ones: the counts differ
    pl = _pipeline(2, place=place, sets=sets)
    assert pl.capacity() == cap
    got = [t.clone() for t in _three_calls(pl, dg, cap, ref, f"lanes place {place} sets {sets}")]
    pl.close()
    # chains in the same library: the same bytes in every slot of every block
    pc = _pipeline(2, lanes=0)
    chains = _three_calls(pc, dg, cap, ref, "chains")
    for a, b, name in zip(got, chains, ("counts", "keypoints", "descriptors", "matches", "match counts")):
        assert torch.equal(a, b), name
    pc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("place", (0, 1))
def test_lanes_four_full_sub_batches_equal_single_handle_calls(long_sequence, place):
    import torch
    dg, cap, ref = long_sequence
    pl = _pipeline(128, place=place)
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(512, cap)
    pl.extract_match_device(dg.data_ptr(), 512, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(), nm.data_ptr(),
                            stream=st)
    torch.cuda.synchronize()
    assert pl.overflow() == 0
    _same(out, ref, 0, 512, f"one call, place {place}")
    pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("place", (0, 1))
def test_lanes_extract_only_call_then_a_matching_call(short_sequence, place):
    import torch
    dg, cap, ref = short_sequence
    pl = _pipeline(2, place=place)
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(11, cap)
    m.fill_(-7)
    pl.extract_match_device(dg[0].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), None, None,
                            flags=pl.NO_JOIN, stream=st)
    pl.extract_match_device(dg[11].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                            nm.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert pl.overflow() == 0
    # without CONTINUE frame 11 has no predecessor: an empty first row; the other rows are the sequence's
    assert int(nm[0]) == 0 and bool((m[0] == -1).all())
    _same(tuple(t[1:] for t in out), ref, 12, 22, "matching call behind an extract-only call")
    assert torch.equal(n[:1], ref[0][11:12])
    # ... and a CONTINUE call behind it finds the carried frame 21
    pl.extract_match_device(dg[22].data_ptr(), 11, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                            nm.data_ptr(), flags=pl.CONTINUE, stream=st)
    torch.cuda.synchronize()
    _same(out, ref, 22, 33, "CONTINUE call")
    pl.close()


@pytest.mark.gpu
def test_a_call_of_one_sub_batch_on_a_lanes_pipeline_runs_as_a_chain(short_sequence):
    import torch
    dg, cap, ref = short_sequence
    pl = _pipeline(2)
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(11, cap)
    calls = [(0, 11, 0), (11, 2, pl.CONTINUE), (13, 1, pl.CONTINUE), (14, 11, pl.CONTINUE)]   # lanes, chain, chain, lanes
    for no_join in (0, pl.NO_JOIN):
        pl.reset_sequence()
        for lo, cnt, fl in calls:
            pl.extract_match_device(dg[lo].data_ptr(), cnt, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                                    nm.data_ptr(), flags=fl | no_join, stream=st)
            if not no_join:
                torch.cuda.synchronize()
                _same(out, ref, lo, lo + cnt, f"call at frame {lo}")
        pl.synchronize()
        torch.cuda.synchronize()
        _same(out, ref, 14, 25, "last call")
        assert pl.overflow() == 0
    pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("queues,pipes", [(2, 5), (4, 3), (16, 5), (1, 12)])
def test_lanes_on_without_their_streams_is_an_argument_error(queues, pipes):
    from orb_slam2_ssd_semantic_amd import FramePipeline, _ffi
    with pytest.raises(_ffi.OrbfeError) as e:
        _pipeline(2, queues=queues, pipes=pipes)
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    # automatic and off are accepted everywhere, and such a pipeline runs in chains
    for mode in (-1, 0):
        pl = FramePipeline(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, sub_batch=2, npipes=pipes, _queues=queues, _lanes=mode)
        pl.close()

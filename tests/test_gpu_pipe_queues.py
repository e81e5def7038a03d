"""The sequence pipeline on every stream plan (csrc/orbfe_pipe_plan.h): created for Q = 1, 2, 4, 16 hardware queues with P = 1, 3, 5
pipes through orbfe_internal_pipeline_create_queues, whatever the process's own queue count is -- 1 to 5 kernel streams, with the
shared side stream (Q >= 2) and without it (Q = 1: the blur in the pipe's own stream).

Case 1: calls of 7 frames in sub-batches of 2 (nsub = 4: with P_eff = 3 and 5 consecutive calls start on different pipes, so the
        slices of index j move to another stream from call to call), two CONTINUE calls behind the first one, every call into the
        SAME output blocks; joined (every call checked) and with NO_JOIN (nothing ordered but by the pipeline's own events; the
        last call's blocks checked, whose first match row needs the carried frame of the call before).
Case 2: 4 x 128 frames, sub-batch 128: the size from which an extractor puts the blur on its side stream -- where the plan has one;
        where it has none the same call takes the in-stream blur.
Case 3: the restart behind a failed call, in chains (16 queues, 3 pipes) and in lanes (4 queues, 5 pipes): a CONTINUE call that the
        extractor rejects, then two more CONTINUE calls -- the first without a predecessor frame, the second with one.
All: counts, keypoints, descriptors and matches byte-identical to orbfe_extract_batch_device on ONE handle plus brute-force
match calls over the same frames (computed once per case)."""
import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame

W, H, NF = 640, 480, 1000
QUEUES, PIPES = (1, 2, 4, 16), (1, 3, 5)
GRID = [(q, p) for q in QUEUES for p in PIPES]


def _reference(frames):
    """(n, kps, desc, match, nm) torch blocks of the whole sequence from one extractor handle and one matcher handle"""
    import torch
    from orb_slam2_ssd_semantic_amd import ORBextractor, ORBmatcher, _ffi
    N = len(frames)
    dg = torch.from_numpy(frames).cuda()
    e = ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=N)
    mt = ORBmatcher(0.9, True)
    cap = e.capacity()
    st = torch.cuda.current_stream().cuda_stream
    k = torch.zeros((N, cap, 7), dtype=torch.int32, device="cuda")
    d = torch.zeros((N, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(N, dtype=torch.int32, device="cuda")
    m = torch.zeros((N, cap), dtype=torch.int32, device="cuda")
    nm = torch.zeros(N, dtype=torch.int32, device="cuda")
    e.extract_batch_device(dg.data_ptr(), N, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), st)
    qf = torch.arange(1, N, dtype=torch.int32, device="cuda")
    tf = qf - 1
    _ffi.check(_ffi.lib().orbfe_match_bf_frames_device(mt.handle, k.data_ptr(), d.data_ptr(), n.data_ptr(), cap, qf.data_ptr(), tf.data_ptr(),
                                                       N - 1, 0.9, 100, 1, m[1].data_ptr(), nm[1:].data_ptr(), st), "match")
    m[0].fill_(-1)
    torch.cuda.synchronize()
    assert e.overflow() == 0 and int(n.min()) > 0.5 * NF
    e.close()
    mt.close()
    return dg, cap, (n, k, d, m, nm)


@pytest.fixture(scope="module")
def short_sequence():
    frames = np.stack([synth_frame(7300 + i, H, W, sparse=(i % 5 == 3)) for i in range(21)])
    return _reference(frames)


@pytest.fixture(scope="module")
def long_sequence():
    base = [synth_frame(7400 + i, H, W, sparse=(i % 5 == 3)) for i in range(8)]
    frames = np.empty((512, H, W), np.uint8)
    for i in range(512):   # lossless rolls: every frame another image
        r = i // 8
        frames[i] = np.roll(base[i % 8], ((37 * r) % H, (101 * r) % W), axis=(0, 1)) if r else base[i % 8]
    return _reference(frames)


def _pipeline(queues, pipes, sub):
    from orb_slam2_ssd_semantic_amd import FramePipeline
    from test_pipe_plan import plan
    pl = FramePipeline(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, sub_batch=sub, npipes=pipes, _queues=queues)
    _, want, _ = plan(pipes, queues, 0)
    assert pl.streams() == (want["S"], want["P_eff"], want["side"])
    assert want["side"] == (1 if queues >= 2 else 0) and want["S"] == (pipes if queues >= pipes + 1 else max(1, queues - 1))
    return pl


def _blocks(n, cap):
    import torch
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    return z(n, torch.int32), z((n, cap, 7), torch.int32), z((n, cap, 32), torch.uint8), z((n, cap), torch.int32), z(n, torch.int32)


def _same(got, ref, lo, hi, label):
    """rows lo .. hi - 1 of the reference against the blocks of a call: counts, whole match rows (the matcher writes all `cap` slots)
    and match counts; keypoint and descriptor rows up to the frame's count (a call leaves the slots behind it alone, and the blocks
    hold an earlier call's there)"""
    import torch
    n, k, d, m, nm = (t[:hi - lo] for t in got)
    rn, rk, rd, rm, rnm = (t[lo:hi] for t in ref)
    assert torch.equal(n, rn), (label, "counts")
    valid = (torch.arange(k.shape[1], device=k.device)[None, :] < n[:, None].to(torch.int64))[:, :, None]
    assert torch.equal(k * valid, rk * valid), (label, "keypoints")
    assert torch.equal(d * valid, rd * valid), (label, "descriptors")
    assert torch.equal(m, rm), (label, "matches")
    assert torch.equal(nm, rnm), (label, "match counts")


@pytest.mark.gpu
@pytest.mark.parametrize("queues,pipes", GRID)
def test_continuing_calls_into_the_same_blocks_equal_single_handle_calls(short_sequence, queues, pipes):
    import torch
    dg, cap, ref = short_sequence
    pl = _pipeline(queues, pipes, 2)
    assert pl.capacity() == cap
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(7, cap)
    for no_join in (0, pl.NO_JOIN):
        pl.reset_sequence()
        for t in out:
            t.zero_()
        for c in range(3):
            lo = 7 * c
            pl.extract_match_device(dg[lo].data_ptr(), 7, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                                    nm.data_ptr(), flags=no_join | (pl.CONTINUE if c else 0), stream=st)
            if not no_join:
                torch.cuda.synchronize()
                if c == 0:   # no predecessor: the single-handle reference holds the same empty row for frame 0
                    assert int(nm[0]) == 0 and bool((m[0] == -1).all())
                _same(out, ref, lo, lo + 7, f"joined call {c}")
        if no_join:
            pl.synchronize()
            torch.cuda.synchronize()
            _same(out, ref, 14, 21, "third unjoined call")
        assert pl.overflow() == 0
    pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("queues,pipes", [(16, 3), (4, 5)])   # chains, lanes
def test_a_failed_call_restarts_the_sequence(short_sequence, queues, pipes):
    """A call that fails behind its fork (a frame one row taller than the pipeline was made for: the extractor of sub-batch 0 answers
    ORBFE_ERR_SIZE before it launches anything) drains the pipes and starts the sequence over: the next CONTINUE call has no
    predecessor frame, the one after it has."""
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi
    dg, cap, ref = short_sequence
    pl = _pipeline(queues, pipes, 2)
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(7, cap)

    def call(lo, flags, h=H):
        pl.extract_match_device(dg[lo].data_ptr(), 7, W, h, W, W * h, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(),
                                nm.data_ptr(), flags=flags, stream=st)
        torch.cuda.synchronize()

    call(0, 0)
    _same(out, ref, 0, 7, "first call")
    with pytest.raises(_ffi.OrbfeError) as err:
        call(7, pl.CONTINUE, h=H + 1)
    assert err.value.status == _ffi.ORBFE_ERR_SIZE
    call(7, pl.CONTINUE)
    assert int(nm[0]) == 0 and bool((m[0] == -1).all())   # the "no predecessor" row
    _same([t[1:] for t in out], ref, 8, 14, "call behind the failed one, rows 1..6")
    first = [t[:1].clone() for t in out]
    first[3], first[4] = ref[3][7:8], ref[4][7:8]         # (row 0 but for its matches)
    _same(first, ref, 7, 8, "call behind the failed one, row 0")
    call(14, pl.CONTINUE)
    _same(out, ref, 14, 21, "second call behind the failed one")   # row 0: frame 14 against the carried frame 13
    assert pl.overflow() == 0
    pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("queues,pipes", GRID)
def test_four_full_sub_batches_equal_single_handle_calls(long_sequence, queues, pipes):
    import torch
    dg, cap, ref = long_sequence
    pl = _pipeline(queues, pipes, 128)
    assert pl.capacity() == cap
    st = torch.cuda.current_stream().cuda_stream
    n, k, d, m, nm = out = _blocks(512, cap)
    pl.extract_match_device(dg.data_ptr(), 512, W, H, W, W * H, k.data_ptr(), d.data_ptr(), cap, n.data_ptr(), m.data_ptr(), nm.data_ptr(),
                            stream=st)
    torch.cuda.synchronize()
    assert pl.overflow() == 0
    _same(out, ref, 0, 512, "one call")
    pl.close()

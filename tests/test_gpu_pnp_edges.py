"""csrc/orbfe_pnp.hip on the cases of tests/pnp_edge_cases.py (what each is for: tests/test_pnp_edge_cases.py), bit for bit
against the oracle's replays: every case through the host call with all it leaves behind (result, both masks, state, every
tap record, the tap errors), the tap errors at iterations 63, 64 and the last one run, every case again in batched launches
run twice on one handle, sets entered with the state of an earlier call, n_keys = 0, keypoint_index values outside the key
slice, the three malformed offsets with sentinel bytes around them, two handles on two streams at once, and the device
constructor at its capacity, index and octave edges.  No tolerance anywhere."""
import numpy as np
import pytest

import pnp_checks as CK
import pnp_edge_cases as EC
import pnp_oracle as PO
from orb_slam2_ssd_semantic_amd import PnP, _ffi

MAX_POINTS = 2048
NAMES = list(EC.inputs())


@pytest.fixture(scope="module")
def pn():
    h = PnP(MAX_POINTS, 32)
    h.set_tap_iteration(0)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_call_edge_case(pn, name):
    sc, prm, runs = EC.table()[name]
    out = CK.run_against_replay(pn, sc, prm, runs)
    res, taps = out[0]
    if name.startswith("refine_") or (name.startswith("size_") and name != "size_4"):   # Refine's own pose left the kernel
        assert res["found"] and res["refined"] and int(res["refine_runs"]) == 1 and taps[0]["refine_ran"]
    if name == "two_changes":
        assert int(res["refine_runs"]) == 2 and list(taps["refine_ran"]) == [0, 1, 0, 1, 0, 0] and not res["refined"] and res["found"]
    if name == "older_across_chunks":   # iteration 65 meets the Refine result iteration 62 left, a chunk earlier
        assert int(res["refine_runs"]) == 1 and taps[62]["refine_ran"] and not taps[65]["refine_ran"]
        assert int(taps[65]["refine_inliers"]) == int(taps[62]["refine_inliers"]) > 0
    if name == "tie_across_chunks":
        assert int(res["refine_runs"]) == 1 and taps[63]["refine_ran"] and not taps[64]["refine_ran"]
    if name.startswith("carried_"):
        assert out[1][0]["found"] and out[1][0]["no_more"] and not out[1][0]["refined"] and int(out[1][0]["refine_runs"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,tap_at", [("return_at_63", 63), ("return_at_64", 63), ("return_at_64", 64), ("return_at_130", 130),
                                         ("best_survives_clamp", 69), ("tie_across_chunks", 64)])
def test_tap_errors_at_the_chunk_boundary_and_the_last_iteration(name, tap_at):
    """error2 of the chosen iteration: the last lane of chunk 0, the first of chunk 1, the iteration a call returns at (written
    before the scan decides the return) and the last one before the clamp"""
    sc, prm, runs = EC.table()[name]
    assert tap_at < runs[0]["out"]["iterations_run"]
    with PnP(64, 1) as h:
        h.set_tap_iteration(tap_at)
        CK.run_against_replay(h, sc, prm, runs, tap_at=tap_at)


def _specs(group):
    """the sets of one launch.  'all': the first call of every case and a negative-length set.  'carried': sets entered with the
    state and best mask of an earlier host call (the second call of carried_1 and carried_63), a set without key slice and two
    whose inliers carry keypoint_index values outside the slice.  'negative' / 'below_zero' / 'past_max': the carried sets with
    one malformed set"""
    tab = EC.table()
    if group == "all":
        return [dict(name=k, replay=tab[k]) for k in NAMES] + [dict(name="negative", replay=tab["size_5"], bad="negative")]
    s = [dict(name="carried_1", replay=tab["carried_1"], call=1),
         dict(name="size_65", replay=tab["size_65"], kp_edges=True),
         dict(name="size_256", replay=tab["size_256"], n_keys=0),
         dict(name="carried_63", replay=tab["carried_63"], call=1, kp_edges=True),
         dict(name="refine_det_neg", replay=tab["refine_det_neg"])]
    if group == "below_zero":
        s.insert(0, dict(name="below_zero", replay=tab["size_5"], bad="below_zero"))
    elif group in ("negative", "past_max"):
        s.append(dict(name=group, replay=tab["size_5"], bad=group))
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["all", "carried", "negative", "below_zero", "past_max"])
def test_batched_launch_twice_on_one_handle(group):
    import torch
    b = CK.build_batch(_specs(group), MAX_POINTS)
    assert len(b["specs"]) <= 32 and len(b["P3"]) <= MAX_POINTS
    with PnP(MAX_POINTS, 32) as h:
        h.set_tap_iteration(0)
        for _ in range(2):   # the second launch meets the slab, the index list and the taps the first one left
            outs = CK.launch_batch(h, b)
            torch.cuda.synchronize()
            CK.check_batch(b, outs, h)


@pytest.mark.gpu
def test_two_handles_two_streams_with_different_edge_cases():
    """two launches per handle, other batches in another order on the other handle, all four enqueued back to back: scratch, index
    list or taps that were not per handle would mix the sets of one with the other's"""
    import torch
    work = {0: ["all", "below_zero"], 1: ["past_max", "all"]}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with PnP(MAX_POINTS, 32) as h0, PnP(MAX_POINTS, 32) as h1:
        handles = [h0, h1]
        b, up, out = {}, {}, {}
        for k in (0, 1):
            handles[k].set_tap_iteration(0)
            for step in range(2):
                b[k, step] = CK.build_batch(_specs(work[k][step]), MAX_POINTS)
                up[k, step] = CK.upload_batch(b[k, step])
        torch.cuda.synchronize()   # the uploads; from here on nothing waits until all four launches are enqueued
        for step in range(2):
            for k in (0, 1):
                out[k, step] = CK.enqueue_batch(handles[k], up[k, step], streams[k])
        for st in streams:
            st.synchronize()
        for (k, step), o in out.items():
            CK.check_batch(b[k, step], o, handles[k] if step == 1 else None)   # the taps are the last call's


# ---- the device constructor ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("short", [None, 0, 1, "all"])
def test_prepare_device_capacity_index_and_octave_edges(pn, short):
    """capacity = the buffers' size (None), the count, the count - 1 and 0: min(count, capacity) rows are written and reported,
    nothing at or past that; an index at or past n_mappoints and an octave outside the levels count as no map point"""
    import torch
    x, y, octave, idx, pos, usable = EC.prepare_inputs()
    n = len(idx)
    keys = np.zeros(n, _ffi.KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = x, y, octave
    sigma2 = (np.float32(1.2) ** (2 * np.arange(EC.N_LEVELS, dtype=np.float32)))
    oP2D, osg, oP3, okp = PO.construct(np.stack([x, y], 1), np.where(usable, octave, 0), sigma2, np.where(usable, idx, -1), pos)
    count = len(okp)
    assert count == int(usable.sum()) > 256
    cap = n if short is None else 0 if short == "all" else count - short
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev).view(dt)   # noqa: E731
    d_keys, d_s2, d_idx, d_pos = t(keys, torch.uint8), t(sigma2, torch.float32), t(idx, torch.int32), t(pos, torch.float32)
    P2D = torch.full((n, 2), -7.0, dtype=torch.float32, device=dev)
    sg = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    P3 = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    kp = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = _ffi.tensor_ptr
    pn._call("prepare_device", pn.h, p(d_keys), n, p(d_s2), EC.N_LEVELS, p(d_idx), p(d_pos), EC.N_MAPPOINTS, p(P2D), p(sg), p(P3), p(kp), p(cnt),
             cap, _ffi.stream_arg(dev, None))
    torch.cuda.synchronize()
    c = min(count, cap)
    assert int(cnt.cpu()[0]) == c
    P2D, sg, P3, kp = (a.cpu().numpy() for a in (P2D, sg, P3, kp))
    assert CK.same_bits(P2D[:c], oP2D[:c]) and CK.same_bits(sg[:c], osg[:c]) and CK.same_bits(P3[:c], oP3[:c]) and np.array_equal(kp[:c], okp[:c])
    assert (P2D[c:] == -7).all() and (sg[c:] == -7).all() and (P3[c:] == -7).all() and (kp[c:] == -7).all()

"""csrc/orbfe_sim3.hip on the cases of tests/sim3_edge_cases.py (what each is for: tests/test_sim3_edge_cases.py), bit for bit
against the canonical oracle: every case through the host call with all it leaves behind (result, both masks, state, best
model, every tap record, tap errors at the first, middle and last iteration run), every case again in batched launches run
twice on one handle, the sets a launch must not touch (negative length, more pairs than the handle holds) with sentinel bytes
around them, idx1 values outside the key slice, n_keys = 0, sets entered with the state of an earlier call, and two handles on
two streams at once.  No tolerance anywhere."""
import numpy as np
import pytest

import sim3_cases as SC
import sim3_checks as CK
import sim3_edge_cases as EC
from orb_slam2_ssd_semantic_amd import Sim3

NAMES = sorted(EC.table())


@pytest.fixture(scope="module")
def sm():
    h = Sim3(EC.MAX_PAIRS, 32)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_call_edge_case(sm, name):
    c = EC.table()[name]
    outs, _ = EC.reference(name)
    state, best_mask = CK.check_case(sm, c, outs)
    if name == "clamp_carried":   # the call after no_more: zero T12, state and best mask as the call before left them
        assert outs[2]["iterations_run"] == 0 and int(state["iterations"][0]) == 32
        assert np.array_equal(best_mask, outs[1]["state"]["best_mask"]) and CK.model_equal(state["best"][0], outs[1]["state"]["best"])
    if name.startswith("tie_"):   # the later model of the tie is the best
        a, b = c["tie"]
        assert CK.same_bits(state["best"][0]["T12"], outs[0]["log"][b]["T12"]) and not CK.same_bits(state["best"][0]["T12"], outs[0]["log"][a]["T12"])
    if name.startswith("zero_tie_"):
        assert int(state["best_inliers"][0]) == 0 and CK.same_bits(state["best"][0]["T12"], outs[0]["log"][1]["T12"])


@pytest.mark.gpu
def test_tap_errors_at_the_chunk_boundary(sm):
    """err1 / err2 of iterations 31 and 32 (the last lane of chunk 0, the first of chunk 1) and of the last iteration run"""
    c = EC.table()["tie_31_32"]
    CK.check_case(sm, c, EC.reference("tie_31_32")[0], errors_at=[0, 31, 32, 39])
    c = EC.table()["clamp_33"]
    CK.check_case(sm, c, EC.reference("clamp_33")[0], errors_at=[0, 32])


def _oversized():
    """520 pairs: more than the handle holds"""
    X1, X2, s1, s2, _ = SC.scene(520, 100, 77)
    return SC.make("oversized", X1, X2, s1, s2, [(2, np.zeros(6, np.int32))], True, 20, max_its=300)


def _specs(group):
    """the sets of one launch.  'all': the first call of every case and a negative-length set.  'carried': sets entered with the
    state and best mask of an earlier call (the second and third call of clamp_carried: 12 iterations to the clamp, then none),
    a set without key slice, two whose inliers carry idx1 values outside the slice, an oversized set and a negative-length set"""
    tab = EC.table()
    ref = lambda k: EC.reference(k)[0]   # noqa: E731
    if group == "all":
        return [dict(case=tab[k], outs=ref(k)) for k in NAMES] + [dict(case=tab["scale_20"], outs=ref("scale_20"), bad="negative")]
    return [dict(case=tab["clamp_carried"], outs=ref("clamp_carried"), call=1),
            dict(case=tab["one_nan_in_chunk"], outs=ref("one_nan_in_chunk"), idx1_edges=True),
            dict(case=tab["pairs_256"], outs=ref("pairs_256"), n_keys=0),
            dict(case=tab["clamp_carried"], outs=ref("clamp_carried"), call=2),
            dict(case=_oversized(), outs=None, bad="oversized"),
            dict(case=tab["count_eq_min_minus_1"], outs=ref("count_eq_min_minus_1"), idx1_edges=True),
            dict(case=tab["scale_20"], outs=ref("scale_20"), bad="negative")]


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["all", "carried"])
def test_batched_launch_twice_on_one_handle(group):
    import torch
    b = CK.build_batch(_specs(group))
    assert len(b["specs"]) <= 32
    with Sim3(EC.MAX_PAIRS, 32) as h:
        h.set_tap_iteration(0)
        for _ in range(2):   # the second launch meets the scratch and the taps the first one left
            outs = CK.launch_batch(h, b)
            torch.cuda.synchronize()
            CK.check_batch(b, outs, h)


@pytest.mark.gpu
def test_two_handles_two_streams_with_different_edge_cases():
    """two launches per handle, the same two batches in the other order on the other handle, all four enqueued back to back:
    scratch or taps that were not per handle would mix the sets of one with the other's"""
    import torch
    work = {0: ["all", "carried"], 1: ["carried", "all"]}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with Sim3(EC.MAX_PAIRS, 32) as h0, Sim3(EC.MAX_PAIRS, 32) as h1:
        handles = [h0, h1]
        b, up, out = {}, {}, {}
        for k in (0, 1):
            handles[k].set_tap_iteration(0)
            for step in range(2):
                b[k, step] = CK.build_batch(_specs(work[k][step]))
                up[k, step] = CK.upload_batch(b[k, step])
        torch.cuda.synchronize()   # the uploads; from here on nothing waits until all four launches are enqueued
        for step in range(2):
            for k in (0, 1):
                out[k, step] = CK.enqueue_batch(handles[k], up[k, step], streams[k])
        for st in streams:
            st.synchronize()
        for (k, step), o in out.items():
            CK.check_batch(b[k, step], o, handles[k] if step == 1 else None)   # the taps are the last call's

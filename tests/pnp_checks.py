"""What tests/test_gpu_pnp.py and tests/test_gpu_pnp_edges.py share: the bit comparison and the replay of an oracle run of
tests/pnp_cases.replay_custom on a PnP handle, with everything a call leaves behind compared."""
import contextlib

import numpy as np

import pnp_cases as PC
from orb_slam2_ssd_semantic_amd import pnp as PN


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def params_of(prm, th2=5.991):
    params = np.zeros(1, PN.PARAMS_DTYPE)
    params["min_inliers"], params["epsilon"], params["max_its"], params["th2"] = prm[0], prm[1], prm[2], np.float32(th2)
    return params


def check_result(res, mask, o, where):
    """a RESULT_DTYPE record and the mask of a call against the oracle's out dict"""
    assert int(res["iterations_run"]) == o["iterations_run"], where
    assert bool(res["found"]) == (o["Tcw"] is not None) and bool(res["no_more"]) == o["no_more"], where
    assert int(res["n_inliers"]) == o["n_inliers"], where
    assert np.array_equal(np.asarray(mask).astype(bool), o["mask"]), where
    assert same_bits(res["Tcw"], o["Tcw"] if o["Tcw"] is not None else np.zeros((4, 4), np.float32)), where


def check_state(state, best_mask, r, where):
    """a STATE_DTYPE record and the best mask after a call against the oracle's run dict"""
    assert int(state["iterations"]) == r["iterations"] and int(state["best_inliers"]) == r["best_inliers"], where
    assert np.array_equal(np.asarray(best_mask).astype(bool), r["best_mask"]), where
    assert same_bits(state["best_Tcw"], r["best_Tcw"]), where


def check_taps(taps, want, where):
    """the iteration records of a call against the oracle's taps"""
    assert len(taps) == min(len(want), PN.TAP_ITERS), where
    for k, (g, t) in enumerate(zip(taps, want)):
        assert list(g["quad"]) == list(t["quad"]) and int(g["N"]) == t["N"], (where, k)
        assert same_bits(g["R"], t["R"]) and same_bits(g["t"], t["t"]), (where, k)
        assert int(g["n_inliers"]) == t["n_inliers"] and int(g["refine_inliers"]) == t["refine_inliers"], (where, k)


def run_against_replay(pn, sc, prm, runs, tap_at=0, th2=5.991):
    """replays the oracle's calls on the device and compares everything a call leaves behind.  tap_at: the iteration the
    handle's set_tap_iteration names; its errors are compared in every call that ran it"""
    params = params_of(prm, th2)
    state = np.zeros(1, PN.STATE_DTYPE)
    best_mask = np.zeros(len(sc["P3Dw"]), np.uint8)
    results = []
    for ci, r in enumerate(runs):
        res, mask = pn.iterate(sc["P3Dw"], sc["P2D"], sc["sigma2"], PC.K, params, r["n_iterations"], r["draws"], state, best_mask)
        o = r["out"]
        check_result(res, mask, o, ci)
        check_state(state[0], best_mask, r, ci)
        taps = pn.tap(0, PN.TAP_ITERATIONS) if o["iterations_run"] else np.zeros(0, PN.ITER_DTYPE)
        check_taps(taps, r["taps"], ci)
        if o["iterations_run"] > tap_at:
            assert same_bits(pn.tap(0, PN.TAP_ERRORS), r["taps"][tap_at]["error2"]), ci
        results.append((res, taps))
    return results


# ---- the batched form against the oracle ---------------------------------------------------------------------------------------
SENTINEL, PAD = 0xA5, 16
NOTHING = np.zeros(1, PN.RESULT_DTYPE)
NOTHING["no_more"] = 1   # what the kernel writes for a set it cannot run: every word of the result, and nothing else


def state_record(r):
    """the oracle's state after a call (a run dict of pnp_cases.replay_custom; None: a new solver) as a STATE_DTYPE [1]"""
    s = np.zeros(1, PN.STATE_DTYPE)
    if r is not None:
        s["iterations"], s["best_inliers"], s["best_Tcw"] = r["iterations"], r["best_inliers"], r["best_Tcw"]
    return s


def build_batch(specs, max_points):
    """CSR arrays of one launch.  A spec: dict(name, replay=(scene, params, runs), call=0, n_keys=None, kp_edges=False, bad=None).
    `call` k enters with the oracle's state and best mask after call k - 1.  n_keys: the size of the set's key slice (default
    n + 7; 0: no scatter).  kp_edges: the keypoint_index values of the first three inliers of the returned mask are -1, n_keys
    and n_keys + 5 (no byte may be written for them; the key mask has PAD sentinel bytes before the first and after the last
    slice).  bad: a set the kernel must not run -- "negative" (offsets[i + 1] < offsets[i]; the last set), "below_zero"
    (offsets[i] < 0; the first set) or "past_max" (offsets[i + 1] > max_points; the last set); such a set brings no rows"""
    off, rows, sets, draws, kps, state, best, koff = [0], [], np.zeros(len(specs), PN.SET_DTYPE), [], [], [], [], PAD
    for i, sp in enumerate(specs):
        sc, prm, runs = sp["replay"]
        k = sp.get("call", 0)
        r, prev = runs[k], (runs[k - 1] if k else None)
        n = len(sc["P3Dw"])
        n_keys = n + 7 if sp.get("n_keys") is None else sp["n_keys"]
        room = max(n_keys, 5)   # bytes of the key mask that belong to this set (some even when it asks for no scatter)
        kp = np.sort(np.random.default_rng(i).permutation(max(n_keys, n))[:n]).astype(np.int32)
        if sp.get("kp_edges"):
            pos = np.flatnonzero(r["out"]["mask"])[:3]
            assert len(pos) == 3
            kp[pos] = (-1, n_keys, n_keys + 5)
        bad = sp.get("bad")
        if bad == "negative":
            assert i == len(specs) - 1
            off.append(off[-1] - 5)
        elif bad == "below_zero":
            assert i == 0
            off = [-3, 0]
        elif bad == "past_max":
            assert i == len(specs) - 1
            off.append(max_points + 1)
        else:
            off.append(off[-1] + n)
            rows.append(sc)
            kps.append(kp)
            best.append(prev["best_mask"].astype(np.uint8) if prev else np.zeros(n, np.uint8))
        sets[i]["K"] = PC.K
        sets[i]["params"] = params_of(prm)[0]
        sets[i]["n_iterations"], sets[i]["draws_offset"] = r["n_iterations"], sum(len(x) for x in draws)
        sets[i]["key_offset"], sets[i]["n_keys"] = koff, n_keys
        draws.append(np.asarray(r["draws"], np.int32))
        state.append(state_record(prev))
        sp.update(n=n, lo=off[-2], hi=off[-1], koff=koff, room=room, kp=kp, nk=n_keys, run=r)
        koff += room
    cat = lambda key, w: np.concatenate([np.asarray(sc[key], np.float32).reshape(-1, w) for sc in rows])   # noqa: E731
    return dict(specs=specs, off=np.array(off, np.int32), sets=sets, draws=np.concatenate(draws + [np.zeros(1, np.int32)]),
                kp=np.concatenate(kps), nkeys=koff + PAD, state=np.concatenate(state), best=np.concatenate(best),
                P3=cat("P3Dw", 3), P2=cat("P2D", 2), sg=cat("sigma2", 1).ravel())


def upload_batch(b):
    """the device tensors of one launch: every output starts as sentinel bytes, the state and best mask of a set that runs as
    the batch gives them.  The copies run on the default stream and nothing here waits for them"""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    N = len(b["P3"])
    st = b["state"].copy().view(np.uint8).reshape(len(b["sets"]), -1)
    for i, sp in enumerate(b["specs"]):
        if sp.get("bad"):
            st[i] = SENTINEL
    return dict(state=t(st), best_mask=t(b["best"]),
                result=torch.full((len(b["sets"]), PN.RESULT_DTYPE.itemsize), SENTINEL, dtype=torch.uint8, device=dev),
                mask=torch.full((max(N, 1),), SENTINEL, dtype=torch.uint8, device=dev),
                key_mask=torch.full((b["nkeys"],), SENTINEL, dtype=torch.uint8, device=dev), kp=t(b["kp"]),
                ins=[t(b["off"]), t(b["P3"]), t(b["P2"]), t(b["sg"]), t(b["sets"].view(np.uint8).reshape(len(b["sets"]), -1)), t(b["draws"])])


def enqueue_batch(h, up, stream=None):
    """one iterate_device over uploaded tensors on `stream`, no synchronisation.  -> the outputs check_batch takes (the whole
    upload rides along: the inputs stay alive until the caller has synchronised)"""
    import torch
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        h.iterate_device(*up["ins"], up["state"], up["best_mask"], result=up["result"], mask=up["mask"], keypoint_index=up["kp"],
                         key_mask=up["key_mask"])
    return up["state"], up["best_mask"], up["result"], up["mask"], up["key_mask"], up


def launch_batch(h, b, stream=None):
    """upload, wait for the copies, enqueue"""
    import torch
    up = upload_batch(b)
    torch.cuda.synchronize()   # the fills ran on the default stream
    return enqueue_batch(h, up, stream)


def check_batch(b, outs, h=None, tap_at=0):
    """the outputs of launch_batch (synchronised) against the oracle, set by set; h: the handle, for the taps of its first sets"""
    state, best_mask, result_raw, mask, key_mask = (x.cpu().numpy() for x in outs[:5])
    state_raw = state
    state = state.view(PN.STATE_DTYPE).ravel()
    result = result_raw.view(PN.RESULT_DTYPE).ravel()
    assert (key_mask[:PAD] == SENTINEL).all() and (key_mask[-PAD:] == SENTINEL).all()
    covered = np.zeros(len(mask), bool)
    for i, sp in enumerate(b["specs"]):
        name = (i, sp["name"])
        lo, hi = sp["lo"], sp["hi"]
        keys = key_mask[sp["koff"]:sp["koff"] + sp["room"]]
        if sp.get("bad"):   # the result's words and nothing else
            assert result_raw[i].tobytes() == NOTHING.tobytes(), name
            assert (state_raw[i] == SENTINEL).all() and (keys == SENTINEL).all(), name
            continue
        covered[lo:hi] = True
        r = sp["run"]
        check_result(result[i], mask[lo:hi], r["out"], name)
        check_state(state[i], best_mask[lo:hi], r, name)
        want = np.full(sp["room"], SENTINEL, np.uint8)
        if sp["nk"] > 0:
            want[:sp["nk"]] = 0
            ix = sp["kp"][r["out"]["mask"]]
            want[ix[(ix >= 0) & (ix < sp["nk"])]] = 1
        assert np.array_equal(keys, want), name
        if h is not None and i < PN.TAP_SETS and r["out"]["iterations_run"]:
            taps = h.tap(i, PN.TAP_ITERATIONS)
            check_taps(taps, r["taps"], name)
            if r["out"]["iterations_run"] > tap_at:
                assert same_bits(h.tap(i, PN.TAP_ERRORS), r["taps"][tap_at]["error2"]), name
    assert (mask[~covered] == SENTINEL).all()

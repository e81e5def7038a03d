"""The sequence pipeline's lane rule (orb_pipe_lanes in csrc/orbfe_pipe_plan.h) without a GPU, through the test hook
orbfe_internal_pipe_lanes, over the grid of test_pipe_plan.py times the sub-batch counts 1, 2 and 5.

The rule, restated here independently of the header.  A device-entry call runs in lanes -- its four streams carry one stage group
each instead of one whole sub-batch each -- exactly when
  * the plan has no copy streams (the host entry point keeps its plan),
  * it is short of queues: fewer kernel streams than pipes,
  * it has exactly 3 kernel streams and the side stream,
  * the call has at least two sub-batches;
min(P, 8) extractor handles then rotate as buffer sets.  Everywhere else the answer is "chains" with the plan's own P_eff handles,
and the plan itself (orbfe_internal_pipe_plan) is what it was.  Also: the rule under AddressSanitizer / UBSan
(tests/cpp/test_pipe_lanes_sanitize.cpp, a child process without a device)."""
import ctypes as C
import os
import subprocess

import pytest

from orb_slam2_ssd_semantic_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPES = (1, 2, 3, 4, 5, 8, 12, 16, 64)
QUEUES = (1, 2, 3, 4, 8, 16, 32)
NSUB = (1, 2, 5)
GRID = [(P, Q, c, n) for P in PIPES for Q in QUEUES for c in (0, 1) for n in NSUB]
LANE_SETS = 8


def lanes(P, Q, copies, nsub):
    """(ok, lanes, sets)"""
    f = _ffi.lib().orbfe_internal_pipe_lanes
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    f.restype = C.c_int32
    out = (C.c_int32 * 2)(-99, -99)
    if f(P, Q, copies, nsub, out) != 0:
        return False, None, None
    return True, out[0], out[1]


def plan_head(P, Q, copies):
    f = _ffi.lib().orbfe_internal_pipe_plan
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    f.restype = C.c_int32
    out = (C.c_int32 * (9 + 64))()
    assert f(P, Q, copies, out) == 0
    return dict(zip(("P", "Q", "copies", "S", "P_eff", "side", "first", "side_index", "nstreams"), list(out)[:9]))


def expected(P, Q, copies, nsub):
    """the rule from the stream counts, worked out here from P and Q alone"""
    left = max(1, Q - (2 if copies else 0))
    if left >= P + 1:
        S, side = P, 1
    else:
        S, side = max(1, left - 1), 1 if left >= 2 else 0
    on = (not copies) and S < P and S == 3 and side == 1 and nsub >= 2
    return (1, min(P, LANE_SETS)) if on else (0, min(P, S))


@pytest.mark.parametrize("P,Q,copies,nsub", GRID)
def test_lanes_follow_the_rule(P, Q, copies, nsub):
    ok, on, sets = lanes(P, Q, copies, nsub)
    assert ok
    assert (on, sets) == expected(P, Q, copies, nsub)
    assert 1 <= sets <= P
    p = plan_head(P, Q, copies)
    if on:
        # the same four streams the plan creates: three kernel streams and the side stream, nothing more
        assert (p["S"], p["side"], p["nstreams"], p["copies"]) == (3, 1, 4, 0) and P > 3 and nsub >= 2
    else:
        assert sets == p["P_eff"]   # chains: the plan's own pipes take the sub-batches


def test_where_lanes_apply():
    """without copy streams and with two sub-batches or more: exactly 4 queues and more than 3 pipes"""
    for P in PIPES:
        for Q in QUEUES:
            assert lanes(P, Q, 0, 2)[1] == (1 if Q == 4 and P >= 4 else 0), (P, Q)
            assert lanes(P, Q, 1, 5)[1] == 0 and lanes(P, Q, 0, 1)[1] == 0
    assert lanes(12, 4, 0, 24) == (True, 1, 8)      # the headline shape
    assert lanes(12, 16, 0, 24) == (True, 0, 12)    # enough queues: the plan of P + 1 streams, in chains
    assert lanes(3, 4, 0, 24) == (True, 0, 3)
    assert lanes(12, 2, 0, 24) == (True, 0, 1)
    for P in (0, -1, 65):
        assert not lanes(P, 4, 0, 2)[0]
    assert lanes(12, 4, 0, 0)[1] == 0 and lanes(12, 4, 0, -3)[1] == 0


def test_lane_rule_under_sanitizers(tmp_path):
    """The header alone, host-only with AddressSanitizer and UBSan, walks the grid in a child process; its lines are the library's."""
    from orb_slam2_ssd_semantic_amd import _build
    exe = str(tmp_path / "test_pipe_lanes_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", _build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_pipe_lanes_sanitize.cpp"), "-o", exe])
    grid = GRID + [(0, 4, 0, 2), (65, 4, 0, 2), (12, 0, 1, 2), (12, 1000, 0, 5), (64, -7, 0, 2), (12, 4, 0, 0), (12, 4, 0, -1),
                   (12, 4, 0, 2 ** 31 - 1)]
    req = [f"lanes {P} {Q} {c} {n}" for P, Q, c, n in grid]
    r = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(req)
    for (P, Q, c, n), line in zip(grid, lines):
        ok, on, sets = lanes(P, Q, c, n)
        assert line == (f"1 {on} {sets}" if ok else "0"), (P, Q, c, n)

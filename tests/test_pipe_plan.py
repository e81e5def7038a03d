"""The sequence pipeline's stream plan (csrc/orbfe_pipe_plan.h) without a GPU, through the test hooks orbfe_internal_pipe_plan and
orbfe_internal_pipe_parse_queues / orbfe_internal_pipe_env_queues.

The rules, restated here independently of the header (P pipes asked for, Q hardware queues, copy streams of the host entry point
in use or not):
  * the two copy streams, where in use, come first and take their queues off the top: `left` = max(1, Q - 2) or Q;
  * kernel-carrying streams (kernel streams + side stream) never outnumber `left`: no two of them share a queue;
  * with left >= P + 1 the plan is the one the pipeline had before it knew about queues: P streams, one shared side stream;
  * otherwise S = left - 1 kernel streams (the variant that measured faster than S = left: profiles/pipe_queues.md), and the side
    stream exists exactly when that leaves a queue spare: with left = 1 there is one kernel stream and the blur runs in it;
  * P_eff = min(P, S) pipes take the sub-batches round robin, and the P handles are dealt over the S streams evenly.
Also: the parsing of GPU_MAX_HW_QUEUES, and the planner under AddressSanitizer / UBSan (tests/cpp/test_pipe_plan_sanitize.cpp, a
child process without a device)."""
import ctypes as C
import os
import subprocess

import pytest

from orb_slam2_ssd_semantic_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPES = (1, 2, 3, 4, 5, 8, 12, 16, 64)
QUEUES = (1, 2, 3, 4, 8, 16, 32)
GRID = [(P, Q, c) for P in PIPES for Q in QUEUES for c in (0, 1)]
FIELDS = ("P", "Q", "copies", "S", "P_eff", "side", "first", "side_index", "nstreams")
MAX_PIPES = 64
# text of the variable -> queues (None: not set)
PARSE = [(None, 4), ("", 4), ("abc", 4), ("4x", 4), ("0", 4), ("-3", 4), ("1", 1), ("2", 2), ("4", 4), ("16", 16), ("32", 32), ("33", 32),
         ("64", 32), ("99999999999999999999999", 32), ("-99999999999999999999999", 4), (" 8", 8), ("8 ", 8), ("1.5", 4), ("0x10", 4)]


def plan(P, Q, copies):
    """(ok, fields dict, [stream of pipe i])"""
    L = _ffi.lib()
    f = L.orbfe_internal_pipe_plan
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    f.restype = C.c_int32
    out = (C.c_int32 * (len(FIELDS) + MAX_PIPES))(*([-99] * (len(FIELDS) + MAX_PIPES)))
    s = f(P, Q, copies, out)
    if s != 0:
        return False, None, None
    v = list(out)
    return True, dict(zip(FIELDS, v[:len(FIELDS)])), v[len(FIELDS):]


def parse(text):
    f = _ffi.lib().orbfe_internal_pipe_parse_queues
    f.argtypes = [C.c_char_p]
    f.restype = C.c_int32
    return f(None if text is None else text.encode())


@pytest.mark.parametrize("P,Q,copies", GRID)
def test_plan_follows_the_rules(P, Q, copies):
    ok, p, sop = plan(P, Q, copies)
    assert ok and (p["P"], p["Q"], p["copies"]) == (P, Q, copies)
    first = 2 if copies else 0
    left = max(1, Q - first)
    S = p["S"]
    # the stream count bound: kernel-carrying streams fit the queues the copy streams leave; at least one kernel stream
    assert 1 <= S <= P
    assert S + p["side"] <= left
    assert p["nstreams"] == first + S + p["side"] and p["first"] == first
    if Q >= first + 1:
        assert p["nstreams"] <= Q
    # every pipe has a stream; the pipes are dealt evenly; streams beyond P are not claimed
    assert all(0 <= s < S for s in sop[:P]) and all(s == -1 for s in sop[P:])
    load = [sop[:P].count(s) for s in range(S)]
    assert min(load) >= 1 and max(load) - min(load) <= 1
    # P_eff and an even split of the sub-batches: pipes 0 .. P_eff - 1 sit on P_eff distinct streams, so sub-batch j on pipe
    # (rot + j) mod P_eff loads every stream alike whatever rot is
    assert p["P_eff"] == min(P, S)
    assert sorted(sop[:p["P_eff"]]) == list(range(p["P_eff"])) and p["P_eff"] == S
    for rot in range(p["P_eff"]):
        hits = [0] * S
        for j in range(3 * p["P_eff"]):
            hits[sop[(rot + j) % p["P_eff"]]] += 1
        assert hits == [3] * S
    # the side stream exists exactly when a queue is spare
    assert p["side"] == (1 if left - S >= 1 else 0)
    assert p["side_index"] == (first + S if p["side"] else -1)
    # the earlier plan wherever the queues allow it: P streams, pipe i on stream i, one shared side stream
    if left >= P + 1:
        assert S == P and p["side"] == 1 and sop[:P] == list(range(P))
    else:
        assert S == max(1, left - 1)


@pytest.mark.parametrize("P,Q", [(P, Q) for P in PIPES for Q in QUEUES if Q >= P + 1])
def test_plan_is_the_earlier_one_when_the_queues_allow(P, Q):
    """without copy streams: Q >= P + 1; with them the same holds once they have taken their two queues (Q - 2 >= P + 1)"""
    ok, p, sop = plan(P, Q, 0)
    assert ok and (p["S"], p["P_eff"], p["side"], p["nstreams"]) == (P, P, 1, P + 1) and sop[:P] == list(range(P))
    ok, p, sop = plan(P, Q + 2, 1)
    assert ok and (p["S"], p["P_eff"], p["side"], p["nstreams"]) == (P, P, 1, P + 3) and sop[:P] == list(range(P))


def test_plan_is_deterministic_and_clamps():
    for P, Q, c in GRID:
        assert plan(P, Q, c) == plan(P, Q, c)
    # Q outside 1 .. 32 is clamped, P outside 1 .. 64 refused
    assert plan(12, 0, 0)[1]["Q"] == 1 and plan(12, -5, 1)[1]["Q"] == 1 and plan(12, 1000, 0)[1]["Q"] == 32
    assert plan(12, 1000, 0)[1:] == plan(12, 32, 0)[1:]
    for P in (0, -1, 65):
        assert not plan(P, 4, 0)[0]
    # the headline shape on the runtime's default: three chains and the side stream; with the copy streams one; on one queue one
    assert (plan(12, 4, 0)[1]["S"], plan(12, 4, 0)[1]["side"]) == (3, 1)
    assert (plan(12, 4, 1)[1]["S"], plan(12, 4, 1)[1]["side"]) == (1, 1)
    assert (plan(1, 4, 1)[1]["S"], plan(1, 4, 1)[1]["side"]) == (1, 1)
    assert (plan(12, 1, 0)[1]["S"], plan(12, 1, 0)[1]["side"]) == (1, 0)


@pytest.mark.parametrize("text,want", PARSE)
def test_queue_count_from_the_variable(text, want):
    assert parse(text) == want


def test_the_library_reads_the_environment_once():
    f = _ffi.lib().orbfe_internal_pipe_env_queues
    f.restype = C.c_int32
    want = parse(os.environ.get("GPU_MAX_HW_QUEUES"))
    assert f() == want and f() == want


def test_planner_under_sanitizers(tmp_path):
    """The header alone, host-only with AddressSanitizer and UBSan, walks the grid and the parsing cases in a child process; its
    lines are the library's."""
    from orb_slam2_ssd_semantic_amd import _build
    exe = str(tmp_path / "test_pipe_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", _build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_pipe_plan_sanitize.cpp"), "-o", exe])
    extra = [(0, 4, 0), (65, 4, 0), (12, 0, 1), (12, 1000, 0), (64, -7, 1)]
    req = [f"plan {P} {Q} {c}" for P, Q, c in GRID + extra]
    req += ["parse-null" if t is None else f"parse {t}" for t, _ in PARSE] + ["env"]
    r = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(req)
    for (P, Q, c), line in zip(GRID + extra, lines):
        ok, p, sop = plan(P, Q, c)
        want = "0" if not ok else "1 " + " ".join(str(p[k]) for k in FIELDS) + " |" + "".join(f" {s}" for s in sop[:P])
        assert line == want, (P, Q, c)
    n = len(GRID) + len(extra)
    assert [int(x) for x in lines[n:n + len(PARSE)]] == [w for _, w in PARSE]
    a, b = lines[-1].split()
    assert a == b == str(parse(os.environ.get("GPU_MAX_HW_QUEUES")))

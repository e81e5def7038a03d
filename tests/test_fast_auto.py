"""The automatic FAST mode (csrc/orbfe_fast_auto.h; orbfe_set_fast_mode 3, the default) without a GPU, through the test hook
orbfe_internal_fast_auto: n calls of a fresh handle in, the form (0 dense, 2 lane-compacting) and the probe flag of each out.

The rules, restated here independently of the header.  A call has a size in wave row steps and sees a probe outstanding or not;
the three counters {row steps, batches, parked pairs} of a finished probe may arrive before it.
  * a call below 140 000 row steps is dense, never probes, takes no answer (it waits for the next large call) and changes nothing;
  * an answer says "dense" when c0 > 0 and c2 > 0.25 * 128 * c0 (strictly, in double precision), else "compacting";
  * "dense": the next `hold` large calls are dense, hold starting at 16 and doubling with every such answer in a row up to 256;
    then one compacting call probes -- unless a probe is outstanding: such calls stay dense and do not probe;
  * "compacting" (and before any answer): calls are compacting, the hold goes back to 16; among the compacting calls that see
    no probe outstanding every 8th probes, counted from the first call of a fresh handle and from the answer (which counts as
    the first of its eight) -- calls that see a probe outstanding are not counted.
Also: the header under AddressSanitizer / UBSan (tests/cpp/test_fast_auto_sanitize.cpp, a child process without a device)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG, SMALL = 140000, 139999
ABOVE, BELOW = (1000, 7, 32001), (1000, 7, 32000)     # answers on either side of the threshold


def run(calls):
    """calls: [(row steps, pending, None or (c0, c1, c2))] -> [(form, probe)] of a fresh state"""
    f = _ffi.lib().orbfe_internal_fast_auto
    f.argtypes = [C.c_int32] + [C.c_void_p] * 6
    f.restype = C.c_int32
    n = len(calls)
    steps = np.array([c[0] for c in calls], np.int64)
    pend = np.array([c[1] for c in calls], np.uint8)
    has = np.array([c[2] is not None for c in calls], np.uint8)
    ans = np.array([c[2] or (0, 0, 0) for c in calls], np.uint64).reshape(n, 3)
    form, probe = np.full(n, -9, np.int32), np.full(n, 9, np.uint8)
    assert f(n, *(a.ctypes.data for a in (steps, pend, has, ans, form, probe))) == 0
    assert set(form.tolist()) <= {0, 2} and set(probe.tolist()) <= {0, 1}
    return list(zip(form.tolist(), map(bool, probe.tolist())))


class Model:
    """the rules of the module docstring"""

    def __init__(self):
        self.says_dense = False
        self.dense_to_go = 0
        self.next_hold = 16
        self.counted = 0       # compacting calls without a probe outstanding, since the count was last started
        self.mail = None

    def call(self, steps, pending, answer):
        if answer is not None:
            self.mail = answer
        if steps < 140000:
            return 0, False
        if self.mail is not None:
            c0, _, c2 = self.mail
            self.mail = None
            self.says_dense = c0 > 0 and float(c2) > 0.25 * 128.0 * float(c0)     # in double precision, as the library compares
            if self.says_dense:
                self.dense_to_go = self.next_hold
                self.next_hold = min(256, 2 * self.next_hold)
            else:
                self.next_hold = 16
                self.counted = 1
        if self.says_dense:
            if self.dense_to_go:
                self.dense_to_go -= 1
                return 0, False
            return (0, False) if pending else (2, True)
        if pending:
            return 2, False
        self.counted += 1
        return 2, self.counted % 8 == 1


def model(calls):
    m = Model()
    return [m.call(*c) for c in calls]


def with_small_calls(calls, seed):
    """the same calls with small ones strewn in; -> (calls, indices of the original ones)"""
    rng = random.Random(seed)
    out, keep = [], []
    for c in calls:
        for _ in range(rng.choice((0, 0, 1, 3))):
            out.append((rng.choice((SMALL, 1, 4890)), rng.random() < 0.5, None))
        keep.append(len(out))
        out.append(c)
    out.append((SMALL, False, None))
    return out, keep


def check(calls, want):
    """the hook gives `want`, the model agrees, and small calls in between change nothing (and are dense themselves)"""
    assert model(calls) == want
    assert run(calls) == want
    for seed in (1, 2):
        mixed, keep = with_small_calls(calls, seed)
        got = run(mixed)
        assert [got[i] for i in keep] == want
        assert all(got[i] == (0, False) for i in range(len(mixed)) if i not in keep)


D, Cq, CP = (0, False), (2, False), (2, True)     # dense, compacting, compacting + probe


def test_fresh_state_probes_first_and_then_every_eighth_compacting_call():
    check([(BIG, False, None)] * 26, ([CP] + [Cq] * 7) * 3 + [CP, Cq])


def test_nothing_probes_while_a_probe_is_pending():
    check([(BIG, False, None)] + [(BIG, True, None)] * 30, [CP] + [Cq] * 30)
    # ... and the calls that saw it pending are not counted towards the eight
    check([(BIG, False, None)] + [(BIG, True, None)] * 5 + [(BIG, False, None)] * 9, [CP] + [Cq] * 5 + [Cq] * 7 + [CP, Cq])


def test_small_calls_are_dense_and_140000_is_not_small():
    assert run([(SMALL, False, None)] * 5) == [D] * 5
    assert run([(BIG, False, None)]) == [CP]
    assert run([(SMALL, False, None)] * 20 + [(BIG, False, None)]) == [D] * 20 + [CP]     # the first large call still probes
    # an answer that arrives before a small call is taken by the next large one
    assert run([(BIG, False, None), (SMALL, True, ABOVE), (BIG, False, None)]) == [CP, D, D]


def test_answer_above_the_threshold_holds_16_dense_calls_then_probes():
    calls = [(BIG, False, None), (BIG, False, ABOVE)] + [(BIG, False, None)] * 15 + [(BIG, False, None)] + [(BIG, True, None)] * 6
    check(calls, [CP] + [D] * 16 + [CP] + [D] * 6)


def test_pending_probe_at_the_end_of_a_hold_keeps_the_calls_dense_without_a_probe():
    calls = [(BIG, False, None), (BIG, True, ABOVE)] + [(BIG, True, None)] * 20 + [(BIG, False, None)]
    check(calls, [CP] + [D] * 21 + [CP])


def test_consecutive_answers_above_the_threshold_double_the_hold_up_to_256():
    calls, want = [(BIG, False, None)], [CP]
    for hold in (16, 32, 64, 128, 256, 256):
        calls += [(BIG, False, ABOVE)] + [(BIG, False, None)] * (hold - 1) + [(BIG, False, None)]
        want += [D] * hold + [CP]
    check(calls, want)


def test_answer_below_the_threshold_goes_back_to_compacting_and_to_a_hold_of_16():
    calls = [(BIG, False, None), (BIG, False, ABOVE)] + [(BIG, False, None)] * 15 + [(BIG, False, None)]     # hold 16, probe
    want = [CP] + [D] * 16 + [CP]
    calls += [(BIG, False, ABOVE)] + [(BIG, False, None)] * 31 + [(BIG, False, None)]                          # hold 32, probe
    want += [D] * 32 + [CP]
    # "below": compacting at once; the answering call is the first of eight, so the 8th call from it probes
    calls += [(BIG, False, BELOW)] + [(BIG, False, None)] * 8
    want += [Cq] * 7 + [CP, Cq]
    # the next "above" holds 16 again, not 64
    calls += [(BIG, False, ABOVE)] + [(BIG, False, None)] * 15 + [(BIG, False, None)]
    want += [D] * 16 + [CP]
    check(calls, want)


@pytest.mark.parametrize("answer,dense", [((1000, 0, 32000), False), ((1000, 0, 32001), True), ((0, 0, 32001), False), ((0, 0, 0), False),
                                           ((0, 5, 2 ** 63), False), ((1, 0, 32), False), ((1, 0, 33), True),
                                           ((2 ** 40, 0, 2 ** 45), False), ((2 ** 40, 0, 2 ** 45 + 2 ** 20), True)])
def test_threshold_edge(answer, dense):
    check([(BIG, False, None), (BIG, False, answer)], [CP, D if dense else Cq])


def test_seeded_random_sequences_follow_the_model():
    for seed in (3, 4, 5):
        rng = random.Random(seed)
        m, calls, pending = Model(), [], False
        for _ in range(3000):
            steps = rng.choice((BIG, BIG, BIG, 10 ** 7, SMALL, 4890, 0))
            answer = None
            if pending and rng.random() < 0.2:      # the outstanding probe answers before this call
                c0 = rng.choice((0, 1, 1000, 123456))
                answer = (c0, rng.randrange(100), rng.choice((0, 32 * c0, 32 * c0 + 1, 50 * c0, 5 * c0)))
                pending = False
            elif rng.random() < 0.02:
                pending = not pending               # (the hook takes the flag as given: any sequence of flags is a case)
            calls.append((steps, pending, answer))
            pending = pending or m.call(steps, pending, answer)[1]
        want = model(calls)
        got = run(calls)
        assert got == want, next(i for i in range(len(calls)) if got[i] != want[i])
        assert {D, Cq, CP} <= set(want) and sum(w == CP for w in want) > 20


def test_header_under_sanitizers(tmp_path):
    """The header alone, host-only with AddressSanitizer and UBSan, replays a random sequence in a child process; its lines are
    the library's."""
    from orb_slam2_ssd_semantic_amd import _build
    exe = str(tmp_path / "test_fast_auto_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", _build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_fast_auto_sanitize.cpp"), "-o", exe])
    rng = random.Random(6)
    calls = []
    for _ in range(2000):
        c0 = rng.choice((0, 1000, 2 ** 50))
        answer = (c0, 1, rng.choice((0, 32 * c0, 32 * c0 + 1, 2 ** 64 - 1))) if rng.random() < 0.1 else None
        calls.append((rng.choice((BIG, SMALL, 2 ** 62, -5)), rng.random() < 0.3, answer))
    lines = [" ".join(map(str, (s, int(p)) + (a or ()))) for s, p, a in calls]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    got = [tuple(map(int, l.split())) for l in r.stdout.split("\n") if l]
    assert got == [(f, int(p)) for f, p in run(calls)] == [(f, int(p)) for f, p in model(calls)]

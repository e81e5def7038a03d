"""The sequence pipeline's call graph (csrc/orbfe_pipe_graph.h) without a GPU: tests/cpp/test_pipe_graph.cpp walks it with a sink that
prints, built plain and with AddressSanitizer / UBSan, over scripts of pipeline calls.

(a) The log is the rule: a twin written here from the two diagrams of DESIGN.md section 6 (frames instead of bytes, one pass per
    call) gives the same operations for every script.
(b) No hazard is unordered.  From the log alone: every stream is a FIFO, a wait follows the latest record of its event, an
    extraction begins on its start stream and ends on its tail stream (the FAST and blur streams of a lane call add no edge: the
    conservative choice), a joined call ends with the caller's stream waiting for every end event.  In the transitive closure every
    two operations that touch the same frame, match row or carry slot, one of them writing, are ordered.
(c) The error path: a sink that fails at its k-th call stops the walk there, for every k; behind the reset the next CONTINUE call
    has no predecessor frame.

The scripts are the smallest at which each rule matters: sub-batches of F = 2 frames, calls of 7 (four sub-batches), 1 and 3 frames."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, CAP = 2, 64
CONTINUE, NO_JOIN = 1, 2
LANE_SETS, LANE_PLACE = 8, 1   # the defaults of csrc/orbfe_pipe_plan.h

# (pipes, queues, lane sets asked for, placement): chains on 1, 3 and 5 kernel streams; lanes with 2, 4 and 8 sets, both placements
CHAINS = [(1, 16, 0, -1), (3, 16, 0, -1), (5, 16, 0, -1), (3, 4, 0, -1)]
LANES = [(12, 4, s, p) for s in (2, 4, 8) for p in (0, 1)] + [(5, 4, 0, -1)]


def _calls(*calls):
    """(frames, base frame, match blocks, flags) or "reset_sequence" -> the same, spelled out"""
    return [c if c == "reset_sequence" else dict(nframes=c[0], base=c[1], match=c[2], flags=c[3]) for c in calls]


C, N = CONTINUE | NO_JOIN, NO_JOIN
SEQUENCES = {
    "three CONTINUE calls into the same blocks": _calls((7, 0, 1, N), (7, 0, 1, C), (7, 0, 1, C), (7, 0, 1, C)),
    "the same, joined": _calls((7, 0, 1, 0), (7, 0, 1, CONTINUE), (7, 0, 1, CONTINUE), (7, 0, 1, CONTINUE)),
    "7, 1, 3 and 7 frames": _calls((7, 0, 1, N), (1, 0, 1, C), (3, 0, 1, C), (7, 0, 1, C), (1, 0, 1, C), (1, 0, 1, C)),
    "extract only, then matching": _calls((7, 0, 0, N), (7, 0, 0, C), (7, 0, 1, C), (7, 0, 1, C), (3, 0, 0, C), (7, 0, 1, C)),
    "no CONTINUE in mid-sequence": _calls((7, 0, 1, N), (7, 0, 1, C), (7, 0, 1, N), (7, 0, 1, C)),
    "reset_sequence": _calls((7, 0, 1, N), (7, 0, 1, C), "reset_sequence", (7, 0, 1, C), (7, 0, 1, C)),
    "blocks shifted by 1 and by F frames, longer after shorter": _calls((7, 0, 1, N), (7, 1, 1, C), (7, 1 + F, 1, C), (3, 1 + F, 1, C),
                                                                        (7, 1 + F, 1, C), (7, 2 + F, 1, C)),
    "blocks shifted forth and back": _calls((7, 0, 1, N), (7, F, 1, C), (7, 0, 1, C), (7, 1, 1, C), (7, 0, 1, C), (3, F, 1, C), (7, 1, 1, C)),
}
GRID = [(cfg, name) for cfg in CHAINS + LANES for name in SEQUENCES]


def _line(cfg, c, fail_at=0):
    if c == "reset_sequence":
        return c
    P, Q, sets, place = cfg
    return f"call {P} {Q} 0 -1 {sets} {place} {F} {CAP} {c['nframes']} {c['base']} {c['match']} {c['flags']} {fail_at}"


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the program, plain and under the sanitizers"""
    from orb_slam2_ssd_semantic_amd import _build
    d = tmp_path_factory.mktemp("pipe_graph")
    src = os.path.join(ROOT, "tests", "cpp", "test_pipe_graph.cpp")
    out = []
    for name, flags in (("plain", ["-O1"]), ("sanitize", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(d / f"test_pipe_graph_{name}")
        subprocess.check_call(["g++", "-std=c++17", *flags, "-I", _build.CSRC, src, "-o", exe])
        out.append(exe)
    return out


def _run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def _log(programs, lines):
    """the log of a script; both builds print the same"""
    plain, sanitized = (_run(exe, lines) for exe in programs)
    assert plain == sanitized
    return plain


def _per_call(log):
    """the log cut behind every "status" / "reset_sequence" line: [(operations, status or None)]"""
    out, cur = [], []
    for ln in log:
        if ln.startswith("status "):
            out.append((cur, int(ln.split()[1])))
            cur = []
        elif ln == "reset_sequence":
            out.append(([], None))
        else:
            cur.append(ln)
    assert not cur
    return out


# ---- (a) the twin: DESIGN.md section 6, in frames ---------------------------------------------------
class Twin:
    """What a pipeline remembers between calls, and the operations of a call.  Output addresses are absolute frame numbers (base
    frame of the call + frame in the call): all blocks of a call move together, so slices overlap where their frames do."""

    def __init__(self):
        self.ext, self.match, self.frames = set(), set(), {}   # indices with a recorded ev_ext / ev_match; frames under an index
        self.slot = 0            # carry slot the next call reads
        self.copy_of = {}        # index whose last frame a carry copy read -> the slot it went to
        self.predecessor = False # the next call's frame 0 has one
        self.m0, self.written = set(), set()   # slots with an unconsumed ev_m0 / that have been written
        self.rot = self.lane_rot = 0

    @staticmethod
    def plan(P, Q):
        """(kernel streams, side stream or None) of the device entry point, as pool indices"""
        if Q >= P + 1:
            S = P
        else:
            S = max(1, Q - 1)
        return list(range(S)), (S if Q >= 2 else None)

    def call(self, cfg, nframes, base, match, flags):
        P, Q, want, place = cfg
        kernel, side = self.plan(P, Q)
        nsub = -(-nframes // F)
        ops = []
        lanes = len(kernel) == 3 and side is not None and len(kernel) < P and nsub >= 2
        if lanes:   # by stage: pyramid on kernel stream 0, FAST on 1, quadtree + descriptor on 2, the blur beside them
            sets = min(P, want or LANE_SETS)
            blur_on_side = (LANE_PLACE if place < 0 else place) == 1
            blur, matcher = (side, kernel[2]) if blur_on_side else (kernel[0], side)
            first = self.lane_rot % sets
            where = lambda j: (kernel[0], kernel[2], matcher)  # noqa: E731
            carrying = kernel + [side]
            lane = (kernel[0], kernel[1], kernel[2], blur)
        else:       # by sub-batch: pipe (rot + j) mod P_eff, everything of the sub-batch on its stream
            sets = min(P, len(kernel))
            self.rot %= sets
            first = self.rot
            where = lambda j: (kernel[(first + j) % sets],) * 3  # noqa: E731
            carrying = kernel[:sets]
            lane = (-1, -1, -1, -1)
        cont = bool(flags & CONTINUE) and self.predecessor and bool(match)
        earlier = dict(self.frames)
        ops.append("record -1 fork 0")
        ops += [f"wait {s} fork 0" for s in carrying]
        for j in range(nsub):
            h = (first + j) % sets
            start, tail, sm = where(j)
            lo = j * F
            nf = min(F, nframes - lo)
            mine = set(range(base + lo, base + lo + nf))
            overlapping = [i for i in sorted(earlier) if i != j and earlier[i] & mine]   # as the previous calls left them
            for i in [j] + overlapping:
                ops += [f"wait {start} ext {i}"] * (i in self.ext) + [f"wait {start} match {i}"] * (i in self.match)
                ops += [f"wait {start} match {i + 1}"] * (i + 1 in self.match)
                ops += [f"wait {start} carry {self.copy_of[i]}"] if i in self.copy_of else []
            ops.append(f"extract {h} {lo} {nf} {start} {tail} " + " ".join(map(str, lane)))
            ops.append(f"record {tail} ext {j}")
            self.ext.add(j)
            self.frames[j] = mine
            self.copy_of.pop(j, None)
            if not match:
                continue
            if sm != tail:
                ops.append(f"wait {sm} ext {j}")
            if j:
                ops.append(f"wait {sm} ext {j - 1}")
            q0 = max(lo, 1)
            if lo + nf > q0:
                ops.append(f"match {h} {sm} {q0} {lo + nf - q0}")
            if j == 0:
                if cont:
                    ops += [f"wait {sm} carry {self.slot}", f"match_carry {h} {sm} {self.slot}", f"record {sm} m0 {self.slot}"]
                    self.m0.add(self.slot)
                else:
                    ops.append(f"clear_row0 {sm}")
            ops.append(f"record {sm} match {j}")
            self.match.add(j)
        # the last sub-batch's matcher stream copies the last frame into the other slot, behind the slot's last reader and writer
        _, tail, cs = where(nsub - 1)
        into = self.slot ^ 1
        if cs != tail:
            ops.append(f"wait {cs} ext {nsub - 1}")
        if into in self.m0:
            ops.append(f"wait {cs} m0 {into}")
            self.m0.discard(into)
        if into in self.written:
            ops.append(f"wait {cs} carry {into}")
        ops += [f"carry_copy {cs} {into} {nframes - 1}", f"record {cs} carry {into}"]
        self.written.add(into)
        self.slot, self.predecessor = into, True
        self.copy_of[nsub - 1] = into
        ops += [f"record {s} end {i}" for i, s in enumerate(carrying)]
        if lanes:
            self.lane_rot = (first + nsub) % sets
        else:
            self.rot = (first + nsub) % sets
        return ops

    def reset_sequence(self):
        self.predecessor = False


@pytest.mark.parametrize("cfg,name", GRID)
def test_the_log_is_the_rule(programs, cfg, name):
    seq = SEQUENCES[name]
    got = _per_call(_log(programs, [_line(cfg, c) for c in seq]))
    twin = Twin()
    assert len(got) == len(seq)
    for c, (ops, status) in zip(seq, got):
        if c == "reset_sequence":
            twin.reset_sequence()
            assert status is None
        else:
            assert status == 0
            assert ops == twin.call(cfg, **c), (cfg, name, c)


def test_the_scripts_reach_both_cuts_and_every_rule(programs):
    """what the scripts are there for does happen in them"""
    for cfg in CHAINS + LANES:
        log = _log(programs, [_line(cfg, c) for name in SEQUENCES for c in SEQUENCES[name]])
        staged = [ln.split()[4:] for ln in log if ln.startswith("extract") and ln.split()[6] != "-1"]
        assert bool(staged) == (cfg in LANES)
        assert all(s[:5] == ["0", "2", "0", "1", "2"] for s in staged)   # from kernel stream 0 to 2, FAST on 1
        for what in ("match_carry", "clear_row0", "wait", " m0 ", " carry "):
            assert any(what in ln for ln in log), (cfg, what)


# ---- (b) hazards -------------------------------------------------------------------------------------
def _hazards(seq, per_call):
    """unordered conflicting pairs of a script's log, as text"""
    nodes = []     # (stream, text)
    edges = []     # (from, to)
    last_on, last_record, ended = {}, {}, set()
    accesses = []  # (first node, last node, object, writes, text)

    def node(stream, text):
        nodes.append((stream, text))
        k = len(nodes) - 1
        if stream in last_on:
            edges.append((last_on[stream], k))
        last_on[stream] = k
        return k

    for c, (ops, status) in zip(seq, per_call):
        if c == "reset_sequence":
            continue
        base = c["base"]
        for op in ops:
            w = op.split()
            a = [int(x) for x in w[1:] if x.lstrip("-").isdigit()]
            if w[0] == "record":
                last_record[(w[2], w[3])] = node(int(w[1]), op)
                if w[2] == "end":
                    ended.add(w[3])
            elif w[0] == "wait":
                assert (w[2], w[3]) in last_record, f"wait for an event never recorded: {op}"
                edges.append((last_record[(w[2], w[3])], node(int(w[1]), op)))
            elif w[0] == "extract":
                _, lo, nf, start, tail = a[:5]
                b = node(start, op + " (begin)")
                e = b if tail == start else node(tail, op + " (end)")
                if e != b:
                    edges.append((b, e))
                accesses += [(b, e, ("frame", base + f), True, op) for f in range(lo, lo + nf)]
            elif w[0] == "match":
                _, s, q0, np_ = a
                k = node(s, op)
                accesses += [(k, k, ("frame", base + f), False, op) for f in range(q0 - 1, q0 + np_)]
                accesses += [(k, k, ("row", base + f), True, op) for f in range(q0, q0 + np_)]
            elif w[0] == "match_carry":
                k = node(a[1], op)
                accesses += [(k, k, ("frame", base), False, op), (k, k, ("slot", a[2]), False, op), (k, k, ("row", base), True, op)]
            elif w[0] == "clear_row0":
                k = node(a[0], op)
                accesses.append((k, k, ("row", base), True, op))
            elif w[0] == "carry_copy":
                k = node(a[0], op)
                accesses += [(k, k, ("frame", base + a[2]), False, op), (k, k, ("slot", a[1]), True, op)]
            else:
                raise AssertionError(op)
        if status == 0 and not c["flags"] & NO_JOIN:   # orbfe_pipeline_join on the caller's stream
            for i in sorted(ended):
                edges.append((last_record[("end", i)], node(-1, f"join end {i}")))
    # transitive closure: nodes are in log order and every edge points forward
    before = [0] * len(nodes)   # bit i of before[k]: node i happens before node k
    into = {}
    for u, v in edges:
        assert u < v
        into.setdefault(v, []).append(u)
    for k in range(len(nodes)):
        for u in into.get(k, ()):
            before[k] |= before[u] | (1 << u)
    bad = []
    by_object = {}
    for acc in accesses:
        by_object.setdefault(acc[2], []).append(acc)
    for obj, accs in by_object.items():
        for x in range(len(accs)):
            for y in range(x + 1, len(accs)):
                (b1, e1, _, w1, t1), (b2, e2, _, w2, t2) = accs[x], accs[y]
                if not (w1 or w2) or (b1, e1) == (b2, e2):
                    continue
                if not before[b2] >> e1 & 1:   # (log order: the first of the two can only come first)
                    bad.append(f"{obj}: [{t1}] and [{t2}]")
    return bad


@pytest.mark.parametrize("cfg,name", GRID)
def test_no_hazard_is_unordered(programs, cfg, name):
    seq = SEQUENCES[name]
    bad = _hazards(seq, _per_call(_run(programs[0], [_line(cfg, c) for c in seq])))
    assert not bad, "\n".join(bad[:20])


def test_the_hazard_check_sees_a_missing_edge(programs):
    """the check itself: without the wait of a sub-batch for the previous call's matcher of the same slices there is a hazard"""
    cfg, seq = CHAINS[1], SEQUENCES["three CONTINUE calls into the same blocks"]
    per_call = _per_call(_run(programs[0], [_line(cfg, c) for c in seq]))
    assert not _hazards(seq, per_call)
    cut = [([op for op in ops if not (op.startswith("wait") and " match " in op)], st) for ops, st in per_call]
    assert cut != per_call and _hazards(seq, cut)


# ---- (c) the error path --------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [CHAINS[1], LANES[-1]])
def test_a_failing_sink_stops_the_walk_and_the_sequence_restarts(programs, cfg):
    first, second, third = _calls((7, 0, 1, N), (7, 0, 1, C), (7, 0, 1, C))
    whole = _per_call(_run(programs[1], [_line(cfg, first), _line(cfg, second), _line(cfg, third)]))
    ops = whole[1][0]
    assert any(op.startswith("match_carry") for op in ops) and any(op.startswith("match_carry") for op in whole[2][0])
    for k in range(1, len(ops) + 1):
        got = _per_call(_run(programs[1], [_line(cfg, first), _line(cfg, second, fail_at=k), _line(cfg, third)]))
        assert got[0] == whole[0]
        assert got[1] == (ops[:k - 1], -4), k        # nothing behind the failed sink call
        after, status = got[2]
        assert status == 0
        assert sum(op.startswith("clear_row0") for op in after) == 1 and not any(op.startswith("match_carry") for op in after), k
        assert not any(" m0 " in op for op in after), k   # no reader of a carry slot is waited for or recorded
    beyond = _per_call(_run(programs[1], [_line(cfg, first), _line(cfg, second, fail_at=len(ops) + 1), _line(cfg, third)]))
    assert beyond == whole

"""Lane placement 2 of the sequence pipeline (csrc/orbfe_pipe_plan.h, csrc/orbfe_pipe_graph.h) without a GPU: FAST on two streams -- the
launches of even sub-batches on kernel stream 1, of odd ones on the side stream --, the blur behind the pyramid on kernel stream 0, the
matcher behind the descriptor on kernel stream 2.  The program and the hazard check are the ones of tests/test_pipe_graph.py.

(a) No hazard is unordered, over pipes x queues x buffer sets (2, 3, 4, 5, 8) x call lists (plain calls, CONTINUE joined, CONTINUE |
    NO_JOIN, output blocks re-used and shifted back): frames, match rows and carry slots by test_pipe_graph._hazards, which gives the
    FAST and blur streams no edge (the conservative choice); buffer sets in a graph that has the stage streams -- an extraction is
    pyramid -> (FAST, blur) -> tail, every stream a FIFO, and a handle's call begins behind the handle's previous one (run_batch makes
    the pyramid's stream wait for ev_last) -- in which two uses of a set must not overlap anywhere, FAST stream included.
(b) FAST of sub-batch j is on the stream of j's parity, whichever buffer set it uses; with an odd number of sets a set alternates.
(c) No stream beyond the four appears in a log.
(d) The rule refuses lanes where it did: such calls run in chains whatever the placement says.
(e) A sink that fails at its k-th call stops the walk there; the sequence restarts behind it."""
import pytest

from test_pipe_graph import C, CONTINUE, F, N, NO_JOIN, _calls, _hazards, _line, _per_call, _run, programs  # noqa: F401

PLACE = 2
K0, K1, K2, SIDE = 0, 1, 2, 3   # pool indices of the device entry point's plan on 4 queues
SETS = (2, 3, 4, 5, 8)
CONFIGS = [(P, 4, s, PLACE) for P in (5, 12) for s in SETS]
SEQUENCES = {
    "plain calls": _calls((7, 0, 1, 0), (7, 0, 1, 0), (5, 0, 0, 0), (7, 0, 1, 0)),
    "CONTINUE, joined": _calls((7, 0, 1, 0), (7, 0, 1, CONTINUE), (7, 0, 1, CONTINUE), (7, 0, 1, CONTINUE)),
    "CONTINUE | NO_JOIN": _calls((7, 0, 1, N), (7, 0, 1, C), (7, 0, 1, C), (7, 0, 1, C)),
    "blocks re-used and shifted back": _calls((7, 0, 1, N), (7, F, 1, C), (7, 0, 1, C), (7, 1, 1, C), (7, 0, 1, C), (3, F, 1, C), (7, 1, 1, C)),
    "7, 1, 3 and 7 frames": _calls((7, 0, 1, N), (1, 0, 1, C), (3, 0, 1, C), (7, 0, 1, C), (1, 0, 1, C), (1, 0, 1, C)),
}
GRID = [(cfg, name) for cfg in CONFIGS for name in SEQUENCES]


def _extracts(ops):
    """(handle, lo, nf, start, tail, lane[0..3]) of every extraction of a call"""
    return [tuple(int(x) for x in op.split()[1:]) for op in ops if op.startswith("extract ")]


def _set_hazards(seq, per_call, handle_events=True):
    """pairs of extractions on the same buffer set that the graph with the stage streams leaves unordered"""
    nodes, edges, last_on, last_record = [], [], {}, {}
    uses = {}   # handle -> [(begin, end, text)]

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
        for op in ops:
            w = op.split()
            if w[0] == "record":
                last_record[(w[2], w[3])] = node(int(w[1]), op)
            elif w[0] == "wait":
                edges.append((last_record[(w[2], w[3])], node(int(w[1]), op)))
            elif w[0] == "extract":
                h, _, _, start, tail, l0, l1, l2, l3 = (int(x) for x in w[1:])
                if l0 < 0:   # a chain call: one stream
                    b = e = node(start, op)
                else:
                    assert (start, tail) == (l0, l2)
                    b = node(l0, op + " (pyramid)")
                    blur = node(l3, op + " (blur)")   # (behind the pyramid in every placement: a fork, or the same stream)
                    fast = node(l1, op + " (FAST)")
                    e = node(l2, op + " (quadtree, descriptor)")
                    edges.extend([(b, blur), (b, fast), (fast, e), (blur, e)])
                if h in uses and handle_events:   # the handle's own event: the call begins behind the handle's previous one
                    edges.append((uses[h][-1][1], b))
                uses.setdefault(h, []).append((b, e, op))
            else:
                node(int(w[2]) if w[0] in ("match", "match_carry") else int(w[1]), op)
    before = [0] * len(nodes)
    into = {}
    for u, v in edges:
        assert u < v
        into.setdefault(v, []).append(u)
    for k in range(len(nodes)):
        for u in into.get(k, ()):
            before[k] |= before[u] | (1 << u)
    bad = []
    for h, us in uses.items():
        for x in range(len(us)):
            for y in range(x + 1, len(us)):
                if not before[us[y][0]] >> us[x][1] & 1:
                    bad.append(f"set {h}: [{us[x][2]}] and [{us[y][2]}]")
    return bad


@pytest.mark.parametrize("cfg,name", GRID)
def test_no_hazard_is_unordered_and_fast_alternates(programs, cfg, name):  # noqa: F811
    seq = SEQUENCES[name]
    per_call = _per_call(_run(programs[0], [_line(cfg, c) for c in seq]))
    assert len(per_call) == len(seq) and all(status == 0 for _, status in per_call)
    bad = _hazards(seq, per_call) + _set_hazards(seq, per_call)
    assert not bad, "\n".join(bad[:20])
    sets = min(cfg[0], cfg[2])
    lane_calls = 0
    for c, (ops, _) in zip(seq, per_call):
        ext = _extracts(ops)
        nsub = -(-c["nframes"] // F)
        assert len(ext) == nsub
        for j, (h, lo, nf, start, tail, l0, l1, l2, l3) in enumerate(ext):
            assert lo == j * F
            if nsub < 2:   # one sub-batch: a chain, as in every placement
                assert (l0, l1, l2, l3) == (-1, -1, -1, -1) and start == tail
                continue
            # (b) the FAST stream is a function of the sub-batch index alone
            assert (start, tail, l0, l2, l3) == (K0, K2, K0, K2, K0), ops
            assert l1 == (SIDE if j & 1 else K1), (j, ops)
            assert 0 <= h < sets
        lane_calls += nsub >= 2
        # the matcher and the carry copy stay behind the descriptor
        assert all(int(op.split()[2]) == K2 for op in ops if op.startswith(("match ", "match_carry ")) and nsub >= 2)
        # (c) the four streams and the caller's, nothing else
        for op in ops:
            w = op.split()
            if w[0] in ("wait", "record", "clear_row0", "carry_copy"):
                assert int(w[1]) in (-1, K0, K1, K2, SIDE), op
        if nsub >= 2:   # every one of the four ends the call with an event of its own
            assert [op for op in ops if " end " in op] == [f"record {s} end {i}" for i, s in enumerate((K0, K1, K2, SIDE))]
    assert lane_calls >= 3


def test_an_odd_number_of_sets_alternates_a_set_between_the_fast_streams(programs):  # noqa: F811
    cfg = (5, 4, 3, PLACE)
    seq = SEQUENCES["CONTINUE | NO_JOIN"]
    per_call = _per_call(_run(programs[0], [_line(cfg, c) for c in seq]))
    streams_of = {}
    for ops, _ in per_call:
        for h, *_, l1, _l2, _l3 in _extracts(ops):
            streams_of.setdefault(h, set()).add(l1)
    assert streams_of == {0: {K1, SIDE}, 1: {K1, SIDE}, 2: {K1, SIDE}}


def test_the_set_check_sees_a_missing_edge(programs):  # noqa: F811
    """the check itself: without the handles' own events two uses of a set inside one call are unordered (the walk orders frames, not sets)"""
    cfg, seq = (5, 4, 3, PLACE), SEQUENCES["CONTINUE | NO_JOIN"]
    per_call = _per_call(_run(programs[0], [_line(cfg, c) for c in seq]))
    assert not _set_hazards(seq, per_call)
    assert _set_hazards(seq, per_call, handle_events=False)


@pytest.mark.parametrize("pipes,queues", [(3, 4), (5, 16), (5, 2), (12, 1), (3, 16)])
def test_the_rule_refuses_lanes_where_it_did(programs, pipes, queues):  # noqa: F811
    seq = SEQUENCES["CONTINUE | NO_JOIN"]
    for place in (1, PLACE):
        cfg = (pipes, queues, 4, place)
        per_call = _per_call(_run(programs[0], [_line(cfg, c) for c in seq]))
        for ops, status in per_call:
            assert status == 0
            assert all(e[5:] == (-1, -1, -1, -1) and e[3] == e[4] for e in _extracts(ops))
        assert not _hazards(seq, per_call)
    # ... and placement 2 changes nothing in a chain call
    logs = [_run(programs[0], [_line((pipes, queues, 4, place), c) for c in seq]) for place in (1, PLACE)]
    assert logs[0] == logs[1]


def test_a_failing_sink_stops_the_walk_and_the_sequence_restarts(programs):  # noqa: F811
    cfg = (5, 4, 3, PLACE)
    first, second, third = _calls((7, 0, 1, N), (7, 0, 1, C), (7, 0, 1, C))
    whole = _per_call(_run(programs[1], [_line(cfg, first), _line(cfg, second), _line(cfg, third)]))
    ops = whole[1][0]
    assert any(op.startswith("match_carry") for op in ops)
    for k in range(1, len(ops) + 1):
        got = _per_call(_run(programs[1], [_line(cfg, first), _line(cfg, second, fail_at=k), _line(cfg, third)]))
        assert got[0] == whole[0]
        assert got[1] == (ops[:k - 1], -4), k
        after, status = got[2]
        assert status == 0
        assert sum(op.startswith("clear_row0") for op in after) == 1 and not any(op.startswith("match_carry") for op in after), k
        assert [e[6] for e in _extracts(after)] == [K1, SIDE, K1, SIDE], k   # the parity rule holds behind a failure as well

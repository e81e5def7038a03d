"""The matrix-core brute-force matcher k_match_bf<tiles> (csrc/orbfe_match.hip) with 1, 2 and 4 query tiles of 32 per wave: a workgroup
takes 128, 256 or 512 queries, everything else is the same code, and every result is the oracle's, bit for bit.

Harness and planted inputs are those of tests/test_gpu_matcher_edges.py (host, device, frames and blocks forms against
oracle.match_bf); what is new here is the handle's tile count (orbfe_internal_matcher_set_bf_tiles) and the sizes at which it matters:
query counts at the edges of 32 (a tile) and of 128 x tiles (a workgroup), train counts at the edges of the 32-row train tile."""
import numpy as np
import pytest

import hamming_cases as H
from test_gpu_matcher_edges import _case, _device, _extreme_cases, _position_case, check_bf

pytestmark = pytest.mark.gpu

TILES = (1, 2, 4)
NQ = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513)
NT = (1, 32, 33, 1000)


@pytest.fixture(scope="module")
def mts():
    from orb_slam2_ssd_semantic_amd import ORBmatcher, _ffi
    out = {}
    for k in TILES:
        out[k] = ORBmatcher(0.6, True)
        out[k].set_bf_tiles(k)
    with pytest.raises(_ffi.OrbfeError):   # 3 tiles compile, and are not instantiated
        out[4].set_bf_tiles(3)
    yield out
    for m in out.values():
        m.close()


@pytest.fixture(scope="module")
def pool():
    """513 queries and 1000 train rows: row j sits 2 + j % 45 bits from query 7 j mod 513, so that every query count has matches,
    rejections by the ratio and by the threshold in every train count but 1"""
    rng = np.random.default_rng(77)
    q = H.random_rows(rng, max(NQ))
    t = np.stack([H.at_distance(rng, q[(7 * j) % len(q)], 2 + j % 45) for j in range(max(NT))])
    return q, t, rng.uniform(0, 360, len(q)).astype(np.float32), rng.uniform(0, 360, len(t)).astype(np.float32)


@pytest.mark.parametrize("nt", NT)
def test_query_and_train_counts_at_the_tile_edges(oracle, mts, pool, nt):
    q, t, qa, ta = pool
    cases = [_case(q[:nq], t[:nt], None, qa[:nq], ta[:nt]) for nq in NQ]
    refs = check_bf(oracle, mts, cases, 0.8, 40, True, forms=("device", "frames", "blocks"))
    if nt == 1000:
        assert sum(r[3] for r in refs) > 300 and any((r[1] > 40).any() for r in refs)
    # the three tile counts agree with each other byte for byte, best and second distances included
    for c in cases:
        got = [_device(mts[k], c, 0.8, 40, True) for k in TILES]
        for g in got[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(g[:3], got[0][:3])) and g[3] == got[0][3]


def test_duplicate_train_rows_across_a_tile_edge_the_lowest_index_wins(oracle, mts):
    """the same descriptor in the last row of one 32-row train tile and the first row of the next, for queries in every query tile of
    every tile count's workgroup: best == second, and with nnratio > 1 the match is the earlier row"""
    rng = np.random.default_rng(12)
    nq, nt = 300, 32 * 9
    q, t = H.random_rows(rng, nq), H.random_rows(rng, nt)
    where = {0: 1, 31: 2, 33: 3, 69: 4, 127: 5, 129: 6, 255: 7, 256: 8, 299: 4}   # query -> the tile edge its twins straddle
    for qi, e in where.items():
        if qi != 299:
            t[32 * e - 1] = t[32 * e] = H.at_distance(rng, q[qi], 4 + e)
    q[299] = q[69]   # (a second query on the same twins)
    refs = check_bf(oracle, mts, [_case(q, t, rng)], 1.5, 100, False)
    m, best, second, _ = refs[0]
    for qi, e in where.items():
        assert (m[qi], best[qi], second[qi]) == (32 * e - 1, 4 + e, 4 + e), qi
    check_bf(oracle, mts, [_case(q, t, rng)], 0.9, 100, False)   # ... and a tie fails every ratio <= 1
    # the planted single-query layouts of the edge tests: halves of a tile, three-way ties, the last partial tile
    cases = []
    for nt1, plants in ((64, [(31, 6), (32, 6)]), (64, [(5, 6), (33, 6)]), (129, [(128, 3), (96, 3)]), (33, [(32, 2), (0, 2)]),
                        (40, [(12, 9), (16, 9), (20, 9)])):
        q1, t1 = H.planted_bf(rng, 1, nt1, [(0, r, d) for r, d in plants])
        cases.append(_case(q1, t1, rng))
    refs = check_bf(oracle, mts, cases, 1.5, 100, False)
    assert [int(r[0][0]) for r in refs] == [31, 5, 96, 0, 12]


@pytest.mark.parametrize("ratio", [0.6, 0.8])
def test_ratio_edges_at_every_query_position(oracle, mts, ratio):
    rng = np.random.default_rng(int(ratio * 10))
    built = [_position_case(rng, nq, ratio) for nq in (129, 257, 513)]
    refs = check_bf(oracle, mts, [b[0] for b in built], ratio, 100, False)
    for (c, plants, perm), ref in zip(built, refs):
        for qi, r, d in plants[::2]:
            assert ref[1][qi] == d
    # just inside the edge: accepted
    for r, (b, s) in ((0.6, (3, 6)), (0.8, (4, 6))):
        q, t = H.planted_bf(rng, 1, 50, [(0, 17, b), (0, 40, s)])
        assert check_bf(oracle, mts, [_case(q, t, rng)], r, 100, False)[0][0][0] == 17


def test_th_high_edges_and_distance_extremes(oracle, mts):
    rng = np.random.default_rng(4)
    q, t = H.planted_bf(rng, 3, 50, [(0, 10, 100), (1, 11, 101), (2, 12, 99)])   # TH_HIGH = 100: at, above, below
    ref = check_bf(oracle, mts, [_case(q, t, rng)], 1.5, 100, False)[0]
    assert ref[1].tolist() == [100, 101, 99] and ref[0].tolist() == [10, -1, 12]
    for th, ratio in ((50, 0.9), (0, 0.9), (256, 1.5)):   # rows at 0 and at 256, best == th and th + 1, identical rows
        check_bf(oracle, mts, _extreme_cases(np.random.default_rng(3)), ratio, th, False)


@pytest.mark.parametrize("cap", [300, 513])
def test_batched_forms_with_counts_zero_and_cap(oracle, mts, pool, cap):
    """the frames form and the two-block form (query and train frames in different blocks: what the pipeline's carry match uses) with
    per-frame counts 0, 1, cap and in between; slots behind a frame's count are -1 in every workgroup of every tile count"""
    q, t, qa, ta = pool
    sizes = [(0, 40), (cap, cap), (129, 0), (1, 1), (cap, 33), (257, cap), (0, 0)]
    cases = [_case(q[:a], t[:b], None, qa[:a], ta[:b]) for a, b in sizes]
    refs = check_bf(oracle, mts, cases, 0.8, 40, True, cap=cap, forms=("frames", "blocks"))
    assert refs[1][3] > 50

"""The operand encoding and the ranking key of the matrix-core brute-force matcher k_match_bf (csrc/orbfe_match.hip): every descriptor
bit is one FP4 nibble on both sides of the scaled MFMA, and the fp32 bit pattern of an accumulator is the (distance, row) key.

Inputs are built so that the answer is known before anything runs, and every case goes through 1, 2 and 4 query tiles per wave
against oracle.match_bf with `best` and `second` read back (orbfe_match_bf_device), and through the blocks form the pipeline's lane
calls use:
  * single flipped bits, on the query side and on the train side, and their complements: a dropped, duplicated or mis-signed
    nibble, or a bit -> k assignment that differs between the two operands, changes a distance of 1 (or 255);
  * distances 0, 128 and 256 (the ends and the middle of the key range) on the first and last row of a full 32-row train tile
    and of the masked last tile, alone among rows at 256 or at 200, and twice at the same distance in one or two tiles;
  * 33 train tiles with every best row repeated 992 rows later: the forced field and the index latch over the whole run."""
import numpy as np
import pytest

import hamming_cases as H
from test_gpu_matcher_edges import _case, check_bf

pytestmark = pytest.mark.gpu

TILES = (1, 2, 4)
FORMS = ("device", "blocks")


@pytest.fixture(scope="module")
def mts():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    out = {}
    for k in TILES:
        out[k] = ORBmatcher(0.6, True)
        out[k].set_bf_tiles(k)
    yield out
    for m in out.values():
        m.close()


def _one_bit_rows(base):
    return np.stack([H.flip(base, [i]) for i in range(256)])


def test_every_bit_counts_once_on_the_query_side(oracle, mts):
    """query i = train row 0 with bit i inverted; train rows 1..32 (the tile edge is crossed) sit 40 + j bits from row 0, so 39 + j
    at the least from any query"""
    rng = np.random.default_rng(256)
    base = H.random_rows(rng, 1)[0]
    t = np.stack([base] + [H.at_distance(rng, base, 40 + j) for j in range(1, 33)])
    q = _one_bit_rows(base)
    m, best, second, n = check_bf(oracle, mts, [_case(q, t, rng)], 0.9, 100, False, forms=FORMS)[0]
    assert (best == 1).all() and (m == 0).all() and n == 256
    assert (second >= 40).all() and (second <= 42).all()
    # the complement of every query: 255 from row 0; the only rows that do not beat that for some query are copies of row 0
    t = np.stack([base] * 33)
    m, best, second, n = check_bf(oracle, mts, [_case(~q, t, rng)], 1.5, 256, False, forms=FORMS)[0]
    assert (best == 255).all() and (second == 255).all() and (m == 0).all()


def test_every_bit_counts_once_on_the_train_side(oracle, mts):
    """one query, train row i = the query with bit i inverted: 256 rows at distance 1, the lowest index wins"""
    rng = np.random.default_rng(257)
    base = H.random_rows(rng, 1)[0]
    t = _one_bit_rows(base)
    q = base[None]
    refs = check_bf(oracle, mts, [_case(q, t, rng), _case(q, ~t, rng)], 1.5, 256, False, forms=FORMS)
    assert [(int(r[0][0]), int(r[1][0]), int(r[2][0])) for r in refs] == [(0, 1, 1), (0, 255, 255)]
    # ... and one row at a time among rows at 256: a bit that counted for nothing or twice would show as 0 or 2
    cases = []
    for i in range(0, 256, 5):
        rows = np.stack([~base] * 33)
        rows[i % 33] = t[i]
        cases.append(_case(q, rows, rng))
    refs = check_bf(oracle, mts, cases, 1.5, 256, False, forms=FORMS)
    assert [(int(r[0][0]), int(r[1][0]), int(r[2][0])) for r in refs] == [(i % 33, 1, 256) for i in range(0, 256, 5)]


def _tile_end_rows(nt):
    """first and last row of the full tile, first and last valid row of the masked last tile"""
    return sorted({0, 31} | ({32, nt - 1} if nt > 32 else set()))


@pytest.mark.parametrize("nt", [32, 33, 63])
def test_key_range_ends_at_the_ends_of_a_tile(oracle, mts, nt):
    rng = np.random.default_rng(nt)
    q = H.random_rows(rng, 1)
    cases, want = [], []
    for fill in (256, 200):
        filler = np.stack([H.at_distance(rng, q[0], fill) for _ in range(nt)])
        for row in _tile_end_rows(nt):
            for d in (0, 128, 256):
                t = filler.copy()
                t[row] = H.at_distance(rng, q[0], d)
                cases.append(_case(q, t, rng))
                if d < fill:
                    want.append((row, d, fill))
                elif fill == 256:          # every row at 256: nothing ever becomes the best
                    want.append((-1, 256, 256))
                else:                      # the row at 256 loses to the first filler row that is not it
                    want.append((1 if row == 0 else 0, 200, 200))
    # the same distance twice, in one tile or in two: the older row wins, second == best
    rows = _tile_end_rows(nt)
    for a in rows:
        for b in rows:
            if a < b:
                for d in (0, 1, 128):
                    t = np.stack([~q[0]] * nt)
                    t[a] = t[b] = H.at_distance(rng, q[0], d)
                    cases.append(_case(q, t, rng))
                    want.append((a if d else -1, d, d))   # 0 < nnratio * 0 fails: a tie at distance 0 is no match
    refs = check_bf(oracle, mts, cases, 1.5, 256, False, forms=FORMS)
    assert [(int(r[0][0]), int(r[1][0]), int(r[2][0])) for r in refs] == want


def test_duplicate_of_the_best_row_33_tiles_later(oracle, mts):
    """nt = 1025 (32 full tiles and one row), nq = 129 (a partial second workgroup of the 1-tile form): query i sits 3 + i % 11 bits
    from train row i % 33, and rows 992..1024 repeat rows 0..32; everything else is random (>= 60 away in practice, checked)"""
    rng = np.random.default_rng(1025)
    nq, nt = 129, 1025
    t = H.random_rows(rng, nt)
    t[992:] = t[:33]
    q = np.stack([H.at_distance(rng, t[i % 33], 3 + i % 11) for i in range(nq)])
    D = H.distances(q, t)
    D[np.arange(nq), np.arange(nq) % 33] = 999
    D[np.arange(nq), np.arange(nq) % 33 + 992] = 999
    assert D.min() >= 60
    m, best, second, n = check_bf(oracle, mts, [_case(q, t, rng)], 1.5, 100, False, forms=FORMS)[0]
    assert np.array_equal(m, np.arange(nq) % 33) and n == nq
    assert np.array_equal(best, 3 + np.arange(nq) % 11) and np.array_equal(second, best)

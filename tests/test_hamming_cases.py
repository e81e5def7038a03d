"""The planted-distance builders of tests/hamming_cases.py, and the CPU oracle's matchers on what they build.  CPU only.

Every builder is checked against np.unpackbits counts; the oracle's match_bf, search_by_bow and three_maxima are checked
against the plain numpy restatements in hamming_cases on the planted edge cases that tests/test_gpu_matcher_edges.py
feeds to the HIP kernels, and against the answers the plantings were made for."""
import numpy as np
import pytest

import hamming_cases as H
import test_gpu_matcher_edges as E


def unpack_dist(a, b):
    return int(np.unpackbits(np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)).sum())


def test_distances_equal_unpackbits():
    rng = np.random.default_rng(0)
    a, b = H.random_rows(rng, 300), H.random_rows(rng, 41)
    b[3] = a[7]
    b[4] = np.bitwise_not(a[7])
    D = H.distances(a, b)
    for i, j in [(7, 3), (7, 4), (0, 0), (299, 40)] + [tuple(x) for x in rng.integers(0, [300, 41], (200, 2))]:
        assert D[i, j] == unpack_dist(a[i], b[j])
    assert D[7, 3] == 0 and D[7, 4] == 256 and H.distances(a[:0], b).shape == (0, 41)


def test_planted_distances_are_exact():
    rng = np.random.default_rng(1)
    for d in (0, 1, 3, 50, 128, 200, 255, 256):
        r = H.random_rows(rng, 1)[0]
        assert unpack_dist(r, H.at_distance(rng, r, d)) == d
        assert unpack_dist(r, H.at_distance(rng, r, min(d, 128), 128, 256)) == min(d, 128)
    plants = [(0, 5, 7), (0, 9, 7), (3, 0, 0), (3, 99, 256), (7, 50, 31)]
    q, t = H.planted_bf(rng, 8, 100, plants)
    for qi, row, d in plants:
        assert unpack_dist(q[qi], t[row]) == d
    base = H.random_rows(rng, 1)[0]
    near, far = H.near_rows(rng, base, 40, 16), H.far_rows(rng, base, 60, 4)
    D = H.distances(near, far)
    assert D.min() >= 200 and all(unpack_dist(f, np.bitwise_not(base)) == 4 for f in far)
    assert all(unpack_dist(x, base) <= 16 for x in near)


@pytest.mark.parametrize("seed", range(4))
def test_best2_equals_the_sequential_idiom(seed):
    rng = np.random.default_rng(seed)
    q, t = H.random_rows(rng, 30), H.random_rows(rng, 70)
    t[rng.integers(0, 70, 25)] = t[rng.integers(0, 70, 25)]
    t[:5] = np.bitwise_not(q[:5])
    D = H.distances(q, t)
    D[10] = 256                          # no row below 256: no best index
    D[11, :] = 40                        # all tied
    b1, idx, b2 = H.best2_np(D)
    for i in range(len(q)):
        assert (b1[i], idx[i], b2[i]) == H.best2(D[i]), i
    assert (b1[10], idx[10], b2[10]) == (256, -1, 256) and (b1[11], idx[11], b2[11]) == (40, 0, 40)


def test_float_boundaries():
    """the binary32 rounding each edge list is built on, and that a double computation would differ there"""
    for ratio, pairs in H.RATIO_EDGES.items():
        for b, s in pairs:
            assert not H.ratio_pass(b, s, ratio) and b < float(np.float32(ratio)) * s
    for m1, m2 in H.MAXIMA_EDGES:
        counts = np.zeros(13, np.int32)
        counts[[2, 6]] = m1, m2
        assert H.three_maxima(counts) == (2, 6, -1) and m2 < float(np.float32(0.1)) * m1
    for a1, a2, rb, rint_bin in H.HALF_BIN_ANGLES:
        f = np.float32
        rot = f(f(a1) - f(a2))
        rot = f(rot + f(360)) if rot < 0 else rot
        x = f(rot * (f(1) / f(30)))
        assert x == np.floor(x) + f(0.5)                       # exactly on a half bin
        assert H.rot_bin(a1, a2) == rb and int(np.rint(x)) == rint_bin != rb


def test_oracle_rot_bin_and_three_maxima(oracle):
    for a1, a2, rb, _ in H.HALF_BIN_ANGLES:
        assert oracle.rot_bin(a1, a2) == rb
    rng = np.random.default_rng(2)
    for a1, a2 in rng.uniform(0, 360, (2000, 2)).astype(np.float32):
        assert oracle.rot_bin(a1, a2) == H.rot_bin(a1, a2)
    vectors = [np.zeros(30, np.int32)]
    for m1, m2 in H.MAXIMA_EDGES:
        for at in ((0, 1, 2), (12, 0, 5), (3, 11, 7)):
            for m3 in (0, m2 - 1, m2, m2 + 1):
                c = np.zeros(30, np.int32)
                c[at[0]], c[at[1]], c[at[2]] = m1, m2 if m3 <= m2 else m3, min(m3, m2) if m3 <= m2 else m2
                vectors.append(c)
    for eq in ((7, 7, 7, 7), (5, 9, 9, 9, 9), (3, 3)):   # equal counts: the earliest bins win
        c = np.zeros(30, np.int32)
        c[[1, 4, 8, 12, 11][:len(eq)]] = eq
        vectors.append(c)
    for c in vectors:
        assert oracle.three_maxima(c) == H.three_maxima(c), c.tolist()
    c = np.zeros(30, np.int32)
    c[[12, 1, 6, 3]] = 200, 150, 20, 19
    assert oracle.three_maxima(c) == (12, 1, 6)


def test_histogram_builder():
    rng = np.random.default_rng(3)
    for counts in ([5, 0, 0, 7, 1, 0, 0, 0, 0, 0, 0, 0, 9], [0] * 12 + [4], [30], [1] * 13):
        a1, a2, bins = H.angles_for_histogram(rng, counts)
        got = np.bincount([H.rot_bin(x, y) for x, y in zip(a1, a2)], minlength=13)
        assert got.tolist() == list(counts) + [0] * (13 - len(counts))
        assert (a1 < a2).any() or len(counts) < 13         # some differences wrap through +360
    for name, groups in E.ROTATION_CASES.items():
        qa, ta = E._rotation_groups(groups)
        hist = np.bincount([H.rot_bin(x, y) for x, y in zip(qa, ta)], minlength=13)
        for count, kind, v in groups:
            assert hist[v] >= count, name


def test_oracle_match_bf_on_planted_cases(oracle):
    """oracle.match_bf == the numpy restatement on the tie, extreme, position and rotation cases the GPU tests use"""
    rng = np.random.default_rng(4)
    sets = [E._tie_cases(np.random.default_rng(11)), E._extreme_cases(np.random.default_rng(3)),
            [E._position_case(rng, 513, 0.6)[0]], [E._rotation_bf_case(n) for n in E.ROTATION_CASES]]
    for cases in sets:
        for ratio, th, ori in ((1.5, 100, False), (0.6, 100, True), (0.8, 256, False), (1.5, 256, False), (1.0, 0, True)):
            for q, t, qa, ta in cases:
                ref = oracle.match_bf(q, t, qa, ta, ratio, th, ori)
                npy = H.match_bf(q, t, qa, ta, ratio, th, ori)
                for r, g in zip(ref[:3], npy[:3]):
                    assert np.array_equal(r, g)
                assert ref[3] == npy[3]


def test_planted_bf_answers(oracle):
    """the tie layouts give the earliest tied row, the extremes their planted distances, the rotation cases the kept
    counts the histograms were built for"""
    refs = [oracle.match_bf(*c, 1.5, 100, False) for c in E._tie_cases(np.random.default_rng(11))]
    assert [int(r[0][0]) for r in refs[:12]] == [4, 3, 12, 31, 5, 13, 127, 100, 0, 60, 96, 0]
    assert [int(r[2][0]) for r in refs[:12]] == [7, 7, 9, 6, 6, 6, 11, 11, 15, 9, 3, 2]
    assert (refs[-1][0][::3] >= 0).all()
    ext = [oracle.match_bf(*c, 1.5, 256, False) for c in E._extreme_cases(np.random.default_rng(3))]
    assert (ext[0][1][0], ext[0][2][0], ext[0][0][0]) == (256, 256, -1)
    assert (ext[4][1][0], ext[4][2][0], ext[4][0][0]) == (7, 256, 0) and ext[5][0][0] == 1
    kept = {n: oracle.match_bf(*E._rotation_bf_case(n), 0.6, 100, True)[3] for n in E.ROTATION_CASES}
    assert kept == E.ROTATION_KEPT, kept


def test_oracle_search_by_bow_on_planted_cases(oracle):
    rng = np.random.default_rng(5)
    pairs = E._chunk_tie_pairs(rng) + E._claim_pairs(rng) + E._th_ratio_pairs(rng, 0.6) + E._invalid_pairs(rng)
    pairs += [E._many_nodes_pair(rng, 150, E.ROTATION_CASES["half135"])]
    for ratio, strict, ori in ((0.6, False, False), (0.8, True, True), (1.5, False, True), (1.5, True, False)):
        for kf, f in pairs:
            vF = f[1] if strict else None
            ref = oracle.search_by_bow(kf[0], kf[1], kf[2], kf[3], f[0], vF, f[2], f[3], ratio, 50, strict, ori)
            npy = H.search_by_bow(kf[0], kf[1], kf[2], kf[3], f[0], vF, f[2], f[3], ratio, 50, strict, ori)
            assert np.array_equal(ref[0], npy[0]) and ref[1] == npy[1]


def test_planted_search_by_bow_answers(oracle):
    """TH_LOW equality in both modes, the float ratio edges, claimed ties, chunk-edge ties with nnratio 1.5"""
    kf, f = E._th_ratio_pairs(np.random.default_rng(6), 0.6)[1]
    for strict, expect in ((False, [0, 1, -1]), (True, [0, -1, -1])):
        m, _ = oracle.search_by_bow(kf[0], None, kf[2], kf[3], f[0], None, f[2], f[3], 0.6, 50, strict, False)
        assert [int(m[i]) for i in range(3)] == expect
        # ratio edges (3, 5), (6, 10), (9, 15), (12, 20) fail in float; (3, 6) and (2, 4) pass
        assert [int(m[4 + 2 * k]) for k in range(6)] == [-1, -1, -1, -1, 7, 8]
    kf, f = E._claim_pairs(np.random.default_rng(1))[0]
    m, _ = oracle.search_by_bow(kf[0], None, kf[2], kf[3], f[0], None, f[2], f[3], 0.8, 50, False, False)
    assert (m[3], m[20], m[18], m[35], m[5], m[6]) == (0, 1, 2, 3, -1, -1)
    m, _ = oracle.search_by_bow(kf[0], None, kf[2], kf[3], f[0], None, f[2], f[3], 1.5, 50, False, False)
    assert m[5] == 4 and m[6] == -1                       # the earlier of the tied positions
    for kf, f in E._chunk_tie_pairs(np.random.default_rng(7))[:4]:
        m, n = oracle.search_by_bow(kf[0], None, kf[2], kf[3], f[0], None, f[2], f[3], 1.5, 50, False, False)
        assert n >= 6

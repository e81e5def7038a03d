"""Inputs for the BoW transform (k_bow_descend + k_bow_aggregate) and for ComputeDistinctiveDescriptors (k_distinctive) that
sit on the edges of those kernels: sort widths around every power of two up to the 8192 limit, word runs that cross
hundreds of per-thread chunks, weights whose sum depends on the order of addition, vocabulary trees that are not regular,
descents that tie, and observation counts around the 64-row passes of the distinctive kernel with medians PLANTED on
ties, cluster boundaries and the first bisection split.  numpy only (CPU); tests/test_bow_cases.py checks every builder,
tests/test_gpu_bow_edges.py feeds the cases to the HIP kernels.

Vocabulary builders return the dict orbfe_vocabulary_create takes (child_off, child_idx, node_desc, word_id, weight, L).
TRANSFORM_CASES and DISTINCTIVE_CASES are tables of named cases; `doc` says which line of the kernel a case is for."""
import numpy as np

from hamming_cases import POPC, at_distance, flip, random_rows
from orb_slam2_ssd_semantic_amd.synth import regular_vocabulary

WIDTHS = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192)
BOW_MAX_FEATURES = 8192
DD_MAX_OBS = 1024


# ------------------------------------------------------------------------------------------------ vocabularies
def tree(spec):
    """Nested lists -> (child_off, child_idx, level) with breadth-first ids (children after parents, siblings consecutive):
    a list is a node with those children, anything else a leaf.  `spec` is the root."""
    nodes, level, kids = [spec], [0], []
    i = 0
    while i < len(nodes):
        ch = nodes[i] if isinstance(nodes[i], list) else []
        kids.append(list(range(len(nodes), len(nodes) + len(ch))))
        nodes.extend(ch)
        level.extend([level[i] + 1] * len(ch))
        i += 1
    child_off = np.zeros(len(nodes) + 1, np.uint32)
    child_off[1:] = np.cumsum([len(k) for k in kids])
    child_idx = np.asarray([c for k in kids for c in k], np.uint32)
    return child_off, child_idx, np.asarray(level, np.int32)


def leaves_of(voc):
    return np.flatnonzero(voc["child_off"][1:] == voc["child_off"][:-1])


def levels_of(voc):
    co, ci = voc["child_off"], voc["child_idx"]
    lev = np.zeros(len(co) - 1, np.int32)
    for p in range(len(lev)):   # parents precede children
        lev[ci[co[p]:co[p + 1]]] = lev[p] + 1
    return lev


def flat(nleaf, weights=None, word_ids=None, seed=0):
    """Depth 1: the root and nleaf leaves (node i + 1 = leaf i).  weights / word_ids per leaf; by default random weights
    in [0.1, 9) and word i for leaf i."""
    rng = np.random.default_rng(1000 + seed)
    nodes = nleaf + 1
    child_off = np.concatenate([[0], np.full(nodes, nleaf)]).astype(np.uint32)
    child_idx = np.arange(1, nodes, dtype=np.uint32)
    node_desc = random_rows(rng, nodes)
    weight = np.zeros(nodes)
    weight[1:] = rng.uniform(0.1, 9.0, nleaf) if weights is None else np.asarray(weights, np.float64)
    word_id = np.zeros(nodes, np.uint32)
    word_id[1:] = np.arange(nleaf) if word_ids is None else np.asarray(word_ids, np.uint32)
    return dict(child_off=child_off, child_idx=child_idx, node_desc=node_desc, word_id=word_id, weight=weight, L=1)


# root -> A (a level-1 leaf), B, C (a single child, whose child has a single child), D; leaves at levels 1, 2, 3 and 4
RAGGED_SPEC = [0,
               [0, [[0, 0]], [0, [0, 0, 0]]],
               [[[0, 0]]],
               [0, [0, 0], [[0, 0], 0]]]


def ragged(seed):
    """A tree as DBoW2's k-means leaves it when small clusters stop early: L = 4, leaves at every level 1 .. 4, nodes with
    one child, a leaf directly under the root; ids in creation order.  A child's descriptor is its parent's with 20 bits
    inverted (the root's children are independent random rows), so that a query planted on a node descends to it.  Word
    ids go to the leaves in id order; one leaf in five has weight 0."""
    rng = np.random.default_rng(2000 + seed)
    child_off, child_idx, level = tree(RAGGED_SPEC)
    nodes = len(level)
    node_desc = random_rows(rng, nodes)
    for p in range(nodes):
        for c in child_idx[child_off[p]:child_off[p + 1]]:
            if p > 0:
                node_desc[c] = at_distance(rng, node_desc[p], 20)
    leaf = child_off[1:] == child_off[:-1]
    word_id = np.zeros(nodes, np.uint32)
    word_id[leaf] = np.arange(leaf.sum(), dtype=np.uint32)
    weight = rng.uniform(0.1, 9.0, nodes)
    weight[np.flatnonzero(leaf)[2::5]] = 0.0
    return dict(child_off=child_off, child_idx=child_idx, node_desc=node_desc, word_id=word_id, weight=weight, L=4)


def tied(k, L, seed=0):
    """Regular k-ary tree of depth L in which all siblings carry the same descriptor: every descent step is a k-way tie
    and the first child must win at every level."""
    voc = regular_vocabulary(k, L, seed=3000 + seed)
    co, ci = voc["child_off"], voc["child_idx"]
    for p in range(len(co) - 1):
        ch = ci[co[p]:co[p + 1]]
        if len(ch):
            voc["node_desc"][ch] = voc["node_desc"][ch[0]]
    return voc


def shared_words():
    """Depth 1, 12 leaves on 5 words: several leaves per word, the leaf -> word mapping not monotone, weights from 1e-3 to
    1e3 inside one word, so that a word's sum depends on the order its features are added in."""
    word_ids = [5, 2, 5, 9, 2, 5, 0, 9, 2, 7, 5, 0]
    weights = [1e-3, 7.7e2, 3.1, 1e3, 1.3e-3, 4.4e2, 0.37, 2.9e-2, 55.0, 6.1, 9.9e2, 1e-3]
    return flat(12, weights, word_ids, seed=7)


# ------------------------------------------------------------------------------------------------ transform cases
TRANSFORM_CASES = {}


def _case(name, voc, desc, levelsup, doc, regular=False, **extra):
    """regular: a full-depth tree with word ids in leaf order that the text loader of a DBoW2-shaped class can hold
    (k <= 20), so that class can be asked as well."""
    TRANSFORM_CASES[name] = dict(name=name, voc=voc, desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
                                 levelsup=levelsup, doc=doc, regular=regular, **extra)


WIDTHS_VOC = regular_vocabulary(4, 3, seed=41, zero_frac=0.1)


def widths(n):
    """n random descriptors (a prefix of one fixed sequence) through WIDTHS_VOC (k = 4, L = 3, one word in ten of weight
    0), levelsup 1."""
    desc = random_rows(np.random.default_rng(42), BOW_MAX_FEATURES)[:n]
    return dict(name=f"widths[{n}]", voc=WIDTHS_VOC, desc=desc, levelsup=1, regular=True,
                doc="k_bow_aggregate: P = the next power of two >= n, chunk = P / 1024 keys per thread; n = P leaves no padding key")


for _n in WIDTHS:
    TRANSFORM_CASES[f"widths[{_n}]"] = widths(_n)

_case("one_word", flat(1, [0.7]), random_rows(np.random.default_rng(50), 8192), 0,
      "k_bow_aggregate per-word sum: ONE run over all 8192 keys, walked by thread 0 across all 1024 chunks; value 1.0")
_case("three_words", flat(3, [1e-6, 3.3, 7e5]), random_rows(np.random.default_rng(51), 8192), 0,
      "k_bow_aggregate per-word sum: three runs of about 2700 keys, each across hundreds of chunks; the sequential sum of "
      "3.3 differs from count * 3.3")
_ad = flat(2048, seed=3)
_case("all_distinct", _ad, _ad["node_desc"][1:][::-1], 0,
      "bow_bitonic_sort with n = P = 2048: no padding key, every run of length 1, the keys arrive in descending order")
_case("shared_order", shared_words(), random_rows(np.random.default_rng(52), 8192), 0,
      "k_bow_aggregate per-word sum: `map[word] += weight` in FEATURE order, weights 1e-3 .. 1e3 inside one word")


def _zero_cases():
    base = regular_vocabulary(4, 3, seed=43)
    leaves = leaves_of(base)
    for n in (1024, 1025):
        desc = random_rows(np.random.default_rng(60 + n), n)
        leaf = descend(base, desc)[0]
        for kind in ("all", "half", "ends"):
            voc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
            if kind == "all":
                voc["weight"][:] = 0.0
            elif kind == "half":
                voc["weight"][leaves[::2]] = 0.0
            else:
                voc["weight"][np.concatenate([leaf[:5], leaf[-5:]])] = 0.0
            _case(f"zero_{kind}[{n}]", voc, desc, 1,
                  "k_bow_descend `keep = w > 0` and the ~0 sort keys of dropped features in k_bow_aggregate: " +
                  dict(all="every key is padding, counts 0 / 0 / 0", half="half of the words dropped",
                       ends="features 0 .. 4 and n - 5 .. n - 1 dropped")[kind], regular=True)


def descend(voc, desc):
    """The descent alone, vectorised over the features: (leaf node, node at every level 1 .. L or 0 past the leaf)."""
    co, ci = voc["child_off"].astype(np.int64), voc["child_idx"].astype(np.int64)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    cur = np.zeros(n, np.int64)
    path = np.zeros((n, voc["L"] + 1), np.int64)
    for lev in range(1, voc["L"] + 1):
        for p in np.unique(cur):
            ch = ci[co[p]:co[p + 1]]
            if len(ch) == 0:
                continue
            rows = np.flatnonzero(cur == p)
            d = POPC[desc[rows][:, None, :] ^ voc["node_desc"][ch][None, :, :]].sum(2, dtype=np.int32)
            cur[rows] = ch[d.argmin(1)]   # first minimum
            path[rows, lev] = cur[rows]
    return cur, path


_zero_cases()

_lv = regular_vocabulary(3, 4, seed=44, zero_frac=0.1)
for _ls in (0, 1, 3, 4, 6):
    _case(f"levels[{_ls}]", _lv, random_rows(np.random.default_rng(70), 400), _ls,
          "k_bow_descend `if (level == nid_level) nid = fin` with nid_level = L - levelsup = 4, 3, 1, 0, -2: the leaf itself, "
          "level 3, level 1, the root, below the root (node 0)", regular=True)


def ragged_queries(voc, n, seed):
    """n descriptors, the first half planted on the leaf descriptors of the tree (every leaf in turn, up to 3 bits
    inverted) so that leaves of every depth are reached, the rest random.  Returns (desc, planted leaf per feature or -1)."""
    rng = np.random.default_rng(seed)
    desc = random_rows(rng, n)
    leaves = leaves_of(voc)
    target = np.full(n, -1, np.int64)
    for i in range(n // 2):
        target[i] = leaves[i % len(leaves)]
        desc[i] = at_distance(rng, voc["node_desc"][target[i]], rng.integers(0, 4))
    perm = rng.permutation(n)
    return desc[perm], target[perm]


RAGGED_VOC = ragged(0)
_rq, RAGGED_TARGET = ragged_queries(RAGGED_VOC, 500, 80)
for _ls in (0, 1, 2, 4):
    _case(f"ragged[{_ls}]", RAGGED_VOC, _rq, _ls,
          "k_bow_descend on leaves above level L (`while (c1 != c0)` ends early), single children (the inner loop does not "
          "run) and `nid` left at 0 when the leaf is reached above level L - levelsup", target=RAGGED_TARGET)

_case("ties[tied]", tied(5, 3), random_rows(np.random.default_rng(90), 300), 1,
      "k_bow_descend `if (d < best)`: a 5-way tie at every level, the first child wins three times", regular=True)


def planted_ties(seed=0):
    """A random regular tree (k = 6, L = 3, no zero weights) and 300 queries of which the first six are planted, query j
    under level-1 node 1 + j (rewritten to sit 10 bits from the query): four are equidistant (30) from two of that node's
    children -- positions (0, 1), (2, 3), (4, 5), (0, 5) -- and closer to them than to the rest; one equals child 2
    (distance 0); one is the complement of child 0 (distance 256).  Returns (voc, desc, expected level-2 node per planted
    query)."""
    rng = np.random.default_rng(4000 + seed)
    voc = regular_vocabulary(6, 3, seed=45)
    co, ci, nd = voc["child_off"], voc["child_idx"], voc["node_desc"]
    desc = random_rows(rng, 300)
    expect = []
    for j, plan in enumerate([(0, 1), (2, 3), (4, 5), (0, 5), "zero", "far"]):
        p = int(ci[co[0] + j])
        ch = ci[co[p]:co[p + 1]]
        q = desc[j]
        nd[p] = at_distance(rng, q, 10)
        if plan == "zero":
            nd[ch[2]] = q
            expect.append(int(ch[2]))
        elif plan == "far":
            nd[ch[0]] = np.bitwise_not(q)
            nd[ch[3]] = at_distance(rng, q, 90)
            expect.append(int(ch[3]))
        else:
            a, b = plan
            nd[ch[a]] = at_distance(rng, q, 30)
            nd[ch[b]] = at_distance(rng, q, 30)
            expect.append(int(ch[a]))
    return voc, desc, np.asarray(expect)


_pv, _pd, PLANTED_TIE_NODES = planted_ties()
_case("ties[planted]", _pv, _pd, 1,
      "k_bow_descend `if (d < best)`: two siblings at the same distance at the first, a middle and the last position of the "
      "child list; a child at distance 0 and one at distance 256", regular=True)


# ------------------------------------------------------------------------------------------------ distinctive cases
DISTINCTIVE_CASES = {}


def two_clusters(rng, sizes, spread=3):
    """rows around two independent random centres, sizes[0] around the first then sizes[1] around the second, each with up
    to `spread` bits inverted"""
    centres = random_rows(rng, 2)
    rows = [at_distance(rng, centres[c], rng.integers(0, spread + 1)) for c in (0, 1) for _ in range(sizes[c])]
    return np.stack(rows) if rows else np.zeros((0, 32), np.uint8)


def pack_points(rng, points, shuffle=True):
    """list of [n_p, 32] row blocks -> (pool, off, idx): the pool holds all rows in a random order, idx points back"""
    rows = np.concatenate([p.reshape(-1, 32) for p in points]) if points else np.zeros((0, 32), np.uint8)
    perm = rng.permutation(len(rows)) if shuffle else np.arange(len(rows))
    pool = np.zeros_like(rows)
    pool[perm] = rows
    off = np.zeros(len(points) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in points])
    return pool, off, perm.astype(np.uint32)


def _dcase(name, points, doc, seed, expect=None, shuffle=True):
    pool, off, idx = pack_points(np.random.default_rng(seed), points, shuffle)
    DISTINCTIVE_CASES[name] = dict(name=name, pool=pool, off=off, idx=idx, doc=doc, expect=expect)


SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 0, 127, 128, 129, 1023, 1024, 0)


def _sizes():
    rng = np.random.default_rng(5000)
    pts = []
    for n in SIZES:
        a = (2 * n) // 3
        spread = 3 + (n % 7)      # medians differ from point to point
        pts.append(two_clusters(rng, (a, n - a), spread))
    _dcase("sizes", pts, "k_distinctive `for (i0 = 0; i0 < n; i0 += 64)`: n around every multiple of 64 up to DD_MAX_OBS, "
           "`ic = min(i, n - 1)` on the lanes past the end, points without observations between the others", 5001)


def _cluster_edge():
    rng = np.random.default_rng(5100)
    pts = []
    for n in (10, 11, 64, 65):
        k = int(0.5 * (n - 1))
        pts.append(two_clusters(rng, (k + 1, n - k - 1)))
        pts.append(two_clusters(rng, (k, n - k)))
    _dcase("cluster_edge", pts, "k_distinctive `k = (int)(0.5 * (n - 1))` and `cnt >= k + 1`: the median element is the last "
           "row of the own cluster, then the first of the other one", 5101, shuffle=False)


def cross_pass_point(rng, better_at=None):
    """200 rows.  c is a random row, A1 = c with bits 0 .. 9 inverted, A2 = c with bits 10 .. 19 inverted, S = c with bit 20
    inverted when `better_at` is given and c otherwise.  Rows 3, 67, 131 = S; row better_at = c; 96 or 97 rows A1 / A2 in
    halves; 100 independent random rows.  Medians (element 99 of the sorted row): S rows 10 (11 with `better_at`), the c
    row 10, A rows 20, random rows about 128 -- so row 3 wins with 10, or row better_at with 10 against 11."""
    c = random_rows(rng, 1)[0]
    a1, a2 = flip(c, range(0, 10)), flip(c, range(10, 20))
    s = c if better_at is None else flip(c, [20])
    rows = random_rows(rng, 200)
    special = [3, 67, 131] + ([] if better_at is None else [better_at])
    rest = [i for i in range(200) if i not in special]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    na = 100 - len(special)
    for t, i in enumerate(rest[:na]):
        rows[i] = a1 if t < 48 else a2
    for i in (3, 67, 131):
        rows[i] = s
    if better_at is not None:
        rows[better_at] = c
    return rows


def _cross_pass_ties():
    rng = np.random.default_rng(5200)
    pts = [cross_pass_point(rng), cross_pass_point(rng, 64), cross_pass_point(rng, 199)]
    _dcase("cross_pass_ties", pts, "k_distinctive `bestkey = min(bestkey, (lo << 16) | i)` across the passes i0 = 0, 64, 128, 192 "
           "and the lane reduction: equal medians in three passes, the first row wins; a better median in a later pass wins",
           5201, expect=(np.array([3, 64, 199], np.int32), np.array([10, 10, 10], np.int32)), shuffle=False)


def triple(rng, d, common):
    """c, c ^ A, c ^ B with |A| = |B| = d and |A & B| = common: distances d, d and 2 * (d - common)"""
    c = random_rows(rng, 1)[0]
    bits = rng.permutation(256)
    a = bits[:d]
    b = np.concatenate([bits[:common], bits[d:2 * d - common]])
    return np.stack([c, flip(c, a), flip(c, b)])


EQUILATERAL_D = (2, 64, 128, 170)   # three rows at equal pairwise distance d need 3 * d even: 1, 127 and 129 cannot be built
ISOSCELES_D = (1, 127, 129)         # ... those get two sides d and a third of d + 1: the median of the apex row is d as well


def _equilateral():
    rng = np.random.default_rng(5300)
    pts = [triple(rng, d, d // 2) for d in EQUILATERAL_D] + [triple(rng, d, (d - 1) // 2) for d in ISOSCELES_D]
    ds = np.array(EQUILATERAL_D + ISOSCELES_D, np.int32)
    _dcase("equilateral", pts, "k_distinctive bisection `mid = (lo + hi) >> 1`, `cnt += d <= mid`: medians on both sides of the "
           "first split at 128 and at the ends of the range", 5301, expect=(np.zeros(len(ds), np.int32), ds), shuffle=False)


def _extremes():
    rng = np.random.default_rng(5400)
    a = random_rows(rng, 4)
    pts = [np.repeat(a[0:1], 5, 0), np.repeat(a[1:2], 130, 0), np.stack([a[2], ~a[2]]), np.stack([a[3], ~a[3], ~a[3]])]
    pool, off, idx = pack_points(rng, pts, shuffle=False)
    # a point that observes the same pool row three times
    off = np.concatenate([off, [off[-1] + 3]]).astype(np.uint32)
    idx = np.concatenate([idx, [7, 7, 7]]).astype(np.uint32)
    DISTINCTIVE_CASES["extremes"] = dict(
        name="extremes", pool=pool, off=off, idx=idx, expect=(np.array([0, 0, 0, 1, 0], np.int32), np.zeros(5, np.int32)),
        doc="k_distinctive with every distance 0 (all rows tie, in one pass and across three), distance 256, and one pool row "
            "observed three times")


_sizes()
_cluster_edge()
_cross_pass_ties()
_equilateral()
_extremes()

"""Planted inputs for the projection-gated searches (csrc/orbfe_grid.hip, csrc/orbfe_projection.hip): every case sits on one
comparison that decides a single candidate, or on a size at which the host changes code path.  numpy + the CPU oracle only;
tests/test_proj_edge_cases.py checks that every case reaches its edge, tests/test_gpu_projection_edges.py feeds them to the
HIP kernels.  Test support only.

An edge is a pair or triple of inputs one float step (np.nextafter in binary32), one Hamming bit, one candidate or one
feature apart whose answers differ, so a comparison written the wrong way round fails at least one member.  The members
are queries of one call where only the query moves, separate calls where the frame moves.

A projection case is dict(calls=[call, ...], differ=[((call, query), (call, query)), ...]); a call is
dict(ci=core_inputs, q, qd, th, nnratio, rule, is2, want) with want = the planted answers per query, any of
  ncand / cands  candidates of GetFeaturesInArea (count / the list in the reference's order)
  rect           the cell rectangle (x0, y0, nx, ny) of the restatement below, None = the query leaves early
  match / best / second   the core's answer
`differ` names the members whose answers must differ.  Where the members differ only in `rect`, no output can: the
rectangle is conservative by construction (a feature of a column below floor((u - minx - r) * gw_inv) lies left of u - r),
so it decides which cells are walked, not which features are found; those cases pin the walked cells of the restatement
and the kernels must still find the same candidates.

A grid case is dict(xy, bounds, cell=[planted cell per keypoint, -1 = left out]); a triangulation case is
dict(calls=[dict(k1, k2, F12, ex, ey, th_low, want)], differ=[(call, call), ...])."""
import numpy as np

import hamming_cases as H
import proj_cases as PC
from oracle import oracle_ffi as O

F = np.float32
COLS, ROWS = PC.GRID_COLS, PC.GRID_ROWS
ORIGIN = (0.0, 640.0, 0.0, 480.0)                 # (minx, maxx, miny, maxy): ComputeImageBounds without distortion
DISTORTED = (float(F(-7.3)), float(F(651.8)), float(F(-4.9)), float(F(487.6)))   # undistorted corners of a barrel-distorted image
BOUNDS = {"origin": ORIGIN, "distorted": DISTORTED}


def up(x):
    return np.nextafter(F(x), F(np.inf))


def dn(x):
    return np.nextafter(F(x), F(-np.inf))


def grid_params(b):
    """(minx, miny, gw_inv, gh_inv) in binary32, as Frame's constructor computes them (src/Frame.cc:95-96)"""
    minx, maxx, miny, maxy = (F(v) for v in b)
    return minx, miny, F(F(COLS) / F(maxx - minx)), F(F(ROWS) / F(maxy - miny))


def adjacent(x, pred):
    """the neighbouring binary32 values (lo, hi) near x with pred(lo) false and pred(hi) true; pred is monotone in x"""
    x = F(x)
    for _ in range(1 << 16):
        if pred(x):
            lo = dn(x)
            if not pred(lo):
                return lo, x
            x = lo
        else:
            hi = up(x)
            if pred(hi):
                return x, hi
            x = hi
    raise AssertionError("no crossing near %r" % x)


# ------------------------------------------------------------------------------------------------ plain restatements
def rect_of(g, u, v, r):
    """the cell rectangle of GetFeaturesInArea (src/Frame.cc:470-484), every operation rounded to binary32"""
    minx, miny, gwi, ghi = g
    u, v, r = F(u), F(v), F(r)
    x0 = max(int(np.floor(F(F(F(u - minx) - r) * gwi))), 0)
    if x0 >= COLS:
        return None
    x1 = min(int(np.ceil(F(F(F(u - minx) + r) * gwi))), COLS - 1)
    if x1 < 0:
        return None
    y0 = max(int(np.floor(F(F(F(v - miny) - r) * ghi))), 0)
    if y0 >= ROWS:
        return None
    y1 = min(int(np.ceil(F(F(F(v - miny) + r) * ghi))), ROWS - 1)
    if y1 < 0:
        return None
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def _round_away(x):
    return np.copysign(np.floor(np.abs(np.float64(x)) + 0.5), np.float64(x))   # C roundf: half away from zero


def cell_of(g, x, y):
    """PosInGrid (src/Frame.cc:523-531): the cell px * 48 + py, or -1; a coordinate that is not finite or whose rounded
    product does not fit an int converts to INT_MIN on the CPU and is out of the grid"""
    minx, miny, gwi, ghi = g
    with np.errstate(all="ignore"):
        px, py = _round_away(F(F(F(x) - minx) * gwi)), _round_away(F(F(F(y) - miny) * ghi))
    if not (np.isfinite(px) and np.isfinite(py)) or not (0 <= px < COLS and 0 <= py < ROWS):
        return -1
    return int(px) * ROWS + int(py)


# ------------------------------------------------------------------------------------------------ frames and calls
def frame(xy, bounds=ORIGIN, octave=None, desc=None, uRight=None, blocked=None, seed=0):
    """a frame dict in proj_cases' layout around planted keypoints"""
    rng = np.random.default_rng(977 + seed)
    xy = np.asarray(xy, F).reshape(-1, 2)
    cur = PC.current_frame(rng, len(xy), stereo=False, dense_states=False)
    minx, miny, gwi, ghi = grid_params(bounds)
    cur.update(xy=xy, bounds=tuple(float(F(v)) for v in bounds), gw_inv=gwi, gh_inv=ghi)
    cur["octave"] = np.zeros(len(xy), np.int32) if octave is None else np.asarray(octave, np.int32)
    if desc is not None:
        cur["desc"] = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    if uRight is not None:
        cur["uRight"] = np.asarray(uRight, F)
    if blocked is not None:
        cur["state"] = np.where(np.asarray(blocked) != 0, 2, 0).astype(np.uint8)
    return cur


def queries(rows):
    """rows of (u, v, r[, (min_level, max_level)[, ur[, flags]]]) -> PROJ_QUERY_DTYPE"""
    q = np.zeros(len(rows), O.PROJ_QUERY_DTYPE)
    q["min_level"], q["max_level"] = -1, -1
    for i, row in enumerate(rows):
        q["u"][i], q["v"][i], q["r"][i] = row[:3]
        if len(row) > 3 and row[3] is not None:
            q["min_level"][i], q["max_level"][i] = row[3]
        if len(row) > 4:
            q["ur"][i] = row[4]
        if len(row) > 5:
            q["flags"][i] = row[5]
    return q


def call(cur, q, qd=None, th=100, nnratio=0.0, rule=0, is2=None, blocked="state", uRight="frame", **want):
    ci = PC.core_inputs(cur)
    if blocked is None:
        ci["blocked"] = None
    if uRight is None:
        ci["uRight"] = None
    if qd is None:
        qd = np.random.default_rng(len(q) + 31 * len(cur["xy"])).integers(0, 256, (len(q), 32), dtype=np.uint8)
    return dict(ci=ci, q=q, qd=np.ascontiguousarray(qd, np.uint8).reshape(-1, 32), th=th, nnratio=nnratio, rule=rule, is2=is2, want=want)


def run_core(fn, c):
    """the core of one call through fn = oracle_ffi.search_by_projection or ORBmatcher.SearchByProjectionCore"""
    return fn(queries=c["q"], qdesc=c["qd"], th=c["th"], nnratio=c["nnratio"], ratio_rule=c["rule"], inv_level_sigma2=c["is2"], **c["ci"])


def oracle_area(c, i):
    """GetFeaturesInArea of query i of a call (oracle)"""
    ci, q = c["ci"], c["q"]
    return O.features_in_area(ci["xyF"], ci["octF"], ci["grid"][0], ci["grid"][1], *[float(v) for v in ci["bounds"]], float(q["u"][i]),
                              float(q["v"][i]), float(q["r"][i]), int(q["min_level"][i]), int(q["max_level"][i]))


def _case(calls, differ=()):
    return dict(calls=list(calls), differ=list(differ))


def _scatter(seed, n, bounds, margin=0.0):
    """n keypoints spread over the grid's area (not planted: they only give the walked cells something to hold)"""
    rng = np.random.default_rng(4000 + seed)
    minx, maxx, miny, maxy = bounds
    return np.stack([rng.uniform(minx - margin, maxx + margin, n), rng.uniform(miny - margin, maxy + margin, n)], 1).astype(F)


# ------------------------------------------------------------------------------------------------ WINDOW_CASES
def w_box_radius(b):
    """features at exactly u +- r and v +- r: no candidates but the centre at r and one step below it, all five one step above"""
    xy = [(320, 240), (330, 240), (310, 240), (320, 250), (320, 230)]
    c = call(frame(xy, b), queries([(320, 240, dn(10)), (320, 240, 10), (320, 240, up(10))]),
             cands=[[0], [0], [2, 4, 0, 3, 1]])
    return _case([c], [((0, 1), (0, 2))])


def w_box_feature_step(b):
    """the same edge from the feature's side: x or y one step inside the box, on it, one step outside"""
    xy = [(dn(330), 240), (330, 240), (up(330), 240), (up(310), 240), (310, 240), (dn(310), 240),
          (320, dn(250)), (320, 250), (320, up(250)), (320, up(230)), (320, 230), (320, dn(230))]
    c = call(frame(xy, b), queries([(320, 240, 10)]), cands=[[3, 9, 6, 0]])
    return _case([c])


def _crossings(g, axis, side, k, r):
    """three neighbouring query centres around the one at which (c - min -+ r) * inv reaches the integer k (side -1: the
    floor of the lower edge, +1: the ceil of the upper edge)"""
    mn, inv = (g[0], g[2]) if axis == 0 else (g[1], g[3])
    r = F(r)

    def val(c):
        d = F(F(c) - mn)
        return F((F(d - r) if side < 0 else F(d + r)) * inv)
    # side -1: floor(val) goes k-1 -> k where val reaches k; side +1: ceil(val) goes k -> k+1 where val exceeds k
    lo, hi = adjacent(F(k) / inv + mn + (r if side < 0 else -r), (lambda c: val(c) >= k) if side < 0 else (lambda c: val(c) > k))
    return [dn(lo), lo, hi, up(hi)]


def w_rect_ties(b):
    """(u - minx +- r) * gw_inv on an integer and a step to either side, for the four edges of the rectangle; the walked
    cells change by one column / row at the step, the candidates must not"""
    g = grid_params(b)
    xy = _scatter(1, 900, b, 10.0)
    rows, rect, differ = [], [], []
    for axis, side, k, r in ((0, -1, 20, 15), (0, 1, 41, 15), (1, -1, 11, 15), (1, 1, 30, 15), (0, -1, 1, 7), (0, 1, 62, 7),
                             (1, -1, 1, 7), (1, 1, 46, 7)):
        for c in _crossings(g, axis, side, k, r):
            rows.append((c, 243.5, r) if axis == 0 else (317.25, c, r))
            rect.append(rect_of(g, *rows[-1]))
        n = len(rows)
        differ.append(((0, n - 3), (0, n - 2)))
        lo, hi = rect[n - 3], rect[n - 2]
        edge = (lo[axis], hi[axis]) if side < 0 else (lo[axis] + lo[axis + 2] - 1, hi[axis] + hi[axis + 2] - 1)
        assert edge == ((k - 1, k) if side < 0 else (k, k + 1)), (axis, side, k, edge)
    return _case([call(frame(xy, b, octave=np.arange(900) % 8), queries(rows), rect=rect)], differ)


def w_clipped(b):
    """rectangles clipped at column 0 / 63 and row 0 / 47, with keypoints in the border cells (also the ones a little outside the
    bounds that still round into cell 0)"""
    g = grid_params(b)
    minx, maxx, miny, maxy = (float(F(v)) for v in b)
    xy = np.concatenate([_scatter(2, 500, b, 12.0),
                         [(minx - 2, miny - 2), (minx + 1, miny + 200), (maxx - 6, miny + 200), (minx + 300, miny - 3),
                          (minx + 300, maxy - 6), (maxx - 7, maxy - 7)]]).astype(F)
    rows = [(minx + 3, miny + 200, 10), (maxx - 3, miny + 200, 10), (minx + 300, miny + 2, 10), (minx + 300, maxy - 2, 10),
            (minx - 4, miny - 4, 9), (maxx + 4, maxy + 4, 14), (minx - 5, maxy + 5, 16), (maxx + 5, miny - 5, 16)]
    rect = [rect_of(g, *r) for r in rows]
    assert rect[0][0] == 0 and rect[2][1] == 0 and rect[1][0] + rect[1][2] == COLS and rect[3][1] + rect[3][3] == ROWS
    assert rect[4][:2] == (0, 0) and rect[5][0] + rect[5][2] == COLS and rect[5][1] + rect[5][3] == ROWS
    return _case([call(frame(xy, b), queries(rows), rect=rect)])


def _extent(mn, inv, c, r, n):
    """cells along one axis of the rectangles of centres c (vectorised rect_of)"""
    d = (np.asarray(c, F) - mn).astype(F)
    lo = np.maximum(np.floor(((d - r).astype(F) * inv).astype(F)), 0)
    hi = np.minimum(np.ceil(((d + r).astype(F) * inv).astype(F)), n - 1)
    return np.where((lo >= n) | (hi < 0), 0, hi - lo + 1)


def _find_window(g, b, nx, ny):
    """(u, v, r) whose rectangle has exactly nx by ny cells"""
    minx, maxx, miny, maxy = b
    us, vs = np.arange(minx - 40, maxx + 40, 1.0).astype(F), np.arange(miny - 40, maxy + 40, 1.0).astype(F)
    for r in np.arange(0.5, 120.0, 0.5).astype(F):
        iu, iv = np.flatnonzero(_extent(g[0], g[2], us, r, COLS) == nx), np.flatnonzero(_extent(g[1], g[3], vs, r, ROWS) == ny)
        if len(iu) and len(iv):
            return float(us[iu[len(iu) // 2]]), float(vs[iv[len(iv) // 2]]), float(r)
    raise AssertionError((nx, ny))


def w_cell_counts(b):
    """rectangles of exactly 1, 64, 65 and all 3072 cells: a wave's 64 lanes take ceil(ncell / 64) cells each"""
    g = grid_params(b)
    minx, maxx, miny, maxy = (float(F(v)) for v in b)
    xy = np.concatenate([_scatter(3, 1500, b), [(minx - 1, miny - 1)]]).astype(F)
    rows = [(minx - 6, miny - 6, 5.5), _find_window(g, b, 8, 8), _find_window(g, b, 5, 13), _find_window(g, b, 13, 5),
            (minx + 300, miny + 200, 1000)]
    rect = [rect_of(g, *r) for r in rows]
    assert [r[2] * r[3] for r in rect] == [1, 64, 65, 65, 3072]
    c = call(frame(xy, b, octave=np.arange(len(xy)) % 8), queries(rows), rect=rect)
    c["want"]["ncand"] = [1, None, None, None, None]
    return _case([c])


def w_zero_radius(b):
    """r = 0 on top of a keypoint: |dx| < 0 never holds; the smallest normal radius takes it"""
    c = call(frame([(320, 240), (100.5, 50.25)], b), queries([(320, 240, 0), (320, 240, np.finfo(F).tiny), (100.5, 50.25, 0)]),
             cands=[[], [0], []])
    return _case([c], [((0, 0), (0, 1))])


def w_outside(b):
    """windows entirely outside the grid on each side leave early; the neighbouring centre one step nearer walks the border column"""
    g = grid_params(b)
    minx, maxx, miny, maxy = (float(F(v)) for v in b)
    xy = np.concatenate([_scatter(4, 300, b, 12.0), [(minx - 3, miny + 100), (minx + 100, miny - 3)]]).astype(F)
    r = F(10)
    rows, differ = [(minx - 500, miny + 100, 10), (maxx + 500, miny + 100, 10), (minx + 100, miny - 900, 10), (minx + 100, maxy + 900, 10)], []
    # upper edge: ceil((c - min + r) * inv) < 0 leaves; lower edge: floor((c - min - r) * inv) >= 64 / 48 leaves
    for axis, mn, inv, n in ((0, g[0], g[2], COLS), (1, g[1], g[3], ROWS)):
        lo, hi = adjacent(mn - r - F(1) / inv, lambda c: F(F(F(F(c) - mn) + r) * inv) > -1)
        a, bq = adjacent(mn + r + F(n) / inv, lambda c: F(F(F(F(c) - mn) - r) * inv) >= n)
        for c in (lo, hi, a, bq):
            rows.append((c, miny + 100, r) if axis == 0 else (minx + 100, c, r))
        differ += [((0, len(rows) - 4), (0, len(rows) - 3)), ((0, len(rows) - 2), (0, len(rows) - 1))]
    rect = [rect_of(g, *q) for q in rows]
    assert [x is None for x in rect] == [True] * 4 + [True, False, False, True] * 2
    c = call(frame(xy, b), queries(rows), rect=rect)
    c["want"]["ncand"] = [0, 0, 0, 0] + [None] * 8
    return _case([c], differ)


LEVEL_WINDOWS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (0, 0), (3, 3), (2, 5), (5, 2), (-1, 7)]


def w_levels(b):
    """the level filter is on only if min_level > 0 or max_level >= 0; a window with one keypoint on every octave 0..7"""
    xy = [(300 + 5 * o, 236 + 3 * (o % 3)) for o in range(8)]
    want = [8, 8, 7, 1, 1, 1, 4, 0, 8]
    c = call(frame(xy, b, octave=np.arange(8)[::-1]), queries([(318, 240, 30, lv) for lv in LEVEL_WINDOWS]), ncand=want)
    return _case([c], [((0, 1), (0, 2)), ((0, 0), (0, 3)), ((0, 6), (0, 7))])


_WINDOW_BUILDERS = dict(box_radius=w_box_radius, box_feature_step=w_box_feature_step, rect_ties=w_rect_ties, clipped=w_clipped,
                        cell_counts=w_cell_counts, zero_radius=w_zero_radius, outside=w_outside, levels=w_levels)
WINDOW_CASES = {"%s-%s" % (k, bn): (lambda f=f, b=b: f(b)) for k, f in _WINDOW_BUILDERS.items() for bn, b in BOUNDS.items()}


# ------------------------------------------------------------------------------------------------ GRID_CASES
def _grid_case(xy, b, cell):
    return dict(xy=np.asarray(xy, F).reshape(-1, 2), bounds=b, cell=[int(c) for c in cell])


def _tie(mn, inv, k):
    """neighbouring coordinates (lo, hi): (lo - mn) * inv rounds to k, (hi - mn) * inv to k + 1"""
    return adjacent((F(k) + F(0.5)) / inv + mn, lambda c: F(F(F(c) - mn) * inv) >= F(k) + F(0.5))


def g_round_ties(b):
    """(x - minx) * gw_inv on k + 0.5 (round() goes away from zero) and a step to either side; at the last column / row the
    keypoint is inside one step below the tie and outside at it"""
    g = grid_params(b)
    minx, miny, gwi, ghi = g
    xy, cell = [], []
    for k in (0, 1, 31, 62, 63):
        lo, hi = _tie(minx, gwi, k)
        for x, kk in ((dn(lo), k), (lo, k), (hi, k + 1), (up(hi), k + 1)):
            xy.append((x, miny + 100))
            cell.append(-1 if kk >= COLS else kk * ROWS + cell_of(g, minx + 100, miny + 100) % ROWS)
    for k in (0, 23, 46, 47):
        lo, hi = _tie(miny, ghi, k)
        for y, kk in ((dn(lo), k), (lo, k), (hi, k + 1), (up(hi), k + 1)):
            xy.append((minx + 100, y))
            cell.append(-1 if kk >= ROWS else (cell_of(g, minx + 100, miny + 100) // ROWS) * ROWS + kk)
    return _grid_case(xy, b, cell)


def g_min_edge(b):
    """keypoints at minx / miny exactly and a little below: still cell 0 while the product is above -0.5 (round(-0.5) = -1)"""
    g = grid_params(b)
    minx, miny, gwi, ghi = g
    xo, xi = adjacent(minx - F(0.5) / gwi, lambda c: F(F(F(c) - minx) * gwi) > F(-0.5))
    yo, yi = adjacent(miny - F(0.5) / ghi, lambda c: F(F(F(c) - miny) * ghi) > F(-0.5))
    xy = [(minx, miny), (minx - F(0.4) / gwi, miny), (minx, miny - F(0.4) / ghi), (xi, miny), (xo, miny), (minx, yi), (minx, yo), (xi, yi),
          (xo, yo), (minx + 50, yi), (xi, miny + 50)]
    far = cell_of(g, minx + 50, miny), cell_of(g, minx, miny + 50)
    return _grid_case(xy, b, [0, 0, 0, 0, -1, 0, -1, 0, -1, far[0], far[1]])


def g_nonfinite(b):
    """NaN, +-Inf and +-1e30 coordinates among ordinary keypoints: PosInGrid's int conversion puts them out of the grid"""
    g = grid_params(b)
    bad = [(np.nan, 100), (100, np.nan), (np.nan, np.nan), (np.inf, 100), (100, -np.inf), (-np.inf, np.inf), (1e30, 100), (100, -1e30),
           (-1e30, 1e30), (np.nan, np.inf)]
    good = _scatter(5, 40, b)
    xy, isbad = [], []
    for i in range(40):   # interleaved with ordinary keypoints
        xy.append(good[i])
        isbad.append(False)
        if i < len(bad):
            xy.append(bad[i])
            isbad.append(True)
    xy += [(g[0] + 1, g[1] + 100), (g[0] + 100, g[1] + 1), (g[0] + 1, g[1] + 1)]   # column 0 / row 0, where a NaN converted to 0 would land
    isbad += [False] * 3
    xy = np.asarray(xy, F)
    cell = [-1 if bad_ else cell_of(g, x, y) for (x, y), bad_ in zip(xy, isbad)]
    assert all(cell_of(g, x, y) == -1 for (x, y), bad_ in zip(xy, isbad) if bad_) and cell[-3:] != [-1] * 3
    return _grid_case(xy, b, cell)


def g_one_cell(b, n):
    """all n keypoints in one cell: the per-cell insertion sort and the placement atomics of one counter"""
    g = grid_params(b)
    rng = np.random.default_rng(n)
    cx, cy = g[0] + F(32) / g[2], g[1] + F(24) / g[3]   # the middle of cell (32, 24)
    xy = np.stack([cx + rng.uniform(-3, 3, n), cy + rng.uniform(-3, 3, n)], 1).astype(F)
    c = 32 * ROWS + 24
    case = _grid_case(xy, b, [c] * n)
    assert all(cell_of(g, x, y) == c for x, y in xy)
    return case


def g_spread(b, n):
    """n keypoints over the grid, some outside: the 1024-thread strides at n = 1023, 1024, 1025"""
    g = grid_params(b)
    xy = _scatter(n, n, b, 15.0)
    return _grid_case(xy, b, [cell_of(g, x, y) for x, y in xy])


_GRID_BUILDERS = dict(round_ties=g_round_ties, min_edge=g_min_edge, nonfinite=g_nonfinite)
_GRID_BUILDERS.update({"one_cell_%d" % n: (lambda b, n=n: g_one_cell(b, n)) for n in (1, 2, 300, 2000)})
_GRID_BUILDERS.update({"spread_%d" % n: (lambda b, n=n: g_spread(b, n)) for n in (1023, 1024, 1025)})
GRID_CASES = {"%s-%s" % (k, bn): (lambda f=f, b=b: f(b)) for k, f in _GRID_BUILDERS.items() for bn, b in BOUNDS.items()}


# ------------------------------------------------------------------------------------------------ SLAB_CASES
PJ_SLAB, PJ_MAX_NF, WD_MAX_NF = 512, 15360, 65535


def _random_frame_queries(seed, nF, nq, r=6.0, bounds=ORIGIN, per_slot=None):
    """a seeded frame and queries aimed at its keypoints (several per keypoint when nq > nF: contended slots, so the rounds
    re-scan); claims on most queries, the ratio rule's levels mixed"""
    rng = np.random.default_rng(seed)
    cur = PC.current_frame(rng, nF)
    tgt = rng.integers(0, nF, nq) if per_slot is None else rng.integers(0, max(nq // per_slot, 1), nq) % nF
    q = np.zeros(nq, O.PROJ_QUERY_DTYPE)
    q["u"] = cur["xy"][tgt, 0] + rng.normal(0, 1.5, nq).astype(F)
    q["v"] = cur["xy"][tgt, 1] + rng.normal(0, 1.5, nq).astype(F)
    q["r"] = F(r)
    q["min_level"], q["max_level"] = -1, -1
    q["ur"] = np.where(cur["uRight"][tgt] > 0, cur["uRight"][tgt] + rng.normal(0, 3, nq), 0).astype(F)
    q["flags"] = np.where(rng.random(nq) < 0.85, 1, 0) | 2
    return cur, q, PC.noisy_copy(rng, cur["desc"][tgt], 60)


def s_candidates(n):
    """one query with exactly n - 1 and one with exactly n candidates among ordinary queries: n - 1 keypoints in a cluster
    and one at u + 25; r = 25 leaves it out, one step above takes it in.  n = 513 is the first count above the slab"""
    rng = np.random.default_rng(n)
    cur, q, qd = _random_frame_queries(n, 200, 24)
    keep = ~((np.abs(cur["xy"][:, 0] - 400) < 60) & (np.abs(cur["xy"][:, 1] - 300) < 60))   # nothing else near the cluster
    xy = np.concatenate([cur["xy"][keep], np.stack([400 + rng.uniform(-9, 9, n - 1), 300 + rng.uniform(-9, 9, n - 1)], 1), [(425, 300)]]).astype(F)
    nF = len(xy)
    desc = np.concatenate([cur["desc"][keep], rng.integers(0, 256, (n, 32), dtype=np.uint8)])
    cur2 = frame(xy, ORIGIN, octave=rng.integers(0, 8, nF), desc=desc,
                 uRight=np.where(rng.random(nF) < 0.5, xy[:, 0] - 20, -1), blocked=rng.random(nF) < 0.2)
    big = queries([(400, 300, 25, None, 380, 3), (400, 300, up(25), None, 380, 3)])
    q2 = np.concatenate([q[:12], big[:1], q[12:], big[1:]])
    qd2 = np.concatenate([qd[:12], qd[:1], qd[12:], qd[1:2]])
    want = [None] * len(q2)
    want[12], want[-1] = n - 1, n
    return _case([call(cur2, q2, qd2, th=100, nnratio=0.8, rule=1, ncand=want)], [((0, 12), (0, len(q2) - 1))])


def s_lds(total):
    """max(nF, 1) + 8 nq = total: 16384 words fill the one-launch form's LDS exactly, 16385 take the four-kernel form"""
    nq = 1024
    cur, q, qd = _random_frame_queries(total, total - 8 * nq, nq)
    return _case([call(cur, q, qd, th=100, nnratio=0.8, rule=1)])


def s_queries(nq):
    """nq = 1, 4, 5 (four queries share a workgroup of k_proj_fused), 64, 65 (queries that re-scan per pass of k_proj_rounds),
    1024, 1025 (thread strides); three to four queries contend for every slot"""
    cur, q, qd = _random_frame_queries(nq, 300, nq, per_slot=4)
    return _case([call(cur, q, qd, th=100, nnratio=0.9, rule=1)])


def s_max_features():
    """nF = 15360, the largest owner table, with a handful of queries (the last keypoint among their candidates)"""
    cur, q, qd = _random_frame_queries(7, PJ_MAX_NF, 8, r=9.0)
    q["u"][0], q["v"][0] = cur["xy"][-1]
    qd[0] = cur["desc"][-1]
    c = call(cur, q, qd, th=100, nnratio=0.8, rule=1)
    return _case([c])


def s_window_distances_max():
    """nF = 65535, the largest 16-bit index of an entry: orbfe_window_distances only"""
    rng = np.random.default_rng(65535)
    xy = np.stack([rng.uniform(0, 640, WD_MAX_NF), rng.uniform(0, 480, WD_MAX_NF)], 1).astype(F)
    xy[-1] = (321.5, 243.25)
    cur = frame(xy, ORIGIN, octave=rng.integers(0, 8, WD_MAX_NF), desc=rng.integers(0, 256, (WD_MAX_NF, 32), dtype=np.uint8))
    q = queries([(xy[-1, 0], xy[-1, 1], 4.0), (320, 240, 6.0, (2, 5)), (5, 5, 8.0), (xy[0, 0], xy[0, 1], 3.0)])
    c = call(cur, q)
    c["wd_only"] = True
    return _case([c])


SLAB_CASES = {"candidates_%d" % n: (lambda n=n: s_candidates(n)) for n in (511, 512, 513)}
SLAB_CASES.update({"lds_words_%d" % t: (lambda t=t: s_lds(t)) for t in (16384, 16385)})
SLAB_CASES.update({"queries_%d" % n: (lambda n=n: s_queries(n)) for n in (1, 4, 5, 64, 65, 1024, 1025)})
SLAB_CASES.update(features_15360=s_max_features, window_distances_65535=s_window_distances_max)


# ------------------------------------------------------------------------------------------------ DECISION_CASES
def _window_call(cands, th, nnratio=0.0, rule=0, blocked=(), no_blocked=False, seed=0):
    """one query at (320, 240), r = 30, over candidates given in CANDIDATE order as (distance, level): candidate p sits in its
    own grid column (x = 297 + 10 p), so the order is the columns' and not the keypoint indices', which are scrambled.
    Returns (call, idx) with idx[p] = the keypoint index of candidate p; `blocked` lists candidate positions"""
    rng = np.random.default_rng(50 + seed)
    n = len(cands)
    assert n <= 6
    idx = rng.permutation(n) if n > 1 else np.arange(n)
    if n > 1 and idx[0] == 0:
        idx = np.roll(idx, 1)   # the first candidate is never keypoint 0
    base = H.random_rows(rng, 1)[0]
    xy, desc, octv, bl = np.zeros((n, 2), F), np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for p, (d, lv) in enumerate(cands):
        xy[idx[p]] = (297 + 10 * p, 240)
        desc[idx[p]] = H.at_distance(rng, base, d)
        octv[idx[p]] = lv
        bl[idx[p]] = p in blocked
    c = call(frame(xy, ORIGIN, octave=octv, desc=desc, blocked=bl), queries([(320, 240, 30)]), [base], th=th, nnratio=nnratio, rule=rule,
             blocked=None if no_blocked else "state")
    c["want"]["cands"] = [[int(i) for i in idx]]
    return c, [int(i) for i in idx]


def _decided(cands, match_pos, best, second, **kw):
    c, idx = _window_call(cands, **kw)
    c["want"].update(match=[idx[match_pos] if match_pos is not None else -1], best=[best], second=[second])
    return c


def d_threshold(th):
    """bestDist <= th: best == th is accepted, best == th + 1 is not (th = 255: 256 is every bit, and 'no candidate')"""
    return _case([_decided([(th, 0)], 0, th, 256, th=th), _decided([(th + 1, 0)], None, th + 1 if th < 255 else 256, 256, th=th)], [(0, 1)])


def d_tied_best(n):
    """n candidates tied at the best distance in different cells: the first in candidate order wins (not the lowest index),
    and the tie's other members are the second best; one bit more on the first moves the match to the next"""
    tie = [(7, 0)] * n + [(30, 0)]
    worse = [(8, 0)] + tie[1:]
    return _case([_decided(tie, 0, 7, 7, th=100), _decided(worse, 1, 7, 7 if n > 2 else 8, th=100, seed=1)], [(0, 1)])


def d_second_level(order):
    """distances [5, 5, 3], [5, 3, 5], [3, 5, 5] with the two 5s on levels A != B: the second best is the FIRST 5 in candidate
    order, and only when the best shares ITS level does the ratio rule (3 > 0.5 * 5) reject"""
    A, Bv = 2, 4
    pos3 = order.index(3)
    first5 = order.index(5)
    calls = []
    for lv3, accept in ((A, False), (Bv, True)):   # the first 5 is on level A, the other on B
        cands = []
        for p, d in enumerate(order):
            cands.append((3, lv3) if d == 3 else (5, A if p == first5 else Bv))
        calls.append(_decided(cands, pos3 if accept else None, 3, 5, th=100, nnratio=0.5, rule=1, seed=len(calls)))
    return _case(calls, [(0, 1)])


def d_ratio(nnratio):
    """(float)best > nnratio * (float)second rejects; equality passes.  Every pair of RATIO_EDGES sits on equality in binary32,
    the pair one bit worse is rejected -- but only with both on one level, with a second at all, and with the rule on"""
    calls, differ = [], []
    for b, s in H.RATIO_EDGES[nnratio]:
        k = len(calls)
        calls += [_decided([(b, 1), (s, 1)], 0, b, s, th=100, nnratio=nnratio, rule=1, seed=k),
                  _decided([(b + 1, 1), (s, 1)], None, b + 1, s, th=100, nnratio=nnratio, rule=1, seed=k + 1),
                  _decided([(b + 1, 1), (s, 3)], 0, b + 1, s, th=100, nnratio=nnratio, rule=1, seed=k + 2),
                  _decided([(b + 1, 1)], 0, b + 1, 256, th=100, nnratio=nnratio, rule=1, seed=k + 3),
                  _decided([(b + 1, 1), (s, 1)], 0, b + 1, s, th=100, nnratio=nnratio, rule=0, seed=k + 4)]
        differ += [(k, k + 1), (k + 1, k + 2), (k + 1, k + 3), (k + 1, k + 4)]
    return _case(calls, differ)


def d_blocked():
    """a blocked best hands the match to the second; everything blocked leaves -1 / 256; blocked = None blocks nothing"""
    cands = [(9, 0), (3, 0), (5, 0)]
    return _case([_decided(cands, 1, 3, 5, th=100), _decided(cands, 2, 5, 9, th=100, blocked=(1,)),
                  _decided(cands, None, 256, 256, th=100, blocked=(0, 1, 2)), _decided(cands, 1, 3, 5, th=100, blocked=(1,), no_blocked=True)],
                 [(0, 1), (1, 2), (1, 3)])


DECISION_CASES = {"threshold_%d" % th: (lambda th=th: d_threshold(th)) for th in (0, 50, 100, 255)}
DECISION_CASES.update({"tied_best_%d" % n: (lambda n=n: d_tied_best(n)) for n in (2, 3)})
DECISION_CASES.update({"second_level_%s" % "".join(map(str, o)): (lambda o=o: d_second_level(o)) for o in ((5, 5, 3), (5, 3, 5), (3, 5, 5))})
DECISION_CASES.update({"ratio_%s" % r: (lambda r=r: d_ratio(r)) for r in H.RATIO_EDGES})
DECISION_CASES.update(blocked=d_blocked)


# ------------------------------------------------------------------------------------------------ GATE_CASES
FLAG_CLAIMS, FLAG_RIGHT, FLAG_CHI2 = 1, 2, 4


def _near_far(uR_near, seed=0):
    """two candidates of one window: keypoint 0 at distance 3 with mvuRight = uR_near, keypoint 1 at distance 9, monocular"""
    rng = np.random.default_rng(70 + seed)
    base = H.random_rows(rng, 1)[0]
    desc = np.stack([H.at_distance(rng, base, 3), H.at_distance(rng, base, 9)])
    return frame([(320, 240), (323, 242)], ORIGIN, desc=desc, uRight=[uR_near, -1.0]), base


def t_right_gate():
    """ur > 0 && |Q.ur - ur| > r skips: equality is kept, one step above is not, the flag off or no mvuRight array gates
    nothing, and a keypoint with mvuRight 0.0 or -1.0 is never gated however far Q.ur is"""
    cur, base = _near_far(100.0)
    q = queries([(320, 240, 8, None, 108, 2), (320, 240, 8, None, up(108), 2), (320, 240, 8, None, up(108), 0),
                 (320, 240, 8, None, 92, 2), (320, 240, 8, None, dn(92), 2), (320, 240, 8, None, dn(92), 1)])
    a = call(cur, q, [base] * 6, th=50, match=[0, 1, 0, 0, 1, 0], best=[3, 9, 3, 3, 9, 3])
    b = call(cur, q, [base] * 6, th=50, uRight=None, match=[0] * 6, best=[3] * 6)
    calls, differ = [a, b], [((0, 0), (0, 1)), ((0, 1), (0, 2)), ((0, 3), (0, 4)), ((0, 1), (1, 1))]
    for k, ur in enumerate((0.0, -1.0, float(np.finfo(F).tiny))):
        cur2, base2 = _near_far(ur, seed=1 + k)
        gated = ur > 0
        calls.append(call(cur2, queries([(320, 240, 8, None, 500, 2)]), [base2], th=50, match=[1 if gated else 0], best=[9 if gated else 3]))
    differ.append(((2, 0), (4, 0)))
    return _case(calls, differ)


CHI2_BOUNDS = dict(stereo_over=F(7.8), stereo_under=dn(F(7.8)), mono_under=F(5.99), mono_over=up(F(5.99)))


def t_chi2_gate():
    """Fuse's gate e2 * invSigma2 > 7.8 (mvuRight >= 0, three terms) or > 5.99 (two terms), a float product compared as double:
    with e2 = 1 exactly, invSigma2 = float32(7.8) = 7.80000019 exceeds 7.8 and the float below it does not; float32(5.99) =
    5.98999977 does not exceed 5.99 and the float above it does.  A compare in float would keep / skip the wrong ones"""
    is2 = np.array([CHI2_BOUNDS["stereo_over"], CHI2_BOUNDS["stereo_under"], CHI2_BOUNDS["mono_under"], CHI2_BOUNDS["mono_over"], 7.0], F)
    # (mvuRight, octave, kept): level 4 (7.0) lies between the bounds, so it tells a stereo from a monocular keypoint
    feats = [(30.0, 0, 0), (30.0, 1, 1), (0.0, 0, 0), (0.0, 1, 1), (0.0, 4, 1), (-1.0, 2, 1), (-1.0, 3, 0), (-1.0, 4, 0),
             (-1.0, 9, 0), (30.0, 9, 1), (30.0, -3, 0), (30.0, 1, 1), (-1.0, 1, 0)]
    n = len(feats)
    rng = np.random.default_rng(90)
    xy = np.array([(60 + 40 * i, 100 + 25 * (i % 3)) for i in range(n)], F)
    desc = H.random_rows(rng, n)
    cur = frame(xy, ORIGIN, octave=[f[1] for f in feats], desc=desc, uRight=[f[0] for f in feats])
    rows = [(xy[i, 0] + 1, xy[i, 1], 5, None, feats[i][0], FLAG_CHI2) for i in range(n)]
    rows += [(xy[i, 0] + 1, xy[i, 1], 5, None, feats[i][0], 0) for i in (0, 6)]              # the flag off in the same call
    rows += [(xy[i, 0] + 1, xy[i, 1], 5, None, feats[i][0], FLAG_CHI2 | FLAG_RIGHT | FLAG_CLAIMS) for i in (1, 5)]
    q = queries(rows)
    qd = np.stack([H.at_distance(rng, desc[i], 4) for i in list(range(n)) + [0, 6, 1, 5]])
    kept = [i if feats[i][2] else -1 for i in range(n)] + [0, 6, 1, 5]
    a = call(cur, q, qd, th=50, is2=is2, blocked=None, match=kept, best=[4 if k >= 0 else 256 for k in kept])
    b = call(cur, q, qd, th=50, is2=None, blocked=None, match=list(range(n)) + [0, 6, 1, 5], best=[4] * len(q))
    differ = [((0, 0), (0, 1)), ((0, 2), (0, 3)), ((0, 5), (0, 6)), ((0, 4), (0, 7)), ((0, 8), (0, 9)), ((0, 10), (0, 11)), ((0, 0), (0, n)),
              ((0, 0), (1, 0))]
    return _case([a, b], differ)


GATE_CASES = dict(right_gate=t_right_gate, chi2_gate=t_chi2_gate)


# ------------------------------------------------------------------------------------------------ ROUND_CASES
def _chain(L, no_claim=None, extra=False, seed=0):
    """L + 1 queries and slots on a line, 8 px apart: query i's window (centre 4 px left of slot i, r = 6) holds slot i at
    distance 8 and slot i - 1 at distance 9, both on one level.  With nnratio 0.8 (8 > 7.2) query i is rejected while
    slot i - 1 is free, and accepted (a single free candidate) once query i - 1 has claimed it: link i settles in round i."""
    rng = np.random.default_rng(600 + L + seed)
    n = L + 1
    xy = np.array([(40 + 8 * (i % 70), 100 + 40 * (i // 70)) for i in range(n)], F)
    qd, desc = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    qd[0] = H.random_rows(rng, 1)[0]
    for i in range(n):
        desc[i] = H.at_distance(rng, qd[i], 8)
        if i + 1 < n:
            qd[i + 1] = H.at_distance(rng, desc[i], 9)
    rows = [(xy[i, 0] - 4, xy[i, 1], 6, None, 0, 0 if i == no_claim else FLAG_CLAIMS) for i in range(n)]
    match = [i if (no_claim is None or i <= no_claim) else -1 for i in range(n)]
    if extra:   # a later query whose only candidate is the slot of the link that did not claim: two queries end on it
        rows.append((xy[no_claim, 0], xy[no_claim, 1], 3, None, 0, FLAG_CLAIMS))
        qd = np.concatenate([qd, [H.at_distance(rng, desc[no_claim], 2)]])
        match.append(no_claim)
    c = call(frame(xy, ORIGIN, octave=np.full(n, 3), desc=desc), queries(rows), qd, th=100, nnratio=0.8, rule=1, match=match)
    c["chain"] = L if no_claim is None else no_claim
    return c


def r_chain(L):
    return _case([_chain(L)])


def r_broken_chain(L, at):
    """the same chain with the claim flag cleared on link `at`: it matches but leaves its slot free, every later link stays
    rejected, and a last query matches the slot that link already has"""
    return _case([_chain(L, None, seed=1), _chain(L, at, True, seed=1)], [((0, at + 1), (1, at + 1))])


def r_shared_slot():
    """two queries with one best slot: when the earlier one does not claim, both keep it; when it claims, the later takes
    its second best"""
    rng = np.random.default_rng(800)
    base = H.random_rows(rng, 1)[0]
    desc = np.stack([H.at_distance(rng, base, 4), H.at_distance(rng, base, 20)])
    cur = frame([(200, 200), (204, 203)], ORIGIN, octave=[1, 5], desc=desc)
    calls = [call(cur, queries([(201, 201, 10, None, 0, fl), (202, 202, 10, None, 0, FLAG_CLAIMS)]), [base, base], th=100, nnratio=0.8, rule=1,
                  match=[0, want2], best=[4, b2]) for fl, want2, b2 in ((0, 0, 4), (FLAG_CLAIMS, 1, 20))]
    return _case(calls, [((0, 1), (1, 1))])


ROUND_CASES = {"chain_%d" % L: (lambda L=L: r_chain(L)) for L in (1, 15, 16, 17, 63, 64, 65)}
ROUND_CASES.update({"broken_chain_%d_at_%d" % (L, at): (lambda L=L, at=at: r_broken_chain(L, at)) for L, at in ((17, 9), (65, 63))})
ROUND_CASES.update(shared_slot=r_shared_slot)


# ------------------------------------------------------------------------------------------------ TRI_CASES
TRI_F = np.array([0, 0, 0, 0, 0, 0, 0, 1, -100], F)   # the epipolar line of every keyframe-1 keypoint is y2 = 100: dsqr = (y2 - 100)^2
TRI_EX, TRI_EY = F(200), F(100)


def _tri_call(f2, want, th_low=50, stereo1=0, elig1=1, F12=TRI_F, node2=7, seed=0):
    """one keyframe-1 keypoint (node 7) against keyframe-2 keypoints f2 = [(distance, x2, y2, octave, stereo, eligible)] in
    FeatureVector order, in the layout proj_cases.tri_core_inputs returns"""
    rng = np.random.default_rng(900 + seed)
    sf = PC.scale_factors()
    base = H.random_rows(rng, 1)[0]
    n2 = len(f2)
    k1 = dict(desc=base[None], xy=np.array([[50, 60]], F), elig=np.array([elig1], np.uint8), stereo=np.array([stereo1], np.uint8),
              fv=H.csr({7: [0]}))
    k2 = dict(desc=np.stack([H.at_distance(rng, base, f[0]) for f in f2]) if n2 else np.zeros((0, 32), np.uint8),
              xy=np.array([(f[1], f[2]) for f in f2], F).reshape(-1, 2), octave=np.array([f[3] for f in f2], np.int32),
              stereo=np.array([f[4] for f in f2], np.uint8), elig=np.array([f[5] for f in f2], np.uint8),
              fv=H.csr({node2: list(range(n2))}) if n2 else H.csr({}), scale_factors=sf, level_sigma2=(sf * sf).astype(F))
    return dict(k1=k1, k2=k2, F12=np.asarray(F12, F), ex=TRI_EX, ey=TRI_EY, th_low=th_low, want=[want])


def _on(x=300.0, d=20, o=0, st=0, el=1, y=100.0):
    return (d, x, y, o, st, el)


def tri_dsqr_steps(o):
    """neighbouring y2 (y_in, y_out) with (double)dsqr < 3.84 * level_sigma2[o] at y_in and not at y_out, their dsqr, the bound"""
    sf = PC.scale_factors()
    bound = 3.84 * float(F(sf[o] * sf[o]))

    def dsqr(y):
        num = F(F(y) - F(100))
        return float(F(num * num))
    y_in, y_out = adjacent(F(100) + F(np.sqrt(bound)), lambda y: not dsqr(y) < bound)
    return y_in, y_out, dsqr(y_in), dsqr(y_out), bound


def x_threshold():
    """dist > th_low skips: dist == th_low matches, one bit more does not"""
    return dict(calls=[_tri_call([_on(d=50)], 0), _tri_call([_on(d=51)], -1, seed=1), _tri_call([_on(d=0)], -1, th_low=-1, seed=2),
                       _tri_call([_on(d=0)], 0, th_low=0, seed=3)], differ=[(0, 1), (2, 3)])


def x_tie():
    """dist > bestDist skips, so an equal distance takes over: of two keyframe-2 keypoints at one distance the LATER wins when
    both pass the gates, the earlier stays when the later fails the epipolar test or is one bit worse"""
    return dict(calls=[_tri_call([_on(300), _on(340)], 1), _tri_call([_on(300), _on(340, y=140.0)], 0, seed=1),
                       _tri_call([_on(300), _on(340, d=21)], 0, seed=2), _tri_call([_on(300, d=21), _on(340)], 1, seed=3),
                       _tri_call([_on(300), _on(340), _on(380)], 2, seed=4)], differ=[(0, 1), (0, 2)])


def x_epipole():
    """the epipole gate (both keypoints monocular): squared distance < 100 * scale_factors[o] skips; equality passes"""
    sf = PC.scale_factors()
    calls, differ = [], []
    for o in (0, 2):
        lim = F(F(100) * sf[o])

        def d2(x):
            dx = F(TRI_EX - F(x))
            return F(F(dx * dx) + F(0))
        x_in, x_out = adjacent(TRI_EX - F(np.sqrt(float(lim))), lambda x: d2(x) < lim)   # larger x = nearer the epipole
        k = len(calls)
        calls += [_tri_call([_on(x_in, o=o)], 0, seed=k), _tri_call([_on(x_out, o=o)], -1, seed=k + 1),
                  _tri_call([_on(x_out, o=o)], 0, stereo1=1, seed=k + 2), _tri_call([_on(x_out, o=o, st=1)], 0, seed=k + 3)]
        differ += [(k, k + 1), (k + 1, k + 2), (k + 1, k + 3)]
    # equality itself: 10 px from the epipole on level 0 is exactly 100
    calls += [_tri_call([_on(190.0)], 0, seed=20), _tri_call([_on(up(190.0))], -1, seed=21)]
    differ.append((len(calls) - 2, len(calls) - 1))
    return dict(calls=calls, differ=differ)


def x_epipolar_line():
    """(double)dsqr < 3.84 * level_sigma2[o]: y2 one step either side of the bound"""
    calls, differ = [], []
    for o in (0, 3, 7):
        y_in, y_out = tri_dsqr_steps(o)[:2]
        k = len(calls)
        calls += [_tri_call([_on(y=y_in, o=o)], 0, seed=k), _tri_call([_on(y=y_out, o=o)], -1, seed=k + 1)]
        differ.append((k, k + 1))
    return dict(calls=calls, differ=differ)


def x_zero_f():
    """F12 all zero: den == 0, CheckDistEpipolarLine is false, no match"""
    return dict(calls=[_tri_call([_on()], 0), _tri_call([_on()], -1, F12=np.zeros(9, F))], differ=[(0, 1)])


def x_eligibility():
    """a keypoint that is not eligible on either side is passed over"""
    return dict(calls=[_tri_call([_on(300, d=10), _on(340, d=20)], 0), _tri_call([_on(300, d=10, el=0), _on(340, d=20)], 1, seed=1),
                       _tri_call([_on(300, d=10), _on(340, d=20)], -1, elig1=0, seed=2)], differ=[(0, 1), (0, 2)])


def x_nodes():
    """a node present on one side only, and empty FeatureVectors"""
    empty = _tri_call([], -1, seed=2)
    empty["k1"]["fv"] = H.csr({})
    return dict(calls=[_tri_call([_on()], 0), _tri_call([_on()], -1, node2=8, seed=1), _tri_call([_on()], -1, node2=6, seed=1),
                       _tri_call([], -1, seed=2), empty], differ=[(0, 1), (0, 2)])


def x_sizes(n1):
    """n1 = 255, 256, 257 keyframe-1 keypoints around the 256-thread workgroup edge, on a seeded scene"""
    rng = np.random.default_rng(n1)
    k1, k2, F12 = PC.triangulation_case(rng, n1, 300, 12)
    a, b, ex, ey = PC.tri_core_inputs(k1, k2, False)
    return dict(calls=[dict(k1=a, k2=b, F12=F12, ex=ex, ey=ey, th_low=50, want=None)], differ=[])


TRI_CASES = dict(threshold=x_threshold, tie=x_tie, epipole=x_epipole, epipolar_line=x_epipolar_line, zero_f=x_zero_f,
                 eligibility=x_eligibility, nodes=x_nodes)
TRI_CASES.update({"sizes_%d" % n: (lambda n=n: x_sizes(n)) for n in (255, 256, 257)})


def run_tri(fn, c):
    return fn(c["k1"], c["k2"], c["F12"], c["ex"], c["ey"], c["th_low"])


TABLES = dict(WINDOW_CASES=WINDOW_CASES, GRID_CASES=GRID_CASES, SLAB_CASES=SLAB_CASES, DECISION_CASES=DECISION_CASES,
              GATE_CASES=GATE_CASES, ROUND_CASES=ROUND_CASES, TRI_CASES=TRI_CASES)

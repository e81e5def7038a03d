"""The rotation-histogram cases: angle pairs planted on the edges of the reference's binning (roundf at exact half bins, wraps
through +360) and of ComputeThreeMaxima (the binary32 0.1f * max1 boundary, equal counts).  For the prune kernels
(tests/test_gpu_matcher_edges.py) and for the host entry point that runs the same three-maxima code (tests/test_hostgeom.py)."""
import numpy as np

import hamming_cases as H


def _rotation_groups(groups):
    """groups: list of (count, kind, value): kind 'bin' -> rotations inside bin `value`, 'pair' -> the exact (a1, a2) pairs
    of H.HALF_BIN_ANGLES whose roundf bin is `value`.  Returns (qa, ta) for queries matched to train row i = query i."""
    rng = np.random.default_rng(sum(c for c, _, _ in groups))
    qa, ta = [], []
    for count, kind, v in groups:
        if kind == "bin":
            a1, a2, _ = H.angles_for_histogram(rng, [0] * v + [count])
            qa += list(a1)
            ta += list(a2)
        else:
            pairs = [(a1, a2) for a1, a2, b, _ in H.HALF_BIN_ANGLES if b == v]
            for j in range(count):
                qa.append(pairs[j % len(pairs)][0])
                ta.append(pairs[j % len(pairs)][1])
    perm = rng.permutation(len(qa))
    return np.asarray(qa, np.float32)[perm], np.asarray(ta, np.float32)[perm]


ROTATION_CASES = {
    # half-bin groups outvote a neighbour only under roundf; under rintf they would join the bin below
    "half15": [(40, "pair", 1), (35, "bin", 0), (30, "bin", 3), (25, "bin", 5), (20, "bin", 7)],
    "half135": [(40, "pair", 5), (35, "bin", 4), (30, "bin", 8), (25, "bin", 10), (20, "bin", 2)],
    "half255": [(60, "pair", 9), (50, "bin", 8), (45, "bin", 11), (40, "bin", 0), (5, "bin", 12)],
    # ComputeThreeMaxima: max2 == 0.1f * max1 keeps the second maximum, max3 likewise
    "max2_edge": [(100, "bin", 2), (10, "bin", 6), (9, "bin", 12)],
    "max3_edge": [(200, "bin", 12), (150, "bin", 1), (20, "bin", 6), (19, "bin", 3)],
    "max2_below": [(100, "bin", 4), (9, "bin", 7)],
    # equal counts: the earliest bins win
    "equal": [(70, "bin", 11), (70, "bin", 3), (70, "bin", 9), (70, "bin", 7), (30, "bin", 0)],
}
# matches that survive the prune (every planted pair matches): roundf and binary32 0.1f * max1 as the reference computes
# them; rintf would keep 130 / 130 / 195 of the half-bin cases, a double 0.1 * max1 100 of max2_edge and 350 of max3_edge
ROTATION_KEPT = {"half15": 105, "half135": 105, "half255": 155, "max2_edge": 110, "max3_edge": 370, "max2_below": 100,
                 "equal": 210}

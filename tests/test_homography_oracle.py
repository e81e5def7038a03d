"""tests/homography_oracle.py checked on its own (CPU): it recovers known homographies from clean and contaminated planar
pairs, its JacobiImpl_ agrees with numpy.linalg.eigh, RANSACUpdateNumIters gives the textbook values, and its RNG stream and
getSubset draws equal a C twin compiled here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import homography_cases as HC
import homography_oracle as HO

# dyadic affine map: every dst coordinate of an integer src point is exact in float32
H_EXACT = np.array([[1.25, 0.125, 3.5], [-0.0625, 0.875, -2.25], [0.0, 0.0, 1.0]])


def _exact_pairs(n, seed, outliers=0.0):
    rng = np.random.default_rng(seed)
    src = np.round(rng.random((n, 2)) * [640, 480])
    dst = src @ H_EXACT[:2, :2].T + H_EXACT[:2, 2]
    inl = np.ones(n, bool)
    bad = rng.permutation(n)[:int(round(n * outliers))]
    inl[bad] = False
    dst[bad] = np.round(rng.random((len(bad), 2)) * [640, 480]) + 100.5   # far from the plane
    return src.astype(np.float32), dst.astype(np.float32), inl


@pytest.mark.parametrize("method", [HO.RANSAC, 0])
def test_recovers_noise_free_homography(method):
    s, d, _ = _exact_pairs(200, 1)
    H, mask = HO.find_homography(s, d, method=method)
    assert np.abs(H - H_EXACT).max() <= 1e-9 * np.abs(H_EXACT).max()
    assert mask.all()


def test_recovers_with_30_percent_outliers_and_mask_is_the_inlier_set():
    s, d, inl = _exact_pairs(300, 2, outliers=0.3)
    H, mask = HO.find_homography(s, d)
    assert np.abs(H - H_EXACT).max() <= 1e-9 * np.abs(H_EXACT).max()
    assert np.array_equal(mask.astype(bool), inl)


def test_projective_recovery_from_float_pairs():
    s, d, inl = HC.planar(400, 0.7, 3, noise=0.0)
    H, mask = HO.find_homography(s, d)
    assert np.abs(H - HC.H_TRUE).max() < 1e-4
    assert np.array_equal(mask.astype(bool), inl)


@pytest.mark.parametrize("n", [8, 9])
def test_jacobi_agrees_with_eigh(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        A = rng.normal(size=(n, n))
        A = A @ A.T if _ % 2 else A + A.T
        W, V = HO.jacobi(A)
        w, v = np.linalg.eigh(A)
        assert np.all(np.diff(W) <= 0)
        assert np.allclose(W, w[::-1], rtol=1e-12, atol=1e-12 * np.abs(w).max())
        for k in range(n):
            vk = v[:, n - 1 - k]
            assert min(np.abs(V[k] - vk).max(), np.abs(V[k] + vk).max()) < 1e-9


def test_update_num_iters():
    assert HO.update_num_iters(0.995, 0.5, 4, 2000) == 82
    assert HO.update_num_iters(0.995, 1.0, 4, 2000) == 2000    # log(denom) = 0
    assert HO.update_num_iters(0.995, 0.95, 4, 2000) == 2000   # more than maxIters needed
    assert HO.update_num_iters(0.995, 0.9, 4, 7) == 7
    assert HO.update_num_iters(0.995, 0.0, 4, 2000) == 0       # denom < DBL_MIN
    assert HO.update_num_iters(0.99, 0.2, 4, 2000) == 9


def test_degenerate_cases():
    c = HC.table(64)
    for name in ("collinear", "zero_spread_method_0", "zero_spread_n4", "n_3", "n_0"):
        s, d, kw = c[name]
        H, mask = HO.find_homography(s, d, **kw)
        assert H is None and not mask.any(), name
    r = HO.ransac(*c["collinear"][:2])
    assert not r["ok"] and r["iters"] == 0


TWIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <math.h>
#include <float.h>
static uint64_t state = (uint64_t)-1;
static unsigned next_(void) { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
static int uniform(int a, int b) { return a == b ? a : (int)(next_() % (unsigned)(b - a) + a); }
static float px[4096], py[4096], qx[4096], qy[4096];
static int collinear(const float *x, const float *y, const int *idx) {
    int i = 3;
    for (int j = 0; j < i; j++) {
        double dx1 = x[idx[j]] - x[idx[i]], dy1 = y[idx[j]] - y[idx[i]];
        for (int k = 0; k < j; k++) {
            double dx2 = x[idx[k]] - x[idx[i]], dy2 = y[idx[k]] - y[idx[i]];
            if (fabs(dx2*dy1 - dy2*dx1) <= FLT_EPSILON*(fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return 1;
        }
    }
    return 0;
}
int main(int argc, char **argv) {
    int ndraw = atoi(argv[1]), count, nsub = atoi(argv[2]);
    for (int i = 0; i < ndraw; i++) printf("%u\n", next_());
    state = (uint64_t)-1;
    if (scanf("%d", &count) != 1) return 1;
    for (int i = 0; i < count; i++) if (scanf("%f %f %f %f", &px[i], &py[i], &qx[i], &qy[i]) != 4) return 1;
    for (int s = 0; s < nsub; s++) {
        int idx[4], i = 0, iters = 0;
        for (; iters < 10000; iters++) {
            for (i = 0; i < 4 && iters < 10000;) {
                int v;
                for (;;) { int j; v = idx[i] = uniform(0, count); for (j = 0; j < i; j++) if (v == idx[j]) break; if (j == i) break; }
                i++;
            }
            if (i == 4 && (collinear(px, py, idx) || collinear(qx, qy, idx))) continue;
            break;
        }
        if (i == 4 && iters < 10000) printf("%d %d %d %d\n", idx[0], idx[1], idx[2], idx[3]); else printf("fail\n");
    }
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_rng_and_get_subset_equal_c_twin(tmp_path):
    src = tmp_path / "twin.c"
    exe = tmp_path / "twin"
    src.write_text(TWIN)
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", str(src), "-lm", "-o", str(exe)])
    s, d, _ = HC.planar(60, 0.5, 4)
    s[10:20] = s[0]   # duplicates: collinear rejections inside the draws
    d[10:20] = d[0]
    inp = f"{len(s)}\n" + "".join(f"{a!r} {b!r} {c!r} {e!r}\n" for (a, b), (c, e) in zip(s.tolist(), d.tolist()))
    out = subprocess.run([str(exe), "10000", "500"], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in out[:10000]] == HO.rng_stream(10000).tolist()
    rng = HO.RNG()
    sl = [(float(a), float(b)) for a, b in s]
    dl = [(float(a), float(b)) for a, b in d]
    for k in range(500):
        got = HO.get_subset(sl, dl, rng)
        assert out[10000 + k] == (" ".join(map(str, got)) if got is not None else "fail"), k


def test_threshold_boundary_case_separates_float_from_double_error():
    """computeError is float: on this case a double error would change the RANSAC mask"""
    s, d = HC.threshold_boundary()
    r = HO.ransac(s, d)
    h = r["H"]
    M, m = s.astype(np.float64), d.astype(np.float64)
    ww = 1 / (h[6] * M[:, 0] + h[7] * M[:, 1] + 1)
    ed = ((h[0] * M[:, 0] + h[1] * M[:, 1] + h[2]) * ww - m[:, 0]) ** 2 + ((h[3] * M[:, 0] + h[4] * M[:, 1] + h[5]) * ww - m[:, 1]) ** 2
    assert np.array_equal(r["mask"], HO.compute_error(s, d, h) <= np.float32(9))
    assert np.count_nonzero(r["mask"] != (ed <= 9)) >= 5

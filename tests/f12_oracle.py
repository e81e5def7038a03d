"""numpy restatement of csrc/orbfe_f12.h, function by function under the same names: what LocalMapping::CreateNewMapPoints
computes per neighbour before SearchForTriangulation (src/LocalMapping.cc:390-417, :848-867; src/ORBmatcher.cc:833-843), as
OpenCV 3.2 evaluates the cv::Mat expressions.  LocalMapping.cc is not among the compiled reference sources, so nothing pins this
file to a compiled body (like tests/geometry_oracle.py); the epipole alone is pinned, through tests/proj_cases.py::tri_core_inputs.

Every float operation is one np.float32 operation, every double one a Python float operation."""
import numpy as np

f32 = np.float32


def geo_gemm_store(t):
    """cv::gemm's float shortcut: (float)(t * alpha + c * beta), alpha = 1, c = 0, beta = 0, in double"""
    return f32(float(t) * 1.0 + 0.0 * 0.0)


def geo_inv3(S):
    """cv::invert, 3x3 CV_32F: determinant and cofactors in double"""
    s = [float(v) for v in np.asarray(S, f32).reshape(9)]
    d = s[0] * (s[4] * s[8] - s[5] * s[7]) - s[1] * (s[3] * s[8] - s[5] * s[6]) + s[2] * (s[3] * s[7] - s[4] * s[6])
    if d == 0.0:
        return np.zeros(9, f32)
    d = 1.0 / d
    return np.array([(s[4] * s[8] - s[5] * s[7]) * d, (s[2] * s[7] - s[1] * s[8]) * d, (s[1] * s[5] - s[2] * s[4]) * d,
                     (s[5] * s[6] - s[3] * s[8]) * d, (s[0] * s[8] - s[2] * s[6]) * d, (s[2] * s[3] - s[0] * s[5]) * d,
                     (s[3] * s[7] - s[4] * s[6]) * d, (s[1] * s[6] - s[0] * s[7]) * d, (s[0] * s[4] - s[1] * s[3]) * d], f32)


def f12_dot3(a0, b0, a1, b1, a2, b2):
    return f32(f32(f32(a0 * b0) + f32(a1 * b1)) + f32(a2 * b2))


def f12_mul33(A, B):
    return np.array([geo_gemm_store(f12_dot3(A[i * 3], B[j], A[i * 3 + 1], B[3 + j], A[i * 3 + 2], B[6 + j]))
                     for i in range(3) for j in range(3)], f32)


def f12_compute(T1, T2, fx, fy, cx, cy):
    """F12 [9] from two poses [12] (row-major 3x4) and the shared pinhole parameters"""
    T1, T2 = np.asarray(T1, f32).reshape(12), np.asarray(T2, f32).reshape(12)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    R12 = np.zeros(9, f32)
    for i in range(3):           # R1w * R2w.t(): GEMM_2_T, double accumulation
        for j in range(3):
            s0 = 0.0
            for k in range(3):
                s0 += float(T1[i * 4 + k]) * float(T2[j * 4 + k])
            s0 += (0.0 + 0.0) + 0.0
            R12[i * 3 + j] = f32(s0 * 1.0)
    t12 = np.zeros(3, f32)
    for i in range(3):           # gemm(R12, t2w, -1, t1w, 1): the shortcut with alpha and beta
        t = f12_dot3(R12[i * 3], T2[3], R12[i * 3 + 1], T2[7], R12[i * 3 + 2], T2[11])
        t12[i] = f32(float(t) * -1.0 + float(T1[i * 4 + 3]) * 1.0)
    z = f32(0)
    tx = np.array([z, -t12[2], t12[1], t12[2], z, -t12[0], -t12[1], t12[0], z], f32)
    K1t = np.array([fx, 0, 0, 0, fy, 0, cx, cy, 1], f32)
    K2 = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], f32)
    return f12_mul33(f12_mul33(f12_mul33(geo_inv3(K1t), tx), R12), geo_inv3(K2))


def f12_epipole(T2, Ow1, fx, fy, cx, cy):
    T2, C = np.asarray(T2, f32).reshape(12), np.asarray(Ow1, f32).reshape(3)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    C2 = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        for y in range(3):
            s = f32(0)
            for k in range(3):
                s = f32(s + f32(T2[y * 4 + k] * C[k]))
            C2[y] = f32(s + T2[y * 4 + 3])
        invz = f32(f32(1.0) / C2[2])
        return f32(f32(f32(fx * C2[0]) * invz) + cx), f32(f32(f32(fy * C2[1]) * invz) + cy)


def f12_baseline(Ow1, Ow2):
    """cv::norm(Ow2 - Ow1) as the float the reference stores"""
    s = 0.0
    for k in range(3):
        v = f32(f32(Ow2[k]) - f32(Ow1[k]))
        s += float(v) * float(v)
    return f32(np.sqrt(s))


def f12_baseline_skip(Ow1, Ow2, mono, mb, median_depth2):
    b = f12_baseline(Ow1, Ow2)
    if not mono:
        return bool(b < f32(mb))
    with np.errstate(all="ignore"):
        return bool(float(f32(b / f32(median_depth2))) < 0.01)

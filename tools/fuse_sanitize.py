"""Build tools/fuse_sanitize.hip -- the host path of trk_gate_fuse (csrc/orbfe_track_geom.h), a stand-alone program -- with
-fsanitize=address,undefined (host code only, no GPU, nothing loaded into Python), run it over the CPU cases of tests/fuse_cases.py
(the fuse_case seeds under both poses and the planted edges) and compare every line with tests/fuse_oracle.py.  Exit status 0 =
clean and equal."""
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import fuse_cases as FC  # noqa: E402
import fuse_oracle as FO  # noqa: E402
from orb_slam2_ssd_semantic_amd import _build  # noqa: E402

f32 = np.float32
SEEDS = (0, 1, 2, 5, 6, 9, 10, 11, 14, 15)


def cases():
    out = []
    for seed in SEEDS:
        kf, mps, th = FC.seed_case(seed)
        for mode, Scw in ((FO.PLAIN, None), (FO.SIM3, FC.scw_of(kf, 1.7))):
            T, Ow = FC.pose_of(kf, mode, Scw)
            out.append((T, Ow, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], mps["world_pos"], mps["normal"], mps["min_dist"],
                        mps["max_dist"], mode))
    p = FC.planted_gate()
    arr = [np.array([c[k] for c in p], f32) for k in (1, 2, 3, 4)]
    for mode in (FO.PLAIN, FO.SIM3):
        out.append((FC.IDENTITY, np.zeros(3, f32), FC.K0, FC.BOUNDS0, 3.0, FC.SF, FC.LOG_SF, arr[0], arr[1], arr[2], arr[3], mode))
    return out


def pack(c):
    T, Ow, K, bounds, th, sf, log_sf, wp, nr, mn, mx, mode = c
    head = np.concatenate([np.asarray(v, f32).reshape(-1) for v in (T, Ow, K[:5], bounds, [th], [log_sf])])
    assert len(head) == 26
    sf = np.asarray(sf, f32)
    return (head.tobytes() + struct.pack("<iii", len(sf), mode, len(mn)) + sf.tobytes() + np.asarray(wp, f32).tobytes() + np.asarray(nr, f32).tobytes() +
            np.asarray(mn, f32).tobytes() + np.asarray(mx, f32).tobytes())


def main():
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "fuse_sanitize"), os.path.join(tmp, "cases.bin")
        cmd = [_build.hipcc(), "-x", "hip", "--cuda-host-only", f"--offload-arch={_build.ARCH}", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", _build.CSRC,
               os.path.join(ROOT, "tools", "fuse_sanitize.hip"), "-o", exe]
        subprocess.run(cmd, check=True)
        with open(data, "wb") as f:
            f.write(struct.pack("<i", len(cs)) + b"".join(pack(c) for c in cs))
        r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print("sanitizer run failed: exit status %d" % r.returncode)
            return 1
    lines = r.stdout.splitlines()
    want = []
    for T, Ow, K, bounds, th, sf, log_sf, wp, nr, mn, mx, mode in cs:
        q, level, ok = FO.gate_points(np.asarray(T, f32).reshape(3, 4), Ow, K, bounds, th, sf, log_sf, np.asarray(wp, f32).reshape(-1, 3),
                                      np.asarray(nr, f32).reshape(-1, 3), mn, mx, mode == FO.PLAIN)
        want += ["%d %d " % (ok[i], level[i]) + " ".join("%08x" % w for w in q[i]) for i in range(len(ok))]
    bad = len(lines) != len(want) or sum(a != b for a, b in zip(lines, want))
    print("%d points of %d lists under address + undefined-behaviour sanitizers: %s differ from the oracle" % (len(want), len(cs), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

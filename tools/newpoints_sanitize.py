"""Build tools/newpoints_sanitize.hip -- the host path of csrc/orbfe_newpoints.h and the round planner, a stand-alone program --
with -fsanitize=address,undefined (host code only, no GPU, nothing loaded into Python), run it over the CPU cases of
tests/newpoints_cases.py and compare every line with tests/newpoints_oracle.py.  Exit status 0 = clean and equal."""
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import newpoints_cases as NC  # noqa: E402
import newpoints_oracle as NO  # noqa: E402
from orb_slam2_ssd_semantic_amd import _build  # noqa: E402

f32 = np.float32


def pack(args):
    T1, O1, T2, O2, cam, mb, k1, k2, sf, s2, scale_factor = args
    def key(k):
        return [k["ux"], k["uy"], k["rx"], k["ry"], k["depth"], k["uright"]]
    fl = np.concatenate([np.asarray(v, f32).reshape(-1) for v in (T1, O1, T2, O2, [cam[c] for c in ("fx", "fy", "cx", "cy", "bf")], [mb], key(k1),
                                                                    key(k2), sf, s2, [scale_factor])])
    assert len(fl) == 65
    return fl.astype(f32).tobytes() + struct.pack("<ii", k1["octave"], k2["octave"])


def main():
    cases = [c["args"] for c in NC.planted()]
    for seed in NC.SEEDS:
        frames, pairs, _, _, _, _ = NC.scene_matches(seed)
        cases += [NC.match_args(frames, 0, 1, a, b) for a, b in pairs]
    rng = np.random.default_rng(9)
    lists = [([], [])] + [(rng.integers(0, 9, P), rng.integers(0, 9, P)) for P in rng.integers(1, 60, 40)]
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "newpoints_sanitize"), os.path.join(tmp, "cases.bin")
        cmd = [_build.hipcc(), "-x", "hip", "--cuda-host-only", f"--offload-arch={_build.ARCH}", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", _build.CSRC,
               os.path.join(ROOT, "tools", "newpoints_sanitize.hip"), "-o", exe]
        subprocess.run(cmd, check=True)
        with open(data, "wb") as f:
            f.write(struct.pack("<i", len(cases)) + b"".join(pack(c) for c in cases))
            f.write(struct.pack("<i", len(lists)))
            for k1, k2 in lists:
                f.write(struct.pack("<i", len(k1)) + np.asarray(k1, np.int32).tobytes() + np.asarray(k2, np.int32).tobytes())
        r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            print("sanitizer run failed: exit status %d" % r.returncode)
            return 1
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) + len(lists)
    bad = 0
    for j, (c, line) in enumerate(zip(cases, lines)):
        v, x = NO.triangulate_match(*c)
        z = NO.np_cam_coord(np.asarray(c[0], f32).reshape(12), 2, x)
        want = "%d %08x %08x %08x %08x" % ((v,) + tuple(int(b) for b in np.asarray(x, f32).view(np.uint32)) + (int(f32(z).view(np.uint32)),))
        if v == NO.W_ZERO:
            want, line = want[:1], line[:1]
        bad += want != line
    for (k1, k2), line in zip(lists, lines[len(cases):]):
        r_of, order, off = NO.plan_rounds(k1, k2)
        want = "%d | %s | %s | %s" % (len(off) - 1, " ".join(map(str, r_of)), " ".join(map(str, order)), " ".join(map(str, off)))
        bad += " ".join(want.split()) != " ".join(line.split())
    print("%d matches and %d pair lists under address + undefined-behaviour sanitizers: %d differ from the oracle" % (len(cases), len(lists), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

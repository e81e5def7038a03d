"""Are the gfx950 kernels of two source trees the same code?  For refactors that move kernels between files.
usage: python tools/kernel_asm_diff.py OLD_TREE [NEW_TREE] [-- extra hipcc flags, e.g. -DORBFE_DEVELOPER]

Compiles every csrc/*.hip of both trees to device assembly with the flags of _build.py (needs hipcc, no GPU), cuts the output
per function symbol and compares, by demangled name: the set of kernels, every function's instruction text and every
kernel's .amdhsa_ block (registers, LDS, scratch).  Comment lines are dropped; block labels are numbered per function (the
compiler numbers them per file), and the per-file hash in the names of anonymous-namespace kernels is blanked.  Exit 0 = identical."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from orb_slam2_ssd_semantic_amd import _build  # noqa: E402

FLAGS = [*_build.FLAGS, "--cuda-device-only", "-S", "-w"]   # what ships, stopped at the device assembly, warnings off


def assembly(tree, extra, tmp):
    csrc = os.path.join(tree, "orb_slam2_ssd_semantic_amd", "csrc")

    def one(src):
        out = os.path.join(tmp, os.path.basename(src) + ".s")
        subprocess.check_call([_build.hipcc(), *FLAGS, *extra, "-I", os.path.join(tree, "include"), "-I", csrc, src, "-o", out])
        return open(out).read()

    with ThreadPoolExecutor(min(_build.MAX_COMPILES, os.cpu_count() or 1)) as ex:
        return list(ex.map(one, sorted(glob.glob(os.path.join(csrc, "*.hip")))))


def demangle(names):
    out = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.split("\n")))


def functions(text):
    """{symbol: [normalised lines]} for every function, {symbol: [.amdhsa_ lines]} for every kernel"""
    text = re.sub(r"__hip_cuid_[0-9a-f]+|(?<=_GLOBAL__N_)[A-Za-z0-9_]*?[0-9a-f]{8,}(?=[A-Z_0-9])", "CUID", text)
    lines = text.split("\n")
    funcs, desc, cur, hsa = {}, {}, None, None
    for l in lines:
        t = l.split(";")[0].rstrip() if not l.lstrip().startswith(".ascii") and not l.lstrip().startswith(".asciz") else l.rstrip()
        if not t.strip():
            continue
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", t)
        if m:
            cur = m.group(1)
            funcs[cur] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", t)
        if m:
            hsa = m.group(1)
            desc[hsa] = []
        elif hsa is not None:
            if ".end_amdhsa_kernel" in t:
                hsa = None
            else:
                desc[hsa].append(t.strip())
        elif cur is not None:
            if re.match(r"\s*\.size\s+" + re.escape(cur) + r"\b", t):
                cur = None
            elif not (re.match(r"\s*\.(loc|file|cfi_|p2align|globl|protected|weak|hidden|section|text)\b", t) or re.match(r"\.L(tmp|func_)", t)):
                funcs[cur].append(re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", t).strip())
    return funcs, desc


def collect(tree, extra):
    funcs, desc = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for text in assembly(tree, extra, tmp):
            f, d = functions(text)
            for k, v in f.items():
                assert k not in funcs or funcs[k] == v, f"{k}: defined twice, differently, in {tree}"
                funcs[k] = v
            desc.update(d)
    dm = demangle(sorted(funcs))
    return {dm[k]: v for k, v in funcs.items()}, {dm[k]: v for k, v in desc.items()}


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    old, new = argv[0], argv[1] if len(argv) > 1 else HERE
    (fa, da), (fb, db) = collect(old, extra), collect(new, extra)
    bad = 0
    for what, a, b in (("kernel", da, db), ("function", fa, fb)):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                print(f"{what} only in {'new' if k in b else 'old'}: {k}")
                bad += 1
            elif a[k] != b[k]:
                n = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
                print(f"{what} differs: {k}\n   old[{n}]: {a[k][n] if n < len(a[k]) else '<end>'}\n   new[{n}]: {b[k][n] if n < len(b[k]) else '<end>'}")
                bad += 1
    print(f"{len(da)} kernels / {len(fa)} functions in old, {len(db)} / {len(fb)} in new, flags {' '.join(extra) or '(release)'}: "
          + ("all identical" if not bad else f"{bad} DIFFERENCES"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

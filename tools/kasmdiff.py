#!/usr/bin/env python3
"""Device code of two trees, kernel by kernel:  tools/kasmdiff.py [--rename OLD=NEW ...] OTHER_CSRC_DIR unit [unit ...]   (units: k_momrk k_stencil ...)
Compiles every unit of this tree's cales_amd/csrc and of OTHER_CSRC_DIR (cales_amd/csrc INSIDE a full checkout of the commit to compare with, e.g. a
git worktree: common.hpp includes ../../include/cales.h) to gfx950 assembly, FP64 and
-DCALES_SINGLE, and compares per kernel: the same set of kernels, the same instructions between a symbol's label and its .Lfunc_end (comments
and section directives dropped, the function index of local labels removed: a refactor of the host side may change the ORDER in which the kernels
are emitted, and a kernel moved into a header as an inline function the SECTION it is emitted into) and the same
.amdhsa_ resource lines. Exit status 1 when anything differs. No GPU needed.

Kernels are paired by their demangled name without the argument list (`k_spec_x<true>`). --rename OLD=NEW, repeated, pairs the kernel OLD of the other
tree with NEW of this one (an OLD given twice: the NEW that this tree has, as where a name spells the precision); a unit written HERE=OTHER1+OTHER2 compares this tree's unit HERE with the kernels of the other tree's units OTHER1 and OTHER2
together. Of a pair that differs both instruction counts and the .amdhsa_ lines that differ are printed."""
import os, re, subprocess, sys, tempfile

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cales_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
SP = ["-DCALES_SINGLE", "-Wno-c++11-narrowing", "-Wno-implicit-const-int-float-conversion"]


def kernels(path):
    """{kernel name: (instruction lines, .amdhsa_ lines)}"""
    body, res, cur, hsa = {}, {}, None, None
    lines = open(path).readlines()
    names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel")}      # (kernels inside extern "C" keep their plain names)
    for line in lines:
        t = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        m = re.match(r"(\w+):$", t)
        if m and m.group(1) not in names: m = None
        if t.startswith(".amdhsa_kernel"): hsa = t.split()[1]; res[hsa] = []      # (the descriptor sits between the label and .Lfunc_end)
        elif t.startswith(".end_amdhsa_kernel"): hsa = None
        elif hsa is not None: res[hsa].append(t)
        elif m and cur is None: cur = m.group(1); body[cur] = []
        elif cur is not None and t.startswith(".Lfunc_end"): cur = None
        elif cur is not None and t.startswith((".text", ".section")): pass      # (where the code goes, not what it is: a kernel defined inline in a header sits in a section of its own)
        elif cur is not None and t: body[cur].append(t)
    syms = [k for k in body if k in res]      # (kernels only: device functions have no descriptor)
    plain = subprocess.run(["c++filt"] + syms, capture_output=True, text=True).stdout.split("\n") if syms else []
    # the symbol itself occurs in its own code (the address of the kernarg segment, the end label): replaced by the name, which a renamed pair shares
    return {re.sub(r"^void ", "", p.split("(")[0]): ([l.replace(k, "KERNEL") for l in body[k]], [l.replace(k, "KERNEL") for l in res[k]]) for k, p in zip(syms, plain)}


def main():
    args, rename = sys.argv[1:], []
    while args and args[0] == "--rename":
        rename.append(tuple(x.strip() for x in args[1].split("=", 1))); args = args[2:]
    other, units, bad = args[0], args[1:], 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            here, _, theirs = unit.partition("=")
            for prec, extra in (("fp64", []), ("fp32", SP)):
                ks = []
                for tag, src, names in (("a", HERE, [here]), ("b", other, (theirs or here).split("+"))):
                    ks.append({})
                    for name in names:
                        out = os.path.join(tmp, f"{name}.{prec}.{tag}.s")
                        r = subprocess.run(["/opt/rocm/bin/hipcc", "-w"] + FLAGS + extra + [name + ".hip", "-o", out], cwd=src, capture_output=True, text=True)
                        if r.returncode: sys.exit(f"compiling {name}.hip in {src} ({prec}) failed:\n{r.stderr}")
                        ks[-1].update(kernels(out))
                ks[1] = {next((new for old, new in rename if old == k and new in ks[0]), k): v for k, v in ks[1].items()}
                diff = sorted(set(ks[0]) ^ set(ks[1])) + sorted(k for k in set(ks[0]) & set(ks[1]) if ks[0][k] != ks[1][k])
                print(f"{unit} {prec}: {len(ks[0])} / {len(ks[1])} kernels, {len(diff)} differ")
                for k in diff:
                    if k not in ks[0] or k not in ks[1]: print("   ", k, "-- only in", "this tree" if k in ks[0] else "the other tree"); continue
                    (ia, ra), (ib, rb) = ks[0][k], ks[1][k]
                    print("   ", k, f"-- {len(ia)} / {len(ib)} instructions" + ("" if ia != ib else ", identical"))
                    for la, lb in zip(ra, rb):
                        if la != lb: print("       ", la, "/", lb.split()[-1])
                bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

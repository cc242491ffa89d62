#!/usr/bin/env python3
"""Generates tests/golden/local/*.npz -- states from the REFERENCE ITSELF built NOT to average the Germano identity of the dynamic model at all
(src/sgs.f90:368-377, _CAVITY): visct = max(|S| MijLij / MijMij, 0) cell by cell.

  local       -D_CAVITY. The branch sits behind `#elif defined(_CHANNEL)` and sgs.f90 defines _CHANNEL at its head, so the flag alone cannot reach it:
              as for the x lines of gen_golden_average.py the committed recipe oracle/ref/Makefile gets REF = a temporary directory of links to the
              reference's sources in which sgs.f90 is the reference's file minus that one line (gen_golden_average.build_variant does both).
  local_f2d   the same with -D_FILTER_2D (the plane filter, tests/golden/gen_golden_filter2d.py).

The builds go to oracle/_ref/{cavity,cavity_f2d}, beside the default build and out of history like it. oracle.ref.refpy.REFDIR is pointed there IN MEMORY
and the cases run through gen_golden.run_case -- the same names, edits, operator sequence and keys as the plane-averaged goldens. Every file carries the
extra key `dsmag_average` = 'local', the plane-filter one `filter2d = 1` too. Files: local/<variant>_<case>.npz with a manifest of their own. Like
gen_golden.py it runs only where the reference tree exists.

The clip max(.,0) (sgs.f90:377) hides every error of a cell it has zeroed, so the generator requires of every file: every *_visct key finite (no cell
with 0/0), and more than two fifths of the interior cells of r3_s9_visct non-zero (the reference gives 0.46-0.55 on these cases).

Usage:  python tests/golden/gen_golden_local.py                        # builds the variants, all cases (one subprocess per case), manifest
        python tests/golden/gen_golden_local.py --variant V --case NAME
        python tests/golden/gen_golden_local.py --noise-seeds              # how much more the un-averaged reference moves under a perturbation (prints only)

--noise-seeds: tests/test_gpu_dsmag_local.py compares the tile form of the device code with the kernel-per-loop sequence on the case's initial field
plus 2 % white noise (tests/test_gpu_filter2d.py, _shaped_case and _fields). There the local field is spiky -- cells with a small MijMij -- and a
pointwise ratio answers round-off differences of its operands more strongly than a ratio of plane sums. How much more is measured on the REFERENCE: for
each shape of NOISE_SHAPES and each seed 1..12 one cmpt_sgs of the -D_CAVITY build and one of the default (plane-averaged) build on the test's field, and
each again with u, v, w changed by a relative 1e-14 (uniform numbers in [-1, 1) of RandomState(1000 + seed), the same for both builds). Printed: both
responses in the metric of tests/util.py relerr (maximum difference over the field maximum) and their ratio A, local over planes. The test's bar is
1e-11 max(1, A) for the seed with the smallest A; the test file quotes the lines it takes from this list.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
import gen_golden_average as GA  # noqa: E402
from gen_golden_filter2d import FILE_LIMIT, save  # noqa: E402

ROOT = gen_golden.ROOT
OUT = os.path.join(HERE, "local")
# variant: (value of dsmag_average, plane filter, directory under oracle/_ref, extra flags, stage-by-stage cases, end-of-step cases)
VARIANTS = {
    "local": ("local", False, "cavity", "-D_CAVITY", ("cavity_dsmag", "cavity_dsmag_wm_mixed", "tgv_dsmag_ppp", "chan_dsmag", "chan_dsmag_wm", "duct_dsmag"),
              ("tgv_dsmag_ppp_x64", "chan_dsmag_x64")),
    "local_f2d": ("local", True, "cavity_f2d", "-D_CAVITY -D_FILTER_2D", ("chan_dsmag",), ()),
}
DEFAULT_REFDIR = os.path.join(ROOT, "oracle", "_ref")      # the plane-averaged build of oracle/ref/Makefile (refpy's own default)


def refdir(variant):
    return os.path.join(ROOT, "oracle", "_ref", VARIANTS[variant][2])


def build_variant(variant):
    """gen_golden_average.build_variant with this file's table: its `xlines` branch is the removal of the `#define _CHANNEL` line, which _CAVITY needs too."""
    _, f2d, sub, flags, stages, end = VARIANTS[variant]
    key = "_local_build_" + variant
    GA.VARIANTS[key] = ("xlines", f2d, sub, flags, stages, end)      # (in memory, for the one call)
    try:
        GA.build_variant(key)
    finally:
        del GA.VARIANTS[key]


def live_cells(visct):
    """(interior cells with a non-zero value, interior cells) of a haloed eddy-viscosity field"""
    inner = visct[1:-1, 1:-1, 1:-1]
    return int((inner != 0.).sum()), inner.size


def run_case(variant, name):
    from oracle.ref import refpy
    ave, f2d, _, _, stages, end = VARIANTS[variant]
    assert name in stages + end, (variant, name)
    refpy.REFDIR = refdir(variant)
    out = os.path.join(OUT, variant + "_" + name + ".npz")
    gen_golden.run_case(name, out)
    G = dict(np.load(out))
    G["dsmag_average"] = np.array(ave)
    if f2d:
        G["filter2d"] = np.array(1)
    assert G["r3_div"][1] < 1e-12, (name, G["r3_div"])
    for k in G:
        if k.endswith("_visct"):
            assert np.isfinite(G[k]).all(), (variant, name, k, "a cell with 0/0")
    live, nc = live_cells(G["r3_s9_visct"])
    assert 5 * live > 2 * nc, (variant, name, "clipped cells hide errors", live, nc)
    save(out, G)
    assert os.path.getsize(out) <= FILE_LIMIT, (out, os.path.getsize(out))
    print(variant, name, f"cells with a coefficient: {live} of {nc} ({live / nc:.2f})", "divmax", float(G["r3_div"][1]), "file KB:", os.path.getsize(out) // 1024, flush=True)


# (golden whose input.nml is used, grid): the shapes of test_tile_form_equals_the_sequence in tests/test_gpu_dsmag_local.py
NOISE_SHAPES = [("chan_dsmag", (64, 16, 12)), ("chan_dsmag_wm", (64, 16, 12)), ("chan_dsmag", (126, 20, 9)), ("tgv_dsmag_ppp", (64, 16, 16)), ("duct_dsmag", (64, 12, 12))]


def noise_run(index, seed, local, perturbed):
    """One cmpt_sgs of one build of the reference on the field of _fields(_shaped_case(name, ng), seed), optionally perturbed; the interior field goes to
    stdout's last line as the path of an .npy file."""
    from cales_amd.hotpath import initflow
    from cales_amd.nml import parse_text
    from oracle.ref import refpy
    name, ng = NOISE_SHAPES[index]
    text = str(np.load(os.path.join(HERE, name + ".npz"))["input_nml"])
    case = parse_text(text)
    case.ng[:] = ng
    text = re.sub(r"ng\(1:3\) = .*", "ng(1:3) = %d, %d, %d" % ng, text)
    if np.any(case.lwm != 0):      # (_shaped_case: the sampling height stays above the first cell)
        case.hwm = max(float(case.hwm), 1.6 * max(float(case.l[d]) / ng[d] for d in range(3) if case.lwm[:, d].any()))
        text = re.sub(r"hwm = .*", "hwm = %r" % case.hwm, text)
    if case.inivel == "hcp":
        case.inivel = "poi"
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(seed)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    if perturbed:
        rng = np.random.RandomState(1000 + seed)
        for a in (u, v, w):
            a *= 1. + 1e-14 * (2. * rng.rand(*a.shape) - 1.)
    tmp = tempfile.mkdtemp(prefix="noise_")
    open(os.path.join(tmp, "input.nml"), "w").write(text)
    os.chdir(tmp)
    refpy.REFDIR = refdir("local") if local else DEFAULT_REFDIR
    ref = refpy.Ref(0)
    assert ref.n == tuple(ng), ref.n
    ref.bounduvw(u, v, w, True, False); ref.boundp(p, 0)
    visct = ref.zeros()
    ref.cmpt_sgs(u, v, w, visct)
    inner = visct[1:-1, 1:-1, 1:-1]
    assert np.isfinite(inner).all()
    os.chdir(ROOT); shutil.rmtree(tmp)
    fd, path = tempfile.mkstemp(prefix="noise_", suffix=".npy"); os.close(fd)
    np.save(path, inner)
    print(path, flush=True)


def relerr(a, b):      # tests/util.py
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def noise_seeds():
    build_variant("local")
    me = os.path.abspath(__file__)
    for index, (name, ng) in enumerate(NOISE_SHAPES):
        for seed in range(1, 13):
            f = {}
            for local in (1, 0):
                for pert in (0, 1):      # one process per run: the reference's modules keep state
                    out = subprocess.check_output([sys.executable, me, "--noise-run", str(index), str(seed), str(local), str(pert)], text=True)
                    path = out.strip().split("\n")[-1]
                    f[local, pert] = np.load(path); os.remove(path)
            rl, rp = relerr(f[1, 1], f[1, 0]), relerr(f[0, 1], f[0, 0])
            live = float((f[1, 0] != 0.).mean())
            print(f"{name} {'x'.join(map(str, ng))} seed {seed}: local {rl:.2e}  planes {rp:.2e}  A = {rl / rp:.1f}   (local: max {np.abs(f[1, 0]).max():.3e}, "
                  f"{live:.2f} of the cells non-zero)", flush=True)


def write_manifest():
    files = sorted(f for f in os.listdir(OUT) if f.endswith(".npz"))
    json.dump({"variants": {v: {"dsmag_average": t[0], "filter2d": t[1], "stage_by_stage": list(t[4]), "end_only": list(t[5])} for v, t in VARIANTS.items()},
               "files": {f: hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()[:16] for f in files}},
              open(os.path.join(OUT, "manifest.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=sorted(VARIANTS))
    ap.add_argument("--case")
    ap.add_argument("--noise-seeds", action="store_true")
    ap.add_argument("--noise-run", type=int, nargs=4, metavar=("INDEX", "SEED", "LOCAL", "PERTURBED"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    if a.noise_run:
        noise_run(*a.noise_run)
    elif a.noise_seeds:
        noise_seeds()
    elif a.case:
        run_case(a.variant, a.case)
    else:
        for variant in ([a.variant] if a.variant else list(VARIANTS)):
            build_variant(variant)
            for name in VARIANTS[variant][4] + VARIANTS[variant][5]:      # one process per case: the reference's modules keep state
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--variant", variant, "--case", name])
        write_manifest()

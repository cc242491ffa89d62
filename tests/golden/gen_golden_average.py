#!/usr/bin/env python3
"""Generates tests/golden/average/*.npz -- states from the REFERENCE ITSELF built to average the Germano identity of the dynamic model over the whole
domain or over x lines instead of z planes (src/sgs.f90:359-370).

  volume   -D_DIT: ave0d_dit (sgs.f90:388-431), one coefficient for the domain, weighted by dzf(k). _DIT is tested before _CHANNEL, so the
           `#define _CHANNEL` at the head of sgs.f90 does not matter: the committed recipe oracle/ref/Makefile with OUT and FFLAGS on the command line.
  xlines   _DUCT: ave2d_duct(...,1,...) (sgs.f90:585-612), one coefficient per line (j, k). The branch sits behind `#elif defined(_CHANNEL)`, so the
           flag alone cannot reach it: the recipe gets REF = a temporary directory of links to the reference's sources in which sgs.f90 is the
           reference's file minus that one line, and FFLAGS with -D_DUCT. The directory is deleted right after the build.
  *_f2d    the same with -D_FILTER_2D (the plane filter, tests/golden/gen_golden_filter2d.py).

The builds go to oracle/_ref/{dit,dit_f2d,duct,duct_f2d}, beside the default build and out of history like it. oracle.ref.refpy.REFDIR is pointed there
IN MEMORY and the cases run through gen_golden.run_case -- the same names, edits, operator sequence and keys as the plane-averaged goldens. Every file
carries the extra key `dsmag_average` ('volume' | 'xlines'), the plane-filter ones `filter2d = 1` too. Files: average/<variant>_<case>.npz with a
manifest of their own. Like gen_golden.py it runs only where the reference tree exists.

The clip max(.,0) (sgs.f90:377) hides every error of a coefficient it has zeroed, so the generator requires: volume -- the one coefficient is positive
after every substep the file holds; xlines -- at least two fifths of the (j, k) lines of r3_s9_visct are non-zero.

Usage:  python tests/golden/gen_golden_average.py                        # builds the variants, all cases (one subprocess per case), manifest
        python tests/golden/gen_golden_average.py --variant V --case NAME
        python tests/golden/gen_golden_average.py --noise-seeds              # which seeds of the GPU tests' noise leave a live volume coefficient (prints only)

--noise-seeds: tests/test_gpu_dsmag_average.py compares forms of the device code on the case's initial field plus 2 % white noise
(tests/test_gpu_filter2d.py, _shaped_case and _fields). Under volume averaging the one coefficient of such a field is the remainder of plane sums of
both signs and negative for about half of the seeds: the clip zeroes the field and a comparison would hold 0 against 0. This mode runs one cmpt_sgs of
the -D_DIT builds on every shape of NOISE_SHAPES for the seeds 1..12, and without noise (seed -1: the field the slab tests start from), and prints the
interior maximum of visct; the test file quotes the seeds it takes from this list.
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
from gen_golden_filter2d import FILE_LIMIT, save  # noqa: E402

ROOT = gen_golden.ROOT
OUT = os.path.join(HERE, "average")
RECIPE = os.path.join(ROOT, "oracle", "ref")
# variant: (value of dsmag_average, plane filter, directory under oracle/_ref, extra flags, stage-by-stage cases, end-of-step cases)
VARIANTS = {
    "volume": ("volume", False, "dit", "-D_DIT", ("tgv_dsmag_ppp", "chan_dsmag", "chan_dsmag_wm", "duct_dsmag", "cavity_dsmag"), ("tgv_dsmag_ppp_x64", "chan_dsmag_x64")),
    "volume_f2d": ("volume", True, "dit_f2d", "-D_DIT -D_FILTER_2D", ("tgv_dsmag_ppp", "chan_dsmag"), ()),
    # (cavity_dsmag is left out of the x lines: 32 of its 96 lines carry a coefficient)
    "xlines": ("xlines", False, "duct", "-D_DUCT", ("duct_dsmag", "duct_dsmag_wm", "tgv_dsmag_ppp"), ("duct_dsmag_x64",)),
    "xlines_f2d": ("xlines", True, "duct_f2d", "-D_DUCT -D_FILTER_2D", ("duct_dsmag",), ()),
}


def refdir(variant):
    return os.path.join(ROOT, "oracle", "_ref", VARIANTS[variant][2])


def build_variant(variant):
    ave, _, _, flags, _, _ = VARIANTS[variant]
    args = ["make", "-s", "-C", RECIPE, "OUT=" + refdir(variant), "FFLAGS=-cpp -O2 -fPIC -I/opt/conda/include " + flags]
    tmp = None
    try:
        if ave == "xlines":
            src = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(RECIPE, "Makefile")).read(), re.M).group(1)
            tmp = tempfile.mkdtemp(prefix="ref_duct_")
            for f in os.listdir(src):
                if f != "sgs.f90":
                    os.symlink(os.path.join(src, f), os.path.join(tmp, f))
            lines = open(os.path.join(src, "sgs.f90")).read().split("\n")
            keep = [ln for ln in lines if ln.strip() != "#define _CHANNEL"]
            assert len(keep) == len(lines) - 1, "sgs.f90: expected exactly one `#define _CHANNEL`"
            open(os.path.join(tmp, "sgs.f90"), "w").write("\n".join(keep))
            args.append("REF=" + tmp)
        subprocess.check_call(args + [os.path.join(refdir(variant), "libcales_ref.so")])
    finally:
        if tmp:
            shutil.rmtree(tmp)


def live_lines(visct):
    """(x lines with a non-zero value, lines) of a haloed eddy-viscosity field"""
    inner = visct[1:-1, 1:-1, 1:-1]
    return int((np.abs(inner).max(axis=0) > 0.).sum()), inner.shape[1] * inner.shape[2]


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
    assert np.isfinite(G["r3_s9_visct"]).all() and G["r3_div"][1] < 1e-12, (name, G["r3_div"])
    if ave == "volume":
        keys = [k for k in ("r1_s9_visct", "r2_s9_visct", "r3_s9_visct") if k in G]
        assert all(G[k][1:-1, 1:-1, 1:-1].max() > 0. for k in keys), (variant, name, "the clipped coefficient hides every error")
        note = f"coefficient > 0 after {len(keys)} substep(s)"
    else:
        live, nl = live_lines(G["r3_s9_visct"])
        assert 5 * live >= 2 * nl, (variant, name, "clipped lines hide errors", live, nl)
        note = f"lines with a coefficient: {live} of {nl}"
    save(out, G)
    assert os.path.getsize(out) <= FILE_LIMIT, (out, os.path.getsize(out))
    print(variant, name, note, "divmax", float(G["r3_div"][1]), "file KB:", os.path.getsize(out) // 1024, flush=True)


# (golden whose input.nml is used, grid, plane filter): the shapes of test_tile_form_equals_the_sequence_under_volume
NOISE_SHAPES = [("chan_dsmag", (64, 16, 12), False), ("chan_dsmag_wm", (64, 16, 12), False), ("chan_dsmag", (126, 20, 9), False),
                ("chan_dsmag_wm", (126, 20, 9), False), ("tgv_dsmag_ppp", (64, 16, 16), False), ("chan_dsmag", (64, 16, 12), True)]


def noise_case(index, seed):
    """One cmpt_sgs of the volume-averaged reference on the field of _fields(_shaped_case(name, ng), seed); seed < 0: without the noise."""
    from cales_amd.hotpath import initflow
    from cales_amd.nml import parse_text
    from oracle.ref import refpy
    name, ng, f2d = NOISE_SHAPES[index]
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
    if seed >= 0:
        rng = np.random.RandomState(seed)
        for a in (u, v, w):
            a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    tmp = tempfile.mkdtemp(prefix="noise_")
    open(os.path.join(tmp, "input.nml"), "w").write(text)
    os.chdir(tmp)
    refpy.REFDIR = refdir("volume_f2d" if f2d else "volume")
    ref = refpy.Ref(0)
    assert ref.n == tuple(ng), ref.n
    ref.bounduvw(u, v, w, True, False); ref.boundp(p, 0)
    visct = ref.zeros()
    ref.cmpt_sgs(u, v, w, visct)
    inner = visct[1:-1, 1:-1, 1:-1]
    assert np.isfinite(inner).all()
    print(f"{name} {'x'.join(map(str, ng))}{' plane filter' if f2d else ''} seed {seed}: max visct {inner.max():.3e}", flush=True)
    os.chdir(ROOT); shutil.rmtree(tmp)


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
    ap.add_argument("--noise-case", type=int, nargs=2, metavar=("INDEX", "SEED"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    if a.noise_case:
        noise_case(*a.noise_case)
    elif a.noise_seeds:
        for variant in ("volume", "volume_f2d"):
            build_variant(variant)
        for index in range(len(NOISE_SHAPES)):
            for seed in [-1] + list(range(1, 13)):      # one process per run: the reference's modules keep state
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--noise-case", str(index), str(seed)])
    elif a.case:
        run_case(a.variant, a.case)
    else:
        for variant in ([a.variant] if a.variant else list(VARIANTS)):
            build_variant(variant)
            for name in VARIANTS[variant][4] + VARIANTS[variant][5]:      # one process per case: the reference's modules keep state
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--variant", variant, "--case", name])
        write_manifest()

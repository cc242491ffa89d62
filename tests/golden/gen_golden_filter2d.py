#!/usr/bin/env python3
"""Generates tests/golden/filter2d/*.npz -- states from the REFERENCE ITSELF built with -D_FILTER_2D.

With that flag the dynamic model test-filters in the x-y planes only (filter2d, src/sgs.f90:824-848, called at 236-247 and 316-327) and uses
alph2 = 2.52 everywhere (sgs.f90:817-821). The recipe oracle/ref/Makefile builds that variant when OUT and FFLAGS are given on the command
line (OUT absolute: the recipe changes into it); it goes to oracle/_ref/filter2d, beside the default build and out of history like it.
oracle.ref.refpy.REFDIR is pointed there IN MEMORY and the cases run through gen_golden.run_case -- the same names, the same edits of the
reference's examples, the same operator sequence and keys as the goldens of the 3-D filter, so the generators cannot drift. Every file
carries the extra key `filter2d = 1`. The files go to a sub-directory with a manifest of their own: tests/golden/manifest.json stays as it is.
Like gen_golden.py it runs only where the reference tree exists.

A plane whose coefficient the clip max(.,0) (sgs.f90:372-380) has set to zero hides every error of its plane sums, so the generator requires
that in every case at least half of the z planes of r3_s9_visct carry a non-zero coefficient.

Usage:  python tests/golden/gen_golden_filter2d.py            # builds the variant, all cases (one subprocess per case), manifest
        python tests/golden/gen_golden_filter2d.py --case NAME
"""
import argparse
import hashlib
import io
import json
import lzma
import os
import struct
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

ROOT = gen_golden.ROOT
OUT = os.path.join(HERE, "filter2d")
REFDIR = os.path.join(ROOT, "oracle", "_ref", "filter2d")
STAGES = ("chan_dsmag", "chan_dsmag_wm", "tgv_dsmag_ppp", "duct_dsmag", "duct_dsmag_wm", "cavity_dsmag")      # stage by stage
END = ("chan_dsmag_x64", "chan_dsmag_x128", "tgv_dsmag_ppp_x64", "duct_dsmag_x64")                             # end-of-step states only
FILE_LIMIT = 1 << 20      # of a file in history
MAX_BYTES = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz"))      # the largest golden of the 3-D filter


def build_variant():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref"), "OUT=" + REFDIR,
                           "FFLAGS=-cpp -O2 -fPIC -I/opt/conda/include -D_FILTER_2D", os.path.join(REFDIR, "libcales_ref.so")])


def nonzero_planes(visct):
    """(planes with a non-zero coefficient, planes) of a haloed eddy-viscosity field"""
    inner = visct[1:-1, 1:-1, 1:-1]
    return int((np.abs(inner).reshape(-1, inner.shape[2]).max(axis=0) > 0.).sum()), inner.shape[2]


def save(out, G):
    """np.savez_compressed; a file that deflate leaves above FILE_LIMIT (64 x 16 x 16 cells, nine fields of doubles with random mantissas) is written
    again as a zip archive of LZMA members with literal-position bits for 8-byte words (lc 0, lp 3, pb 3) -- numpy.load reads either kind."""
    np.savez_compressed(out, **G)
    if os.path.getsize(out) <= FILE_LIMIT:
        return
    filt = {"id": lzma.FILTER_LZMA1, "preset": 9 | lzma.PRESET_EXTREME, "lc": 0, "lp": 3, "pb": 3}

    class Doubles(zipfile.LZMACompressor):      # zipfile fixes the encoder's properties; the member header (APPNOTE 5.8.8) carries ours
        def _init(self):
            props = lzma._encode_filter_properties(filt)
            self._comp = lzma.LZMACompressor(lzma.FORMAT_RAW, filters=[lzma._decode_filter_properties(lzma.FILTER_LZMA1, props)])
            return struct.pack("<BBH", 9, 4, len(props)) + props

    stock, zipfile.LZMACompressor = zipfile.LZMACompressor, Doubles
    try:
        with zipfile.ZipFile(out, "w", compression=zipfile.ZIP_LZMA) as z:
            for k, v in G.items():
                b = io.BytesIO(); np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False); z.writestr(k + ".npy", b.getvalue())
    finally:
        zipfile.LZMACompressor = stock
    H = np.load(out)
    assert sorted(H.files) == sorted(G) and all(np.array_equal(H[k], G[k]) for k in G), out


def run_case(name):
    from oracle.ref import refpy
    refpy.REFDIR = REFDIR
    out = os.path.join(OUT, name + ".npz")
    gen_golden.run_case(name, out)
    G = dict(np.load(out))
    G["filter2d"] = np.array(1)
    live, n3 = nonzero_planes(G["r3_s9_visct"])
    assert 2 * live >= n3, (name, "clipped planes hide errors", live, n3)
    assert np.isfinite(G["r3_s9_visct"]).all() and G["r3_div"][1] < 1e-12, (name, G["r3_div"])
    save(out, G)
    assert os.path.getsize(out) <= min(MAX_BYTES, FILE_LIMIT), (name, os.path.getsize(out), MAX_BYTES)
    print(name, "planes with a coefficient:", live, "of", n3, "file KB:", os.path.getsize(out) // 1024)


def write_manifest():
    files = sorted(f for f in os.listdir(OUT) if f.endswith(".npz"))
    json.dump({"cases": list(STAGES + END), "stage_by_stage": list(STAGES), "end_only": list(END),
               "files": {f: hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()[:16] for f in files}},
              open(os.path.join(OUT, "manifest.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    if a.case:
        assert a.case in STAGES + END, a.case
        run_case(a.case)
    else:
        build_variant()
        for name in STAGES + END:      # one process per case: the reference's modules keep state
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name])
        write_manifest()

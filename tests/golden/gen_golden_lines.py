#!/usr/bin/env python3
"""Generates tests/golden/lines/*.npz -- end-of-step states from the REFERENCE ITSELF at row lengths of 3, 5, 9 times 2^p.

The cases of gen_golden.py END_ONLY stop at power-of-two rows; the radix-8 register transforms now also take x rows and y lines of r 2^p
points (r = 3, 5, 9), and with them fillps inside the forward x pass, wrapped x ghost columns and the projection folded into the strain-rate
pass. This file adds such cases to gen_golden's tables IN MEMORY and runs them through its run_case (same sequence, same END_KEYS), so the
two generators cannot drift. The files go to a sub-directory with a manifest of their own: tests/golden/manifest.json lists the files beside
it and stays as it is. Like gen_golden.py it runs only where the reference tree and oracle/_ref exist.

Usage:  python tests/golden/gen_golden_lines.py            # all cases (one subprocess per case)
        python tests/golden/gen_golden_lines.py --case NAME
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

OUT = os.path.join(HERE, "lines")
# a row of THREE 64-cell tiles, 192 = 2 * 3 * 2^5: x lines of 96 complex points (radix 3 first), the dynamic model's folded strain-rate pass
LINES = {
    "chan_dsmag_x192": ("les/_manuscript_turbulent_channel/input.nml",
                        {r"ng\(1:3\) = .*": "ng(1:3) = 192, 8, 8", r"gr = 5\.": "gr = 2.", r"sgstype = 'smag'": "sgstype = 'dsmag'"}, 0),
}
gen_golden.CASES.update(LINES)
gen_golden.END_ONLY.update(LINES)


def write_manifest():
    files = sorted(f for f in os.listdir(OUT) if f.endswith(".npz"))
    json.dump({"cases": sorted(LINES), "files": {f: hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()[:16] for f in files}},
              open(os.path.join(OUT, "manifest.json"), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    if a.case:
        gen_golden.run_case(a.case, os.path.join(OUT, a.case + ".npz"))
    else:
        for name in LINES:      # one process per case: the reference's modules keep state
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--case", name])
        write_manifest()

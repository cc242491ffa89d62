"""Reference-made end-of-step state at a 192-cell row (tests/golden/lines, gen_golden_lines.py): x lines of 96 = 3 * 2^5 complex points, three
64-cell tiles. The oracle's whole step against it, at the bars of test_step_at_power_of_two_rows, and the digest of the file."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import F, GOLD, load_golden, relerr

LINE_CASES = ["lines/chan_dsmag_x192"]


@pytest.mark.parametrize("name", LINE_CASES)
def test_step_at_rows_of_three_times_a_power_of_two(name):
    g, case = load_golden(name)
    assert tuple(int(x) for x in case.ng) == (192, 8, 8) and case.sgstype == "dsmag"
    o = Oracle(case, nthreads=4)
    u, v, w, p = (F(g["s0raw_" + k]) for k in "uvwp")
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    assert abs(o.chkdt(visct, u, v, w) / float(g["dt_cfl"]) - 1) < 1e-12
    dpdl = o.step(float(g["dt"]), u, v, w, p, pp, visct)
    for a, k in zip((u, v, w), "uvw"):
        assert relerr(a, g["r3_s7_" + k]) < 1e-12, k
    pg = g["r3_s8_p"]      # (the constant of the singular solve is defined by round-off: compared mean-free)
    assert relerr(p - p[1:-1, 1:-1, 1:-1].mean(), pg - pg[1:-1, 1:-1, 1:-1].mean()) < 1e-11
    assert relerr(visct, g["r3_s9_visct"]) < 1e-10
    assert np.abs(dpdl - g["dpdl"]).max() < 1e-10 * max(1., np.abs(g["dpdl"]).max())
    assert float(g["r3_div"][1]) < 1e-13      # the reference's own chkdiv after the step


def test_lines_manifest_matches_the_files():
    here = os.path.join(GOLD, "lines")
    man = json.load(open(os.path.join(here, "manifest.json")))
    files = sorted(f for f in os.listdir(here) if f.endswith(".npz"))
    assert sorted(man["files"]) == files == sorted(c + ".npz" for c in man["cases"])
    for f in files:
        assert os.path.getsize(os.path.join(here, f)) < 1 << 20, f
        assert hashlib.sha256(open(os.path.join(here, f), "rb").read()).hexdigest()[:16] == man["files"][f], f

#!/usr/bin/env python3
"""Times whole steps and the passes of the pressure solve at grids of any line length (bench.py measures the flagship workload only).

  python tools/linebench.py les/_manuscript_turbulent_channel:own turbulent_channel.nml:768x384x256:sgs=dsmag duct_wall_model_512.nml:640x320x320:impdiff=2

An entry is CASE:GRID[:key=value,...]. CASE ending in .nml is a file of cales_amd/cases, anything else a key of tests/golden/examples.json (the
namelists of the examples the reference ships, kept as data); GRID is n1xn2xn3 or `own`; keys: sgs (none | smag | dsmag), impdiff (0 | 1 | 2),
filter (2d | 3d: the test filter of the dynamic model, Case.filter2d -- the reference's -D_FILTER_2D; without the key CALES_FILTER_2D decides),
average (planes | volume | xlines | local: what the dynamic model averages the Germano identity over, Case.dsmag_average -- the reference's _CHANNEL / -D_DIT /
_DUCT / _CAVITY; without the key CALES_DSMAG_AVERAGE decides).
Per entry: create the context, warm up, time K steps of cales_step between device synchronisations (K from a pilot so that the window is at
least --window seconds), repeat them with per-kernel events, print ONE JSON line: ms_per_step, the plan string and, per scope of the solve, the ms
per call and the fraction of the 8 TB/s peak at 2 compulsory words per cell and pass (4 with fillps inside the forward x pass, 9 for the correction
pass) -- the pricing of DESIGN.md 3; under "sgs_scopes" the ms per call of cmpt_sgs and of the passes of the dynamic model. CALES_LIB picks the
library, so a job script can alternate two builds."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
SGS_SCOPES = ["cmpt_sgs_dsmag", "cmpt_sgs_smag", "strain_filter_uvw", "correc_strain_filter_uvw", "lij_mij_filter_contract", "strain_rate"]
WORDS = {"fillps_fft_x_fwd": 4, "fft_x_fwd": 2, "fft_y_fwd": 2, "gaussel_z": 2, "fft_y_bwd": 2, "fft_x_bwd": 2, "correc_updatep": 9}


def load(entry):
    from cales_amd.nml import parse_text
    parts = entry.split(":")
    name, grid = parts[0], parts[1] if len(parts) > 1 else "own"
    opts = dict(kv.split("=", 1) for kv in parts[2].split(",")) if len(parts) > 2 else {}
    if name.endswith(".nml"):
        text = open(os.path.join(ROOT, "cales_amd", "cases", name)).read()
    else:
        text = json.load(open(os.path.join(ROOT, "tests", "golden", "examples.json")))[name]
    case = parse_text(text)
    if grid != "own":
        case.ng[:] = [int(x) for x in grid.split("x")]
    if "sgs" in opts:
        case.sgstype = opts["sgs"]
    case.impdiff = int(opts.get("impdiff", 0))
    if "filter" in opts:
        if opts["filter"] not in ("2d", "3d"):
            raise SystemExit(f"{entry}: filter is 2d or 3d")
        case.filter2d = opts["filter"] == "2d"
    if "average" in opts:
        if opts["average"] not in ("planes", "volume", "xlines", "local"):
            raise SystemExit(f"{entry}: average is planes, volume, xlines or local")
        case.dsmag_average = opts["average"]
    return case


def run(entry, window, warmup):
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    case = load(entry)
    ncell = int(case.ng[0]) * int(case.ng[1]) * int(case.ng[2])
    rb = 4.0 if capi.SINGLE else 8.0
    h = HotPath(case)
    try:
        u, v, w, p = initflow(case); h.upload(u, v, w, p); del u, v, w, p
        h.startup()
        dt = 0.5 * h.chkdt()
        for _ in range(warmup):
            h.step(dt)
        h.sync(); t0 = time.perf_counter()
        for _ in range(2):
            h.step(dt)
        h.sync(); pilot = (time.perf_counter() - t0) / 2
        K = max(3, min(20000, int(math.ceil(window / pilot))))
        h.sync(); t0 = time.perf_counter()
        for _ in range(K):
            h.step(dt)
        h.sync(); ms = 1e3 * (time.perf_counter() - t0) / K
        h.profile_reset(); h.profile(True)
        for _ in range(K):
            h.step(dt)
        h.sync(); h.profile(False)
        st = h.profile_stats()
        scopes = {}
        for k, words in WORDS.items():
            calls, tot = st.get(k, (0, 0.))
            if not calls:
                continue
            per_pass = tot / (3 * K)      # three substeps, one solve (and at most one correction pass) each
            scopes[k] = {"ms_per_call": round(tot / calls, 5), "calls_per_step": round(calls / K, 2), "ms_per_step": round(tot / K, 5),
                         "frac_peak": round(words * ncell * rb / (per_pass * 1e-3) / PEAK, 4)}
        sgs = {k: {"ms_per_call": round(st[k][1] / st[k][0], 5), "calls_per_step": round(st[k][0] / K, 2)} for k in SGS_SCOPES if st.get(k, (0, 0.))[0]}
        divmax = h.chkdiv()[1]
        pl = h.describe_plan()
        return {"entry": entry, "ng": [int(x) for x in case.ng], "lib": os.path.basename(capi.LIB_PATH), "steps": K, "ms_per_step": round(ms, 5),
                "divmax": divmax, "plan": ";".join(f"{k}={v}" for k, v in pl.items()), "scopes": scopes, "sgs_scopes": sgs}
    finally:
        h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("entries", nargs="+")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed steps at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="", help="copied into every line (which build, which round)")
    a = ap.parse_args()
    for e in a.entries:
        r = run(e, a.window, a.warmup)
        if a.tag:
            r["tag"] = a.tag
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the reads of include/cales_post.h against the full download of a field (cales_get_field), in one process on one context.

  python tools/boxbench.py [--grid 512x512x512] [--calls 10] [--warmup 2]

An explicit channel without subgrid model at the grid given; per case the wall-clock time of a call as the host sees it -- packing kernel, copy to the
host and the numpy array the call returns -- as the median of --calls calls after --warmup calls. Prints ONE JSON line per case: ms (median), ms_min,
ms_max, the reals and bytes that travel, the time relative to the full download, and the device time of the packing kernel alone (the profile scope
"box_read"). The last line holds the same-box calibration (cales_calibrate) next to which the numbers are to be read. CALES_LIB picks the library."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("get", "u"), ("out2d", "u", 2, None), ("out2d", "u", 1, None), ("out2d", "u", 3, None), ("out3d", "u", (2, 2, 2)), ("out3d", "u", (4, 4, 4))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="", help="copied into every line")
    a = ap.parse_args()
    import numpy as np
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    from cales_amd.nml import parse_text
    case = parse_text(open(os.path.join(ROOT, "cales_amd", "cases", "turbulent_channel.nml")).read())
    case.ng[:] = [int(x) for x in a.grid.split("x")]
    case.sgstype = "none"; case.impdiff = 0
    ng = [int(x) for x in case.ng]
    h = HotPath(case)
    try:
        u, v, w, p = initflow(case); h.upload(u, v, w, p); del v, w, p
        h.startup()
        full_ms = None
        for cs in CASES:
            kind, name = cs[0], cs[1]
            if kind == "out2d":
                args = (cs[2], ng[cs[2] - 1] // 2)
            else:
                args = cs[2:]
            call = (lambda: h.get(name)) if kind == "get" else (lambda: getattr(h, kind)(name, *args))
            for _ in range(a.warmup):
                out = call()
            h.profile_reset(); h.profile(True)
            ts = []
            for _ in range(a.calls):
                h.sync(); t0 = time.perf_counter()
                out = call()
                ts.append(1e3 * (time.perf_counter() - t0))
            h.profile(False)
            st = h.profile_stats().get("box_read", (0, 0.))
            # what came back is what a slice of the field holds (the initial field: nothing has been stepped)
            want = u if kind == "get" else (u[tuple(slice(1, -1) if d != args[0] - 1 else slice(args[1], args[1] + 1) for d in range(3))] if kind == "out2d"
                                            else u[1:-1:args[0][0], 1:-1:args[0][1], 1:-1:args[0][2]])
            inner = (slice(1, -1),) * 3 if kind == "get" else ()      # (the start-up has set the ghost cells of the field on the device)
            ok = bool(out.shape == want.shape and np.array_equal(out[inner], want[inner]))
            med = statistics.median(ts)
            if kind == "get":
                full_ms = med
            r = {"case": kind + "(" + ", ".join([repr(name)] + [str(x) for x in args]) + ")", "ng": ng, "lib": os.path.basename(capi.LIB_PATH), "calls": a.calls,
                 "ms": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "reals": int(out.size), "bytes": int(out.nbytes),
                 "ms_over_full_get": round(med / full_ms, 6), "equals_slice_of_field": ok}
            if st[0]:
                r["box_read_kernel_ms"] = round(st[1] / st[0], 5)
            if a.tag:
                r["tag"] = a.tag
            print(json.dumps(r), flush=True)
        cal = h.calibrate(3)
        print(json.dumps({"calibration": {k: (round(x, 1) if isinstance(x, float) else x) for k, x in cal.items()}, "device": h.device_info()[0]}), flush=True)
    finally:
        h.close()


if __name__ == "__main__":
    main()

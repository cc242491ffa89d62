#!/usr/bin/env python3
"""Times the derived fields of include/cales_derived.h against the route they replace -- the full download of u, v and w (cales_get_field) and numpy
on the host --, in one process, at 512^3.

  python tools/derivedbench.py [--grids 512x512x512] [--calls 10] [--warmup 2] [--rounds 3] [--no-host]

An explicit channel without subgrid model per grid, u, v, w random fields. Per case ONE JSON line: the dense Q volume, a z plane, a y plane, an x plane,
an every-fourth-point sample and cales_derived_to_pp, each in a context of its own per kernel form -- the default (dense boxes by the LDS-tile rows
kernel) and CALES_DERIVED_POINTS=1 (everything by the points kernel), the switch being read when a context is created -- and alternated between the two
on the same fields, --rounds times: the wall-clock time of a call as the host sees it (median of --calls calls after --warmup, ms;
it includes the copy of the result to the host), the device time of its profile scope, and that device time's rate over the compulsory traffic of the
cells it forms (three reads and one write per cell) as a fraction of the same run's copy calibration (cales_calibrate). The download of one field is
timed alone; the host arithmetic (Q in numpy, plain slicing, not held to any order) once. CALES_LIB picks the library."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_q(u, v, w, dxi, dyi, dzci, dzfi):
    """Q = 0.5 (WijWij - SijSij) of src/post.f90 at the interior cells, by slicing (the arithmetic of the host route; operation order as numpy likes it)"""
    import numpy as np
    n1, n2, n3 = (s - 2 for s in u.shape)
    S = lambda a, di, dj, dk: a[1 + di:n1 + 1 + di, 1 + dj:n2 + 1 + dj, 1 + dk:n3 + 1 + dk]
    zk, zm = dzci[None, None, 1:n3 + 1], dzci[None, None, 0:n3]
    str_ = ((S(u, 0, 0, 0) - S(u, -1, 0, 0)) * dxi) ** 2 + ((S(v, 0, 0, 0) - S(v, 0, -1, 0)) * dyi) ** 2 + ((S(w, 0, 0, 0) - S(w, 0, 0, -1)) * dzfi[None, None, 1:n3 + 1]) ** 2
    ens = np.zeros_like(str_)
    for (a, da, ma), (b, db, mb), corners in (((u, (0, 1, 0), dyi), (v, (1, 0, 0), dxi), ((0, 0, 0), (0, -1, 0), (-1, 0, 0), (-1, -1, 0))),
                                              ((u, (0, 0, 1), None), (w, (1, 0, 0), dxi), ((0, 0, 0), (0, 0, -1), (-1, 0, 0), (-1, 0, -1))),
                                              ((v, (0, 0, 1), None), (w, (0, 1, 0), dyi), ((0, 0, 0), (0, 0, -1), (0, -1, 0), (0, -1, -1)))):
        for c in corners:
            p = tuple(x + y for x, y in zip(c, da)); q = tuple(x + y for x, y in zip(c, db))
            ga = (S(a, *p) - S(a, *c)) * (ma if ma is not None else (zk if c[2] == 0 else zm))
            gb = (S(b, *q) - S(b, *c)) * mb
            str_ += 0.125 * (ga + gb) ** 2
            ens += 0.125 * (ga - gb) ** 2
    return 0.5 * (ens - str_)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="512x512x512")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternations between the two kernel forms")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy route")
    ap.add_argument("--tag", default="", help="copied into every line")
    a = ap.parse_args()
    import numpy as np
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initgrid
    from cales_amd.nml import parse_text
    R = capi.np_real
    rsz = np.dtype(R).itemsize

    def emit(r):
        if a.tag:
            r["tag"] = a.tag
        print(json.dumps(r), flush=True)

    for grid in a.grids.split(","):
        case = parse_text(open(os.path.join(ROOT, "cales_amd", "cases", "turbulent_channel.nml")).read())
        case.ng[:] = [int(x) for x in grid.split("x")]
        case.sgstype = "none"; case.impdiff = 0
        ng = [int(x) for x in case.ng]
        shape = tuple(n + 2 for n in ng)
        h = HotPath(case)
        os.environ["CALES_DERIVED_POINTS"] = "1"
        hp = HotPath(case)      # the same case with every box by the points kernel
        del os.environ["CALES_DERIVED_POINTS"]
        try:
            def timed(call, scope=None, calls=a.calls, warmup=a.warmup, h=h):
                for _ in range(warmup):
                    out = call()
                h.profile_reset(); h.profile(True)
                ts = []
                for _ in range(calls):
                    h.sync(); t0 = time.perf_counter()
                    out = call()
                    ts.append(1e3 * (time.perf_counter() - t0))
                h.profile(False)
                st = {k: v for k, v in h.profile_stats().items() if scope and k.startswith(scope) and v[0]}
                return out, statistics.median(ts), min(ts), max(ts), {k: v[1] / v[0] for k, v in st.items()}
            cal = h.calibrate(3)
            base = {"ng": ng, "lib": os.path.basename(capi.LIB_PATH)}
            rng = np.random.RandomState(1)
            fields = []
            for name in ("u", "v", "w"):
                x = np.zeros(shape, order="F", dtype=R); x[...] = rng.standard_normal(shape).astype(R)
                h.set(name, x); hp.set(name, x); fields.append(x)
            _, get_ms, get_min, get_max, _ = timed(lambda: h.get("u"), calls=max(3, a.calls // 2), warmup=1)
            emit(dict(base, case="get_field(u)", ms=round(get_ms, 3), ms_min=round(get_min, 3), ms_max=round(get_max, 3), bytes=int(np.prod(shape)) * rsz))
            host_q = None
            if not a.no_host:
                g = initgrid(case.gtype, ng[2], case.gr, case.l[2])
                t0 = time.perf_counter()
                host_q = numpy_q(*fields, R(ng[0] / case.l[0]), R(ng[1] / case.l[1]), 1 / g["dzc"], 1 / g["dzf"])
                emit(dict(base, case="numpy Q of the downloaded fields (arithmetic only)", ms=round(1e3 * (time.perf_counter() - t0), 1), calls=1,
                          route_ms=round(3 * get_ms + 1e3 * (time.perf_counter() - t0), 1)))
            del fields
            mid = [(n + 1) // 2 for n in ng]
            cases = [("derived_out3d(qcr), dense volume", lambda h: h.derived_out3d("qcr"), ng[0] * ng[1] * ng[2]),
                     ("derived_out3d(vox), dense volume", lambda h: h.derived_out3d("vox"), ng[0] * ng[1] * ng[2]),
                     ("derived_to_pp(qcr)", lambda h: h.derived_to_pp("qcr"), ng[0] * ng[1] * ng[2]),
                     ("derived_out2d(qcr, z plane)", lambda h: h.derived_out2d("qcr", 3, mid[2]), ng[0] * ng[1]),
                     ("derived_out2d(qcr, y plane)", lambda h: h.derived_out2d("qcr", 2, mid[1]), ng[0] * ng[2]),
                     ("derived_out2d(qcr, x plane)", lambda h: h.derived_out2d("qcr", 1, mid[0]), ng[1] * ng[2]),
                     ("derived_out3d(qcr), every fourth point", lambda h: h.derived_out3d("qcr", (4, 4, 4)), ((ng[0] + 3) // 4) * ((ng[1] + 3) // 4) * ((ng[2] + 3) // 4))]
            runs = [(what, call, cells, ctx, rnd) for rnd in range(a.rounds) for what, call, cells in cases for ctx in (h, hp)]
            for what, call, cells, ctx, rnd in runs:
                got, ms, ms_min, ms_max, dev = timed(lambda: call(ctx), "derived", h=ctx)
                dev_ms = sum(dev.values())
                r = dict(base, case=what, round=rnd, context="points" if ctx is hp else "default", ms=round(ms, 4), ms_min=round(ms_min, 4), ms_max=round(ms_max, 4), device_ms=round(dev_ms, 4), scopes=sorted(dev),
                         cells=cells, compulsory_GBps=round(4 * cells * rsz / dev_ms * 1e-6, 1),
                         fraction_of_copy_calibration=round(4 * cells * rsz / dev_ms * 1e-6 / cal["copy_GBps"], 3), ms_over_three_get_field=round(ms / (3 * get_ms), 5))
                if host_q is not None and what.startswith("derived_out3d(qcr), dense"):
                    r["max_error_over_max_value_vs_numpy"] = float(np.abs(got - host_q).max() / np.abs(host_q).max())
                emit(r)
            emit({"calibration": {k: (round(v, 1) if isinstance(v, float) else v) for k, v in cal.items()}, "ng": ng, "device": h.device_info()[0]})
        finally:
            h.close(); hp.close()


if __name__ == "__main__":
    main()

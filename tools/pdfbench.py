#!/usr/bin/env python3
"""Times the histograms of include/cales_pdf.h against the route they replace -- the full download of the field (cales_get_field) and numpy binning on
the host --, in one process, at 512^3 and at 256 x 128 x 128.

  python tools/pdfbench.py [--grids 512x512x512,256x128x128] [--calls 10] [--warmup 2]

An explicit channel without subgrid model per grid. pdf_planes of u with 256 and 4096 bins on three distributions of the samples over the bins: uniform;
Gaussian on every plane with a standard deviation of 8 bins (what turbulence does: a plane's samples sit in a few bins near its mean); all samples in ONE
bin (every LDS atomic of a wave on one address). jpdf_planes of (u, p) on 8 planes with 128 x 128 bins. Per case ONE JSON line: the wall-clock time of
a call as the host sees it (median of --calls calls after --warmup, ms), the device time of its profile scope (kernel and the clearing of the counters),
that device time's read rate as a fraction of the same run's read-only calibration (cales_calibrate), the wall-clock time relative to the download of
the same field measured in the same run, and whether the counts equal numpy's. The download is timed alone and, once, with the numpy binning of the
field on top. CALES_LIB picks the library."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_counts(x, nbins, lo, hi):
    """the bin rule of include/cales_pdf.h on the interior of a haloed field: counts (nbins, n3), outside (2, n3)"""
    import numpy as np
    R = x.dtype.type
    n3 = x.shape[2] - 2
    counts, outside = np.zeros((nbins, n3), dtype=np.int64, order="F"), np.zeros((2, n3), dtype=np.int64, order="F")
    s = R(nbins) / (R(hi) - R(lo))
    for k in range(n3):
        t = (x[1:-1, 1:-1, k + 1] - R(lo)) * s
        below, above = t < 0, ~(t < nbins)
        outside[0, k], outside[1, k] = below.sum(), above.sum()
        counts[:, k] = np.bincount(t[~(below | above)].astype(np.int64), minlength=nbins)
    return counts, outside


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="512x512x512,256x128x128")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="", help="copied into every line")
    a = ap.parse_args()
    import numpy as np
    from cales_amd import capi
    from cales_amd.hotpath import HotPath
    from cales_amd.nml import parse_text
    R = capi.np_real

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
        field_bytes = ng[0] * ng[1] * ng[2] * np.dtype(R).itemsize
        h = HotPath(case)
        try:
            def timed(call, scope=None, calls=a.calls, warmup=a.warmup):
                for _ in range(warmup):
                    out = call()
                h.profile_reset(); h.profile(True)
                ts = []
                for _ in range(calls):
                    h.sync(); t0 = time.perf_counter()
                    out = call()
                    ts.append(1e3 * (time.perf_counter() - t0))
                h.profile(False)
                st = h.profile_stats().get(scope, (0, 0.)) if scope else (0, 0.)
                return out, statistics.median(ts), min(ts), max(ts), (st[1] / st[0] if st[0] else None)
            cal = h.calibrate(3)
            base = {"ng": ng, "lib": os.path.basename(capi.LIB_PATH)}
            rng = np.random.RandomState(1)
            z = np.zeros(shape, order="F", dtype=R); z[...] = rng.standard_normal(shape).astype(R)
            uni = np.zeros(shape, order="F", dtype=R); uni[...] = rng.random_sample(shape).astype(R)
            h.set("p", uni)
            # the route this replaces: the download alone, then with the binning on the host
            h.set("u", uni)
            _, get_ms, get_min, get_max, _ = timed(lambda: h.get("u"), calls=max(3, a.calls // 2), warmup=1)
            emit(dict(base, case="get_field(u)", ms=round(get_ms, 3), ms_min=round(get_min, 3), ms_max=round(get_max, 3), bytes=int(np.prod(shape)) * np.dtype(R).itemsize))
            t0 = time.perf_counter()
            host_counts = numpy_counts(h.get("u"), 256, 0., 1.)
            host_ms = 1e3 * (time.perf_counter() - t0)
            emit(dict(base, case="get_field(u) + numpy binning, 256 bins", ms=round(host_ms, 1), calls=1))
            for dist in ("uniform", "gaussian_8_bins", "one_bin"):
                for nbins in (256, 4096):
                    if dist == "uniform":
                        x = uni
                    elif dist == "gaussian_8_bins":
                        x = (R(0.5) + z * R(8. / nbins)).astype(R, order="F")
                    else:
                        x = np.full(shape, 0.5, order="F", dtype=R)
                    h.set("u", x)
                    (counts, outside), ms, ms_min, ms_max, dev_ms = timed(lambda: h.pdf_planes("u", nbins, 0., 1.), "pdf_planes")
                    want = host_counts if (dist == "uniform" and nbins == 256) else (numpy_counts(x, nbins, 0., 1.) if ng[0] * ng[1] * ng[2] <= 2 ** 23 else None)
                    r = dict(base, case=f"pdf_planes(u, {nbins})", samples=dist, ms=round(ms, 4), ms_min=round(ms_min, 4), ms_max=round(ms_max, 4), device_ms=round(dev_ms, 4),
                             read_GBps=round(field_bytes / dev_ms * 1e-6, 1), fraction_of_read_calibration=round(field_bytes / dev_ms * 1e-6 / cal["read_GBps"], 3),
                             ms_over_get_field=round(ms / get_ms, 5), faster_than_get_field=bool(ms < get_ms), bins_hit=int((counts > 0).sum(0).max()),
                             conserved=bool((counts.sum(0) + outside.sum(0) == ng[0] * ng[1]).all()))
                    if want is not None:
                        r["equals_numpy"] = bool(np.array_equal(counts, want[0]) and np.array_equal(outside, want[1]))
                    emit(r)
            kp = [1 + (q * ng[2]) // 8 for q in range(8)]
            h.set("u", (R(0.5) + z * R(8. / 128)).astype(R, order="F"))
            (jc, jo), ms, ms_min, ms_max, dev_ms = timed(lambda: h.jpdf_planes("u", "p", 128, (0., 1.), (0., 1.), kp), "jpdf_planes")
            jbytes = 2 * 8 * ng[0] * ng[1] * np.dtype(R).itemsize
            emit(dict(base, case="jpdf_planes(u, p, 128, 8 planes)", samples="gaussian_8_bins x uniform", ms=round(ms, 4), ms_min=round(ms_min, 4), ms_max=round(ms_max, 4),
                      device_ms=round(dev_ms, 4), read_GBps=round(jbytes / dev_ms * 1e-6, 1), fraction_of_read_calibration=round(jbytes / dev_ms * 1e-6 / cal["read_GBps"], 3),
                      ms_over_get_field=round(ms / get_ms, 5), faster_than_get_field=bool(ms < get_ms),
                      conserved=bool((jc.sum((0, 1)) + jo == ng[0] * ng[1]).all())))
            emit({"calibration": {k: (round(x, 1) if isinstance(x, float) else x) for k, x in cal.items()}, "ng": ng, "device": h.device_info()[0]})
        finally:
            h.close()
        del z, uni


if __name__ == "__main__":
    main()

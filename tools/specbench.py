#!/usr/bin/env python3
"""Times the spectra of include/cales_spectra.h against the route they replace -- the full download of the field (cales_get_field) and numpy.fft on the
host --, in one process, at 512^3 and at 192 x 128 x 128.

  python tools/specbench.py [--grids 512x512x512,192x128x128] [--calls 10] [--warmup 2]

An explicit channel without subgrid model per grid, u a random field. Per case ONE JSON line: spectra_lines along x and along y on every plane and
spectra_planes on 8 planes -- the wall-clock time of a call as the host sees it (median of --calls calls after --warmup, ms), the device time of its
profile scope (twiddle table, transform and fold kernels), that device time's read rate of the samples it transforms as a fraction of the same run's
read-only calibration (cales_calibrate), the wall-clock time relative to the download of the field measured in the same run, and the largest error
against numpy relative to the largest value. The download is timed alone and, once each, with the numpy transforms of the field on top. CALES_LIB
picks the library.

  python tools/specbench.py --cross [--grids 512x512x512]

times the cross-spectra of include/cales_cospectra.h instead: cospectra_lines(u, w, 1), (u, w, 2) and cospectra_planes(u, w, 8 planes), each ALTERNATED
call by call with the two power-spectrum calls it replaces (u, then w: the same reads and the same two transforms per row pair), and once each against
the download of the two fields with numpy.fft on top. Per case one JSON line with the wall-clock medians and extremes of both, the device times of the
profile scopes, and the cross call's device time over the read-once bound of two fields at the calibration's read rate.

  python tools/specbench.py --digest [--grids 96x12x10,...]

times nothing: for seeded fields u and w it prints per grid one JSON line per entry -- spectra_lines along x and y (with the line sums) and
spectra_planes of u and of w, cospectra_lines along x and y (with the line sums) and cospectra_planes of the pairs (u, w) and (u, u), the planes given out
of order with a repeat -- with the SHA-256 of the raw bytes of every array the entry returned. Two builds of the library whose lines are equal compute
the same bits."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="512x512x512,192x128x128")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="", help="copied into every line")
    ap.add_argument("--cross", action="store_true", help="the cross-spectra of two fields against two power-spectrum calls")
    ap.add_argument("--digest", action="store_true", help="no timing: the SHA-256 of every array the spectra and cross-spectra entries return")
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

    def digest_mode(h, ng, base):
        """--digest: see the head of the file"""
        shape = tuple(n + 2 for n in ng)
        rng = np.random.RandomState(1)
        for name, mean in (("u", 3.), ("w", 0.)):
            x = np.zeros(shape, order="F", dtype=R); x[...] = (mean + rng.standard_normal(shape)).astype(R)
            h.set(name, x)
        kp = [ng[2], 1, 1 + ng[2] // 2, 1]
        sha = lambda out: [hashlib.sha256(np.asfortranarray(v).tobytes(order="F")).hexdigest() for v in (out if isinstance(out, tuple) else (out,))]
        for f in ("u", "w"):
            for idir in (1, 2):
                emit(dict(base, entry=f"spectra_lines({f}, {idir})", sha256=sha(h.spectra_lines(f, idir))))
            emit(dict(base, entry=f"spectra_planes({f}, {kp})", sha256=sha(h.spectra_planes(f, kp))))
        for fa, fb in (("u", "w"), ("u", "u")):
            for idir in (1, 2):
                emit(dict(base, entry=f"cospectra_lines({fa}, {fb}, {idir})", sha256=sha(h.cospectra_lines(fa, fb, idir))))
            emit(dict(base, entry=f"cospectra_planes({fa}, {fb}, {kp})", sha256=sha(h.cospectra_planes(fa, fb, kp))))

    def cross_mode(h, ng, cal, base):
        """--cross: see the head of the file"""
        shape = tuple(n + 2 for n in ng)
        plane_bytes = ng[0] * ng[1] * np.dtype(R).itemsize
        rng = np.random.RandomState(1)
        for name, mean in (("u", 3.), ("w", 0.)):
            x = np.zeros(shape, order="F", dtype=R); x[...] = (mean + rng.standard_normal(shape)).astype(R)
            h.set(name, x)
            del x
        kp = [1 + (q * ng[2]) // 8 for q in range(8)]
        n2 = ng[1]

        def fold(P):
            out = P[:, :n2 // 2 + 1, :].copy()
            out[:, 1:(n2 + 1) // 2, :] += P[:, :n2 // 2:-1, :]
            return out
        host = {}
        for what, fn in (("x", lambda f, g: (np.fft.rfft(f, axis=0) * np.conj(np.fft.rfft(g, axis=0))).sum(1)),
                         ("y", lambda f, g: (np.fft.rfft(f, axis=1) * np.conj(np.fft.rfft(g, axis=1))).sum(0)),
                         ("planes", lambda f, g: fold(np.fft.fft(np.fft.rfft(f[:, :, [k - 1 for k in kp]], axis=0), axis=1)
                                                      * np.conj(np.fft.fft(np.fft.rfft(g[:, :, [k - 1 for k in kp]], axis=0), axis=1))))):
            t0 = time.perf_counter()
            host[what] = fn(h.get("u")[1:-1, 1:-1, 1:-1].astype(np.float64), h.get("w")[1:-1, 1:-1, 1:-1].astype(np.float64))
            emit(dict(base, case=f"get_field(u) + get_field(w) + numpy.fft, {what}", ms=round(1e3 * (time.perf_counter() - t0), 1), calls=1))
        cases = (("x", "cospectra_lines(u, w, 1)", lambda: h.cospectra_lines("u", "w", 1, lsum=False), "cospectra_lines",
                  "spectra_lines(u, 1) + spectra_lines(w, 1)", lambda: (h.spectra_lines("u", 1, lsum=False), h.spectra_lines("w", 1, lsum=False)), "spectra_lines", ng[2]),
                 ("y", "cospectra_lines(u, w, 2)", lambda: h.cospectra_lines("u", "w", 2, lsum=False), "cospectra_lines",
                  "spectra_lines(u, 2) + spectra_lines(w, 2)", lambda: (h.spectra_lines("u", 2, lsum=False), h.spectra_lines("w", 2, lsum=False)), "spectra_lines", ng[2]),
                 ("planes", "cospectra_planes(u, w, 8 planes)", lambda: h.cospectra_planes("u", "w", kp), "cospectra_planes",
                  "spectra_planes(u, 8 planes) + spectra_planes(w, 8 planes)", lambda: (h.spectra_planes("u", kp), h.spectra_planes("w", kp)), "spectra_planes", 8))
        for what, cname, ccall, cscope, pname, pcall, pscope, nplanes in cases:
            for _ in range(a.warmup):
                got = ccall(); pcall()
            h.profile_reset(); h.profile(True)
            tc, tp = [], []
            for _ in range(a.calls):      # alternated: a cross call, then the two power calls
                h.sync(); t0 = time.perf_counter(); got = ccall(); tc.append(1e3 * (time.perf_counter() - t0))
                h.sync(); t0 = time.perf_counter(); pcall(); tp.append(1e3 * (time.perf_counter() - t0))
            h.profile(False)
            st = h.profile_stats()
            dev = lambda scope, per: [per * v[1] / v[0] for k, v in st.items() if k.startswith(scope) and v[0]][0]
            cdev, pdev = dev(cscope, 1), dev(pscope, 2)
            bound_ms = 2 * plane_bytes * nplanes / (cal["read_GBps"] * 1e6)      # both fields read once at the calibration's read rate
            q = lambda ts: dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
            emit(dict(base, case=cname, **q(tc), device_ms=round(cdev, 4), device_over_read_once_bound=round(cdev / bound_ms, 2), read_once_bound_ms=round(bound_ms, 4),
                      against=pname, against_call=q(tp), against_device_ms=round(pdev, 4), ms_over_against=round(statistics.median(tc) / statistics.median(tp), 3),
                      device_over_against=round(cdev / pdev, 3), max_error_over_max_value=float(np.abs(got - host[what]).max() / np.abs(host[what]).max())))

    for grid in a.grids.split(","):
        case = parse_text(open(os.path.join(ROOT, "cales_amd", "cases", "turbulent_channel.nml")).read())
        case.ng[:] = [int(x) for x in grid.split("x")]
        case.sgstype = "none"; case.impdiff = 0
        ng = [int(x) for x in case.ng]
        shape = tuple(n + 2 for n in ng)
        plane_bytes = ng[0] * ng[1] * np.dtype(R).itemsize
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
                st = [v for k, v in h.profile_stats().items() if scope and k.startswith(scope)]
                st = st[0] if st else (0, 0.)
                return out, statistics.median(ts), min(ts), max(ts), (st[1] / st[0] if st[0] else None)
            base = {"ng": ng, "lib": os.path.basename(capi.LIB_PATH)}
            if a.digest:
                digest_mode(h, ng, base)
                continue
            cal = h.calibrate(3)
            if a.cross:
                cross_mode(h, ng, cal, base)
                emit({"calibration": {k: (round(v, 1) if isinstance(v, float) else v) for k, v in cal.items()}, "ng": ng, "device": h.device_info()[0]})
                continue
            rng = np.random.RandomState(1)
            x = np.zeros(shape, order="F", dtype=R); x[...] = rng.standard_normal(shape).astype(R)
            h.set("u", x)
            _, get_ms, get_min, get_max, _ = timed(lambda: h.get("u"), calls=max(3, a.calls // 2), warmup=1)
            emit(dict(base, case="get_field(u)", ms=round(get_ms, 3), ms_min=round(get_min, 3), ms_max=round(get_max, 3), bytes=int(np.prod(shape)) * np.dtype(R).itemsize))
            kp = [1 + (q * ng[2]) // 8 for q in range(8)]
            # the route this replaces, and what the device results are compared with
            host = {}
            for what, fn in (("x", lambda f: (np.abs(np.fft.rfft(f, axis=0)) ** 2).sum(1)), ("y", lambda f: (np.abs(np.fft.rfft(f, axis=1)) ** 2).sum(0)),
                             ("planes", lambda f: np.abs(np.fft.fft(np.fft.rfft(f[:, :, [k - 1 for k in kp]], axis=0), axis=1)) ** 2)):
                t0 = time.perf_counter()
                host[what] = fn(h.get("u")[1:-1, 1:-1, 1:-1].astype(np.float64))
                emit(dict(base, case=f"get_field(u) + numpy.fft, {what}", ms=round(1e3 * (time.perf_counter() - t0), 1), calls=1))
            n2 = ng[1]
            fold = host["planes"][:, :n2 // 2 + 1, :].copy()
            fold[:, 1:(n2 + 1) // 2, :] += host["planes"][:, :n2 // 2:-1, :]
            host["planes"] = fold
            for what, call, scope, nplanes in (("x", lambda: h.spectra_lines("u", 1, lsum=False), "spectra_lines", ng[2]), ("y", lambda: h.spectra_lines("u", 2, lsum=False), "spectra_lines", ng[2]),
                                               ("planes", lambda: h.spectra_planes("u", kp), "spectra_planes", 8)):
                got, ms, ms_min, ms_max, dev_ms = timed(call, scope)
                nbytes = plane_bytes * nplanes
                emit(dict(base, case=f"spectra_lines(u, {1 if what == 'x' else 2})" if what != "planes" else "spectra_planes(u, 8 planes)", ms=round(ms, 4), ms_min=round(ms_min, 4),
                          ms_max=round(ms_max, 4), device_ms=round(dev_ms, 4), read_GBps=round(nbytes / dev_ms * 1e-6, 1),
                          fraction_of_read_calibration=round(nbytes / dev_ms * 1e-6 / cal["read_GBps"], 3), ms_over_get_field=round(ms / get_ms, 5),
                          faster_than_get_field=bool(ms < get_ms), max_error_over_max_value=float(np.abs(got - host[what]).max() / host[what].max())))
            emit({"calibration": {k: (round(v, 1) if isinstance(v, float) else v) for k, v in cal.items()}, "ng": ng, "device": h.device_info()[0]})
        finally:
            h.close()
        del x


if __name__ == "__main__":
    main()

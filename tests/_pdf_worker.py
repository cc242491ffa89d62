"""Worker of tests/test_gpu_pdf.py::test_single_precision_library: runs in a process of its own with CALES_PRECISION=single (the precision is a
process-wide choice) and prints one JSON line: how many calls of include/cales_pdf.h it made on float fields, which of them differ from the bin rule
restated in float32 arrays, and how many of them the rule restated in float64 would have got wrong (so the cases tell the precisions apart)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    from cales_amd import capi
    assert capi.SINGLE and capi.lib().cales_real_size() == 4
    from cales_amd.hotpath import HotPath
    from tests.test_gpu_pdf import JNBINS, NBINS, coded, inner, nosgs_channel, pow2_range, random_field
    from tests.test_pdf_host import jpdf_ref, pdf_ref
    calls, wrong, differs = 0, [], 0

    def check(what, got, want, want64):
        nonlocal calls, differs
        calls += 1
        if any(g.dtype != np.int64 or g.shape != w.shape or not np.array_equal(g, w) for g, w in zip(got, want)):
            wrong.append(what)
        differs += any(not np.array_equal(w, v) for w, v in zip(want, want64))
    for ng in ((96, 96, 6), (40, 12, 10)):      # three blocks per plane with a partial last one | rows of 40 floats: the last 16-byte chunk of a row is whole, the pitch is not n1 + 2
        h = HotPath(nosgs_channel(ng))
        n3 = ng[2]
        a, b = coded(ng, 100000.), random_field(ng, 51)
        b[1, 1, 1] = np.nan; b[ng[0], ng[1], n3] = np.inf; b[3, 2, 2] = -np.inf
        one = np.ones(tuple(n + 2 for n in ng), order="F")
        h.set("u", a); h.set("p", b); h.set("dudt", one)
        fa, fb, f1 = inner(a), inner(b), inner(one)
        assert fa.dtype == np.float32
        for nbins in NBINS:
            lo, hi = pow2_range(nbins, 100000.)
            check(f"coded {ng} {nbins}", h.pdf_planes("u", nbins, lo, hi), pdf_ref(fa, nbins, lo, hi), pdf_ref(fa, nbins, lo, hi, np.float64))
            for lo, hi in ((-1.25, 1.75), (-0.1, 0.3)):
                check(f"random {ng} {nbins} {lo}", h.pdf_planes("p", nbins, lo, hi), pdf_ref(fb, nbins, lo, hi), pdf_ref(fb, nbins, lo, hi, np.float64))
            # lo = 1 + 2^-29 is 1 in float: the samples, all 1, are in bin 0 -- in double they would be below
            lo = 1. + 2. ** -29
            check(f"ones {ng} {nbins}", h.pdf_planes("dudt", nbins, lo, 3.), pdf_ref(f1, nbins, lo, 3.), pdf_ref(f1, nbins, lo, 3., np.float64))
        kp = [n3, 1, 3, 3, 2]
        for nbins in JNBINS:
            ra, rb = pow2_range(64, 100000.), (-1.25, 1.75)
            check(f"joint {ng} {nbins}", h.jpdf_planes("u", "p", nbins, ra, rb, kp), jpdf_ref(fa, fb, nbins, ra, rb, kp), jpdf_ref(fa, fb, nbins, ra, rb, kp, np.float64))
            check(f"joint' {ng} {nbins}", h.jpdf_planes("p", "dudt", nbins, rb, (lo, 3.), kp), jpdf_ref(fb, f1, nbins, rb, (lo, 3.), kp), jpdf_ref(fb, f1, nbins, rb, (lo, 3.), kp, np.float64))
        h.close()
    print("RESULT " + json.dumps({"real": np.dtype(capi.np_real).name, "real_size": capi.lib().cales_real_size(), "calls": calls, "wrong": wrong,
                                  "differs_from_float64": int(differs)}))


if __name__ == "__main__":
    main()

"""Worker of tests/test_gpu_cospectra.py::test_single_precision_library: runs in a process of its own with CALES_PRECISION=single (the precision is a
process-wide choice) and prints one JSON line: how many comparisons of include/cales_cospectra.h results on float fields with the checker it made, which
of them miss the bounds taken with float32's eps, the largest error / bound ratio and its case, and how many miss the same bounds taken with float64's
eps (so the cases tell the precisions apart: a library that computed in double would miss none)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    from cales_amd import capi
    assert capi.SINGLE and capi.lib().cales_real_size() == 4
    from cales_amd.hotpath import HotPath
    from tests.test_gpu_pdf import nosgs_channel
    from tests.test_gpu_cospectra import all_cases
    eps32, eps64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
    calls, wrong, differs, largest, where = 0, [], 0, 0., ""
    # stages 4 4 2 3 | pitch 64 != n1 + 2, the direct sum in y | the direct sum in x | nl = 4 | the cap in x, nl = 2 | the longest staged and direct y
    # lines: tiles of 2 columns, narrower than a 16-byte chunk of floats | six blocks per plane | two batches per block
    for ng in ((96, 12, 10), (40, 26, 6), (56, 20, 4), (1024, 4, 2), (2048, 2, 2), (16, 2000, 2), (16, 2046, 2), (48, 42, 3), (16, 2000, 10)):
        h = HotPath(nosgs_channel(ng))
        for pair in (("u", "w"), ("p", "u")):
            res = all_cases(h, ng, pair, eps32, 61)
            for what, r in res.items():
                calls += 1
                if r > largest:
                    largest, where = r, f"{ng} {pair} {what}"
                if not r <= 1.:
                    wrong.append(f"{ng} {pair} {what}: {r:.3e}")
                differs += bool(r * eps32 / eps64 > 1.)
        h.close()
    print("RESULT " + json.dumps({"real": np.dtype(capi.np_real).name, "real_size": capi.lib().cales_real_size(), "calls": calls, "wrong": wrong,
                                  "largest_ratio": largest, "largest_case": where, "differs_from_float64": int(differs)}))


if __name__ == "__main__":
    main()

"""Worker of tests/test_gpu_derived.py::test_single_precision_library: runs in a process of its own with CALES_PRECISION=single (the precision is a
process-wide choice) and prints one JSON line: how many results of include/cales_derived.h on float fields it compared with the restatement in float32
(np.array_equal), which of them differ, and how many dense volumes differ from the float64 restatement rounded to float (so the cases tell the precisions
apart: a library that computed in double and rounded at the end would match that one instead)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    from cales_amd import capi
    assert capi.SINGLE and capi.lib().cales_real_size() == 4
    from cales_amd.hotpath import HotPath
    from tests.test_derived_host import NAMES, derived_ref, metrics_of
    from tests.test_gpu_derived import KINDS, by_value, case_of, random_state, reference, same
    calls, wrong, differs = 0, [], 0
    # rows longer than a wave | pitch 64 != n1 + 2 | long rows, two planes | smaller than a wave everywhere
    for kind in KINDS:
        for ng in ((96, 12, 10), (40, 26, 6), (1024, 4, 2), (8, 4, 4)):
            case = case_of(kind, ng)
            h = HotPath(case)
            u, v, w = random_state(ng, 300 + ng[0])
            assert u.dtype == np.float32
            h.set("u", u); h.set("v", v); h.set("w", w)
            ref = reference(case, u, v, w)
            n, bad = by_value(h, ng, ref)
            calls += n
            wrong += [f"{kind} {ng} {b}" for b in bad]
            h.derived_to_pp("qcr")
            calls += 1
            if not same(h.read_box("pp", (1, 1, 1), ng), ref["qcr"]):
                wrong.append(f"{kind} {ng} to_pp")
            ref64 = derived_ref(u, v, w, *metrics_of(case, np.float32), np.float64)
            differs += sum(int(not np.array_equal(ref64[name].astype(np.float32), h.derived_out3d(name))) for name in NAMES)
            h.close()
    print("RESULT " + json.dumps({"real": np.dtype(capi.np_real).name, "real_size": capi.lib().cales_real_size(), "calls": calls, "wrong": wrong,
                                  "differs_from_float64": int(differs)}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes plans.json beside this file: the cales_describe_plan strings of the cases of tests/test_gpu_solver_schedule.py, per rank, as the library in use
prints them -- run with the library of the commit to compare with (CALES_LIB=<its libcales_hip.so>), on a GPU. Prints what that library gives for the
other two tests of that file as well: the largest difference between the chunked and the in-order solves, and what a step allocates."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from tests import test_gpu_solver_schedule as T      # noqa: E402


def main():
    plans = {}
    for ng, P, nch in T.SHAPES:
        a, b = T.tgv_run(ng, P, True), T.tgv_run(ng, P, False)
        plans[T._key("tgv_dsmag_ppp", ng, P, True)] = [x[5] for x in a]
        plans[T._key("tgv_dsmag_ppp", ng, P, False)] = [x[5] for x in b]
        diff = max(float(np.abs(a[r][q] - b[r][q]).max()) for r in range(P) for q in range(5))
        print(ng, "ranks", P, "exchanges per step", [x[6] for x in a], [x[6] for x in b], "largest difference second stream - in order", diff, flush=True)
    for P, overlap in ((1, False), (2, True)):
        out = T.memory_run(P, overlap)
        plans[T._key("chan_dsmag", (64, 16, 16), P, overlap)] = [x[2] for x in out]
        for r, (before, after, plan) in enumerate(out):
            print("chan_dsmag (64, 16, 16) ranks", P, "rank", r, "bytes, allocations before the first step", before, "after two", after,
                  "difference", (after[0] - before[0], after[1] - before[1]), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plans.json"), "w") as f:
        json.dump(plans, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

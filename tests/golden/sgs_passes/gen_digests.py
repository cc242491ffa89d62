#!/usr/bin/env python3
"""Writes digests.json beside this file: per case of tests/test_gpu_sgs_passes.py the plan strings and the SHA-256 of the bytes of every result, as
the library in use gives them -- run with the library of the commit to compare with (CALES_LIB=<its libcales_hip.so>), on a GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from tests import test_gpu_sgs_passes as T      # noqa: E402


def main():
    out = {}
    for case in T.CASES:
        out[T.case_id(*case)] = T.run_case(*case)
        print(T.case_id(*case), out[T.case_id(*case)], flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

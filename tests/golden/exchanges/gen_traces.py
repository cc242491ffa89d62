#!/usr/bin/env python3
"""Writes traces.json beside this file: what tests/test_gpu_exchanges.py records of its cases -- per rank the hook calls in their order, the size of the staging
buffers, the plan string and a SHA-256 of every downloaded field -- as the library in use gives them. Run with the library of the commit to compare with
(CALES_LIB=<its libcales_hip.so>), on a GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from tests import test_gpu_exchanges as T      # noqa: E402


def main():
    traces = {}
    for key in sorted(T.CASES):
        traces[key] = T.run(key)
        for r, a in enumerate(traces[key]):
            print(key, "rank", r, "nbuf", a["nbuf"], "calls", len(a["trace"]), a["plan"], flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "traces.json"), "w") as f:
        json.dump(traces, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/reductions/<case>.npz and prints the SEQUENCES literal of tests/test_gpu_reductions.py: the outputs of THIS library's
reduction and statistics entries (one rank and two loopback ranks) and the all-reduce callbacks its hosts see, as the library at hand computes
them. Run on a GPU from the repository root, on the commit whose behaviour is to be pinned:

    python tests/golden/reductions/gen_reductions.py [--check] [--out DIR]

--check: write nothing, run everything a second time and report every value that differs between the two runs (run-to-run reproducibility)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import test_gpu_reductions as T      # noqa: E402


def collect():
    vals, seqs = {}, {}
    for key in sorted(T.CASES):
        vals[key] = {}
        for nranks in (1, 2):
            T.run.cache_clear()
            v, seq = T.run(key, nranks)
            for r in range(nranks):
                for name, a in v[r].items():
                    vals[key][f"p{nranks}_r{r}_{name}"] = a
            if nranks == 2:
                per_rank = [{p: seq[r][p] for p in T.PHASES} for r in range(2)]
                assert per_rank[0] == per_rank[1], (key, per_rank)
                seqs[key] = per_rank[0]
                print(f"# {key}: all-reduces of the entries after the step (not pinned): {seq[0]['entries']}")
    return vals, seqs


def main():
    check = "--check" in sys.argv[1:]
    vals, seqs = collect()
    print("SEQUENCES = {")
    for key in sorted(seqs):
        print(f"    {key!r}: {seqs[key]!r},")
    print("}")
    if check:
        again, seqs2 = collect()
        bad = [(k, n) for k in vals for n in vals[k] if not np.array_equal(vals[k][n], again[k][n])]
        print("second run: sequences", "equal" if seqs2 == seqs else "DIFFER", "; values differing:", bad if bad else "none", "of", sum(len(v) for v in vals.values()))
        return 1 if bad or seqs2 != seqs else 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.dirname(os.path.abspath(__file__))
    os.makedirs(out, exist_ok=True)
    for key, d in vals.items():
        np.savez_compressed(os.path.join(out, key + ".npz"), **d)
        print("wrote", key + ".npz", len(d), "arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())

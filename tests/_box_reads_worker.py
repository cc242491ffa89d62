"""Worker of tests/test_gpu_box_reads.py::test_single_precision_library: runs in a process of its own with CALES_PRECISION=single (the precision is a
process-wide choice) and prints one JSON line: how many reads of include/cales_post.h it made on integer-coded float fields and which of them differ
from numpy slicing of the uploaded array."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    from cales_amd import capi
    assert capi.SINGLE and capi.lib().cales_real_size() == 4
    from cales_amd.hotpath import HotPath
    from tests.test_gpu_box_reads import box_of, coded, nosgs_channel
    ng = (96, 12, 10)
    a = coded(ng).astype(np.float32, order="F")
    h = HotPath(nosgs_channel(ng))
    h.set("u", a)
    top = tuple(n + 1 for n in ng)
    reads, wrong, dtypes = 0, [], set()

    def check(what, got, want):
        nonlocal reads
        reads += 1; dtypes.add(str(got.dtype))
        if got.shape != want.shape or not np.array_equal(got, want):
            wrong.append(what)
    check("whole", h.read_box("u", (0, 0, 0), top), a)
    check("interior", h.read_box("u", (1, 1, 1), ng), a[1:-1, 1:-1, 1:-1])
    for inorm in (1, 2, 3):
        for islice in (1, ng[inorm - 1] // 2, ng[inorm - 1]):
            sl = [slice(1, -1)] * 3; sl[inorm - 1] = slice(islice, islice + 1)
            check(f"out2d {inorm} {islice}", h.out2d("u", inorm, islice), a[tuple(sl)])
    for ns in ((1, 1, 1), (2, 3, 4), (7, 1, 1), (200, 200, 200)):
        check(f"out3d {ns}", h.out3d("u", ns), a[1:-1:ns[0], 1:-1:ns[1], 1:-1:ns[2]])
    rng = np.random.RandomState(9)
    for q in range(10):
        lo = [int(rng.randint(0, t + 1)) for t in top]
        hi = [int(rng.randint(l, t + 1)) for l, t in zip(lo, top)]
        ns = [int(rng.choice([1, 2, 3, 65])) for _ in range(3)]
        check(f"box {lo} {hi} {ns}", h.read_box("u", lo, hi, ns), box_of(a, lo, hi, ns))
    h.close()
    print("RESULT " + json.dumps({"dtype": dtypes.pop() if len(dtypes) == 1 else sorted(dtypes), "real_size": capi.lib().cales_real_size(), "reads": reads, "wrong": wrong}))


if __name__ == "__main__":
    main()

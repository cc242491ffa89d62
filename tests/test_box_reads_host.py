"""include/cales_post.h without a GPU: the header against capi.POST_SYMBOLS and the two libraries, and cales_box_share -- which points of a strided box of
global haloed indices a rank of the y-slab decomposition holds -- against plain Python index arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cales_amd import capi
from cales_amd.hotpath import CalesError, box_share
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = (16, 12, 10)
RANKS = (1, 2, 3, 4, 6)


def post_header_declarations():
    """the text of include/cales_post.h without its comments (they name entries of cales.h)"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cales_post.h")).read(), flags=re.S)


def test_post_header_equals_the_symbol_list_and_both_libraries_export_it():
    hdr = post_header_declarations()
    assert '#include "cales.h"' in hdr
    declared = set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.POST_SYMBOLS) and len(capi.POST_SYMBOLS) == 4, declared ^ set(capi.POST_SYMBOLS)
    assert not set(capi.POST_SYMBOLS) & set(capi.SYMBOLS)      # the list of cales.h is a list of its own
    if os.environ.get("CALES_NO_TORCH") != "1":
        import torch  # noqa: F401  (one HIP runtime per process: see capi.lib)
    for so in ("libcales_hip.so", "libcales_hip_sp.so"):
        L = C.CDLL(os.path.join(ROOT, "cales_amd", so))
        for s in capi.POST_SYMBOLS:
            assert hasattr(L, s), (so, s)
    for s in capi.POST_SYMBOLS:
        assert getattr(capi.lib(), s).argtypes, s      # bound with argument types by capi.lib()


def _case():
    g, case = load_golden("chan_smag")
    case.ng[:] = NG
    return case


def _boxes():
    """200 boxes (lo, hi, nskip), fixed seed: hand-made ones for the edges of the share rule, then random ones"""
    top = [n + 1 for n in NG]
    boxes = [((0, 0, 0), tuple(top), (1, 1, 1)),                                  # the whole haloed field: rows 0 and ng2+1
             ((1, 1, 1), NG, (1, 1, 1)),                                          # the interior
             ((3, 0, 2), (3, 0, 2), (1, 1, 1)), ((3, 13, 2), (3, 13, 2), (1, 1, 1)),      # lo = hi, in the global ghost rows
             ((1, 6, 1), (16, 6, 10), (1, 1, 1)),                                 # one row: empty on every rank but its owner
             ((1, 7, 1), (16, 7, 10), (2, 5, 3)), ((0, 4, 0), (17, 4, 11), (1, 13, 1))]
    for s in (1, 2, 5, 13):
        boxes += [((0, 0, 0), tuple(top), (1, s, 1)), ((2, 1, 1), (9, 12, 4), (3, s, 2)), ((0, 3, 5), (17, 13, 5), (1, s, 1))]
    rng = np.random.RandomState(20)
    while len(boxes) < 200:
        lo = [int(rng.randint(0, t + 1)) for t in top]
        hi = [int(rng.randint(l, t + 1)) for l, t in zip(lo, top)]
        ns = [int(rng.choice([1, 1, 2, 3, 5, 13])) for _ in range(3)]
        boxes.append((tuple(lo), tuple(hi), tuple(ns)))
    return boxes


def _owned_rows(nranks, rank):
    n2 = NG[1] // nranks
    rows = set(range(rank * n2 + 1, (rank + 1) * n2 + 1))
    if rank == 0:
        rows.add(0)
    if rank == nranks - 1:
        rows.add(NG[1] + 1)
    return rows


def test_the_box_set_has_the_cases_that_matter():
    boxes = _boxes()
    assert len(boxes) == 200
    ys = [list(range(lo[1], hi[1] + 1, ns[1])) for lo, hi, ns in boxes]
    assert any(0 in y for y in ys) and any(NG[1] + 1 in y for y in ys) and any(0 in y and NG[1] + 1 in y for y in ys)
    assert {1, 2, 5, 13} <= {ns[1] for _, _, ns in boxes}
    assert any(lo == hi for lo, hi, _ in boxes)


@pytest.mark.parametrize("nranks", RANKS)
def test_box_share_against_index_arithmetic(nranks):
    case = _case()
    empty = 0
    for lo, hi, ns in _boxes():
        pts = [list(range(lo[d], hi[d] + 1, ns[d])) for d in range(3)]
        seen = []
        for rank in range(nranks):
            first, count = box_share(case, lo, hi, ns, nranks=nranks, rank=rank)
            for d in (0, 2):      # x and z: every point of the box
                assert (first[d], count[d]) == (lo[d], len(pts[d])), (lo, hi, ns, rank, d)
            mine = [j for j in pts[1] if j in _owned_rows(nranks, rank)]
            assert count[1] == len(mine), (lo, hi, ns, rank)
            if mine:
                assert first[1] == mine[0] and list(range(first[1], first[1] + count[1] * ns[1], ns[1])) == mine, (lo, hi, ns, rank)
            else:
                empty += 1
            assert not set(mine) & set(seen), (lo, hi, ns, rank)      # disjoint
            seen += mine
        assert seen == pts[1], (lo, hi, ns)      # the union, in rank order, is the global list
    assert (empty > 0) == (nranks > 1)      # shares without a row occur (and cannot on one rank)


@pytest.mark.parametrize("lo,hi,ns,what", [
    ((1, 1, 1), NG, (1, 0, 1), "nskip < 1"), ((1, 1, 1), NG, (-2, 1, 1), "nskip < 1"),
    ((1, -1, 1), NG, (1, 1, 1), "lo < 0"), ((1, 1, 1), (16, 12, 12), (1, 1, 1), "hi > ng+1"), ((18, 1, 1), (18, 12, 10), (1, 1, 1), "hi > ng+1"),
    ((5, 1, 1), (4, 12, 10), (1, 1, 1), "lo > hi")])
def test_box_share_refuses_with_a_message(lo, hi, ns, what):
    case = _case()
    cs = capi.make_case(case, 2, 1)
    i3 = lambda v: (C.c_int32 * 3)(*v)
    first, count = i3((0, 0, 0)), i3((0, 0, 0))
    L = capi.lib()
    assert L.cales_box_share(C.byref(cs), i3(lo), i3(hi), i3(ns), first, count) != 0
    assert what in L.cales_last_error(None).decode()
    with pytest.raises(CalesError, match=re.escape(what)):
        box_share(case, lo, hi, ns, nranks=2, rank=1)
    # ... and the next valid question is answered
    assert box_share(case, (0, 0, 0), (17, 13, 11), (1, 1, 1), nranks=2, rank=1) == ((0, 7, 0), (18, 7, 12))

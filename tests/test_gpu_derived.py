"""include/cales_derived.h on the device: cales_derived_box / _out2d / _out3d / _to_pp (k_derived.hip) by value against the numpy restatement of the
reference's src/post.f90 (tests/test_derived_host.py: derived_ref). The kernels call the functions of derived_math.hpp with contraction off, every
operation one IEEE rounding in the order of post.f90, and the restatement does the same in numpy: the comparison is np.array_equal, in double here and
in single precision through tests/_derived_worker.py, and no tolerance appears anywhere in this file.

The fields are random normal in the interior AND in the ghost cells, with NaN in the eight-fold set of cells with three ghost indices (the corners of
the haloed array): the quantities read ghost cells with one and with two ghost indices, never one with three, and a kernel that did would poison its
result. A quantity is a function of the haloed arrays as the context holds them, so the reference is formed from the very arrays that were set.

Cases: the explicit channel of tests/test_gpu_pdf.py (stretched z: dzci(k-1) != dzci(k), dzfi) and the triply periodic golden tgv_ppp resized
(uniform z).

Two kernel forms (k_derived.hip): a dense box -- nskip = (1, 1, 1), whole rows of at least 64 cells -- goes to k_derived_rows (tiles of 64 x 8 cells marching
along z with the planes k-1, k, k+1 in a ring of three LDS slots; profile scope derived_rows), every other box, and every box under
CALES_DERIVED_POINTS=1, to k_derived_points (derived_points). Grids, chosen for where the kernels can go wrong, not for the workload:
  (96, 12, 10)   rows longer than a wave: the x seam between a full tile and one of 32 cells; 12 rows: a tile of 8 and one of 4
  (40, 26, 6)    row pitch 48 != n1 + 2, and rows shorter than 64 cells: the dense volume takes the points form (the scope is asserted)
  (64, 16, 12)   powers of two
  (1024, 4, 2)   many x tiles, half a y tile, two planes: the ring never wraps
  (64, 4, 40)    the ring wraps many times
  (8, 4, 4)      smaller than a tile everywhere; cales_create accepts it (cales_check_case asks for ng >= 2, ng(1:2) even)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_derived_host import NAMES, derived_ref, metrics_of
from tests.test_gpu_pdf import nosgs_channel
from tests.test_pdf_host import pdf_ref
from tests.util import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(96, 12, 10), (40, 26, 6), (64, 16, 12), (1024, 4, 2), (64, 4, 40), (8, 4, 4)]
KINDS = ("chan", "tgv")


def case_of(kind, ng):
    if kind == "chan":
        return nosgs_channel(ng)
    g, case = load_golden("tgv_ppp"); case.ng[:] = ng
    return case


def random_state(ng, seed):
    """u, v, w: standard normal in every cell, NaN in the eight cells with three ghost indices"""
    from cales_amd import capi
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(3):
        a = np.asfortranarray(rng.randn(*[n + 2 for n in ng]), dtype=capi.np_real)
        for c in np.ndindex(2, 2, 2):
            a[tuple(-q for q in c)] = np.nan
        out.append(a)
    return out


def reference(case, u, v, w, live=NAMES):
    """the restatement on haloed arrays, with the metrics of a context of `case`; `live`: the quantities that must not vanish there"""
    from cales_amd import capi
    dli, dzci, dzfi = metrics_of(case, capi.np_real)
    ref = derived_ref(u, v, w, dli, dzci, dzfi, capi.np_real)
    for name, a in ref.items():
        assert np.isfinite(a).all() and (name not in live or np.abs(a).max() > 0.), name      # (no NaN reaches the restatement either)
    return ref


def box_of(a, lo, hi, ns):
    """the box of GLOBAL indices 1 ... ng of an interior array"""
    return a[tuple(slice(l - 1, h, s) for l, h, s in zip(lo, hi, ns))]


def boxes_of(ng):
    """(lo, hi, nskip): the dense volume, a strided box from the first and one into the last cell, a box of one row, the corner points"""
    mid = tuple((n + 1) // 2 for n in ng)
    return [((1, 1, 1), ng, (1, 1, 1)), ((1, 1, 1), ng, (3, 2, 2)), (tuple(min(2, n) for n in ng), ng, (5, 1, 3)), ((1, mid[1], mid[2]), (ng[0], mid[1], mid[2]), (1, 1, 1)),
            ((1, 1, 1), (1, 1, 1), (1, 1, 1)), (ng, ng, (1, 1, 1)), (mid, mid, (7, 7, 7))]


def scope_of(ng, lo, hi, ns):
    """the profile scope of a box: the dense form takes whole rows of at least 64 cells with nskip = 1"""
    dense = tuple(ns) == (1, 1, 1) and lo[0] == 1 and hi[0] == ng[0] and ng[0] >= 64
    return "derived_rows" if dense else "derived_points"


def same(got, want):
    from cales_amd import capi
    return got.dtype == capi.np_real and got.flags.f_contiguous and got.shape == want.shape and np.array_equal(got, want)


def by_value(h, ng, ref, names=NAMES):
    """every entry that returns values, on the velocity the context holds: (number of comparisons, the ones that differ)"""
    n, wrong = 0, []
    for name in names:
        want = ref[name]
        for lo, hi, ns in boxes_of(ng):
            n += 1
            if not same(h.derived_box(name, lo, hi, ns), box_of(want, lo, hi, ns)):
                wrong.append((name, "box", lo, hi, ns))
        for inorm in (1, 2, 3):
            for islice in sorted({1, (ng[inorm - 1] + 1) // 2, ng[inorm - 1]}):
                sl = [slice(None)] * 3; sl[inorm - 1] = slice(islice - 1, islice)
                n += 1
                if not same(h.derived_out2d(name, inorm, islice), want[tuple(sl)]):
                    wrong.append((name, "out2d", inorm, islice))
        for ns in ((1, 1, 1), (2, 3, 4), (200, 1, 1)):
            n += 1
            if not same(h.derived_out3d(name, ns), want[::ns[0], ::ns[1], ::ns[2]]):
                wrong.append((name, "out3d", ns))
    return n, wrong


@pytest.fixture(scope="module", params=[(k, ng) for k in KINDS for ng in GRIDS], ids=lambda p: p[0] + "-" + "x".join(map(str, p[1])))
def loaded(request):
    """one context per case and grid with a random velocity set, and the restatement on those arrays, computed once; the tests below read only, or
    write pp alone"""
    from cales_amd.hotpath import HotPath
    kind, ng = request.param
    case = case_of(kind, ng)
    h = HotPath(case)
    u, v, w = random_state(ng, 100 + GRIDS.index(ng))
    h.set("u", u); h.set("v", v); h.set("w", w)
    yield h, ng, reference(case, u, v, w)
    h.close()


def test_all_nine_quantities_by_value(loaded):
    h, ng, ref = loaded
    n, wrong = by_value(h, ng, ref)
    assert n == 9 * (7 + 3 + sum(len({1, (m + 1) // 2, m}) for m in ng)) and wrong == [], wrong[:10]


def test_same_bits_from_run_to_run(loaded):
    h, ng, ref = loaded
    first = [h.derived_out3d(name) for name in NAMES]
    for _ in range(2):
        assert all(np.array_equal(a, h.derived_out3d(name)) for a, name in zip(first, NAMES))


def test_the_two_forms_give_the_same_bits(loaded, monkeypatch):
    """the dense volume, a dense slab of rows and planes, and to_pp under CALES_DERIVED_POINTS=1 (read when the context is created) against the
    default; the profile scope shows which form ran"""
    from cales_amd.hotpath import HotPath
    h, ng, ref = loaded
    monkeypatch.setenv("CALES_DERIVED_POINTS", "1")
    hp = HotPath(h.case)
    monkeypatch.delenv("CALES_DERIVED_POINTS")
    top = tuple(n + 1 for n in ng)
    for name in ("u", "v", "w"):
        hp.set(name, h.read_box(name, (0, 0, 0), top))
    part = ((1, min(2, ng[1]), min(2, ng[2])), (ng[0], ng[1], max(ng[2] - 1, min(2, ng[2]))), (1, 1, 1))
    stats = []
    for ctx in (h, hp):
        ctx.profile_reset(); ctx.profile(True)
        out = []
        for name in NAMES:
            out += [ctx.derived_out3d(name), ctx.derived_box(name, *part)]
            ctx.derived_to_pp(name); out.append(ctx.read_box("pp", (1, 1, 1), ng))
        ctx.profile(False)
        stats.append(({k: v[0] for k, v in ctx.profile_stats().items() if v[0] and k.startswith("derived")}, out))
    hp.close()
    (st, out), (stp, outp) = stats
    assert stp == {"derived_points": 3 * len(NAMES)}, stp
    assert st == {("derived_rows" if ng[0] >= 64 else "derived_points"): 3 * len(NAMES)}, st
    for q, (a, b) in enumerate(zip(out, outp)):
        assert np.array_equal(a, b), (NAMES[q // 3], q % 3)
    for q, name in enumerate(NAMES):
        assert same(out[3 * q], ref[name]) and same(out[3 * q + 2], ref[name])


def test_to_pp_writes_the_interior_and_every_read_out_works_on_it(loaded):
    from cales_amd import capi
    h, ng, ref = loaded
    top = tuple(n + 1 for n in ng)
    pp0 = np.asfortranarray(np.random.RandomState(9).randn(*[n + 2 for n in ng]), dtype=capi.np_real)
    for name in ("qcr", "vox", "voz_edge", "str"):
        h.set("pp", pp0)
        h.derived_to_pp(name)
        got = h.read_box("pp", (0, 0, 0), top)
        want = pp0.copy(order="F"); want[1:-1, 1:-1, 1:-1] = ref[name]      # the ghost cells are left as they were
        assert np.array_equal(got, want), name
        assert np.array_equal(h.read_box("pp", (1, 1, 1), ng), h.derived_box(name, (1, 1, 1), ng)), name
    # the integer counts numpy gives on the restatement's Q by the bin rule of include/cales_pdf.h
    h.derived_to_pp("qcr")
    q = ref["qcr"]
    hi = 2. ** np.ceil(np.log2(np.abs(q).max())); lo = -hi      # (the restatement's own range: s = nbins / (hi - lo) is a power of two)
    counts, outside = h.pdf_planes("pp", 64, lo, hi)
    wc, wo = pdf_ref(q, 64, lo, hi)
    assert np.array_equal(counts, wc) and np.array_equal(outside, wo) and counts.sum() + outside.sum() == q.size and counts.sum() >= q.size - 1
    # ... and the line spectrum of a vorticity component is that of the field read back
    h.derived_to_pp("voz")
    from tests.test_spectra_host import line_bounds, spectra_ref
    power = h.spectra_lines("pp", 1, lsum=False)
    f = ref["voz"]
    assert (np.abs(power - spectra_ref(f)["power_x"]) <= line_bounds(f, 1, float(np.finfo(capi.np_real).eps))[0][None, :]).all()


def test_calls_have_one_profile_scope_and_allocate_nothing(loaded):
    h, ng, ref = loaded
    before = h.memory_in_use()
    h.profile_reset(); h.profile(True)
    want = {}
    for q, name in enumerate(NAMES):
        ns, inorm = (1 + q % 3, 1, 1 + q % 2), 1 + q % 3
        h.derived_box(name, (1, 1, 1), ng, ns); h.derived_out2d(name, inorm, 1); h.derived_out3d(name, (2, 1, 1)); h.derived_to_pp(name)
        assert h.memory_in_use() == before
        lo, hi = [1, 1, 1], list(ng); hi[inorm - 1] = 1
        for sc in (scope_of(ng, (1, 1, 1), ng, ns), scope_of(ng, lo, hi, (1, 1, 1)), "derived_points", scope_of(ng, (1, 1, 1), ng, (1, 1, 1))):
            want[sc] = want.get(sc, 0) + 1
    h.profile(False)
    st = {k: v[0] for k, v in h.profile_stats().items() if v[0]}
    assert st == want and sum(st.values()) == 4 * len(NAMES), (st, want)      # one launch per call, under a scope named after its form, and nothing else ran
    assert ("derived_rows" in st) == (ng[0] >= 64)
    assert h.memory_in_use() == before


def test_refusals_launch_nothing_and_leave_the_context_usable(loaded):
    from cales_amd import capi
    from cales_amd.hotpath import CalesError
    h, ng, ref = loaded
    L, H = h.L, h.h
    i3 = lambda v: (C.c_int32 * 3)(*v)
    buf = np.zeros(ng, order="F", dtype=capi.np_real)
    P, cnt = buf.ctypes.data_as(C.c_void_p), i3((0, 0, 0))
    one = (1, 1, 1)
    Q = capi.DERIVED["qcr"]
    box = lambda q=Q, lo=one, hi=ng, ns=one, p=P: L.cales_derived_box(H, q, i3(lo), i3(hi), i3(ns), p, cnt)
    refused = {"quantity -1": lambda: box(q=-1), "quantity 9": lambda: box(q=9), "out2d quantity 9": lambda: L.cales_derived_out2d(H, 9, 1, 1, P, cnt),
               "out3d quantity -1": lambda: L.cales_derived_out3d(H, -1, i3(one), P, cnt), "to_pp quantity 9": lambda: L.cales_derived_to_pp(H, 9),
               "to_pp quantity -1": lambda: L.cales_derived_to_pp(H, -1),
               "nskip < 1": lambda: box(ns=(1, 0, 1)), "nskip < 1 (out3d)": lambda: L.cales_derived_out3d(H, Q, i3((0, 1, 1)), P, cnt),
               "lo > hi": lambda: box(lo=(1, 2, 1), hi=(ng[0], 1, ng[2])), "NULL buf": lambda: box(p=None),
               "NULL lo": lambda: L.cales_derived_box(H, Q, None, i3(ng), i3(one), P, cnt),
               "islice = 0": lambda: L.cales_derived_out2d(H, Q, 2, 0, P, cnt), "islice = ng+1": lambda: L.cales_derived_out2d(H, Q, 3, ng[2] + 1, P, cnt),
               "inorm = 0": lambda: L.cales_derived_out2d(H, Q, 0, 1, P, cnt), "inorm = 4": lambda: L.cales_derived_out2d(H, Q, 4, 1, P, cnt)}
    for d in range(3):      # the quantities are those of interior cells: the ghost cells cales_read_box accepts are refused
        lo = list(one); lo[d] = 0
        hi = list(ng); hi[d] = ng[d] + 1
        refused[f"lo = 0 in {'xyz'[d]}"] = lambda lo=tuple(lo): box(lo=lo)
        refused[f"hi = ng+1 in {'xyz'[d]}"] = lambda hi=tuple(hi): box(hi=hi)
    pp = h.read_box("pp", (0, 0, 0), tuple(n + 1 for n in ng))
    h.profile_reset(); h.profile(True)
    for q, (what, call) in enumerate(refused.items()):
        assert call() != 0, what
        assert L.cales_last_error(H).decode(), what
        name = NAMES[q % 9]
        assert same(h.derived_out3d(name, (1 + q % 2, 1, 1)), ref[name][::1 + q % 2]), what
    h.profile(False)
    st = {k: v[0] for k, v in h.profile_stats().items() if v[0]}
    assert sum(st.values()) == len(refused) and set(st) <= {"derived_points", "derived_rows"}, st      # (the valid calls in between; a refused call launched nothing)
    assert not buf.any() and np.array_equal(h.read_box("pp", (0, 0, 0), tuple(n + 1 for n in ng)), pp, equal_nan=True)
    for bad in (lambda: h.derived_out2d("qcr", 2, 0), lambda: h.derived_out3d("qcr", (1, 0, 1)), lambda: h.derived_box("qcr", (0, 1, 1), ng), lambda: h.derived_to_pp(9)):
        with pytest.raises(CalesError):
            bad()
    with pytest.raises(KeyError):
        h.derived_to_pp("helicity")


# ---------------------------------------------------------------------------------------------- the rules of every field-reading entry
def derived_ctx_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cales_derived.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(\s*(?:const\s+)?cales_ctx\s*\*", hdr)))


def entry_table(ng):
    """every entry of the header on quantity Q, as a host calls it: returns the values it produced as an interior-shaped array or a part of one, and
    the slices of the restatement they are to equal"""
    mid = ng[1] // 2

    def to_pp(h):
        h.derived_to_pp("qcr")
        return h.read_box("pp", (1, 1, 1), ng)
    return {"cales_derived_box": (lambda h: h.derived_box("qcr", (1, 1, 1), ng, (1, 3, 2)), (slice(None), slice(None, None, 3), slice(None, None, 2))),
            "cales_derived_out2d": (lambda h: h.derived_out2d("qcr", 2, mid), (slice(None), slice(mid - 1, mid), slice(None))),
            "cales_derived_out3d": (lambda h: h.derived_out3d("qcr", (1, 1, 1)), (slice(None),) * 3),
            "cales_derived_to_pp": (to_pp, (slice(None),) * 3)}


def test_every_derived_entry_sees_the_projected_state(monkeypatch):
    """The scheme of tests/test_gpu_box_reads.py::test_every_post_entry_sees_the_projected_state for the fifth header: every entry of
    include/cales_derived.h, enumerated from the header, completes a projection that cales_step left pending before it reads -- and what it returns is
    the restatement on the state downloaded afterwards"""
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    g, case = load_golden("cavity_nnn"); case.ng[:] = (32, 16, 12)
    ng = (32, 16, 12)
    entries, table = derived_ctx_entries(), entry_table(ng)
    assert entries and sorted(table) == entries == sorted(capi.DERIVED_SYMBOLS), f"entries of include/cales_derived.h without a rule: {set(entries) ^ set(table)}"
    u0 = initflow(case)
    for e in entries:
        call, part = table[e]
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.5 * h.chkdt()
        ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))
        h.profile(True)
        h.step(dt)
        assert ncorr() == 0, (e, "the step was expected to leave its last projection pending")
        got = call(h)
        n1 = ncorr()
        assert n1 >= 1, (e, "did not complete the pending projection")
        u, v, w = h.download()[:3]
        assert ncorr() == n1, e              # ... and nothing was pending any more
        assert h.chkdiv()[1] < 1e-12, e
        want = reference(case, u, v, w, live=("qcr",))["qcr"][part]
        assert same(got, want), e
        h.profile(False); h.close()


def test_first_reader_of_stale_x_ghost_columns(monkeypatch):
    """The scheme of tests/test_gpu_box_reads.py::test_first_reader_of_stale_x_ghost_columns with every entry of the header in turn as the first entry
    after three steps, on cells that read the columns i = 0 and i = n1 + 1: the same bits as the eager form, in what the entry returns and in
    everything read after it, and the restatement on the downloaded state"""
    from cales_amd.hotpath import HotPath, initflow
    ng = (64, 16, 12)
    g, case = load_golden("chan_dsmag"); case.ng[:] = ng
    u0 = initflow(case)
    rng = np.random.RandomState(2)
    for a in u0[:3]:
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    table = entry_table(ng)

    def run(call):
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.4 * h.chkdt()
        for _ in range(3):
            h.step(dt)
        got = call(h)
        out = [got] + h.download()[:4] + [np.asarray(h.chkdt()), np.asarray(h.chkdiv())]      # (pp is the entry's to overwrite: not compared)
        h.close()
        return out
    for e, (call, part) in table.items():
        monkeypatch.delenv("CALES_EAGER_PROJECTION", raising=False)
        lazy = run(call)
        monkeypatch.setenv("CALES_EAGER_PROJECTION", "1")
        eager = run(call)
        for q, (a, b) in enumerate(zip(lazy, eager)):
            assert np.array_equal(a, b), (e, q)
        assert same(lazy[0], reference(case, *lazy[1:4], live=("qcr",))["qcr"][part]), e


# ---------------------------------------------------------------------------------------------- y-slabs
SLAB_NG = (32, 12, 10)
SLAB_READS = [("vox", "derived_box", ((1, 1, 1), SLAB_NG, (1, 1, 1))),
              ("qcr", "derived_box", ((2, 1, 1), (30, 12, 9), (3, 11, 2))),       # rows 1 and 12 alone: the ranks in the middle hold nothing
              ("str", "derived_box", ((1, 5, 1), (32, 6, 10), (1, 1, 1))),        # two rows: empty on most ranks
              ("voy_edge", "derived_box", ((5, 2, 3), (5, 11, 3), (1, 2, 1))),
              ("ens", "derived_out2d", (1, 16)), ("voz", "derived_out2d", (2, 7)), ("qcr", "derived_out2d", (2, 12)), ("vox_edge", "derived_out2d", (3, 10)),
              ("voy", "derived_out3d", ((2, 5, 3),)), ("qcr", "derived_out3d", ((1, 1, 1),)), ("voz_edge", "derived_out3d", ((1, 1, 1),))]


def _slab_box(kind, args):
    if kind == "derived_box":
        return args
    if kind == "derived_out3d":
        return (1, 1, 1), SLAB_NG, args[0]
    lo, hi = [1, 1, 1], list(SLAB_NG)
    lo[args[0] - 1] = hi[args[0] - 1] = args[1]
    return tuple(lo), tuple(hi), (1, 1, 1)


@pytest.fixture(scope="module")
def one_rank_reads():
    from cales_amd.hotpath import HotPath
    case = nosgs_channel(SLAB_NG)
    u, v, w = random_state(SLAB_NG, 77)
    h = HotPath(case); h.set("u", u); h.set("v", v); h.set("w", w)
    out = [getattr(h, kind)(name, *args) for name, kind, args in SLAB_READS]
    h.derived_to_pp("qcr"); out.append(h.read_box("pp", (1, 1, 1), SLAB_NG))
    h.close()
    ref = reference(case, u, v, w)
    for (name, kind, args), got in zip(SLAB_READS, out):
        assert same(got, box_of(ref[name], *_slab_box(kind, args))), (name, kind, args)
    assert same(out[-1], ref["qcr"])
    return (u, v, w), out


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_slab_shares_make_the_one_rank_result(nranks, one_rank_reads):
    """every rank forms the quantities of its own rows from its haloed slab, exchanging nothing; the shares, placed by cales_box_share, are the one-rank
    result to the bit"""
    from cales_amd import capi
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import box_share
    case = nosgs_channel(SLAB_NG)
    (u, v, w), whole_reads = one_rank_reads

    def body(h, r):
        h.set_global("u", u); h.set_global("v", v); h.set_global("w", w)
        before = h.memory_in_use()
        out = [getattr(h, kind)(name, *args) for name, kind, args in SLAB_READS]
        h.derived_to_pp("qcr"); out.append(h.read_box("pp", (1, 1, 1), SLAB_NG))
        assert h.memory_in_use() == before
        # a rank without a row of the box may pass no buffer at all
        lo, hi, ns = SLAB_READS[2][2]
        i3 = lambda v: (C.c_int32 * 3)(*v)
        cnt = i3((-1, -1, -1))
        rc = h.L.cales_derived_box(h.h, capi.DERIVED["str"], i3(lo), i3(hi), i3(ns), None, cnt)
        return out, rc, tuple(cnt)
    res = run_loopback(case, nranks, body)
    empty = 0
    reads = SLAB_READS + [("qcr", "derived_out3d", ((1, 1, 1),))]      # (the last: pp after to_pp, read back as the interior)
    for q, (name, kind, args) in enumerate(reads):
        lo, hi, ns = _slab_box(kind, args)
        whole = np.full(whole_reads[q].shape, np.nan, order="F")
        for r in range(nranks):
            first, count = box_share(case, lo, hi, ns, nranks=nranks, rank=r)
            share = res[r][0][q]
            assert share.shape == count, (name, kind, args, r)
            empty += count[1] == 0
            j0 = (first[1] - lo[1]) // ns[1]
            assert np.isnan(whole[:, j0:j0 + count[1], :]).all()
            whole[:, j0:j0 + count[1], :] = share
        assert np.array_equal(whole, whole_reads[q]), (name, kind, args)
    assert empty > 0
    for r in range(nranks):      # (the two-row box above: NULL is refused exactly where there is something to write)
        _, rc, cnt = res[r]
        assert (rc != 0) == (cnt[1] > 0) and cnt[0] == 32 and cnt[2] == 10, (r, rc, cnt)
    assert sum(res[r][2][1] for r in range(nranks)) == 2


# ---------------------------------------------------------------------------------------------- single precision, the Fortran host
def test_single_precision_library():
    """libcales_hip_sp.so in a process of its own (the precision is process-wide): the by-value cases on float fields against the restatement in float32"""
    env = dict(os.environ, CALES_PRECISION="single")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_derived_worker.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["real"] == "float32" and res["real_size"] == 4 and res["calls"] >= 8 * 9 * 18 and res["wrong"] == [], res
    assert res["differs_from_float64"] > 0, res      # (the cases tell the precisions apart: the float64 restatement rounded to float is missed)


@pytest.mark.parametrize("nskip", [None, (2, 2, 3)], ids=["dense", "nskip"])
def test_fortran_host_dumps_derived_volumes(tmp_path, nskip):
    """`cales` on the triply periodic case with CALES_OUT3D_DERIVED="vox,qcr" and iout3d = nstep = 4: the files hold the restatement on the velocity of
    the checkpoint written at the same step, its ghost cells wrapped periodically in numpy; with CALES_OUT3D_NSKIP every nskip-th point of it"""
    from cales_amd.nml import parse_text
    from tests import test_gpu_fortran_host as FH
    if not os.path.exists(FH.EXE):
        pytest.skip("Fortran host not built (amdflang absent)")
    text = FH._nml("tgv_ppp", nstep=4, icheck=2, iout0d=2, iout1d=100, iout2d=100, iout3d=4, isave=100000)
    text = re.sub(r"stop_type\(1:3\) = .*", "stop_type(1:3) = T, F, F", text)
    env = dict(os.environ, CALES_OUT3D_DERIVED="vox,qcr")
    if nskip:
        env["CALES_OUT3D_NSKIP"] = ",".join(map(str, nskip))
    out = FH._run(str(tmp_path), text, env=env)
    assert "*** Fim ***" in out
    case = parse_text(text); case.impdiff = 0
    ng = tuple(int(x) for x in case.ng)
    (u, v, w, p), time, istep = FH._read_fld(os.path.join(tmp_path, "fld.bin"), ng)
    assert istep == 4
    ref = reference(case, *[np.asfortranarray(np.pad(a, 1, mode="wrap")) for a in (u, v, w)], live=("vox", "qcr"))
    ns = nskip or (1, 1, 1)
    for name in ("vox", "qcr"):
        want = ref[name][::ns[0], ::ns[1], ::ns[2]]
        got = np.fromfile(os.path.join(tmp_path, f"{name}_fld_0000004.bin"))
        assert got.size == want.size and np.array_equal(got.reshape(want.shape, order="F"), want), name
        assert os.path.exists(os.path.join(tmp_path, f"{name}_fld_0000000.bin"))      # (the initial field, like the other volumes)
    assert not os.path.exists(os.path.join(tmp_path, "voy_fld_0000004.bin"))
    logl = [l.split() for l in open(os.path.join(tmp_path, "log_visu_3d.out")).read().splitlines()]
    assert len(logl) == 14      # five fields and two quantities, for the initial field and for step 4
    assert logl[12][:2] == ["vox_fld_0000004.bin", "Vorticity_X"] and logl[13][:2] == ["qcr_fld_0000004.bin", "Q-criterion"]
    for l in logl[12:]:
        assert l[2:11] == ["1", "1", "1"] + [str(n) for n in ng] + [str(s) for s in ns] and int(l[-1]) == 4, l


def test_fortran_host_refuses_an_unknown_quantity(tmp_path):
    from tests import test_gpu_fortran_host as FH
    if not os.path.exists(FH.EXE):
        pytest.skip("Fortran host not built (amdflang absent)")
    text = FH._nml("tgv_ppp", nstep=1)
    open(os.path.join(tmp_path, "input.nml"), "w").write(text)
    r = subprocess.run([FH.EXE], cwd=str(tmp_path), capture_output=True, text=True, timeout=120, env=dict(os.environ, CALES_OUT3D_DERIVED="vox,helicity"))
    assert r.returncode != 0 and "CALES_OUT3D_DERIVED" in r.stdout + r.stderr

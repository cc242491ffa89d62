"""include/cales_pdf.h on the device: cales_pdf_planes and cales_jpdf_planes (k_pdf.hip) by value against the numpy restatement of the bin rule
(tests/test_pdf_host.py: bin_of, pdf_ref, jpdf_ref) -- integer counts, compared for equality --, and held to the rules every field-reading entry of the
C-ABI keeps: the lazy eddy viscosity is materialised, a pending projection is completed, nothing is allocated, one profile scope per call, a refused call
leaves the context usable; on one rank, on y-slabs, in single precision, and through cales_amd/pdfs.py into the files.

Launch geometry (k_pdf.hip, pdf_geom): a block of 256 threads takes a run of rows of one plane, at least max(4096, counters) samples. The grids of the
box-read tests have planes of 1152 and 480 samples: one block per plane. (96, 96, 6) has planes of 96 rows of 96 samples: runs of ceil(4096 / 96) = 43
rows, so THREE blocks per plane whose last holds 10 rows -- several blocks add into the same global counters, and the last run is partial."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_pdf_host import bin_of, jpdf_ref, pdf_ref
from tests.util import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(96, 12, 10), (40, 12, 10),      # the grids of tests/test_gpu_box_reads.py: one block per plane; row pitch 48 != n1 + 2
         (96, 96, 6)]                     # three blocks per plane, the last with 10 of 43 rows (see above)
FIELD_OFFSET = {"u": 0., "p": 100000., "dudt": -50000.}
NBINS = (1, 2, 64, 100, 4096)
JNBINS = (1, 7, 128)


def coded(ng, offset=0.):
    """a[i, j, k] = i + 128 j + 2048 k + offset: exact in float and double"""
    i, j, k = np.meshgrid(*[np.arange(n + 2, dtype=np.float64) for n in ng], indexing="ij")
    return np.asfortranarray(i + 128. * j + 2048. * k + offset)


def random_field(ng, seed, ghosts=np.nan):
    """standard normal in the interior; the ghost cells hold `ghosts` (NaN: a kernel that counted one would show it as a sample above)"""
    a = np.full(tuple(n + 2 for n in ng), ghosts, order="F")
    a[1:-1, 1:-1, 1:-1] = np.random.RandomState(seed).randn(*ng)
    return a


def inner(a):
    from cales_amd import capi
    return np.asarray(a[1:-1, 1:-1, 1:-1], dtype=capi.np_real)      # the samples as the library stores them


def nosgs_channel(ng):
    """explicit channel without subgrid model"""
    g, case = load_golden("chan_smag")
    case.ng[:] = ng; case.sgstype = "none"
    return case


def pow2_range(nbins, offset):
    """lo, hi with hi - lo = nbins w, w a power of two: s = 1 / w exactly, and the integer-coded samples sit exactly on bin edges"""
    w = 128 if nbins == 100 else 16384 // nbins
    return offset + 3000., offset + 3000. + nbins * w


@pytest.fixture(scope="module", params=GRIDS, ids=lambda ng: "x".join(map(str, ng)))
def ctx(request):
    """one context per grid; the tests set the fields they read"""
    from cales_amd.hotpath import HotPath
    ng = request.param
    h = HotPath(nosgs_channel(ng))
    yield h, ng
    h.close()


def same_pdf(h, name, a, nbins, lo, hi):
    counts, outside = h.pdf_planes(name, nbins, lo, hi)
    wc, wo = pdf_ref(inner(a), nbins, lo, hi)
    for got, want in ((counts, wc), (outside, wo)):
        assert got.dtype == np.int64 and got.flags.f_contiguous and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(outside, wo), (name, nbins, lo, hi)
    assert np.array_equal(counts, wc), (name, nbins, lo, hi)
    # conservation: every interior sample of a plane is counted once
    assert np.array_equal(counts.sum(0) + outside.sum(0), np.full(a.shape[2] - 2, (a.shape[0] - 2) * (a.shape[1] - 2)))
    return counts, outside


@pytest.mark.parametrize("name", list(FIELD_OFFSET))
def test_pdf_planes_by_value(ctx, name):
    h, ng = ctx
    off = FIELD_OFFSET[name]
    # integer-coded, samples on bin edges, some below and some above the range
    a = coded(ng, off)
    h.set(name, a)
    edge_hits = 0
    for nbins in NBINS:
        lo, hi = pow2_range(nbins, off)
        c, o = same_pdf(h, name, a, nbins, lo, hi)
        assert o[0].sum() > 0 and o[1].sum() > 0 and c.sum() > 0, nbins
        edge_hits += int((((inner(a) - lo) * (nbins / (hi - lo))) % 1 == 0).sum())
    assert edge_hits > 0
    c, o = same_pdf(h, name, a, 64, off, off + 32768.)      # ... and a range that holds every sample
    assert o.sum() == 0
    # random, the ghost cells NaN
    a = random_field(ng, 11)
    h.set(name, a)
    for nbins in NBINS:
        same_pdf(h, name, a, nbins, -1.25, 1.75)
        same_pdf(h, name, a, nbins, -6.5, 7.)
    # constant per plane: every sample of a plane in one bin
    vals = 2.5 * np.arange(ng[2] + 2) / ng[2]      # 2.5 / n3 ... 2.5 on the interior planes
    a = np.zeros(tuple(n + 2 for n in ng), order="F") + vals[None, None, :]
    h.set(name, a)
    for nbins in NBINS:
        c, o = same_pdf(h, name, a, nbins, 0., 4.)
        assert ((c > 0).sum(0) == 1).all() and o.sum() == 0 and c.max() == ng[0] * ng[1]
    c, o = same_pdf(h, name, a, 64, 1., 2.)      # ... or all of a plane outside, on either side
    v = inner(a)[0, 0, :]
    assert np.array_equal(o[0], ng[0] * ng[1] * (v < 1)) and np.array_equal(o[1], ng[0] * ng[1] * (v >= 2)) and o[0].any() and o[1].any() and c.any()
    # NaN and the infinities planted among random values, in the first and the last cell of a row too
    a = random_field(ng, 12, ghosts=0.)
    a[1, 1, 1] = np.nan; a[ng[0], ng[1], ng[2]] = np.inf; a[1, ng[1], 2] = -np.inf; a[ng[0], 1, 2] = np.nan; a[5, 3, 4] = np.inf; a[6, 3, 4] = -np.inf
    a[ng[0] - 1, ng[1], 3] = np.nan
    h.set(name, a)
    for nbins in NBINS:
        c, o = same_pdf(h, name, a, nbins, -100., 100.)
        assert o[0].sum() == 2 and o[1].sum() == 5      # -inf twice | NaN three times and +inf twice


def same_jpdf(h, na, nb_, a, b, nbins, ra, rb, kplanes):
    counts, outside = h.jpdf_planes(na, nb_, nbins, ra, rb, kplanes)
    wc, wo = jpdf_ref(inner(a), inner(b), nbins, ra, rb, kplanes)
    assert counts.dtype == np.int64 and outside.dtype == np.int64 and counts.flags.f_contiguous
    assert counts.shape == wc.shape and outside.shape == wo.shape, (counts.shape, outside.shape)
    assert np.array_equal(outside, wo), (na, nb_, nbins, kplanes)
    assert np.array_equal(counts, wc), (na, nb_, nbins, kplanes)
    assert np.array_equal(counts.sum((0, 1)) + outside, np.full(len(kplanes), (a.shape[0] - 2) * (a.shape[1] - 2)))
    return counts, outside


def test_jpdf_planes_by_value(ctx):
    h, ng = ctx
    n3 = ng[2]
    orders = [list(range(1, n3 + 1)), [n3, 1, 3, 3, 2, n3, 3], [4]]      # every plane | out of order and repeated | one
    # integer-coded pairs on bin edges: a plane of (u, p) is a grid of points in the (a, b) plane
    a, b = coded(ng, 0.), coded(ng, 100000.)[::-1, :, :].copy(order="F")
    h.set("u", a); h.set("p", b)
    for nbins in JNBINS:
        w = 2048 if nbins == 7 else 16384 // nbins      # s = 1 / w exactly
        ra, rb = (3000., 3000. + nbins * w), (103000., 103000. + nbins * w)
        inside = outside = 0
        for kp in orders:
            c, o = same_jpdf(h, "u", "p", a, b, nbins, ra, rb, kp)
            inside += c.sum(); outside += o.sum()
        assert inside > 0 and outside > 0
    # random pairs with NaN and infinities in either variable, the ghost cells NaN
    a, b = random_field(ng, 21), random_field(ng, 22)
    a[2, 2, 1] = np.nan; b[3, 2, 1] = np.inf; a[4, 4, 3] = -np.inf; b[4, 4, 3] = np.nan
    b = np.asfortranarray(0.6 * a + 0.8 * b)      # correlated
    b[2, 2, 1] = 0.
    h.set("dudt", a); h.set("p", b)
    for nbins in JNBINS:
        for kp in orders:
            same_jpdf(h, "dudt", "p", a, b, nbins, (-1.5, 2.), (-2.25, 1.75), kp)
    same_jpdf(h, "p", "dudt", b, a, 7, (-2.25, 1.75), (-1.5, 2.), orders[1])      # the first axis is the first field
    same_jpdf(h, "p", "p", b, b, 7, (-2.25, 1.75), (-2.25, 1.75), orders[1])       # a field with itself: the diagonal
    # with a range of B that holds every sample the marginal over B is pdf_planes of A on that plane
    a, b = random_field(ng, 23, ghosts=0.), random_field(ng, 24, ghosts=0.)
    h.set("u", a); h.set("p", b)
    for nbins in JNBINS:
        kp = orders[1]
        jc, jo = same_jpdf(h, "u", "p", a, b, nbins, (-1., 1.5), (-1e6, 1e6), kp)
        c, o = h.pdf_planes("u", nbins, -1., 1.5)
        for q, k in enumerate(kp):
            assert np.array_equal(jc[:, :, q].sum(1), c[:, k - 1]) and jo[q] == o[:, k - 1].sum(), (nbins, k)


def test_calls_have_a_profile_scope_and_allocate_nothing(ctx):
    h, ng = ctx
    a = random_field(ng, 31, ghosts=0.)
    h.set("u", a); h.set("p", a)
    before = h.memory_in_use()
    h.profile_reset(); h.profile(True)
    for q in range(5):
        h.pdf_planes("u", (1, 64, 4096, 100, 2)[q], -1., 1.)
        h.jpdf_planes("u", "p", (1, 7, 128, 128, 2)[q], (-1., 1.), (-2., 2.), [1 + q, 1])
        assert h.memory_in_use() == before
    h.profile(False)
    st = h.profile_stats()
    assert st["pdf_planes"][0] == 5 and st["jpdf_planes"][0] == 5      # one scope per call
    assert h.memory_in_use() == before


def test_results_are_the_same_bits_from_run_to_run(ctx):
    h, ng = ctx
    a = random_field(ng, 32, ghosts=0.)
    h.set("u", a); h.set("p", a[::-1].copy(order="F"))
    first = h.pdf_planes("u", 100, -1., 1.) + h.jpdf_planes("u", "p", 7, (-1., 1.), (-1., 1.), [2, 1])
    for _ in range(3):
        again = h.pdf_planes("u", 100, -1., 1.) + h.jpdf_planes("u", "p", 7, (-1., 1.), (-1., 1.), [2, 1])
        assert all(np.array_equal(x, y) for x, y in zip(first, again))


def test_refusals_leave_the_context_usable(ctx):
    from cales_amd import capi
    from cales_amd.hotpath import CalesError
    h, ng = ctx
    L, H = h.L, h.h
    a = coded(ng)
    h.set("u", a); h.set("p", a)
    n3 = ng[2]
    cnt = np.zeros(4096 * n3 + 128 * 128 * 4, dtype=np.int64); out = np.zeros(2 * n3 + 8, dtype=np.int64)
    PC, PO = cnt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    U, P = capi.FIELDS["u"], capi.FIELDS["p"]
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    kp = i32([1, 2]); K = kp.ctypes.data_as(C.c_void_p)
    bad = {k: i32(v) for k, v in {"k = 0": [1, 0], "k = ng+1": [n3 + 1, 1], "k < 0": [-3, 1]}.items()}
    inf, nan = float("inf"), float("nan")
    pdf = lambda field=U, nbins=8, lo=0., hi=1., c=PC, o=PO: L.cales_pdf_planes(H, field, nbins, lo, hi, c, o)
    jpdf = lambda fa=U, fb=P, nbins=8, ra=(0., 1.), rb=(0., 1.), npl=2, k=K, c=PC, o=PO: L.cales_jpdf_planes(H, fa, fb, nbins, ra[0], ra[1], rb[0], rb[1], npl, k, c, o)
    refused = {
        "field -1": lambda: pdf(field=-1), "field 15": lambda: pdf(field=15), "field not allocated": lambda: pdf(field=capi.FIELDS["dudtd"]),      # (explicit diffusion: no implicit part)
        "nbins 0": lambda: pdf(nbins=0), "nbins -1": lambda: pdf(nbins=-1), "nbins 4097": lambda: pdf(nbins=4097),
        "lo nan": lambda: pdf(lo=nan), "hi nan": lambda: pdf(hi=nan), "lo -inf": lambda: pdf(lo=-inf), "hi inf": lambda: pdf(hi=inf),
        "hi == lo": lambda: pdf(lo=1., hi=1.), "hi < lo": lambda: pdf(lo=1., hi=0.),
        "NULL counts": lambda: pdf(c=None),
        "j field a -1": lambda: jpdf(fa=-1), "j field b 15": lambda: jpdf(fb=15), "j field b not allocated": lambda: jpdf(fb=capi.FIELDS["dwdtd"]),
        "j nbins 0": lambda: jpdf(nbins=0), "j nbins 129": lambda: jpdf(nbins=129),
        "j lo_a nan": lambda: jpdf(ra=(nan, 1.)), "j hi_b inf": lambda: jpdf(rb=(0., inf)), "j lo_b -inf": lambda: jpdf(rb=(-inf, 0.)),
        "j hi_a == lo_a": lambda: jpdf(ra=(2., 2.)), "j hi_b < lo_b": lambda: jpdf(rb=(2., 1.)),
        "j NULL counts": lambda: jpdf(c=None),
        "j nplanes 0": lambda: jpdf(npl=0), "j nplanes -2": lambda: jpdf(npl=-2),
        "j NULL kplanes": lambda: jpdf(k=None),
    }
    for what, v in bad.items():
        refused["j " + what] = lambda v=v: jpdf(k=v.ctypes.data_as(C.c_void_p))
    for q, (what, call) in enumerate(refused.items()):
        assert call() != 0, what
        assert L.cales_last_error(H).decode(), what
        if q % 2:
            same_pdf(h, "u", a, 64, 3000., 3000. + 64 * 256)
        else:
            same_jpdf(h, "u", "p", a, a, 7, (3000., 3000. + 7 * 128), (0., 7 * 4096.), [2, 1, 2])
    for call in (lambda: h.pdf_planes("u", 0, 0., 1.), lambda: h.pdf_planes("u", 5000, 0., 1.), lambda: h.pdf_planes("u", 8, 1., 1.),
                 lambda: h.jpdf_planes("u", "p", 129, (0., 1.), (0., 1.), [1]), lambda: h.jpdf_planes("u", "p", 8, (0., 1.), (0., 1.), []),
                 lambda: h.jpdf_planes("u", "p", 8, (0., 1.), (0., 1.), [n3 + 1])):
        with pytest.raises(CalesError):
            call()
    # outside may be NULL
    assert pdf(nbins=64, lo=3000., hi=3000. + 64 * 256, o=None) == 0
    assert np.array_equal(cnt[:64 * n3].reshape((64, n3), order="F"), pdf_ref(inner(a), 64, 3000., 3000. + 64 * 256)[0])
    assert jpdf(nbins=7, ra=(3000., 3000. + 7 * 128), rb=(0., 7 * 4096.), o=None) == 0
    assert np.array_equal(cnt[:49 * 2].reshape((7, 7, 2), order="F"), jpdf_ref(inner(a), inner(a), 7, (3000., 3000. + 7 * 128), (0., 7 * 4096.), [1, 2])[0])


def dsmag_start():
    from cales_amd.hotpath import initflow
    g, case = load_golden("chan_dsmag"); case.ng[:] = (64, 16, 12)
    u0 = initflow(case)
    rng = np.random.RandomState(3)
    for a in u0[:3]:
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(64, 16, 12) - 0.5)
    return case, u0


@pytest.fixture(scope="module")
def visct_top():
    """the largest eddy viscosity after cmpt_sgs on the start field (the tests below choose their ranges from it before they read anything)"""
    from cales_amd.hotpath import HotPath
    case, u0 = dsmag_start()
    h = HotPath(case); h.upload(*u0); h.startup(); h.cmpt_sgs()
    top = float(h.get("visct")[1:-1, 1:-1, 1:-1].max())
    h.close()
    assert top > 0.
    return top


@pytest.mark.parametrize("first", ["get", "pdf", "jpdf"])
def test_visct_is_materialised(first, visct_top):
    """The dynamic model's tile passes leave visct = |S| cs(k) as |S| and the plane coefficients until somebody other than the momentum pass reads it: a
    histogram is such a reader, whether it comes before or after a full download."""
    from cales_amd.hotpath import HotPath
    case, u0 = dsmag_start()
    h = HotPath(case); h.upload(*u0); h.startup()
    h.cmpt_sgs()
    rv, ru, kp = (0., 0.75 * visct_top), (0.2, 1.4), [6, 1, 12]
    if first == "get":
        full = h.get("visct"); h.cmpt_sgs()
        got = h.pdf_planes("visct", 100, *rv); gotj = h.jpdf_planes("u", "visct", 7, ru, rv, kp)
    elif first == "pdf":
        got = h.pdf_planes("visct", 100, *rv); gotj = h.jpdf_planes("u", "visct", 7, ru, rv, kp)
        full = h.get("visct")
    else:
        gotj = h.jpdf_planes("u", "visct", 7, ru, rv, kp); got = h.pdf_planes("visct", 100, *rv)
        full = h.get("visct")
    u = h.get("u")
    h.close()
    wc, wo = pdf_ref(inner(full), 100, *rv)
    assert wc.sum() > 0 and wo[1].sum() > 0 and (wc > 0).sum() > 20      # the range cuts the distribution, and it is one
    assert np.array_equal(got[0], wc) and np.array_equal(got[1], wo)
    wj = jpdf_ref(inner(u), inner(full), 7, ru, rv, kp)
    assert np.array_equal(gotj[0], wj[0]) and np.array_equal(gotj[1], wj[1])


def pdf_ctx_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cales_pdf.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(\s*(?:const\s+)?cales_ctx\s*\*", hdr)))


def test_every_pdf_entry_sees_the_projected_state(monkeypatch):
    """The scheme of tests/test_gpu_box_reads.py::test_every_post_entry_sees_the_projected_state for the third header: every entry of
    include/cales_pdf.h that takes a context, enumerated from the header, completes a projection that cales_step left pending before it reads."""
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    g, case = load_golden("cavity_nnn"); case.ng[:] = (32, 16, 12)
    entries = pdf_ctx_entries()
    cnt = np.zeros(64 * 64 * 12, dtype=np.int64); out = np.zeros(24, dtype=np.int64)
    PC, PO = cnt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    kp = np.asarray([3, 9], dtype=np.int32)
    U, W = capi.FIELDS["u"], capi.FIELDS["w"]
    table = {"cales_pdf_planes": lambda h: h.L.cales_pdf_planes(h.h, U, 64, -1., 1., PC, PO),
             "cales_jpdf_planes": lambda h: h.L.cales_jpdf_planes(h.h, U, W, 16, -1., 1., -1., 1., 2, kp.ctypes.data_as(C.c_void_p), PC, PO)}
    assert entries and sorted(table) == entries == sorted(capi.PDF_SYMBOLS), f"entries of include/cales_pdf.h without a rule for a pending projection: {set(entries) ^ set(table)}"
    u0 = initflow(case)
    for e in entries:
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.5 * h.chkdt()
        ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))
        h.profile(True)
        h.step(dt)
        assert ncorr() == 0, (e, "the step was expected to leave its last projection pending")
        assert table[e](h) == 0, (e, h.L.cales_last_error(h.h))
        n1 = ncorr()
        assert n1 >= 1, (e, "did not complete the pending projection")
        # what the entry binned was the projected velocity: the counts are those of the field read afterwards
        u, w = h.get("u"), h.get("w")
        if e == "cales_pdf_planes":
            assert np.array_equal(cnt[:64 * 12].reshape((64, 12), order="F"), pdf_ref(inner(u), 64, -1., 1.)[0])
        else:
            assert np.array_equal(cnt[:256 * 2].reshape((16, 16, 2), order="F"), jpdf_ref(inner(u), inner(w), 16, (-1., 1.), (-1., 1.), [3, 9])[0])
        assert h.chkdiv()[1] < 1e-12, e
        assert ncorr() == n1, e              # ... and nothing was pending any more
        h.profile(False); h.close()


SLAB_NG = (32, 12, 10)
SLAB_KP = [10, 1, 4, 4]


def _slab_calls(h):
    return (h.pdf_planes("u", 100, 3000., 3000. + 100 * 128) + h.pdf_planes("p", 64, -1., 1.5) + h.pdf_planes("p", 4096, -3., 3.) +
            h.jpdf_planes("u", "p", 7, (3000., 3000. + 7 * 2048), (-1., 1.5), SLAB_KP) + h.jpdf_planes("p", "u", 128, (-3., 3.), (0., 32768.), SLAB_KP))


@pytest.fixture(scope="module")
def one_rank_counts():
    from cales_amd.hotpath import HotPath
    a, b = coded(SLAB_NG), random_field(SLAB_NG, 41)
    h = HotPath(nosgs_channel(SLAB_NG)); h.set("u", a); h.set("p", b)
    out = _slab_calls(h)
    h.close()
    want = (pdf_ref(inner(a), 100, 3000., 3000. + 100 * 128) + pdf_ref(inner(b), 64, -1., 1.5) + pdf_ref(inner(b), 4096, -3., 3.) +
            jpdf_ref(inner(a), inner(b), 7, (3000., 3000. + 7 * 2048), (-1., 1.5), SLAB_KP) + jpdf_ref(inner(b), inner(a), 128, (-3., 3.), (0., 32768.), SLAB_KP))
    assert len(out) == len(want) == 10
    for x, y in zip(out, want):
        assert np.array_equal(x, y)
    return out


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_slab_counts_add_up_to_the_one_rank_result(nranks, one_rank_counts):
    from cales_amd.decomp import run_loopback
    a, b = coded(SLAB_NG), random_field(SLAB_NG, 41)

    def body(h, r):
        h.set_global("u", a); h.set_global("p", b)
        before = h.memory_in_use()
        out = _slab_calls(h)
        assert h.memory_in_use() == before
        return out
    res = run_loopback(nosgs_channel(SLAB_NG), nranks, body)
    for q, want in enumerate(one_rank_counts):
        parts = [res[r][q] for r in range(nranks)]
        assert all(p.shape == want.shape and p.dtype == np.int64 for p in parts), q
        assert np.array_equal(sum(parts), want), q
        assert any(not np.array_equal(p, want) for p in parts) or not want.any(), q      # (a rank's counts are its own rows', not the total)
    # a rank's own counts are those of its rows
    n2 = SLAB_NG[1] // nranks
    for r in range(nranks):
        rows = slice(r * n2, (r + 1) * n2)
        wc, wo = pdf_ref(inner(b)[:, rows, :], 64, -1., 1.5)
        assert np.array_equal(res[r][2], wc) and np.array_equal(res[r][3], wo), r


def test_single_precision_library():
    """libcales_hip_sp.so in a process of its own (the precision is process-wide): by-value cases on float fields, the checker in float32"""
    env = dict(os.environ, CALES_PRECISION="single")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_pdf_worker.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["real"] == "float32" and res["real_size"] == 4 and res["calls"] >= 40 and res["wrong"] == [], res
    assert res["differs_from_float64"] > 0, res      # (the cases tell the two precisions apart: the float64 rule gives other counts)


def test_collect_write_read_end_to_end(tmp_path):
    """cales_amd/pdfs.py on a stepped dynamic-model channel: what ends up in the four files is the checker's counts of the downloaded fields"""
    from cales_amd import pdfs
    from cales_amd.hotpath import HotPath, initgrid
    case, u0 = dsmag_start()
    h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.4 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    fields = [inner(a) for a in h.download()]      # u, v, w, p, visct
    fields = fields[:3] + [fields[4], fields[3]]   # the file order: u, v, w, visct, p
    # ranges that cut both tails; a constant plane (the clipped eddy viscosity is zero on some) gets a range that starts at its value: all in bin 0
    span = lambda a: (float(a.min() + 0.1 * (a.max() - a.min())), float(a.max() - 0.05 * (a.max() - a.min()))) if a.max() > a.min() else (float(a.min()), float(a.min()) + 1e-6)
    ranges = [span(a) for a in fields]
    kplanes = [2, 11, 6]
    jranges = np.array([[span(a[:, :, k - 1]) for a in fields] for k in kplanes])      # ranges of their own on every plane
    assert all(hi > lo for lo, hi in ranges) and (jranges[:, :, 1] > jranges[:, :, 0]).all()
    before = h.memory_in_use()
    got = pdfs.collect(h, 100, ranges, 16, kplanes, jranges)
    shared = pdfs.collect(h, 100, ranges, 16, kplanes, ranges)
    assert h.memory_in_use() == before
    h.close()
    zc = initgrid(case.gtype, 12, case.gr, case.l[2])["zc"]
    pdfs.write(str(tmp_path), 2, got, zc)
    r = pdfs.read(str(tmp_path), 2)
    assert r["npdf"] == 100 and r["njpdf"] == 16 and r["kplanes"].tolist() == kplanes and np.array_equal(r["zc"], np.asarray(zc, dtype=np.float64)[kplanes])
    for a in range(5):
        wc, wo = pdf_ref(fields[a], 100, *ranges[a])
        assert wc.sum() > 0 and np.array_equal(r["pdf"][:, :, a], wc) and np.array_equal(got["outside"][:, :, a], wo), a
        for b in range(5):
            if b <= a:
                assert not r["jpdf"][:, :, :, a, b].any()
                continue
            for q, k in enumerate(kplanes):
                wj, woj = jpdf_ref(fields[a], fields[b], 16, jranges[q, a], jranges[q, b], [k])
                assert np.array_equal(r["jpdf"][:, :, q, a, b], wj[:, :, 0]) and got["joutside"][q, a, b] == woj[0], (a, b, k)
            wj, woj = jpdf_ref(fields[a], fields[b], 16, ranges[a], ranges[b], kplanes)
            assert np.array_equal(shared["jpdf"][:, :, :, a, b], wj) and np.array_equal(shared["joutside"][:, a, b], woj), (a, b)
    assert r["jpdf"].sum() > 0
    # as the consumer reads them
    stem = os.path.join(str(tmp_path), "pdfs_fld_0000002")
    data = np.fromfile(stem + "_pdf.bin", dtype="float64").reshape((100, 12, 5), order="F")
    assert np.array_equal(data, got["pdf"])
    meta = np.loadtxt(stem + "_jpdf_meta.out")
    assert meta.shape == (3, 13) and meta[:, 1].tolist() == [2., 11., 6.]

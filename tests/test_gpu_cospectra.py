"""include/cales_cospectra.h on the device: cales_cospectra_lines and cales_cospectra_planes (k_spectra.hip, the kernels k_spec_x<2, .>, k_spec_y<2>, k_spec_y2<2>) by value against the numpy restatement of the
header's definitions (tests/test_cospectra_host.py: cospectra_ref) within the bounds derived there (cross_line_bound, cross_plane_bound, and
line_bounds of tests/test_spectra_host.py for the line sums: forward error of an FFT and of a sequential sum, nothing tuned), and held to the rules every
field-reading entry of the C-ABI keeps: the lazy eddy viscosity is materialised, a pending projection is completed, nothing is allocated, one profile
scope per call, the same bits from run to run, a refused call leaves the context usable; on one rank, on y-slabs, in single precision, and through
cales_amd/cospectra.py into the files. Every by-value case prints its largest error / bound ratio (pytest -s shows them).

Launch geometry (spec_geom_x / _y / _y2 of spectral_line.hpp with two fields; the figures are those of the double-precision library): a block keeps nl complex lines of N points twice in LDS,
nl = 8 for N <= 256, 4 for N = 512, 2 above, HALF of them of either field: the x kernel takes runs of rows in batches of nl rows (of both fields), the y
kernel tiles of nl columns, the y pass of the planes nl / 2 mode columns. The grids (tests/test_gpu_spectra.py says why no other shapes exist) and
what they reach:
  (96, 12, 10)   3 2^5 x line (stages 4, 4, 2, 3); two blocks per plane, runs of 8 and 4 rows; twelve tiles of 8 columns
  (40, 26, 6)    row pitch 48 != n1 + 2; 26 rows: runs of 8, 8, 8 and 2; the 26 = 2 13 point y line takes the direct sum
  (56, 20, 4)    factor 7 in x: the direct sum; 5 4 in y
  (1024, 4, 2)   several elements and modes per thread, nl = 2: two rows of either field are one batch
  (512, 6, 2)    nl = 4
  (2048, 2, 2)   the cap in x, 128 KB of LDS: one complex line per field
  (16, 2000, 2)  the longest y line that takes the staged transform; tiles of 2 columns (in single precision narrower than a 16-byte chunk)
  (16, 2046, 2)  the longest y line a context can have; the direct sum
  (48, 42, 3)    six blocks per plane feed the fold, runs of 8 rows and one of 2; 42 = 2 3 7: direct in y
  (16, 2000, 10) the one grid small enough for a test on which a block takes SEVERAL batches (a run is longer than nl rows only where n2 n3 exceeds
                 2048 nl): runs of 16 rows, two batches of 8, in the lines and in the planes"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_cospectra_host import cerr, cospectra_ref, cross_line_bound, cross_plane_bound
from tests.test_gpu_pdf import dsmag_start, inner, nosgs_channel
from tests.test_gpu_spectra import mode_fields, random_field, ratio, smooth, without_plane_means
from tests.test_spectra_host import line_bounds, mode_weights
from tests.util import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(96, 12, 10), (40, 26, 6), (56, 20, 4), (1024, 4, 2), (512, 6, 2), (2048, 2, 2), (16, 2000, 2), (16, 2046, 2), (48, 42, 3), (16, 2000, 10)]
PAIRS = (("u", "w"), ("p", "u"), ("dudt", "p"), ("u", "u"))      # two face fields | centre and face | right-hand side and centre | a field with itself
PHI = 0.7


def lagged(a, axis, phi=PHI, gain=0.5):
    """the haloed field `a` with every mode along `axis` (0: x, 1: y) delayed by phi and scaled: cross(a, lagged a) has the argument phi at every
    mode but 0 and n/2, which stay real"""
    f = a[1:-1, 1:-1, 1:-1]
    n = f.shape[axis]
    F = np.fft.rfft(f, axis=axis)
    ph = np.full(F.shape[axis], np.exp(-1j * phi)); ph[0] = 1.
    if n % 2 == 0:
        ph[-1] = 1.
    b = np.full(a.shape, np.nan, order="F")
    b[1:-1, 1:-1, 1:-1] = gain * np.fft.irfft(F * ph.reshape([-1 if d == axis else 1 for d in range(3)]), n=n, axis=axis)
    return b


def lines_ratio(got, f, g, idir, eps, ref=None):
    """(cross, lsum_a, lsum_b) of HotPath.cospectra_lines against the checker on the samples f, g: the largest of the three error / bound ratios"""
    cross, la, lb = got
    ref = ref or cospectra_ref(f, g)
    d = "x" if idir == 1 else "y"
    want = ref["cross_" + d]
    assert np.iscomplexobj(cross) and cross.flags.f_contiguous and cross.shape == want.shape == la.shape == lb.shape, (cross.shape, want.shape)
    return max(ratio(cerr(cross, want), cross_line_bound(f, g, idir, eps)[None, :]),
               ratio(np.abs(la - ref["lsum_a_" + d]), line_bounds(f, idir, eps)[1][None, :]), ratio(np.abs(lb - ref["lsum_b_" + d]), line_bounds(g, idir, eps)[1][None, :]))


def planes_ratio(got, f, g, kplanes, eps):
    want = cospectra_ref(f, g, kplanes)["cross2"]
    assert np.iscomplexobj(got) and got.flags.f_contiguous and got.shape == want.shape, (got.shape, want.shape)
    return ratio(cerr(got, want), cross_plane_bound(f, g, kplanes, eps)[None, None, :])


def by_value(h, ng, pair, a, b, eps, what, where=None):
    """every entry on the fields `pair` holding a, b (a field with itself: a): {case: error / bound}, all to be <= 1"""
    n3 = ng[2]
    na, nb = pair
    if na == nb:
        b = a
    h.set(na, a)
    if na != nb:
        h.set(nb, b)
    f, g = inner(a), inner(b)
    ref = cospectra_ref(f, g)
    lx, ly = h.cospectra_lines(na, nb, 1), h.cospectra_lines(na, nb, 2)
    every = list(range(1, n3 + 1))
    orders = [every, [every[q % n3] for q in (n3 - 1, 0, 2, 2, 1)], [every[n3 // 2]]]      # every plane | out of order with repeats | one
    out = {f"{what} lines x": lines_ratio(lx, f, g, 1, eps, ref), f"{what} lines y": lines_ratio(ly, f, g, 2, eps, ref)}
    for q, kp in enumerate(orders):
        out[f"{what} planes {('all', 'mixed', 'one')[q]}"] = planes_ratio(h.cospectra_planes(na, nb, kp), f, g, kp, eps)
    if where is not None:      # a single mode in both fields: nothing elsewhere, and where it is the argument is the lag (by value, above)
        for d, got, idir in (("x", lx, 1), ("y", ly, 2)):
            if where[0] in (d, "xy"):
                rest = np.delete(got[0], where[1] if d == "x" else where[-1], axis=0)
                out[f"{what} elsewhere {d}"] = ratio(cerr(rest, 0.), cross_line_bound(f, g, idir, eps)[None, :]) if rest.size else 0.
    return out


def all_cases(h, ng, pair, eps, seed):
    a, b = random_field(ng, seed), random_field(ng, seed + 100, mean=-1.5)
    res = by_value(h, ng, pair, a, b, eps, "random")
    res.update(by_value(h, ng, pair, without_plane_means(a), without_plane_means(b), eps, "random, plane means removed"))
    small = b.copy(order="F"); small[1:-1, 1:-1, 1:-1] = 1e-6 * (b[1:-1, 1:-1, 1:-1] + 1.5)      # a million times smaller than a, which has a mean
    res.update(by_value(h, ng, pair, a, small, eps, "second field 1e-6"))
    for what, m, where in mode_fields(ng):
        res.update(by_value(h, ng, pair, m, lagged(m, 1 if where[0] == "y" else 0), eps, what + " lagged", where))
    return res


@pytest.fixture(scope="module", params=GRIDS, ids=lambda ng: "x".join(map(str, ng)))
def ctx(request):
    """one context per grid; the tests set the fields they read"""
    from cales_amd.hotpath import HotPath
    ng = request.param
    h = HotPath(nosgs_channel(ng))
    yield h, ng
    h.close()


def eps_real():
    from cales_amd import capi
    return float(np.finfo(capi.np_real).eps)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "-".join(p))
def test_cospectra_by_value(ctx, pair):
    h, ng = ctx
    res = all_cases(h, ng, pair, eps_real(), 11 + PAIRS.index(pair))
    worst = max(res, key=res.get)
    small = max(r for k, r in res.items() if k.startswith("second field 1e-6"))
    print(f"\ncospectra error/bound {'x'.join(map(str, ng))} {'-'.join(pair)}: largest {res[worst]:.3e} ({worst}) over {len(res)} comparisons; second field 1e-6: {small:.3e}")
    assert all(r <= 1. for r in res.values()), {k: r for k, r in res.items() if not r <= 1.}


def test_a_phase_lag_is_the_argument(ctx):
    """a field and its copy delayed by PHI along x: the argument of the cross-spectrum along x is PHI at the mode that carries the signal"""
    h, ng = ctx
    n1 = ng[0]
    m0 = max(1, n1 // 3)
    what, a, where = [c for c in mode_fields(ng) if c[2] == ("x", m0)][0]
    assert 0 < 2 * m0 < n1      # (a mode with a phase: 0 and n1/2 are real)
    h.set("u", a); h.set("w", lagged(a, 0))
    cx = h.cospectra_lines("u", "w", 1)[0]
    bound = cross_line_bound(inner(a), inner(lagged(a, 0)), 1, eps_real())
    assert (np.abs(np.angle(cx[m0]) - PHI) <= 2. * bound / np.abs(cx[m0])).all()      # (an error of `bound` in either part turns a vector of length |c| by at most that)


def test_identities_between_the_entries(ctx):
    """on what the DEVICE returned from separate entries; the slack is the entries' own bounds"""
    h, ng = ctx
    n1, n2, n3 = ng
    eps = eps_real()
    a, b = random_field(ng, 17), random_field(ng, 18, mean=0.5)
    h.set("p", a); h.set("u", b)
    f, g = inner(a).astype(np.float64), inner(b).astype(np.float64)
    kp = list(range(1, n3 + 1))
    wx, wy = mode_weights(n1), mode_weights(n2)
    ab = (f * g).sum((0, 1))
    for idir, n, w in ((1, n1, wx), (2, n2, wy)):
        cab, la, lb = h.cospectra_lines("p", "u", idir)
        cba = h.cospectra_lines("u", "p", idir, lsum=False)
        caa = h.cospectra_lines("p", "p", idir, lsum=False)
        cbb = h.cospectra_lines("u", "u", idir, lsum=False)
        pa, sa = h.spectra_lines("p", idir)
        pb, sb = h.spectra_lines("u", idir)
        bab, baa, bbb = cross_line_bound(f, g, idir, eps), cross_line_bound(f, f, idir, eps), cross_line_bound(g, g, idir, eps)
        (bpa, bla), (bpb, blb) = line_bounds(f, idir, eps), line_bounds(g, idir, eps)
        # a field with itself: the power spectrum of cales_spectra_lines, and no quadrature spectrum beyond the bound
        assert (np.abs(caa.real - pa) <= baa + bpa).all() and (np.abs(caa.imag) <= baa).all() and (np.abs(cbb.real - pb) <= bbb + bpb).all()
        # the fields exchanged: the conjugate
        assert (cerr(cba, np.conj(cab)) <= 2. * bab).all()
        # Parseval: the co-spectrum adds up to n sum a b
        assert (np.abs(w @ cab.real - n * ab) <= w.sum() * bab).all()
        # Cauchy-Schwarz mode by mode, |cross|^2 <= power_a power_b, with d(|c|^2) <= 2 |c| sqrt(2) bound + 2 bound^2 and d(pa pb) <= pa dpb + pb dpa + dpa dpb
        slack = 2. * np.sqrt(2.) * np.abs(cab) * bab + 2. * bab ** 2 + pa * bpb + pb * bpa + bpa * bpb
        assert (np.abs(cab) ** 2 <= pa.astype(np.float64) * pb + slack).all()
        # the line sums against those of cales_spectra_lines. Every row (column) is transformed with the same neighbour in both kernels, but the sums are
        # NOT formed in the same order -- the cross kernels cut a plane into runs of multiples of nl rows and tiles of nl columns, the power kernels
        # into multiples of 2 nl rows and tiles of 2 nl columns, and each block's partial is added as a whole --: agreement within the two bounds
        assert (np.abs(la - sa) <= 2. * bla).all() and (np.abs(lb - sb) <= 2. * blb).all()
    # the x marginal of cross2, real and imaginary part
    cx = h.cospectra_lines("p", "u", 1, lsum=False)
    c2 = h.cospectra_planes("p", "u", kp)
    b2, bx = cross_plane_bound(f, g, kp, eps), cross_line_bound(f, g, 1, eps)
    assert (cerr(c2.sum(1), n2 * cx) <= (n2 // 2 + 1) * b2 + n2 * bx).all()
    assert (np.abs(np.einsum("m,mqk->k", wx, c2.real) - n1 * n2 * ab) <= wx.sum() * (n2 // 2 + 1) * b2).all()


def test_results_are_the_same_bits_from_run_to_run(ctx):
    h, ng = ctx
    h.set("u", random_field(ng, 32)); h.set("w", random_field(ng, 33, mean=0.))
    kp = [ng[2], 1, 1]
    call = lambda: h.cospectra_lines("u", "w", 1) + h.cospectra_lines("u", "w", 2) + (h.cospectra_planes("u", "w", kp),)
    first = call()
    for _ in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(first, call()))


def test_calls_have_a_profile_scope_and_allocate_nothing(ctx):
    h, ng = ctx
    h.set("u", random_field(ng, 31)); h.set("w", random_field(ng, 30))
    before = h.memory_in_use()
    h.profile_reset(); h.profile(True)
    for q in range(3):
        h.cospectra_lines("u", "w", 1); h.cospectra_lines("u", "w", 2, lsum=False); h.cospectra_planes("u", "w", [1 + q % ng[2], 1])
        assert h.memory_in_use() == before
    h.profile(False)
    st = {k: v[0] for k, v in h.profile_stats().items() if "spectra" in k}
    want = {}
    for scope, n in (("cospectra_lines" + ("" if smooth(ng[0]) else "_direct"), 3), ("cospectra_lines" + ("" if smooth(ng[1]) else "_direct"), 3),
                     ("cospectra_planes" + ("" if smooth(ng[0]) and smooth(ng[1]) else "_direct"), 3)):
        want[scope] = want.get(scope, 0) + n
    assert st == want, (st, want)      # one scope per call, named after the path it took (and none of the power spectra's)
    assert h.memory_in_use() == before


def test_refusals_leave_the_context_usable(ctx):
    from cales_amd import capi
    from cales_amd.hotpath import CalesError
    h, ng = ctx
    L, H = h.L, h.h
    n1, n2, n3 = ng
    eps = eps_real()
    a, b = random_field(ng, 41), random_field(ng, 42)
    h.set("u", a); h.set("w", b)
    f, g = inner(a), inner(b)
    R = capi.np_real
    nh = max(n1, n2) // 2 + 1
    cr, la, lb = (np.zeros(2 * nh * max(n3, 8), dtype=R) for _ in range(3))
    c2 = np.zeros(2 * (n1 // 2 + 1) * (n2 // 2 + 1) * 4, dtype=R)
    CR, LA, LB, C2 = (x.ctypes.data_as(C.c_void_p) for x in (cr, la, lb, c2))
    U, W = capi.FIELDS["u"], capi.FIELDS["w"]
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    kp = i32([1, 2]); K = kp.ctypes.data_as(C.c_void_p)
    lines = lambda fa=U, fb=W, idir=1, c=CR, sa=LA, sb=LB: L.cales_cospectra_lines(H, fa, fb, idir, c, sa, sb)
    planes = lambda fa=U, fb=W, npl=2, k=K, c=C2: L.cales_cospectra_planes(H, fa, fb, npl, k, c)
    NA = capi.FIELDS["dudtd"]      # (explicit diffusion: no implicit part, the field is not allocated)
    refused = {
        "field_a -1": lambda: lines(fa=-1), "field_b -1": lambda: lines(fb=-1), "field_a 15": lambda: lines(fa=15), "field_b 15": lambda: lines(fb=15),
        "field_a not allocated": lambda: lines(fa=NA), "field_b not allocated": lambda: lines(fb=NA),
        "idir 0": lambda: lines(idir=0), "idir 3": lambda: lines(idir=3), "idir -1": lambda: lines(idir=-1),
        "NULL cross": lambda: lines(c=None), "NULL cross, idir 2": lambda: lines(idir=2, c=None),
        "p field_a -1": lambda: planes(fa=-1), "p field_b 15": lambda: planes(fb=15), "p field_a not allocated": lambda: planes(fa=NA), "p field_b not allocated": lambda: planes(fb=capi.FIELDS["dwdtd"]),
        "p NULL cross2": lambda: planes(c=None), "p nplanes 0": lambda: planes(npl=0), "p nplanes -2": lambda: planes(npl=-2), "p NULL kplanes": lambda: planes(k=None),
    }
    for what, v in {"k = 0": [1, 0], "k = ng+1": [n3 + 1, 1], "k < 0": [-3, 1]}.items():
        refused["p " + what] = lambda v=i32(v): planes(k=v.ctypes.data_as(C.c_void_p))
    for q, (what, call) in enumerate(refused.items()):
        assert call() != 0, what
        assert L.cales_last_error(H).decode(), what
        if q % 3 == 0:
            assert lines_ratio(h.cospectra_lines("u", "w", 1), f, g, 1, eps) <= 1., what
        elif q % 3 == 1:
            assert lines_ratio(h.cospectra_lines("u", "w", 2), f, g, 2, eps) <= 1., what
        else:
            assert planes_ratio(h.cospectra_planes("u", "w", [2, 1, 2]), f, g, [2, 1, 2], eps) <= 1., what
    for call in (lambda: h.cospectra_lines("u", "w", 3), lambda: h.cospectra_planes("u", "w", []), lambda: h.cospectra_planes("u", "w", [n3 + 1])):
        with pytest.raises(CalesError):
            call()
    # lsum_a and lsum_b may be NULL, each on its own
    want = h.cospectra_lines("u", "w", 1)
    flat = lambda z: np.stack([z.real, z.imag]).astype(R).ravel(order="F")
    for sa, sb in ((None, None), (LA, None), (None, LB)):
        cr[:] = 0; la[:] = 0; lb[:] = 0
        assert lines(sa=sa, sb=sb) == 0
        n = 2 * want[0].size
        assert np.array_equal(cr[:n], flat(want[0]))
        assert np.array_equal(la[:n], flat(want[1])) if sa is not None else not la.any()
        assert np.array_equal(lb[:n], flat(want[2])) if sb is not None else not lb.any()
    assert np.array_equal(h.cospectra_lines("u", "w", 1, lsum=False), want[0])


@pytest.mark.parametrize("ng", [(2050, 2, 2)], ids=["x"])
def test_a_line_longer_than_the_cap_is_refused(ng):
    """cales_create accepts the grid; the entries that would transform the long line refuse it and the other direction still works"""
    from cales_amd import capi
    from cales_amd.hotpath import CalesError, HotPath
    assert max(ng) == capi.SPECTRA_MAX_LINE + 2
    h = HotPath(nosgs_channel(ng))
    a, b = random_field(ng, 5), random_field(ng, 6)
    h.set("p", a); h.set("u", b)
    for call in (lambda: h.cospectra_lines("p", "u", 1), lambda: h.cospectra_planes("p", "u", [1])):
        with pytest.raises(CalesError, match="CALES_SPECTRA_MAX_LINE"):
            call()
        assert lines_ratio(h.cospectra_lines("p", "u", 2), inner(a), inner(b), 2, eps_real()) <= 1.
    h.close()


@pytest.mark.parametrize("first", ["get", "lines", "planes"])
def test_visct_is_materialised(first):
    """The dynamic model's tile passes leave visct = |S| cs(k) as |S| and the plane coefficients until somebody other than the momentum pass reads it: a
    cross-spectrum with visct as either field is such a reader, whether it comes before or after a full download."""
    from cales_amd.hotpath import HotPath
    case, u0 = dsmag_start()
    h = HotPath(case); h.upload(*u0); h.startup()
    h.cmpt_sgs()
    kp = [6, 1, 12]
    if first == "get":
        full = h.get("visct"); h.cmpt_sgs()
        gl, gy, gp = h.cospectra_lines("visct", "u", 1), h.cospectra_lines("visct", "u", 2), h.cospectra_planes("visct", "u", kp)
    elif first == "lines":
        gl, gy, gp = h.cospectra_lines("visct", "u", 1), h.cospectra_lines("visct", "u", 2), h.cospectra_planes("visct", "u", kp)
        full = h.get("visct")
    else:
        gp = h.cospectra_planes("u", "visct", kp); gp = np.conj(gp)      # (visct as the SECOND field; compared as the conjugate)
        gl, gy = h.cospectra_lines("visct", "u", 1), h.cospectra_lines("visct", "u", 2)
        full = h.get("visct")
    u = h.get("u")
    h.close()
    f, g, eps = inner(full), inner(u), eps_real()
    assert (f ** 2).sum() > 0. and np.ptp(f.astype(np.float64).mean((0, 1))) > 0.      # there is an eddy viscosity, and it differs from plane to plane
    assert lines_ratio(gl, f, g, 1, eps) <= 1. and lines_ratio(gy, f, g, 2, eps) <= 1. and planes_ratio(np.asfortranarray(gp), f, g, kp, eps) <= 1.


def cospectra_ctx_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cales_cospectra.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(\s*(?:const\s+)?cales_ctx\s*\*", hdr)))


def test_every_cospectra_entry_sees_the_projected_state(monkeypatch):
    """The scheme of tests/test_gpu_spectra.py::test_every_spectra_entry_sees_the_projected_state for the sixth header: every entry of
    include/cales_cospectra.h that takes a context, enumerated from the header, completes a projection that cales_step left pending before it reads."""
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    g, case = load_golden("cavity_nnn"); case.ng[:] = (32, 16, 12)
    entries = cospectra_ctx_entries()
    R, eps = capi.np_real, eps_real()
    cr, la, lb = (np.zeros((2, 17, 12), order="F", dtype=R) for _ in range(3))
    c2 = np.zeros((2, 17, 9, 2), order="F", dtype=R)
    kp = np.asarray([3, 9], dtype=np.int32)
    U, W = capi.FIELDS["u"], capi.FIELDS["w"]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    table = {"cales_cospectra_lines": lambda h: h.L.cales_cospectra_lines(h.h, U, W, 1, vp(cr), vp(la), vp(lb)),
             "cales_cospectra_planes": lambda h: h.L.cales_cospectra_planes(h.h, U, W, 2, vp(kp), vp(c2))}
    assert entries and sorted(table) == entries == sorted(capi.COSPECTRA_SYMBOLS), f"entries of include/cales_cospectra.h without a rule for a pending projection: {set(entries) ^ set(table)}"
    u0 = initflow(case)
    cplx = lambda z: np.asfortranarray(z[0] + 1j * z[1])
    for e in entries:
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.5 * h.chkdt()
        ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))
        h.profile(True)
        h.step(dt)
        assert ncorr() == 0, (e, "the step was expected to leave its last projection pending")
        assert table[e](h) == 0, (e, h.L.cales_last_error(h.h))
        n1 = ncorr()
        assert n1 >= 1, (e, "did not complete the pending projection")
        # what the entry transformed was the projected velocity: the cross-spectrum is that of the fields read afterwards
        f, g_ = inner(h.get("u")), inner(h.get("w"))
        if e == "cales_cospectra_lines":
            assert lines_ratio((cplx(cr), cplx(la), cplx(lb)), f, g_, 1, eps) <= 1.
        else:
            assert planes_ratio(cplx(c2), f, g_, [3, 9], eps) <= 1.
        assert h.chkdiv()[1] < 1e-12, e
        assert ncorr() == n1, e              # ... and nothing was pending any more
        h.profile(False); h.close()


SLAB_NG = (32, 12, 10)


@pytest.fixture(scope="module")
def one_rank_sums():
    from cales_amd.hotpath import HotPath
    a, b = random_field(SLAB_NG, 51), without_plane_means(random_field(SLAB_NG, 52))
    h = HotPath(nosgs_channel(SLAB_NG)); h.set("u", a); h.set("p", b)
    out = h.cospectra_lines("u", "p", 1)
    h.close()
    return a, b, out


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_slab_sums_add_up_to_the_one_rank_result(nranks, one_rank_sums):
    """idir = 1 on y-slabs (with four ranks a rank holds 3 rows: the odd last row of either field rides alone); idir = 2 and the planes are refused there"""
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import CalesError
    a, b, whole = one_rank_sums
    eps = eps_real()

    def body(h, r):
        h.set_global("u", a); h.set_global("p", b)
        before = h.memory_in_use()
        out = h.cospectra_lines("u", "p", 1)
        texts = []
        for call in (lambda: h.cospectra_lines("u", "p", 2), lambda: h.cospectra_planes("u", "p", [1, 2])):
            try:
                call(); texts.append("")
            except CalesError as e:
                texts.append(str(e))
        again = h.cospectra_lines("u", "p", 1)      # the context stays usable
        assert all(np.array_equal(x, y) for x, y in zip(out, again))
        assert h.memory_in_use() == before
        return out, texts
    res = run_loopback(nosgs_channel(SLAB_NG), nranks, body)
    n2 = SLAB_NG[1] // nranks
    f, g = inner(a), inner(b)
    parts = [res[r][0] for r in range(nranks)]
    added = tuple(sum(p[q] for p in parts) for q in range(3))
    assert lines_ratio(added, f, g, 1, eps) <= 1.
    bc, bla, blb = cross_line_bound(f, g, 1, eps), line_bounds(f, 1, eps)[1], line_bounds(g, 1, eps)[1]
    assert ratio(cerr(added[0], whole[0]), bc[None, :]) <= 1. and ratio(np.abs(added[1] - whole[1]), bla[None, :]) <= 1. and ratio(np.abs(added[2] - whole[2]), blb[None, :]) <= 1.
    assert any(not np.array_equal(p[0], whole[0]) for p in parts)      # (a rank's sums are its own rows', not the total)
    for r in range(nranks):      # a rank's own result is that of its rows
        rows = slice(r * n2, (r + 1) * n2)
        assert lines_ratio(parts[r], f[:, rows, :], g[:, rows, :], 1, eps) <= 1., r
    for r in range(nranks):
        assert all("one rank only" in t for t in res[r][1]), res[r][1]


def test_single_precision_library():
    """libcales_hip_sp.so in a process of its own (the precision is process-wide): the by-value cases on float fields, the bounds with float's eps"""
    env = dict(os.environ, CALES_PRECISION="single")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_cospectra_worker.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(f"\ncospectra error/bound single precision: largest {res['largest_ratio']:.3e} ({res['largest_case']}) over {res['calls']} comparisons")
    assert res["real"] == "float32" and res["real_size"] == 4 and res["calls"] >= 40 and res["wrong"] == [], res
    assert res["differs_from_float64"] > 0, res      # (the cases tell the two precisions apart: float64's bounds are missed)


def test_collect_write_read_end_to_end(tmp_path):
    """cales_amd/cospectra.py on a stepped dynamic-model channel: what ends up in the files is the checker's cross-spectra of the downloaded fields,
    normalised as the module says"""
    from cales_amd import cospectra
    from cales_amd.hotpath import HotPath, initgrid
    case, u0 = dsmag_start()
    n1, n2, n3 = 64, 16, 12
    h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.4 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    fields = dict(zip(("u", "v", "w", "p"), [inner(a) for a in h.download()][:4]))
    kplanes = [2, 11, 6]
    before = h.memory_in_use()
    got = cospectra.collect(h, kplanes=kplanes)
    assert h.memory_in_use() == before and got["pairs"] == cospectra.PAIRS
    h.close()
    zc = initgrid(case.gtype, n3, case.gr, case.l[2])["zc"]
    cospectra.write(str(tmp_path), 2, got, zc)
    assert len(os.listdir(str(tmp_path))) == 4 * len(cospectra.PAIRS)
    r = cospectra.read(str(tmp_path), 2, n1, n2)
    assert r["kplanes"].tolist() == kplanes and np.array_equal(r["zc"], np.asarray(zc, dtype=np.float64)[kplanes])
    eps = eps_real()
    nrm = 2. / (n1 * n2)
    for q, (na, nb) in enumerate(cospectra.PAIRS):
        f, g = fields[na], fields[nb]
        ref = cospectra_ref(f, g, kplanes)
        assert (f.astype(np.float64) ** 2).sum() > 0. and (g.astype(np.float64) ** 2).sum() > 0.
        assert ratio(cerr(r["x"][:, :, q], nrm * ref["cross_x"]), nrm * cross_line_bound(f, g, 1, eps)[None, :]) <= 1., (na, nb)
        assert ratio(cerr(r["y"][:, :, q], nrm * ref["cross_y"]), nrm * cross_line_bound(f, g, 2, eps)[None, :]) <= 1., (na, nb)
        assert ratio(cerr(r["c2"][:, :, :, q], ref["cross2"] / float(n1 * n2) ** 2), cross_plane_bound(f, g, kplanes, eps)[None, None, :] / float(n1 * n2) ** 2) <= 1.
        assert ratio(np.abs(got["lsum_a_x"][:, :, q] - ref["lsum_a_x"]), line_bounds(f, 1, eps)[1][None, :]) <= 1.
        assert ratio(np.abs(got["lsum_b_y"][:, :, q] - ref["lsum_b_y"]), line_bounds(g, 2, eps)[1][None, :]) <= 1.
        stem = os.path.join(str(tmp_path), f"cospectra_{na}{nb}_fld_0000002")
        assert np.fromfile(stem + "_1d_x.bin", dtype="float64").size == 2 * 33 * n3 and np.fromfile(stem + "_1d_y.bin", dtype="float64").size == 2 * 9 * n3
        assert np.fromfile(stem + "_2d.bin", dtype="float64").size == 2 * 33 * 9 * 3 and np.loadtxt(stem + "_kplanes.out").shape == (3, 2)
    # irfft(x file of (u, w))[0] / 2 is the plane mean of u w: the Reynolds shear stress of the stored samples
    uw = (fields["u"].astype(np.float64) * fields["w"]).mean((0, 1))
    got_uw = np.fft.irfft(r["x"][:, :, 0], n=n1, axis=0)[0] / 2.
    slack = (mode_weights(n1).sum() / n1) * nrm / 2. * cross_line_bound(fields["u"], fields["w"], 1, eps)      # irfft: (1 / n1) sum_m w_m Re x(m)
    assert cospectra.PAIRS[0] == ("u", "w") and (np.abs(got_uw - uw) <= slack + 4. * eps * np.abs(uw)).all(), (got_uw, uw)

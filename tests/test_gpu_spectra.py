"""include/cales_spectra.h on the device: cales_spectra_lines and cales_spectra_planes (k_spectra.hip, the kernels k_spec_x<1, .>, k_spec_y<1>, k_spec_y2<1>) by value against the numpy restatement of the
header's definitions (tests/test_spectra_host.py: spectra_ref) within the bounds derived there (line_bounds, plane_bound: forward error of an FFT and
of a sequential sum, nothing tuned), and held to the rules every field-reading entry of the C-ABI keeps: the lazy eddy viscosity is materialised, a
pending projection is completed, nothing is allocated, one profile scope per call, the same bits from run to run, a refused call leaves the context
usable; on one rank, on y-slabs, in single precision, and through cales_amd/spectra.py into the files. Every by-value case prints its largest
error / bound ratio (pytest -s shows them).

Launch geometry (spec_geom_x / _y / _y2 of spectral_line.hpp with one field; the figures are those of the double-precision library): a block keeps nl complex lines of N points twice in LDS,
nl = 8 for N <= 256, 4 for N = 512, 2 above; the x kernel takes runs of rows in batches of 2 nl rows, a run being a whole number of batches and
the plane cut into about 2048 / nplanes runs; the y kernel takes tiles of 2 nl columns. The grids and what they reach:
  (96, 12, 10)   3 2^5 x line (stages 4, 4, 2, 3); y line 3 4; six row pairs in one batch; six tiles of 16 columns
  (40, 26, 6)    5 8 x line with a row pitch of 48 != n1 + 2; 26 rows: a whole batch and one of 10 rows; the 26 = 2 13 point y line takes the direct sum;
                 tiles of 16, 16 and 8 columns. The feature's issue asked for (40, 13, 6): cales_check_case refuses an odd ng(2) on any number of ranks, so a y line or
                 a plane of 13 rows cannot exist on the device. 13 stays in as the prime of the direct y line, and an odd number of ROWS, the last one
                 riding alone, is reached where it can occur: on slabs (below, 3 rows per rank with four ranks)
  (64, 16, 12)   powers of two
  (56, 20, 4)    factor 7 in x: the direct sum; 5 4 in y; the last tile holds 8 columns
  (1024, 4, 2)   several elements and modes per thread, nl = 2: four rows are one batch
  (2048, 2, 2)   the cap in x: 128 KB of LDS
  (16, 2046, 2)  the longest y line a context can have, tiles of 4 columns and 128 KB of LDS: cales_check_case refuses ng(3) = 1 (every ng >= 2; two planes
                 are the fewest), and cales_create refuses ng(2) = 2048 (the pressure solve's own y transform keeps a line of ng(2) + 1 points twice
                 in 64 KB). 2046 = 2 3 11 31 takes the direct sum
  (16, 2000, 2)  the longest y line that takes the staged transform (4 4 5 5 5)
  (48, 42, 3)    three blocks per plane feed the fold, runs of 16, 16 and 10 rows; 42 = 2 3 7: direct in y
  (512, 6, 2)    nl = 4 (in single precision (1024, 4, 2) is the grid with nl = 4)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_pdf import dsmag_start, inner, nosgs_channel
from tests.test_spectra_host import line_bounds, mode_weights, plane_bound, spectra_ref
from tests.util import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(96, 12, 10), (40, 26, 6), (64, 16, 12), (56, 20, 4), (1024, 4, 2), (2048, 2, 2), (16, 2046, 2), (16, 2000, 2), (48, 42, 3), (512, 6, 2)]
NAMES = ("u", "p", "dudt")      # a face field, a centre field, a right-hand-side field


def smooth(n):
    """n has no prime factor above 5: the staged transform; otherwise the direct sum (profile scope ..._direct)"""
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def random_field(ng, seed, mean=3.):
    """mean + standard normal in the interior, NaN in every ghost cell: a kernel that read one would poison its plane"""
    a = np.full(tuple(n + 2 for n in ng), np.nan, order="F")
    a[1:-1, 1:-1, 1:-1] = mean + np.random.RandomState(seed).randn(*ng)
    return a


def without_plane_means(a):
    b = a.copy(order="F")
    b[1:-1, 1:-1, 1:-1] -= b[1:-1, 1:-1, 1:-1].mean((0, 1), keepdims=True)
    return b


def mode_fields(ng):
    """single modes along x (the phase varies with j), along y (with i) and products of the two; the plane index scales the amplitude"""
    n1, n2, n3 = ng
    i, j = np.arange(n1)[:, None, None], np.arange(n2)[None, :, None]
    amp = (1. + np.arange(n3))[None, None, :]
    ms = sorted({0, 1, n1 // 2, max(1, n1 // 3)}); qs = sorted({0, 1, n2 // 2, max(1, n2 // 3)})
    out = []
    for m0 in ms:
        out.append((f"x mode {m0}", amp * np.cos(2 * np.pi * m0 * i / n1 + 0.37 * j), ("x", m0)))
    for q0 in qs:
        out.append((f"y mode {q0}", amp * np.cos(2 * np.pi * q0 * j / n2 + 0.23 * i), ("y", q0)))
    for m0, q0 in zip(ms, reversed(qs)):
        out.append((f"xy mode {m0} {q0}", amp * np.cos(2 * np.pi * m0 * i / n1 + 0.4) * np.cos(2 * np.pi * q0 * j / n2 + 0.9), ("xy", m0, q0)))
    res = []
    for what, f, where in out:
        a = np.full(tuple(n + 2 for n in ng), np.nan, order="F"); a[1:-1, 1:-1, 1:-1] = f
        res.append((what, a, where))
    return res


def ratio(err, bound):
    """largest error / bound; an exact zero is demanded where the bound is zero"""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    if not np.isfinite(err).all():
        return np.inf
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.), np.where(err > 0, np.inf, 0.))
    return float(r.max())


def lines_ratio(got, f, idir, eps, ref=None):
    """(power, lsum) of HotPath.spectra_lines against the checker on the samples f: the larger of the two error / bound ratios"""
    from cales_amd import capi
    power, lsum = got
    ref = ref or spectra_ref(f)
    wp, wl = ref["power_x" if idir == 1 else "power_y"], ref["lsum_x" if idir == 1 else "lsum_y"]
    assert power.dtype == capi.np_real and power.flags.f_contiguous and power.shape == wp.shape and lsum.shape == wl.shape, (power.shape, wp.shape)
    bp, bl = line_bounds(f, idir, eps)
    return max(ratio(np.abs(power - wp), bp[None, :]), ratio(np.abs(lsum - wl), bl[None, :]))


def planes_ratio(got, f, kplanes, eps):
    from cales_amd import capi
    want = spectra_ref(f, kplanes)["power2"]
    assert got.dtype == capi.np_real and got.flags.f_contiguous and got.shape == want.shape, (got.shape, want.shape)
    return ratio(np.abs(got - want), plane_bound(f, kplanes, eps)[None, None, :])


def by_value(h, ng, name, a, eps, what, where=None):
    """every entry on field `name` holding `a`: {case: error / bound}, all to be <= 1"""
    n3 = ng[2]
    h.set(name, a)
    f = inner(a)
    ref = spectra_ref(f)
    lx, ly = h.spectra_lines(name, 1), h.spectra_lines(name, 2)
    every = list(range(1, n3 + 1))
    orders = [every, [every[q % n3] for q in (n3 - 1, 0, 2, 2, 1)], [every[n3 // 2]]]      # every plane | out of order with repeats, [n3, 1, 3, 3, 2] | one
    out = {f"{what} lines x": lines_ratio(lx, f, 1, eps, ref), f"{what} lines y": lines_ratio(ly, f, 2, eps, ref)}
    for q, kp in enumerate(orders):
        out[f"{what} planes {('all', 'mixed', 'one')[q]}"] = planes_ratio(h.spectra_planes(name, kp), f, kp, eps)
    if where is not None:      # a single mode: all of the power where the mode is, to the bound
        bpx, bpy = line_bounds(f, 1, eps)[0], line_bounds(f, 2, eps)[0]
        if where[0] in ("x", "xy"):
            rest = np.delete(lx[0], where[1], axis=0)
            out[f"{what} elsewhere x"] = ratio(np.abs(rest), bpx[None, :]) if rest.size else 0.
        if where[0] in ("y", "xy"):
            rest = np.delete(ly[0], where[-1], axis=0)
            out[f"{what} elsewhere y"] = ratio(np.abs(rest), bpy[None, :]) if rest.size else 0.
    return out


def all_cases(h, ng, name, eps, seed):
    a = random_field(ng, seed)
    res = by_value(h, ng, name, a, eps, "random")
    res.update(by_value(h, ng, name, without_plane_means(a), eps, "random, plane means removed"))
    for what, m, where in mode_fields(ng):
        res.update(by_value(h, ng, name, m, eps, what, where))
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


@pytest.mark.parametrize("name", NAMES)
def test_spectra_by_value(ctx, name):
    h, ng = ctx
    res = all_cases(h, ng, name, eps_real(), 11 + NAMES.index(name))
    worst = max(res, key=res.get)
    print(f"\nspectra error/bound {'x'.join(map(str, ng))} {name}: largest {res[worst]:.3e} ({worst}) over {len(res)} comparisons")
    assert all(r <= 1. for r in res.values()), {k: r for k, r in res.items() if not r <= 1.}


def test_identities_between_the_entries(ctx):
    """Parseval and the marginals of the plane spectrum, on what the DEVICE returned from separate entries; the slack is the entries' own bounds"""
    h, ng = ctx
    n1, n2, n3 = ng
    eps = eps_real()
    a = random_field(ng, 17)
    h.set("p", a)
    f = inner(a).astype(np.float64)
    (px, lx), (py, ly) = h.spectra_lines("p", 1), h.spectra_lines("p", 2)
    kp = list(range(1, n3 + 1))
    p2 = h.spectra_planes("p", kp).astype(np.float64)
    wx, wy = mode_weights(n1), mode_weights(n2)
    (bpx, blx), (bpy, bly), b2 = line_bounds(f, 1, eps), line_bounds(f, 2, eps), plane_bound(f, kp, eps)
    e2 = (f ** 2).sum((0, 1))
    assert (np.abs(wx @ px - n1 * e2) <= wx.sum() * bpx).all() and (np.abs(wy @ py - n2 * e2) <= wy.sum() * bpy).all()
    assert (np.abs(np.einsum("m,mqk->k", wx, p2) - n1 * n2 * e2) <= wx.sum() * (n2 // 2 + 1) * b2).all()
    assert (np.abs(p2.sum(1) - n2 * px) <= (n2 // 2 + 1) * b2 + n2 * bpx).all()
    assert (np.abs(np.einsum("m,mqk->qk", wx, p2) - n1 * py * wy[:, None]) <= wx.sum() * b2 + n1 * wy[:, None] * bpy).all()
    assert (np.abs(p2[:, 0, :] - np.abs(lx) ** 2) <= b2 + 2 * np.abs(lx) * blx + blx ** 2).all()


def test_results_are_the_same_bits_from_run_to_run(ctx):
    h, ng = ctx
    h.set("u", random_field(ng, 32))
    kp = [ng[2], 1, 1]
    call = lambda: h.spectra_lines("u", 1) + h.spectra_lines("u", 2) + (h.spectra_planes("u", kp),)
    first = call()
    for _ in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(first, call()))


def test_calls_have_a_profile_scope_and_allocate_nothing(ctx):
    h, ng = ctx
    a = random_field(ng, 31)
    h.set("u", a)
    before = h.memory_in_use()
    h.profile_reset(); h.profile(True)
    for q in range(3):
        h.spectra_lines("u", 1); h.spectra_lines("u", 2, lsum=False); h.spectra_planes("u", [1 + q % ng[2], 1])
        assert h.memory_in_use() == before
    h.profile(False)
    st = {k: v[0] for k, v in h.profile_stats().items() if k.startswith("spectra")}
    want = {}
    for scope, n in (("spectra_lines" + ("" if smooth(ng[0]) else "_direct"), 3), ("spectra_lines" + ("" if smooth(ng[1]) else "_direct"), 3),
                     ("spectra_planes" + ("" if smooth(ng[0]) and smooth(ng[1]) else "_direct"), 3)):
        want[scope] = want.get(scope, 0) + n
    assert st == want, (st, want)      # one scope per call, named after the path it took
    assert h.memory_in_use() == before


def test_refusals_leave_the_context_usable(ctx):
    from cales_amd import capi
    from cales_amd.hotpath import CalesError
    h, ng = ctx
    L, H = h.L, h.h
    n1, n2, n3 = ng
    eps = eps_real()
    a = random_field(ng, 41)
    h.set("u", a)
    f = inner(a)
    R = capi.np_real
    nh = max(n1, n2) // 2 + 1
    pw = np.zeros(nh * max(n3, 8), dtype=R); ls = np.zeros(2 * nh * max(n3, 8), dtype=R); p2 = np.zeros((n1 // 2 + 1) * (n2 // 2 + 1) * 4, dtype=R)
    PW, LS, P2 = (x.ctypes.data_as(C.c_void_p) for x in (pw, ls, p2))
    U = capi.FIELDS["u"]
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    kp = i32([1, 2]); K = kp.ctypes.data_as(C.c_void_p)
    lines = lambda field=U, idir=1, p=PW, s=LS: L.cales_spectra_lines(H, field, idir, p, s)
    planes = lambda field=U, npl=2, k=K, p=P2: L.cales_spectra_planes(H, field, npl, k, p)
    refused = {
        "field -1": lambda: lines(field=-1), "field 15": lambda: lines(field=15), "field not allocated": lambda: lines(field=capi.FIELDS["dudtd"]),      # (explicit diffusion: no implicit part)
        "idir 0": lambda: lines(idir=0), "idir 3": lambda: lines(idir=3), "idir -1": lambda: lines(idir=-1),
        "NULL power": lambda: lines(p=None), "NULL power, idir 2": lambda: lines(idir=2, p=None),
        "p field -1": lambda: planes(field=-1), "p field 15": lambda: planes(field=15), "p field not allocated": lambda: planes(field=capi.FIELDS["dwdtd"]),
        "p NULL power2": lambda: planes(p=None), "p nplanes 0": lambda: planes(npl=0), "p nplanes -2": lambda: planes(npl=-2), "p NULL kplanes": lambda: planes(k=None),
    }
    for what, v in {"k = 0": [1, 0], "k = ng+1": [n3 + 1, 1], "k < 0": [-3, 1]}.items():
        refused["p " + what] = lambda v=i32(v): planes(k=v.ctypes.data_as(C.c_void_p))
    for q, (what, call) in enumerate(refused.items()):
        assert call() != 0, what
        assert L.cales_last_error(H).decode(), what
        if q % 3 == 0:
            assert lines_ratio(h.spectra_lines("u", 1), f, 1, eps) <= 1., what
        elif q % 3 == 1:
            assert lines_ratio(h.spectra_lines("u", 2), f, 2, eps) <= 1., what
        else:
            assert planes_ratio(h.spectra_planes("u", [2, 1, 2]), f, [2, 1, 2], eps) <= 1., what
    for call in (lambda: h.spectra_lines("u", 3), lambda: h.spectra_planes("u", []), lambda: h.spectra_planes("u", [n3 + 1])):
        with pytest.raises(CalesError):
            call()
    # lsum may be NULL
    assert lines(s=None) == 0
    want = spectra_ref(f)["power_x"]
    assert ratio(np.abs(pw[:want.size].reshape(want.shape, order="F") - want), line_bounds(f, 1, eps)[0][None, :]) <= 1.
    assert np.array_equal(h.spectra_lines("u", 1, lsum=False), pw[:want.size].reshape(want.shape, order="F"))


@pytest.mark.parametrize("ng", [(2050, 2, 2)], ids=["x"])
def test_a_line_longer_than_the_cap_is_refused(ng):
    """cales_create accepts the grid; the entries that would transform the long line refuse it and the other direction still works. (No context has a
    y line above the cap: cales_create refuses ng(2) >= 2048, see the module docstring.)"""
    from cales_amd import capi
    from cales_amd.hotpath import CalesError, HotPath
    assert max(ng) == capi.SPECTRA_MAX_LINE + 2
    h = HotPath(nosgs_channel(ng))
    a = random_field(ng, 5)
    h.set("p", a)
    long_dir = 1 if ng[0] > ng[1] else 2
    for call in (lambda: h.spectra_lines("p", long_dir), lambda: h.spectra_planes("p", [1])):
        with pytest.raises(CalesError, match="CALES_SPECTRA_MAX_LINE"):
            call()
        assert lines_ratio(h.spectra_lines("p", 3 - long_dir), inner(a), 3 - long_dir, eps_real()) <= 1.
    h.close()


@pytest.mark.parametrize("first", ["get", "lines", "planes"])
def test_visct_is_materialised(first):
    """The dynamic model's tile passes leave visct = |S| cs(k) as |S| and the plane coefficients until somebody other than the momentum pass reads it: a
    spectrum is such a reader, whether it comes before or after a full download."""
    from cales_amd.hotpath import HotPath
    case, u0 = dsmag_start()
    h = HotPath(case); h.upload(*u0); h.startup()
    h.cmpt_sgs()
    kp = [6, 1, 12]
    if first == "get":
        full = h.get("visct"); h.cmpt_sgs()
        gl, gy, gp = h.spectra_lines("visct", 1), h.spectra_lines("visct", 2), h.spectra_planes("visct", kp)
    elif first == "lines":
        gl, gy, gp = h.spectra_lines("visct", 1), h.spectra_lines("visct", 2), h.spectra_planes("visct", kp)
        full = h.get("visct")
    else:
        gp = h.spectra_planes("visct", kp); gl, gy = h.spectra_lines("visct", 1), h.spectra_lines("visct", 2)
        full = h.get("visct")
    h.close()
    f, eps = inner(full), eps_real()
    assert (f ** 2).sum() > 0. and np.ptp(f.astype(np.float64).mean((0, 1))) > 0.      # there is an eddy viscosity, and it differs from plane to plane
    assert lines_ratio(gl, f, 1, eps) <= 1. and lines_ratio(gy, f, 2, eps) <= 1. and planes_ratio(gp, f, kp, eps) <= 1.


def spectra_ctx_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cales_spectra.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(\s*(?:const\s+)?cales_ctx\s*\*", hdr)))


def test_every_spectra_entry_sees_the_projected_state(monkeypatch):
    """The scheme of tests/test_gpu_pdf.py::test_every_pdf_entry_sees_the_projected_state for the fourth header: every entry of
    include/cales_spectra.h that takes a context, enumerated from the header, completes a projection that cales_step left pending before it reads."""
    from cales_amd import capi
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    g, case = load_golden("cavity_nnn"); case.ng[:] = (32, 16, 12)
    entries = spectra_ctx_entries()
    R, eps = capi.np_real, eps_real()
    pw = np.zeros((17, 12), order="F", dtype=R); ls = np.zeros((2, 17, 12), order="F", dtype=R); p2 = np.zeros((17, 9, 2), order="F", dtype=R)
    kp = np.asarray([3, 9], dtype=np.int32)
    U = capi.FIELDS["u"]
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    table = {"cales_spectra_lines": lambda h: h.L.cales_spectra_lines(h.h, U, 1, vp(pw), vp(ls)),
             "cales_spectra_planes": lambda h: h.L.cales_spectra_planes(h.h, U, 2, vp(kp), vp(p2))}
    assert entries and sorted(table) == entries == sorted(capi.SPECTRA_SYMBOLS), f"entries of include/cales_spectra.h without a rule for a pending projection: {set(entries) ^ set(table)}"
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
        # what the entry transformed was the projected velocity: the spectrum is that of the field read afterwards
        f = inner(h.get("u"))
        if e == "cales_spectra_lines":
            assert lines_ratio((pw, ls[0] + 1j * ls[1]), f, 1, eps) <= 1.
        else:
            assert planes_ratio(p2, f, [3, 9], eps) <= 1.
        assert h.chkdiv()[1] < 1e-12, e
        assert ncorr() == n1, e              # ... and nothing was pending any more
        h.profile(False); h.close()


SLAB_NG = (32, 12, 10)


@pytest.fixture(scope="module")
def one_rank_sums():
    from cales_amd.hotpath import HotPath
    a, b = random_field(SLAB_NG, 51), without_plane_means(random_field(SLAB_NG, 52))
    h = HotPath(nosgs_channel(SLAB_NG)); h.set("u", a); h.set("p", b)
    out = h.spectra_lines("u", 1) + h.spectra_lines("p", 1)
    h.close()
    return a, b, out


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_slab_sums_add_up_to_the_one_rank_result(nranks, one_rank_sums):
    """idir = 1 on y-slabs (with four ranks a rank holds 3 rows: the odd last row rides alone); idir = 2 and the planes are refused there"""
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import CalesError
    a, b, whole = one_rank_sums
    eps = eps_real()

    def body(h, r):
        h.set_global("u", a); h.set_global("p", b)
        before = h.memory_in_use()
        out = h.spectra_lines("u", 1) + h.spectra_lines("p", 1)
        texts = []
        for call in (lambda: h.spectra_lines("u", 2), lambda: h.spectra_planes("u", [1, 2])):
            try:
                call(); texts.append("")
            except CalesError as e:
                texts.append(str(e))
        again = h.spectra_lines("u", 1) + h.spectra_lines("p", 1)      # the context stays usable
        assert all(np.array_equal(x, y) for x, y in zip(out, again))
        assert h.memory_in_use() == before
        return out, texts
    res = run_loopback(nosgs_channel(SLAB_NG), nranks, body)
    n2 = SLAB_NG[1] // nranks
    for q, fld in ((0, a), (2, b)):
        f = inner(fld)
        parts = [res[r][0][q:q + 2] for r in range(nranks)]
        added = (sum(p[0] for p in parts), sum(p[1] for p in parts))
        assert lines_ratio(added, f, 1, eps) <= 1.
        bp, bl = line_bounds(f, 1, eps)
        assert ratio(np.abs(added[0] - whole[q]), bp[None, :]) <= 1. and ratio(np.abs(added[1] - whole[q + 1]), bl[None, :]) <= 1.
        assert any(not np.array_equal(p[0], whole[q]) for p in parts)      # (a rank's sums are its own rows', not the total)
        for r in range(nranks):      # a rank's own result is that of its rows
            assert lines_ratio(parts[r], f[:, r * n2:(r + 1) * n2, :], 1, eps) <= 1., r
    for r in range(nranks):
        assert all("one rank only" in t for t in res[r][1]), res[r][1]


def test_single_precision_library():
    """libcales_hip_sp.so in a process of its own (the precision is process-wide): the by-value cases on float fields, the bounds with float's eps"""
    env = dict(os.environ, CALES_PRECISION="single")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_spectra_worker.py")], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(f"\nspectra error/bound single precision: largest {res['largest_ratio']:.3e} over {res['calls']} comparisons")
    assert res["real"] == "float32" and res["real_size"] == 4 and res["calls"] >= 40 and res["wrong"] == [], res
    assert res["differs_from_float64"] > 0, res      # (the cases tell the two precisions apart: float64's bounds are missed)


def test_collect_write_read_end_to_end(tmp_path):
    """cales_amd/spectra.py on a stepped dynamic-model channel: what ends up in the files is the checker's spectra of the downloaded fields, normalised as the
    module says"""
    from cales_amd import spectra
    from cales_amd.hotpath import HotPath, initgrid
    case, u0 = dsmag_start()
    n1, n2, n3 = 64, 16, 12
    h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.4 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    fields = [inner(a) for a in h.download()][:4]      # u, v, w, p
    kplanes = [2, 11, 6]
    before = h.memory_in_use()
    got = spectra.collect(h, kplanes)
    assert h.memory_in_use() == before
    h.close()
    zc = initgrid(case.gtype, n3, case.gr, case.l[2])["zc"]
    spectra.write(str(tmp_path), 2, got, zc)
    r = spectra.read(str(tmp_path), 2, n1, n2)
    assert r["kplanes"].tolist() == kplanes and np.array_equal(r["zc"], np.asarray(zc, dtype=np.float64)[kplanes])
    eps = eps_real()
    for v, f in enumerate(fields):
        ref = spectra_ref(f, kplanes)
        (bpx, blx), (bpy, bly), b2 = line_bounds(f, 1, eps), line_bounds(f, 2, eps), plane_bound(f, kplanes, eps)
        nx, ny = 2. / (n1 * n2), 2. / (n1 * n2)
        assert (f.astype(np.float64) ** 2).sum() > 0.
        assert ratio(np.abs(r["x0"][:, :, v] - nx * ref["power_x"]), nx * bpx[None, :]) <= 1. and ratio(np.abs(r["y0"][:, :, v] - ny * ref["power_y"]), ny * bpy[None, :]) <= 1.
        # xs = 2 |lsum / n2|^2 / n1: |d|L|^2| <= 2 |L| dL + dL^2
        for key, L, bl, nrm in (("xs", ref["lsum_x"], blx, 2. / (n2 * n2 * n1)), ("ys", ref["lsum_y"], bly, 2. / (n1 * n1 * n2))):
            assert ratio(np.abs(r[key][:, :, v] - nrm * np.abs(L) ** 2), nrm * (2 * np.abs(L) * bl[None, :] + bl[None, :] ** 2)) <= 1., key
        assert ratio(np.abs(r["s2"][:, :, :, v] - ref["power2"] / float(n1 * n2) ** 2), b2[None, None, :] / float(n1 * n2) ** 2) <= 1.
        # as the consumer reads them
        stem = os.path.join(str(tmp_path), f"spectra_{spectra.VARS[v]}_fld_0000002")
        assert np.fromfile(stem + "_2d.bin", dtype="float64").reshape((n1 // 2 + 1, n2 // 2 + 1, 3), order="F").shape == (33, 9, 3)
        assert np.fromfile(stem + "_1d_x.bin", dtype="float64").size == 2 * 33 * n3 and np.fromfile(stem + "_1d_y.bin", dtype="float64").size == 2 * 9 * n3
        assert np.loadtxt(stem + "_kplanes.out").shape == (3, 2)
        assert np.allclose(np.fft.irfft(r["x0"][:, :, v], n=n1, axis=0)[0] / 2., (f.astype(np.float64) ** 2).mean((0, 1)), rtol=1e-5 if eps > 1e-10 else 1e-12)

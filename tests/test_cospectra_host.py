"""include/cales_cospectra.h without a GPU: the header against capi.COSPECTRA_SYMBOLS, the two libraries and the Fortran module; the numpy restatement of
its definitions -- cospectra_ref, the checker the device tests compare with (tests/test_gpu_cospectra.py), and the error bounds they hold the device
to -- on identities a cross-spectrum has to satisfy; the pairing rule (the bounds reject a transform that carries a row of either field); the
staggering phase; and the files of cales_amd/cospectra.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cales_amd import capi, cospectra
from tests.test_spectra_host import declarations, line_bounds, mode_weights, spectra_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the checker
def cospectra_ref(a, b, kplanes=None):
    """a, b: the interior samples (n1, n2, n3) of the two fields as the library stores them (cast to capi.np_real by the caller). In complex128:
    cross_x (n1/2+1, n3) = sum_j F^a conj(F^b) of the lines along x with the line sums lsum_a_x, lsum_b_x; cross_y (n2/2+1, n3), lsum_a_y, lsum_b_y of
    the lines along y; cross2 (n1/2+1, n2/2+1, nplanes) of the planes kplanes (1-based; None: every plane) -- unnormalised forward DFTs, ky folded with
    n2 - ky, each distinct ky once."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n1, n2, n3 = a.shape
    Fa, Fb = np.fft.rfft(a, axis=0), np.fft.rfft(b, axis=0)                 # (n1/2+1, n2, n3)
    Ga, Gb = np.fft.rfft(a, axis=1), np.fft.rfft(b, axis=1)                 # (n1, n2/2+1, n3)
    P = np.fft.fft(Fa, axis=1) * np.conj(np.fft.fft(Fb, axis=1))            # (n1/2+1, n2, n3)
    nhy = n2 // 2 + 1
    fold = np.zeros((Fa.shape[0], nhy, n3), dtype=np.complex128)
    for q in range(nhy):
        fold[:, q, :] = P[:, q, :]
        if (n2 - q) % n2 != q:
            fold[:, q, :] += P[:, n2 - q, :]
    kp = list(range(1, n3 + 1)) if kplanes is None else [int(k) for k in kplanes]
    f = np.asfortranarray
    return dict(cross_x=f((Fa * np.conj(Fb)).sum(1)), lsum_a_x=f(Fa.sum(1)), lsum_b_x=f(Fb.sum(1)),
                cross_y=f((Ga * np.conj(Gb)).sum(0)), lsum_a_y=f(Ga.sum(0)), lsum_b_y=f(Gb.sum(0)), cross2=f(fold[:, :, [k - 1 for k in kp]]))


def cross_line_bound(a, b, idir, eps):
    """The bound of the issue for EACH of the real and the imaginary part of cross, per plane (n3 values): with n_line points per line, n_sum lines added
    and ||a||_k, ||b||_k the 2-norms of the samples of plane k,  eps (24 log2 n_line + n_sum) n_line ||a||_k ||b||_k.
    From the forward error of an FFT, ||dF||_2 <= c eps log2 n ||F||_2 with c ~ 7 (Higham, Accuracy and Stability, 24.1); two rows of ONE field ride in
    a transform, so dF^a of a row is relative to its pair of rows, and Cauchy-Schwarz over the rows gives 2 sqrt(2) c ~ 20, rounded up to 24; n_sum eps
    for the sequential sum. With a = b this is the shape of the power bound (tests/test_spectra_host.py: line_bounds). A transform that carried a row
    of a and a row of b would leave in F^b an error proportional to ||a||: the bound is written in ||a|| ||b|| so that it rejects that."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n_line, n_sum = a.shape[idir - 1], a.shape[2 - idir]
    na, nb = np.sqrt((a ** 2).sum((0, 1))), np.sqrt((b ** 2).sum((0, 1)))
    return eps * (24. * np.log2(n_line) + n_sum) * n_line * na * nb


def cross_plane_bound(a, b, kplanes, eps):
    """each part of cross2:  eps (24 log2(n1 n2) + 2) n1 n2 ||a||_k ||b||_k"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n1, n2 = a.shape[:2]
    nrm = lambda f, k: np.sqrt((f[:, :, k - 1] ** 2).sum())
    return np.array([eps * (24. * np.log2(n1 * n2) + 2.) * n1 * n2 * nrm(a, k) * nrm(b, k) for k in kplanes])


def cerr(got, want):
    """the larger of the errors of the real and of the imaginary part"""
    d = np.asarray(got) - np.asarray(want)
    return np.maximum(np.abs(d.real), np.abs(d.imag))


# ---------------------------------------------------------------------------------------------- header, lists, libraries
def test_cospectra_header_equals_the_symbol_list_and_both_libraries_export_it():
    hdr, declared = declarations("cales_cospectra.h")
    assert '#include "cales.h"' in hdr
    assert declared == set(capi.COSPECTRA_SYMBOLS) == {"cales_cospectra_lines", "cales_cospectra_planes"} and len(capi.COSPECTRA_SYMBOLS) == 2
    if os.environ.get("CALES_NO_TORCH") != "1":
        import torch  # noqa: F401  (one HIP runtime per process: see capi.lib)
    for so in ("libcales_hip.so", "libcales_hip_sp.so"):
        L = C.CDLL(os.path.join(ROOT, "cales_amd", so))
        for s in capi.COSPECTRA_SYMBOLS:
            assert hasattr(L, s), (so, s)
    for s, n in zip(capi.COSPECTRA_SYMBOLS, (7, 6)):
        assert len(getattr(capi.lib(), s).argtypes) == n, s      # bound with argument types by capi.lib()


def test_cospectra_symbols_are_a_list_of_their_own():
    for other in (capi.SYMBOLS, capi.POST_SYMBOLS, capi.PDF_SYMBOLS, capi.SPECTRA_SYMBOLS, capi.DERIVED_SYMBOLS):
        assert not set(capi.COSPECTRA_SYMBOLS) & set(other)
    assert capi.SPECTRA_SYMBOLS == ["cales_spectra_lines", "cales_spectra_planes"]
    for header in ("cales.h", "cales_post.h", "cales_pdf.h", "cales_spectra.h", "cales_derived.h"):
        hdr, declared = declarations(header)
        assert not declared & set(capi.COSPECTRA_SYMBOLS), header
        assert "cales_cospectra" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_fortran_module_declares_the_entries():
    txt = open(os.path.join(ROOT, "cales_amd", "fortran", "cales_c.f90")).read()
    for s in capi.COSPECTRA_SYMBOLS:
        assert re.search(r"function\s+" + s + r"\s*\(([^)]*)\)\s*bind\(C,\s*name='" + s + r"'\)", txt), s
    n_args = lambda s: len(re.search(r"function\s+" + s + r"\s*\(([^)]*)\)", txt).group(1).split(","))
    assert n_args("cales_cospectra_lines") == 7 and n_args("cales_cospectra_planes") == 6


def test_the_package_does_not_name_the_checker_side():
    seen = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "cales_amd")):
        for f in files:
            if f in ("cospectra.py", "k_spectra.hip", "spectral_line.hpp"):
                seen.append(f)
                assert "oracle" not in open(os.path.join(dirpath, f)).read(), f
    assert sorted(seen) == ["cospectra.py", "k_spectra.hip", "spectral_line.hpp"]


# ---------------------------------------------------------------------------------------------- the checker's own properties
SHAPES = [(12, 8, 3), (9, 8, 2), (12, 7, 2), (15, 5, 3), (1, 4, 2), (6, 1, 2)]      # even and odd n1 and n2, and lines of one point


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_identities(shape):
    n1, n2, n3 = shape
    rng = np.random.RandomState(sum(shape))
    a, b = 3. + rng.randn(*shape), -1. + 2. * rng.randn(*shape)
    r, raa, rba, pa = cospectra_ref(a, b), cospectra_ref(a, a), cospectra_ref(b, a), spectra_ref(a)
    wx, wy = mode_weights(n1), mode_weights(n2)
    ab = (a * b).sum((0, 1))
    assert r["cross_x"].shape == (n1 // 2 + 1, n3) and r["cross_y"].shape == (n2 // 2 + 1, n3) and r["cross2"].shape == (n1 // 2 + 1, n2 // 2 + 1, n3)
    # a field with itself: the power spectra, no imaginary part; the line sums are those of the power spectra
    for kc, kp in (("cross_x", "power_x"), ("cross_y", "power_y"), ("cross2", "power2")):
        assert np.allclose(raa[kc].real, pa[kp], rtol=1e-12, atol=1e-10) and np.abs(raa[kc].imag).max() <= 1e-12 * np.abs(raa[kc]).max(), kc
    for d in "xy":
        assert np.array_equal(r["lsum_a_" + d], pa["lsum_" + d]) and np.array_equal(rba["lsum_b_" + d], pa["lsum_" + d])
    # the fields exchanged: the conjugate
    for key in ("cross_x", "cross_y", "cross2"):
        assert np.allclose(rba[key], np.conj(r[key]), rtol=1e-13, atol=1e-11), key
    # Parseval along either direction and in the plane: the co-spectrum adds up to sum a b
    assert np.allclose(wx @ r["cross_x"].real, n1 * ab, rtol=1e-11, atol=1e-9)
    assert np.allclose(wy @ r["cross_y"].real, n2 * ab, rtol=1e-11, atol=1e-9)
    assert np.allclose(np.einsum("m,mqk->k", wx, r["cross2"].real), n1 * n2 * ab, rtol=1e-11, atol=1e-9)
    # the marginals of the plane cross-spectrum are the line cross-spectra: along x real and imaginary part. Along y the real part only: the mode
    # (n1 - m, ky) that w_m = 2 stands for is the conjugate of (m, n2 - ky), so the one-sided sum over m of the folded cross2 keeps Re H^a conj(H^b)
    # and loses the sign of the imaginary part -- the quadrature spectrum along y comes from cross_y, not from cross2
    assert np.allclose(r["cross2"].sum(1), n2 * r["cross_x"], rtol=1e-11, atol=1e-9)
    assert np.allclose(np.einsum("m,mqk->qk", wx, r["cross2"].real), n1 * wy[:, None] * r["cross_y"].real, rtol=1e-11, atol=1e-9)
    # ky = 0 of the plane cross-spectrum is the cross-spectrum of the y-summed lines
    assert np.allclose(r["cross2"][:, 0, :], r["lsum_a_x"] * np.conj(r["lsum_b_x"]), rtol=1e-11, atol=1e-9)
    # chosen planes: any order, repeats
    kp = [n3, 1, n3]
    assert np.array_equal(cospectra_ref(a, b, kp)["cross2"], r["cross2"][:, :, [k - 1 for k in kp]])


@pytest.mark.parametrize("n1,n2", [(12, 8), (9, 7)])
def test_checker_gives_a_phase_lag_as_the_argument(n1, n2):
    i, j = np.arange(n1)[:, None, None], np.arange(n2)[None, :, None]
    amp = np.arange(1., 4.)[None, None, :]
    phi = 0.7
    for m0 in (1, 3, (n1 - 1) // 2):      # (a mode other than 0 and n1/2, which are real: they have no phase)
        a, b = amp * np.cos(2 * np.pi * m0 * i / n1 + 0.3 * j), 2. * amp * np.cos(2 * np.pi * m0 * i / n1 + 0.3 * j - phi)      # b lags a by phi
        cx = cospectra_ref(a, b)["cross_x"]
        assert np.allclose(np.angle(cx[m0]), phi, atol=1e-12) and np.abs(np.delete(cx, m0, axis=0)).max() < 1e-20 * np.abs(cx[m0]).max(), m0
        assert np.allclose(np.abs(cx[m0, 1]) / np.abs(cx[m0, 0]), 4.)      # the plane index scales both amplitudes
    for q0 in (1, 2):
        a, b = amp * np.cos(2 * np.pi * q0 * j / n2 + 0.2 * i), amp * np.cos(2 * np.pi * q0 * j / n2 + 0.2 * i - phi)
        cy = cospectra_ref(a, b)["cross_y"]
        assert np.allclose(np.angle(cy[q0]), phi, atol=1e-12) and np.abs(np.delete(cy, q0, axis=0)).max() < 1e-20 * np.abs(cy[q0]).max(), q0
    # a plane wave exp(I (m0 x + q0 y)): in cross2 at (m0, q0), with the phase
    m0, q0 = 2, 1
    a, b = amp * np.cos(2 * np.pi * (m0 * i / n1 + q0 * j / n2)), amp * np.cos(2 * np.pi * (m0 * i / n1 + q0 * j / n2) - phi)
    c2 = cospectra_ref(a, b)["cross2"][:, :, 0]
    top = c2[m0, q0]; rest = c2.copy(); rest[m0, q0] = 0.
    assert np.allclose(np.angle(top), phi, atol=1e-12) and np.abs(rest).max() < 1e-20 * np.abs(top)


# ---------------------------------------------------------------------------------------------- the bounds
def test_bounds_admit_the_least_accurate_transform_one_would_write():
    """a naive O(n^2) DFT of either field with sequential accumulation in the working precision stays well inside the line bound, in either precision"""
    for real in (np.float64, np.float32):
        eps = np.finfo(real).eps
        ctype = np.complex64 if real == np.float32 else np.complex128
        for n1, n2 in ((40, 12), (56, 14)):
            rng = np.random.RandomState(n1)
            a, b = (3. + rng.randn(n1, n2, 1)).astype(real), (rng.randn(n1, n2, 1) - 0.5).astype(real)
            tw = np.exp(-2j * np.pi * np.arange(n1) / n1).astype(ctype)
            cr = np.zeros(n1 // 2 + 1, dtype=ctype)
            for j in range(n2):
                for m in range(n1 // 2 + 1):
                    fa, fb = ctype(0), ctype(0)
                    for i in range(n1):
                        fa = fa + a[i, j, 0] * tw[(i * m) % n1]; fb = fb + b[i, j, 0] * tw[(i * m) % n1]
                    cr[m] = cr[m] + fa * np.conj(fb)
            ratio = cerr(cr, cospectra_ref(a, b)["cross_x"][:, 0]).max() / cross_line_bound(a, b, 1, eps)[0]
            print(f"naive DFT {np.dtype(real).name} ({n1}, {n2}): error / bound {ratio:.2e}")
            assert ratio < 0.1, (real, n1, ratio)


def hermitian_split(Z):
    """F of the two real lines that rode as real and imaginary part of the complex transform Z (along axis 0), modes 0 ... n/2, in Z's precision"""
    n = Z.shape[0]
    m = np.arange(n // 2 + 1)
    zm, zn = Z[m], np.conj(Z[(n - m) % n])
    half = Z.real.dtype.type(0.5)
    return half * (zm + zn), (half * (zm - zn)) * Z.dtype.type(-1j)


def paired_cross(a, b, mixed, real):
    """cross_x of the plane a, b (n1, n2) from complex transforms in precision `real` that carry two real rows each: rows r, r+1 of ONE field (the rule
    of k_spectra.hip), or -- mixed -- row r of a with row r of b"""
    ctype = np.complex64 if real == np.float32 else np.complex128
    a, b = a.astype(real), b.astype(real)
    if mixed:
        Fa, Fb = hermitian_split(np.fft.fft((a + 1j * b).astype(ctype), axis=0))
    else:
        split = lambda f: np.stack(hermitian_split(np.fft.fft((f[:, 0::2] + 1j * f[:, 1::2]).astype(ctype), axis=0)), axis=-1).reshape(f.shape[0] // 2 + 1, -1)
        Fa, Fb = split(a), split(b)
    assert Fa.dtype == ctype
    return (Fa * np.conj(Fb)).sum(1, dtype=ctype)


@pytest.mark.parametrize("real", [np.float64, np.float32], ids=["float64", "float32"])
def test_bounds_reject_a_transform_that_carries_a_row_of_either_field(real):
    """b a million times smaller than a: a row of a and a row of b in one transform leave in F^b an error of the size of eps ||a||, and the
    cross-spectrum misses the bound; the same data with two rows of one field per transform stays far inside it"""
    eps = np.finfo(real).eps
    for n1, n2 in ((96, 12), (40, 26), (56, 20)):
        rng = np.random.RandomState(n1 + n2)
        a, b = 3. + rng.randn(n1, n2), 1e-6 * rng.randn(n1, n2)
        a, b = a.astype(real).astype(np.float64), b.astype(real).astype(np.float64)      # (the samples as the working precision stores them)
        want, bound = cospectra_ref(a[:, :, None], b[:, :, None])["cross_x"][:, 0], cross_line_bound(a[:, :, None], b[:, :, None], 1, eps)[0]
        mixed, same = cerr(paired_cross(a, b, True, real), want).max() / bound, cerr(paired_cross(a, b, False, real), want).max() / bound
        print(f"{np.dtype(real).name} ({n1}, {n2}): error / bound mixed pairing {mixed:.2e}, same-field pairing {same:.2e}")
        assert mixed > 1. and same < 0.1, (n1, n2, mixed, same)


# ---------------------------------------------------------------------------------------------- staggering
@pytest.mark.parametrize("n", [16, 15])
def test_stagger_phase_undoes_a_half_cell_shift(n):
    """u sits half a cell to the right of p: for a band-limited line sampled at both sets of points the corrected cross-spectrum is the power spectrum"""
    rng = np.random.RandomState(n)
    nh = n // 2 + 1
    coef = rng.randn(nh) + 1j * rng.randn(nh); coef[0] = 2.
    top = (n - 1) // 2      # (no energy at n/2 of an even n: the shifted samples of that mode are not defined by the centred ones)
    coef[top + 1:] = 0.
    m = np.arange(nh)
    at = lambda x: np.real(sum(coef[q] * np.exp(2j * np.pi * q * x / n) for q in range(top + 1)))
    x = np.arange(n, dtype=np.float64)
    centre, face = at(x)[:, None, None], at(x + 0.5)[:, None, None]
    power = spectra_ref(centre)["power_x"][:, 0]
    raw = cospectra_ref(face, centre)["cross_x"][:, 0]
    fixed = raw * cospectra.stagger_phase("u", "p", 1, n)
    assert np.abs(fixed - power).max() <= 3e-15 * power.max()
    assert np.abs(raw.imag).max() > 0.1 * power[1:top + 1].min()      # (uncorrected, the quadrature spectrum is of order one)
    assert np.abs(raw * cospectra.stagger_phase("p", "u", 1, n) - power).max() > 0.1 * power[1:top + 1].min()      # (the sign matters)
    assert np.abs(np.conj(raw) * cospectra.stagger_phase("p", "u", 1, n) - power).max() <= 3e-15 * power.max()
    # what is not staggered along the direction is left alone: v and w along x, u along y, and everything against itself
    one = np.ones(nh)
    for pair, idir in ((("v", "w"), 1), (("u", "w"), 2), (("u", "u"), 1), (("p", "visct"), 2), (("w", "p"), 1)):
        assert np.array_equal(cospectra.stagger_phase(*pair, idir, n), one), pair
    assert np.allclose(cospectra.stagger_phase("p", "v", 2, n)[1], np.exp(1j * np.pi / n)) and cospectra.stagger_phase("u", "p", 1, 16)[-1] == 1.
    with pytest.raises(ValueError):
        cospectra.stagger_phase("u", "w", 3, n)


# ---------------------------------------------------------------------------------------------- the files
def collected_from(fields, pairs, kplanes):
    """what cospectra.collect would return on one rank for the fields {name: interior samples}, from the checker"""
    refs = [cospectra_ref(fields[a], fields[b], kplanes) for a, b in pairs]
    n1, n2, n3 = fields[pairs[0][0]].shape
    st = lambda key: np.asfortranarray(np.stack([r[key] for r in refs], axis=-1))
    out = dict(n1=n1, n2=n2, pairs=tuple(pairs), kplanes=np.asarray(kplanes, dtype=np.int64))
    out.update({key: st(key) for key in ("cross_x", "lsum_a_x", "lsum_b_x", "cross_y", "lsum_a_y", "lsum_b_y", "cross2")})
    return out


@pytest.mark.parametrize("shape", [(12, 8, 4), (9, 7, 4)], ids=["even", "odd"])
def test_files_written_and_read_back(tmp_path, shape):
    n1, n2, nz = shape
    rng = np.random.RandomState(3)
    fields = {name: 2. + rng.randn(*shape) for name in ("u", "v", "w", "p")}
    kplanes = [4, 1]
    c = collected_from(fields, cospectra.PAIRS, kplanes)
    zc = np.array([-0.05, 0.05, 0.3, 0.7, 0.95, 1.05])      # haloed: zc(0 ... nz+1)
    cospectra.write(str(tmp_path), 1200, c, zc)
    assert len(os.listdir(str(tmp_path))) == 4 * len(cospectra.PAIRS)
    r = cospectra.read(str(tmp_path), 1200, n1, n2)
    s = cospectra.normalise(c)
    for key in ("x", "y", "c2"):
        assert r[key].shape == s[key].shape and np.iscomplexobj(r[key]) and np.array_equal(r[key], s[key]), key
    assert r["pairs"] == cospectra.PAIRS and r["kplanes"].tolist() == kplanes and r["zc"].tolist() == [zc[4], zc[1]]
    wx = mode_weights(n1)
    for q, (na, nb) in enumerate(cospectra.PAIRS):
        stem = os.path.join(str(tmp_path), f"cospectra_{na}{nb}_fld_0001200")
        for ext, n in (("_1d_x.bin", n1), ("_1d_y.bin", n2)):      # float64, the real block and then the imaginary block
            size = (n // 2 + 1) * nz
            assert os.path.getsize(stem + ext) == 2 * size * 8
            first = np.fromfile(stem + ext, dtype="float64", count=size, offset=0).reshape((n // 2 + 1, nz), order="F")
            second = np.fromfile(stem + ext, dtype="float64", count=size, offset=size * 8).reshape((n // 2 + 1, nz), order="F")
            key = "x" if n is n1 and ext == "_1d_x.bin" else "y"
            assert np.array_equal(first, s[key][:, :, q].real) and np.array_equal(second, s[key][:, :, q].imag)
        assert os.path.getsize(stem + "_2d.bin") == 2 * 8 * (n1 // 2 + 1) * (n2 // 2 + 1) * 2
        assert np.loadtxt(stem + "_kplanes.out").shape == (2, 2)
        # the normalisation of spectra.py's x0: irfft(x)[0] / 2 is the plane mean of a b, irfft(x) / 2 the cross-correlation at zero y separation
        a, b = fields[na], fields[nb]
        mean_ab = (a * b).mean((0, 1))
        assert np.allclose(np.fft.irfft(s["x"][:, :, q], n=n1, axis=0)[0] / 2., mean_ab, rtol=1e-12)
        assert np.allclose(np.fft.irfft(s["y"][:, :, q], n=n2, axis=0)[0] / 2., mean_ab, rtol=1e-12)
        lag1 = (np.roll(a, -1, axis=0) * b).mean((0, 1))      # a(x + 1) b(x)
        assert np.allclose(np.fft.irfft(s["x"][:, :, q], n=n1, axis=0)[1] / 2., lag1, rtol=1e-10, atol=1e-12)
        assert np.allclose(np.einsum("m,mqp->p", wx, s["c2"][:, :, :, q].real), mean_ab[[3, 0]], rtol=1e-12)
        # what the line sums are collected for: cross(0) - lsum_a(0) conj(lsum_b(0)) / n2 is mode 0 of the fluctuations about the plane means
        fa, fb = a - a.mean((0, 1), keepdims=True), b - b.mean((0, 1), keepdims=True)
        got0 = c["cross_x"][0, :, q] - c["lsum_a_x"][0, :, q] * np.conj(c["lsum_b_x"][0, :, q]) / n2
        assert np.allclose(got0, cospectra_ref(fa, fb)["cross_x"][0], rtol=1e-9, atol=1e-9)
    cospectra.write(str(tmp_path), 1300, c, zc[1:-1])      # interior heights give the same file; a wrong number of heights is refused
    assert open(os.path.join(str(tmp_path), "cospectra_uw_fld_0001200_kplanes.out")).read() == open(os.path.join(str(tmp_path), "cospectra_uw_fld_0001300_kplanes.out")).read()
    with pytest.raises(ValueError):
        cospectra.write(str(tmp_path), 1400, c, zc[:3])


def test_add_ranks_of_two_row_halves_is_the_whole(tmp_path):
    shape = (12, 8, 3)
    rng = np.random.RandomState(9)
    fields = {name: 1. + rng.randn(*shape) for name in ("u", "w", "p")}
    pairs = (("u", "w"), ("p", "u"))
    whole = collected_from(fields, pairs, [2])
    parts = []
    for rows in (slice(0, 4), slice(4, 8)):
        p = collected_from({k: f[:, rows, :] for k, f in fields.items()}, pairs, [2])
        p.update(n2=8, cross_y=None, lsum_a_y=None, lsum_b_y=None, cross2=None)      # a rank knows the global n2 and gathers x only
        parts.append(p)
    both = cospectra.add_ranks(parts)
    for key in ("cross_x", "lsum_a_x", "lsum_b_x"):
        assert np.allclose(both[key], whole[key], rtol=1e-13, atol=1e-12), key
    assert both["cross_x"].flags.f_contiguous and both["cross_y"] is None
    s, w = cospectra.normalise(both), cospectra.normalise(whole)
    assert np.allclose(s["x"], w["x"], rtol=1e-13, atol=1e-14) and s["y"] is None and s["c2"] is None
    cospectra.write(str(tmp_path), 5, both, np.arange(3.))      # several ranks: the x files only
    assert sorted(os.listdir(str(tmp_path))) == sorted(f"cospectra_{a}{b}_fld_0000005_1d_x.bin" for a, b in pairs)

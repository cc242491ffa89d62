"""include/cales_spectra.h without a GPU: the header against capi.SPECTRA_SYMBOLS, the two libraries and the Fortran module; the numpy restatement of its
definitions -- spectra_ref, the checker the device tests compare with (tests/test_gpu_spectra.py), and the error bounds they hold the device to -- on
identities a spectrum has to satisfy; and the files of cales_amd/spectra.py, read the way their consumer reads them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cales_amd import capi, spectra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the checker
def spectra_ref(a, kplanes=None):
    """a: the interior samples (n1, n2, n3) as the library stores them (cast to capi.np_real by the caller). In float64: power_x (n1/2+1, n3) and the
    complex lsum_x of the lines along x, power_y (n2/2+1, n3) and lsum_y of the lines along y, power2 (n1/2+1, n2/2+1, nplanes) of the planes
    kplanes (1-based; None: every plane) -- unnormalised forward DFTs, ky folded with n2 - ky, each distinct ky once."""
    a = np.asarray(a, dtype=np.float64)
    n1, n2, n3 = a.shape
    F = np.fft.rfft(a, axis=0)                 # (n1/2+1, n2, n3)
    G = np.fft.rfft(a, axis=1)                 # (n1, n2/2+1, n3)
    H = np.fft.fft(F, axis=1)                  # (n1/2+1, n2, n3)
    P = np.abs(H) ** 2
    nhy = n2 // 2 + 1
    fold = np.zeros((F.shape[0], nhy, n3))
    for q in range(nhy):
        fold[:, q, :] = P[:, q, :]
        if (n2 - q) % n2 != q:
            fold[:, q, :] += P[:, n2 - q, :]
    kp = list(range(1, n3 + 1)) if kplanes is None else [int(k) for k in kplanes]
    return dict(power_x=np.asfortranarray((np.abs(F) ** 2).sum(1)), lsum_x=np.asfortranarray(F.sum(1)),
                power_y=np.asfortranarray((np.abs(G) ** 2).sum(0)), lsum_y=np.asfortranarray(G.sum(0)),
                power2=np.asfortranarray(fold[:, :, [k - 1 for k in kp]]))


def mode_weights(n):
    """w_m of the one-sided sum over m = 0 ... n/2: 1 for m = 0 and for m = n/2 when n is even, 2 otherwise"""
    w = np.full(n // 2 + 1, 2.)
    w[0] = 1.
    if n % 2 == 0:
        w[-1] = 1.
    return w


def line_bounds(a, idir, eps):
    """The bounds of the issue for the sums over lines of plane k, per plane (n3 values each): with n_line points per line, n_sum lines added and
    T_k = n_line sum f^2 (Parseval), |power - want| <= eps (16 log2 n_line + n_sum) T_k and
    |lsum - want| <= eps (8 log2 n_line + n_sum) sqrt(n_line) sum over the lines of ||f_line||_2. From the forward error of an FFT,
    ||dF||_2 <= c eps log2 n ||F||_2 with c ~ 7 (Higham, Accuracy and Stability, 24.1), and n_sum eps for the sequential sum."""
    a = np.asarray(a, dtype=np.float64)
    ax = idir - 1
    n_line, n_sum = a.shape[ax], a.shape[1 - ax]
    T = n_line * (a ** 2).sum((0, 1))
    norms = np.sqrt((a ** 2).sum(ax)).sum(0)      # sum over the lines of a plane of ||f_line||_2
    lg = np.log2(n_line)
    return eps * (16. * lg + n_sum) * T, eps * (8. * lg + n_sum) * np.sqrt(n_line) * norms


def plane_bound(a, kplanes, eps):
    """|power2 - want| <= eps (16 log2(n1 n2) + 2) n1 n2 sum f^2 of the plane"""
    a = np.asarray(a, dtype=np.float64)
    n1, n2 = a.shape[:2]
    return np.array([eps * (16. * np.log2(n1 * n2) + 2.) * n1 * n2 * (a[:, :, k - 1] ** 2).sum() for k in kplanes])


# ---------------------------------------------------------------------------------------------- header, lists, libraries
def declarations(header):
    """the names a header of include/ declares, its comments left out"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(", hdr))


def test_spectra_header_equals_the_symbol_list_and_both_libraries_export_it():
    hdr, declared = declarations("cales_spectra.h")
    assert '#include "cales.h"' in hdr
    assert declared == set(capi.SPECTRA_SYMBOLS) == {"cales_spectra_lines", "cales_spectra_planes"} and len(capi.SPECTRA_SYMBOLS) == 2
    m = re.search(r"#define\s+CALES_SPECTRA_MAX_LINE\s+(\d+)\b", hdr)
    assert m and int(m.group(1)) == capi.SPECTRA_MAX_LINE == 2048
    if os.environ.get("CALES_NO_TORCH") != "1":
        import torch  # noqa: F401  (one HIP runtime per process: see capi.lib)
    for so in ("libcales_hip.so", "libcales_hip_sp.so"):
        L = C.CDLL(os.path.join(ROOT, "cales_amd", so))
        for s in capi.SPECTRA_SYMBOLS:
            assert hasattr(L, s), (so, s)
    for s in capi.SPECTRA_SYMBOLS:
        assert getattr(capi.lib(), s).argtypes, s      # bound with argument types by capi.lib()


def test_spectra_symbols_are_a_list_of_their_own():
    for other in (capi.SYMBOLS, capi.POST_SYMBOLS, capi.PDF_SYMBOLS):
        assert not set(capi.SPECTRA_SYMBOLS) & set(other)
    for header in ("cales.h", "cales_post.h", "cales_pdf.h"):
        hdr, declared = declarations(header)
        assert not declared & set(capi.SPECTRA_SYMBOLS), header
        assert "cales_spectra" not in open(os.path.join(ROOT, "include", header)).read(), header


def test_fortran_module_declares_the_entries():
    txt = open(os.path.join(ROOT, "cales_amd", "fortran", "cales_c.f90")).read()
    for s in capi.SPECTRA_SYMBOLS:
        assert re.search(r"function\s+" + s + r"\s*\(([^)]*)\)\s*bind\(C,\s*name='" + s + r"'\)", txt), s
    n_args = lambda s: len(re.search(r"function\s+" + s + r"\s*\(([^)]*)\)", txt).group(1).split(","))
    assert n_args("cales_spectra_lines") == 5 and n_args("cales_spectra_planes") == 5


def test_the_package_does_not_name_the_checker_side():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "cales_amd")):
        for f in files:
            if f in ("spectra.py", "k_spectra.hip"):
                assert "oracle" not in open(os.path.join(dirpath, f)).read(), f


# ---------------------------------------------------------------------------------------------- the checker's own properties
SHAPES = [(12, 8, 3), (9, 8, 2), (12, 7, 2), (15, 5, 3), (1, 4, 2), (6, 1, 2), (2, 2, 1)]      # even and odd n1 and n2, and lines of one and two points


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_identities(shape):
    n1, n2, n3 = shape
    a = 3. + np.random.RandomState(sum(shape)).randn(*shape)
    r = spectra_ref(a)
    wx, wy = mode_weights(n1), mode_weights(n2)
    e2 = (a ** 2).sum((0, 1))
    assert r["power_x"].shape == (n1 // 2 + 1, n3) and r["power_y"].shape == (n2 // 2 + 1, n3) and r["power2"].shape == (n1 // 2 + 1, n2 // 2 + 1, n3)
    # Parseval along either direction and in the plane
    assert np.allclose(wx @ r["power_x"], n1 * e2, rtol=1e-12)
    assert np.allclose(wy @ r["power_y"], n2 * e2, rtol=1e-12)
    assert np.allclose(np.einsum("m,mqk->k", wx, r["power2"]), n1 * n2 * e2, rtol=1e-12)
    # the marginals of the plane spectrum are the line spectra
    assert np.allclose(r["power2"].sum(1), n2 * r["power_x"], rtol=1e-11, atol=1e-9)
    assert np.allclose(np.einsum("m,mqk->qk", wx, r["power2"]), n1 * r["power_y"] * wy[:, None], rtol=1e-11, atol=1e-9)
    # ky = 0 of the plane spectrum is the spectrum of the y-summed line, and likewise m = 0
    assert np.allclose(r["power2"][:, 0, :], np.abs(r["lsum_x"]) ** 2, rtol=1e-11, atol=1e-9)
    assert np.allclose(r["power2"][0, :, :] , np.abs(r["lsum_y"]) ** 2 * wy[:, None], rtol=1e-11, atol=1e-9)
    # chosen planes: any order, repeats
    kp = [n3, 1, n3]
    assert np.array_equal(spectra_ref(a, kp)["power2"], r["power2"][:, :, [k - 1 for k in kp]])


@pytest.mark.parametrize("n1,n2", [(12, 8), (9, 7)])
def test_checker_puts_a_single_mode_where_it_belongs(n1, n2):
    i, j = np.arange(n1)[:, None, None], np.arange(n2)[None, :, None]
    amp = np.arange(1., 4.)[None, None, :]
    for m0 in (0, 1, n1 // 2, 3):
        a = amp * np.cos(2 * np.pi * m0 * i / n1 + 0.3 * j)
        px = spectra_ref(a)["power_x"]
        rest = np.abs(np.delete(px, m0, axis=0)).max()
        assert rest < 1e-20 * px[m0].max() and px[m0].min() > 0.1, (m0, rest)      # (the squares of float64 rounding errors)
        assert np.allclose(px[m0, 1] / px[m0, 0], 4.) and np.allclose(px[m0, 2] / px[m0, 0], 9.)      # the plane index scales the amplitude
    for q0 in (0, 1, n2 // 2):
        for m0 in (0, 2, n1 // 2):
            a = amp * np.cos(2 * np.pi * m0 * i / n1 + 0.4) * np.cos(2 * np.pi * q0 * j / n2 + 0.9)
            p2 = spectra_ref(a)["power2"][:, :, 0]
            top = p2[m0, q0]
            p2 = p2.copy(); p2[m0, q0] = 0.
            assert top > 0.1 and p2.max() < 1e-20 * top + 1e-22, (m0, q0)


def test_bounds_admit_the_least_accurate_transform_one_would_write():
    """a naive O(n^2) DFT with sequential accumulation in the working precision stays well inside the line bound, in either precision"""
    for real in (np.float64, np.float32):
        eps = np.finfo(real).eps
        for n1, n2 in ((40, 12), (56, 14)):
            a = (3. + np.random.RandomState(n1).randn(n1, n2, 1)).astype(real)
            tw = np.exp(-2j * np.pi * np.arange(n1) / n1).astype(np.complex64 if real == np.float32 else np.complex128)
            pw = np.zeros(n1 // 2 + 1, dtype=real)
            for j in range(n2):
                for m in range(n1 // 2 + 1):
                    acc = tw.dtype.type(0)
                    for i in range(n1):
                        acc = acc + a[i, j, 0] * tw[(i * m) % n1]
                    pw[m] += real(acc.real * acc.real + acc.imag * acc.imag)
            bp, _ = line_bounds(a, 1, eps)
            ratio = np.abs(pw - spectra_ref(a)["power_x"][:, 0]).max() / bp[0]
            assert ratio < 0.1, (real, n1, ratio)


# ---------------------------------------------------------------------------------------------- the files
def collected_from(a4, kplanes):
    """what spectra.collect would return on one rank for the four fields a4 (interior samples), from the checker"""
    n1, n2, n3 = a4[0].shape
    refs = [spectra_ref(a, kplanes) for a in a4]
    st = lambda key: np.asfortranarray(np.stack([r[key] for r in refs], axis=-1))
    return dict(n1=n1, n2=n2, kplanes=np.asarray(kplanes, dtype=np.int64), power_x=st("power_x"), lsum_x=st("lsum_x"), power_y=st("power_y"), lsum_y=st("lsum_y"),
                power2=st("power2"))


@pytest.mark.parametrize("shape", [(12, 8, 4), (9, 7, 4)], ids=["even", "odd"])
def test_files_as_their_consumer_reads_them(tmp_path, shape):
    n1, n2, nz = shape
    rng = np.random.RandomState(3)
    a4 = [2. + rng.randn(*shape) for _ in range(4)]
    kplanes = [4, 1]
    c = collected_from(a4, kplanes)
    zc = np.array([-0.05, 0.05, 0.3, 0.7, 0.95, 1.05])      # haloed: zc(0 ... nz+1)
    spectra.write(str(tmp_path), 1200, c, zc)
    assert len(os.listdir(str(tmp_path))) == 16
    r = spectra.read(str(tmp_path), 1200, n1, n2)
    s = spectra.normalise(c)
    for key in ("x0", "xs", "y0", "ys", "s2"):
        assert r[key].shape == s[key].shape and np.array_equal(r[key], s[key]), key
    assert r["kplanes"].tolist() == kplanes and r["zc"].tolist() == [zc[4], zc[1]]
    wx = mode_weights(n1)
    for v, var in enumerate(spectra.VARS):
        stem = os.path.join(str(tmp_path), f"spectra_{var}_fld_0001200")
        # the consumer's average_spectra_1d: count and offset of the two blocks, reshaped in Fortran order
        for ext, n, k0, ks in (("_1d_x.bin", n1, "x0", "xs"), ("_1d_y.bin", n2, "y0", "ys")):
            size = (n // 2 + 1) * nz
            assert os.path.getsize(stem + ext) == 2 * size * 8
            first = np.fromfile(stem + ext, dtype="float64", count=size, offset=0).reshape((n // 2 + 1, nz), order="F")
            second = np.fromfile(stem + ext, dtype="float64", count=size, offset=size * 8).reshape((n // 2 + 1, nz), order="F")
            assert np.array_equal(first, s[k0][:, :, v]) and np.array_equal(second, s[ks][:, :, v])
        data = np.fromfile(stem + "_2d.bin", dtype="float64").reshape((n1 // 2 + 1, n2 // 2 + 1, 2), order="F")
        assert np.array_equal(data, s["s2"][:, :, :, v])
        meta = np.loadtxt(stem + "_kplanes.out")
        assert meta.shape == (2, 2) and meta[:, 0].tolist() == [4., 1.]
        # the consumer's compute_scales: irfft(x0, axis=0)[0] / 2 is what it calls the variance -- the plane mean of f^2
        mean2 = (a4[v] ** 2).mean((0, 1))
        assert np.allclose(np.fft.irfft(s["x0"][:, :, v], n=n1, axis=0)[0] / 2., mean2, rtol=1e-12)
        assert np.allclose(np.fft.irfft(s["y0"][:, :, v], n=n2, axis=0)[0] / 2., mean2, rtol=1e-12)
        # ... and irfft(x0) / 2 the autocorrelation along x at zero y separation
        r1 = (a4[v] * np.roll(a4[v], -1, axis=0)).mean((0, 1))
        assert np.allclose(np.fft.irfft(s["x0"][:, :, v], n=n1, axis=0)[1] / 2., r1, rtol=1e-10, atol=1e-12)
        # xs: the spectrum of the y-averaged line
        line = a4[v].mean(1)
        assert np.allclose(s["xs"][:, :, v], 2. * np.abs(np.fft.rfft(line, axis=0)) ** 2 / n1, rtol=1e-11, atol=1e-14)
        assert np.allclose(s["ys"][:, :, v], 2. * np.abs(np.fft.rfft(a4[v].mean(0), axis=0)) ** 2 / n2, rtol=1e-11, atol=1e-14)
        # sum w_m S2 is the plane mean of f^2
        assert np.allclose(np.einsum("m,mqp->p", wx, s["s2"][:, :, :, v]), mean2[[3, 0]], rtol=1e-12)
    # interior heights give the same file; a wrong number of heights is refused
    spectra.write(str(tmp_path), 1300, c, zc[1:-1])
    assert open(os.path.join(str(tmp_path), "spectra_u_fld_0001200_kplanes.out")).read() == open(os.path.join(str(tmp_path), "spectra_u_fld_0001300_kplanes.out")).read()
    with pytest.raises(ValueError):
        spectra.write(str(tmp_path), 1400, c, zc[:3])


def test_add_ranks_of_two_row_halves_is_the_whole(tmp_path):
    shape = (12, 8, 3)
    rng = np.random.RandomState(9)
    a4 = [1. + rng.randn(*shape) for _ in range(4)]
    whole = collected_from(a4, [2])
    parts = []
    for rows in (slice(0, 4), slice(4, 8)):
        p = collected_from([a[:, rows, :] for a in a4], [2])
        p.update(n2=8, power_y=None, lsum_y=None, power2=None)      # a rank knows the global n2 and gathers x only
        parts.append(p)
    both = spectra.add_ranks(parts)
    assert np.allclose(both["power_x"], whole["power_x"], rtol=1e-13) and np.allclose(both["lsum_x"], whole["lsum_x"], rtol=1e-13, atol=1e-12)
    assert both["power_x"].flags.f_contiguous and both["power_y"] is None
    s, w = spectra.normalise(both), spectra.normalise(whole)
    assert np.allclose(s["x0"], w["x0"], rtol=1e-13) and np.allclose(s["xs"], w["xs"], rtol=1e-12, atol=1e-15) and s["y0"] is None and s["s2"] is None
    spectra.write(str(tmp_path), 5, both, np.arange(3.))      # several ranks: the x files only
    assert sorted(os.listdir(str(tmp_path))) == sorted(f"spectra_{v}_fld_0000005_1d_x.bin" for v in spectra.VARS)

"""include/cales_derived.h without a GPU: the header against capi.DERIVED_SYMBOLS, the two libraries and the Fortran module; the numpy restatement of the
reference's src/post.f90 (derived_ref) that the GPU tests compare with, pinned on analytic fields; the arithmetic the kernels call
(cales_amd/csrc/derived_math.hpp) compiled for the host and held to the bits of the restatement; the files of cales_amd/derived.py.

derived_ref evaluates every expression of post.f90 term by term in the order it is written there, as Fortran parses it (left to right within one
precedence level, x**2 as x * x), in the arrays' own dtype: every numpy operation is one IEEE rounding, and so is every operation of derived_math.hpp
(contraction off). The two therefore agree bit for bit, in float64 and in float32, and the tests ask for np.array_equal."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cales_amd import capi
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cales_amd", "csrc")
NAMES = ("vox", "voy", "voz", "str", "ens", "qcr", "vox_edge", "voy_edge", "voz_edge")      # in the order of enum cales_derived


# ---------------------------------------------------------------------------------------------- the restatement
def derived_ref(u, v, w, dli, dzci, dzfi, dtype):
    """{name: (n1, n2, n3)} of the nine quantities at the interior cells of the haloed arrays u, v, w (0:n1+1, 0:n2+1, 0:n3+1); dli = (dxi, dyi[, dzi]),
    dzci, dzfi (0:n3+1). Everything is converted to `dtype` first and stays in it."""
    T = np.dtype(dtype).type
    ux, uy, uz = (np.asarray(a, dtype=T) for a in (u, v, w))
    n1, n2, n3 = (s - 2 for s in ux.shape)
    dxi, dyi = T(dli[0]), T(dli[1])
    zc, zf = np.asarray(dzci, dtype=T), np.asarray(dzfi, dtype=T)
    dzc_k, dzc_m, dzf_k = zc[None, None, 1:n3 + 1], zc[None, None, 0:n3], zf[None, None, 1:n3 + 1]      # dzci(k), dzci(k-1), dzfi(k)
    q25, two, half = T(0.25), T(2), T(0.5)

    def S(a, di, dj, dk):
        return a[1 + di:n1 + 1 + di, 1 + dj:n2 + 1 + dj, 1 + dk:n3 + 1 + dk]
    X = lambda di, dj, dk: S(ux, di, dj, dk)
    Y = lambda di, dj, dk: S(uy, di, dj, dk)
    Z = lambda di, dj, dk: S(uz, di, dj, dk)
    out = {}
    # post.f90:33-38
    out["vox"] = q25 * ((Z(0, 1, 0) - Z(0, 0, 0)) * dyi - (Y(0, 0, 1) - Y(0, 0, 0)) * dzc_k +
                        (Z(0, 1, -1) - Z(0, 0, -1)) * dyi - (Y(0, 0, 0) - Y(0, 0, -1)) * dzc_m +
                        (Z(0, 0, 0) - Z(0, -1, 0)) * dyi - (Y(0, -1, 1) - Y(0, -1, 0)) * dzc_k +
                        (Z(0, 0, -1) - Z(0, -1, -1)) * dyi - (Y(0, -1, 0) - Y(0, -1, -1)) * dzc_m)
    # :40-45
    out["voy"] = q25 * ((X(0, 0, 1) - X(0, 0, 0)) * dzc_k - (Z(1, 0, 0) - Z(0, 0, 0)) * dxi +
                        (X(0, 0, 0) - X(0, 0, -1)) * dzc_m - (Z(1, 0, -1) - Z(0, 0, -1)) * dxi +
                        (X(-1, 0, 1) - X(-1, 0, 0)) * dzc_k - (Z(0, 0, 0) - Z(-1, 0, 0)) * dxi +
                        (X(-1, 0, 0) - X(-1, 0, -1)) * dzc_m - (Z(0, 0, -1) - Z(-1, 0, -1)) * dxi)
    # :47-52
    out["voz"] = q25 * ((Y(1, 0, 0) - Y(0, 0, 0)) * dxi - (X(0, 1, 0) - X(0, 0, 0)) * dyi +
                        (Y(1, -1, 0) - Y(0, -1, 0)) * dxi - (X(0, 0, 0) - X(0, -1, 0)) * dyi +
                        (Y(0, 0, 0) - Y(-1, 0, 0)) * dxi - (X(-1, 1, 0) - X(-1, 0, 0)) * dyi +
                        (Y(0, -1, 0) - Y(-1, -1, 0)) * dxi - (X(-1, 0, 0) - X(-1, -1, 0)) * dyi)
    # :126, :136, :146
    out["vox_edge"] = (Z(0, 1, 0) - Z(0, 0, 0)) * dyi - (Y(0, 0, 1) - Y(0, 0, 0)) * dzc_k
    out["voy_edge"] = (X(0, 0, 1) - X(0, 0, 0)) * dzc_k - (Z(1, 0, 0) - Z(0, 0, 0)) * dxi
    out["voz_edge"] = (Y(1, 0, 0) - Y(0, 0, 0)) * dxi - (X(0, 1, 0) - X(0, 0, 0)) * dyi

    def sq(t):
        return t * t

    def cross(sgn):
        """the three sums .25*(t1**2 + t2**2 + t3**2 + t4**2)*.25 of strain_rate (sgn = +1, :80-97) and rotation_rate (sgn = -1, :172-189)"""
        pm = (lambda a, b: a + b) if sgn > 0 else (lambda a, b: a - b)
        x12 = q25 * (sq(pm((X(0, 1, 0) - X(0, 0, 0)) * dyi, (Y(1, 0, 0) - Y(0, 0, 0)) * dxi)) +
                     sq(pm((X(0, 0, 0) - X(0, -1, 0)) * dyi, (Y(1, -1, 0) - Y(0, -1, 0)) * dxi)) +
                     sq(pm((X(-1, 1, 0) - X(-1, 0, 0)) * dyi, (Y(0, 0, 0) - Y(-1, 0, 0)) * dxi)) +
                     sq(pm((X(-1, 0, 0) - X(-1, -1, 0)) * dyi, (Y(0, -1, 0) - Y(-1, -1, 0)) * dxi))) * q25
        x13 = q25 * (sq(pm((X(0, 0, 1) - X(0, 0, 0)) * dzc_k, (Z(1, 0, 0) - Z(0, 0, 0)) * dxi)) +
                     sq(pm((X(0, 0, 0) - X(0, 0, -1)) * dzc_m, (Z(1, 0, -1) - Z(0, 0, -1)) * dxi)) +
                     sq(pm((X(-1, 0, 1) - X(-1, 0, 0)) * dzc_k, (Z(0, 0, 0) - Z(-1, 0, 0)) * dxi)) +
                     sq(pm((X(-1, 0, 0) - X(-1, 0, -1)) * dzc_m, (Z(0, 0, -1) - Z(-1, 0, -1)) * dxi))) * q25
        x23 = q25 * (sq(pm((Y(0, 0, 1) - Y(0, 0, 0)) * dzc_k, (Z(0, 1, 0) - Z(0, 0, 0)) * dyi)) +
                     sq(pm((Y(0, 0, 0) - Y(0, 0, -1)) * dzc_m, (Z(0, 1, -1) - Z(0, 0, -1)) * dyi)) +
                     sq(pm((Y(0, -1, 1) - Y(0, -1, 0)) * dzc_k, (Z(0, 0, 0) - Z(0, -1, 0)) * dyi)) +
                     sq(pm((Y(0, -1, 0) - Y(0, -1, -1)) * dzc_m, (Z(0, 0, -1) - Z(0, -1, -1)) * dyi))) * q25
        return x12, x13, x23
    # :77-98
    s11, s22, s33 = sq((X(0, 0, 0) - X(-1, 0, 0)) * dxi), sq((Y(0, 0, 0) - Y(0, -1, 0)) * dyi), sq((Z(0, 0, 0) - Z(0, 0, -1)) * dzf_k)
    s12, s13, s23 = cross(+1)
    out["str"] = s11 + s22 + s33 + two * (s12 + s13 + s23)
    # :172-190
    e12, e13, e23 = cross(-1)
    out["ens"] = two * (e12 + e13 + e23)
    # :207
    out["qcr"] = half * (out["ens"] - out["str"])
    for k, a in out.items():
        assert a.dtype == T and a.shape == (n1, n2, n3), (k, a.dtype, a.shape)
    return {k: np.asfortranarray(out[k]) for k in NAMES}


def metrics_of(case, dtype):
    """dli, dzci, dzfi of a context of this case in the library's arithmetic (api.hip, cales_create): dl = l / ng, dli = 1 / dl, dzci = 1 / dzc, dzfi = 1 / dzf,
    each one rounding in `dtype` (a quotient of two floats formed in double and rounded to float is the correctly rounded float quotient)"""
    from cales_amd.hotpath import initgrid
    T = np.dtype(dtype).type
    assert T == capi.np_real      # (initgrid works in the library's precision)
    g = initgrid(case.gtype, int(case.ng[2]), case.gr, case.l[2])
    dli = [T(1) / (T(l) / T(float(n))) for l, n in zip(case.l, case.ng)]
    return dli, T(1) / g["dzc"], T(1) / g["dzf"]


# ---------------------------------------------------------------------------------------------- header, lists, libraries
def declarations(header):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(", hdr))


def test_derived_header_equals_the_symbol_list_and_both_libraries_export_it():
    hdr, declared = declarations("cales_derived.h")
    assert '#include "cales_post.h"' in hdr
    assert declared == set(capi.DERIVED_SYMBOLS) == {"cales_derived_box", "cales_derived_out2d", "cales_derived_out3d", "cales_derived_to_pp"}
    assert len(capi.DERIVED_SYMBOLS) == 4
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r"CALES_DERIVED_([A-Z_]+)\s*=\s*(\d+)", hdr))
    assert enum == capi.DERIVED and tuple(sorted(enum, key=enum.get)) == NAMES
    assert int(re.search(r"CALES_NDERIVED\s*=\s*(\d+)", hdr).group(1)) == len(NAMES) == 9
    if os.environ.get("CALES_NO_TORCH") != "1":
        import torch  # noqa: F401  (one HIP runtime per process: see capi.lib)
    for so in ("libcales_hip.so", "libcales_hip_sp.so"):
        L = C.CDLL(os.path.join(ROOT, "cales_amd", so))
        for s in capi.DERIVED_SYMBOLS:
            assert hasattr(L, s), (so, s)
    for s in capi.DERIVED_SYMBOLS:
        assert getattr(capi.lib(), s).argtypes, s      # bound with argument types by capi.lib()


def test_derived_symbols_are_a_list_of_their_own_and_the_field_enum_is_untouched():
    for other in (capi.SYMBOLS, capi.POST_SYMBOLS, capi.PDF_SYMBOLS, capi.SPECTRA_SYMBOLS):
        assert not set(capi.DERIVED_SYMBOLS) & set(other)
    for header in ("cales.h", "cales_post.h", "cales_pdf.h", "cales_spectra.h"):
        hdr, declared = declarations(header)
        assert not declared & set(capi.DERIVED_SYMBOLS), header
        assert "cales_derived" not in open(os.path.join(ROOT, "include", header)).read(), header
    hdr, _ = declarations("cales.h")
    assert int(re.search(r"CALES_NFIELDS\s*=\s*(\d+)", hdr).group(1)) == len(capi.FIELDS) == 15


def test_fortran_module_declares_the_entries():
    txt = open(os.path.join(ROOT, "cales_amd", "fortran", "cales_c.f90")).read()
    for s in capi.DERIVED_SYMBOLS:
        assert re.search(r"function\s+" + s + r"\s*\(([^)]*)\)\s*bind\(C,\s*name='" + s + r"'\)", txt), s
    n_args = lambda s: len(re.search(r"function\s+" + s + r"\s*\(([^)]*)\)", txt).group(1).split(","))
    assert [n_args(s) for s in capi.DERIVED_SYMBOLS] == [7, 6, 5, 2]
    for name, v in capi.DERIVED.items():
        assert re.search(r"CALES_DERIVED_" + name.upper() + r"\s*=\s*" + str(v) + r"\b", txt), name


def test_the_package_does_not_name_the_checker_side():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "cales_amd")):
        for f in files:
            if f in ("derived.py", "k_derived.hip", "derived_math.hpp"):
                assert "oracle" not in open(os.path.join(dirpath, f)).read(), f


# ---------------------------------------------------------------------------------------------- the restatement's own pins
# A grid on which every input of the pins is exact in float32 and float64: n = (8, 8, 8), dx = dy = 1/8, faces zf(k) = (k/8)^2, centres
# zc(k) = (zf(k) + zf(k-1)) / 2 (multiples of 1/128), so dzc, dzf and the fields below are exact and only 1/dzc, 1/dzf are rounded.
PIN_N = 8


def pin_grid(T):
    n = PIN_N
    k = np.arange(-1, n + 2, dtype=np.float64)
    zf = (k / n) ** 2 * np.sign(k)                      # faces -1 ... n+1 (odd continuation below the wall: still stretched, still exact)
    zc = 0.5 * (zf[1:] + zf[:-1])                       # centres 0 ... n+1
    dzc = np.append(zc[1:] - zc[:-1], zc[-1] - zc[-2])  # dzc(k) = zc(k+1) - zc(k), k = 0 ... n+1 (the last one is never used)
    dzf = zf[1:] - zf[:-1]                              # dzf(k) = zf(k) - zf(k-1)
    x = np.arange(0, n + 2, dtype=np.float64) / n       # faces 0 ... n+1: x(i) = i / n; centres x(i) - 1 / (2 n)
    for a in (zf, zc, dzc, dzf, x):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return dict(zc=zc, xf=x, xc=x - 0.5 / n, dli=(T(n), T(n)), dzci=T(1) / dzc.astype(T), dzfi=T(1) / dzf.astype(T))


def fields(T, fu, fv, fw, g):
    """u at (x face, y centre, z centre), v at (x centre, y face, z centre), w at (x centre, y centre, z face is not needed by the pins)"""
    xf, xc, zc = g["xf"], g["xc"], g["zc"]
    mesh = lambda a, b, c: np.meshgrid(a, b, c, indexing="ij")
    u = fu(*mesh(xf, xc, zc)); v = fv(*mesh(xc, xf, zc)); w = fw(*mesh(xc, xc, zc))
    out = [np.asfortranarray(a, dtype=T) for a in (u, v, w)]
    for a, b in zip(out, (u, v, w)):
        assert np.array_equal(a.astype(np.float64), b)      # the fields are exact in T
    return out


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["float64", "float32"])
def test_pins_of_the_restatement(T):
    """eps = np.finfo(T).eps, two unit roundoffs. Every input is exact (pin_grid), so a difference of two samples is exact and a term (difference) * metric
    carries at most the rounding of the reciprocal metric and of the product: (1 + d), |d| <= eps. Where the metric is a power of two (x, y) it carries
    none. A sum of four terms of size t adds three roundings of partial sums <= 4 t: <= 4.5 eps t; the factors .25, .5 and 2 are exact.
      shear u = a + b zc:     voy = .25 (4 terms b (1 + d)): |voy - b| <= (4 eps b + 4.5 eps b) / 4 < 3 eps b.
                              t^2 = b^2 (1 + 2.5 eps), the sum of four 4 b^2 (1 + 2.5 eps + 1.125 eps): SijSij = WijWij = b^2 / 2 within 4 eps b^2,
                              Q = .5 (WijWij - SijSij) within 4 eps b^2 of 0 (in fact 0: x + 0 and x - 0 are the same bits)
      rotation, plane strain: dx = dy = 1/8, every term is exact: the pins hold exactly; they are asserted within the same 4 eps of the scale"""
    eps = float(np.finfo(T).eps)
    g = pin_grid(T)
    zero = lambda x, y, z: 0. * x
    close = lambda got, want, scale, n: np.abs(got.astype(np.float64) - want).max() <= n * eps * scale
    # linear shear
    a, b = 0.5, 3.
    r = derived_ref(*fields(T, lambda x, y, z: a + b * z, zero, zero, g), g["dli"], g["dzci"], g["dzfi"], T)
    assert close(r["voy"], b, b, 3) and close(r["voy_edge"], b, b, 1) and close(r["str"], b * b / 2, b * b, 4) and close(r["ens"], b * b / 2, b * b, 4)
    assert close(r["qcr"], 0., b * b, 4) and not r["vox"].any() and not r["voz"].any()
    # solid-body rotation about z
    om = 1.5
    r = derived_ref(*fields(T, lambda x, y, z: -om * (y - 0.5), lambda x, y, z: om * (x - 0.5), zero, g), g["dli"], g["dzci"], g["dzfi"], T)
    assert close(r["voz"], 2 * om, om, 4) and close(r["str"], 0., om * om, 4) and close(r["ens"], 2 * om * om, om * om, 4) and close(r["qcr"], om * om, om * om, 4)
    assert close(r["voz_edge"], 2 * om, om, 4) and not r["vox"].any() and not r["voy"].any()
    # plane strain
    al = 0.75
    r = derived_ref(*fields(T, lambda x, y, z: al * x, lambda x, y, z: -al * y, zero, g), g["dli"], g["dzci"], g["dzfi"], T)
    assert close(r["str"], 2 * al * al, al * al, 4) and close(r["ens"], 0., al * al, 4) and close(r["qcr"], -al * al, al * al, 4)
    assert not r["vox"].any() and not r["voy"].any() and not r["voz"].any()


@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["float64", "float32"])
def test_centre_vorticity_is_the_mean_of_the_four_edges(T):
    """On random fields the centre value sums eight terms left to right, the mean of the edges sums four differences of two: the same eight terms t in
    another association. Either sum makes seven roundings of partial sums <= 8 max|t|: each is within 28 eps / 2 max|t| of the exact sum, so the two
    differ by at most .25 * 28 eps max|t| = 7 eps max|t|, and max|t| <= 2 max|velocity| max(metric) =: scale. Asserted: 8 eps scale."""
    eps = float(np.finfo(T).eps)
    rng = np.random.RandomState(7)
    n = (7, 6, 5)
    u, v, w = (np.asfortranarray(rng.randn(*[m + 2 for m in n]), dtype=T) for _ in range(3))
    dzc = 0.1 + rng.rand(n[2] + 2); dzf = 0.1 + rng.rand(n[2] + 2)
    dli, dzci, dzfi = (T(7.), T(3.)), (1 / dzc).astype(T), (1 / dzf).astype(T)
    r = derived_ref(u, v, w, dli, dzci, dzfi, T)
    scale = 2. * max(float(np.abs(a).max()) for a in (u, v, w)) * max(7., 3., float(dzci.max()))
    q = T(0.25)
    e = r["vox_edge"]; mean = q * (e[:, 1:, 1:] + e[:, 1:, :-1] + e[:, :-1, 1:] + e[:, :-1, :-1])
    assert np.abs(r["vox"][:, 1:, 1:].astype(np.float64) - mean).max() <= 8 * eps * scale
    e = r["voy_edge"]; mean = q * (e[1:, :, 1:] + e[1:, :, :-1] + e[:-1, :, 1:] + e[:-1, :, :-1])
    assert np.abs(r["voy"][1:, :, 1:].astype(np.float64) - mean).max() <= 8 * eps * scale
    e = r["voz_edge"]; mean = q * (e[1:, 1:, :] + e[1:, :-1, :] + e[:-1, 1:, :] + e[:-1, :-1, :])
    assert np.abs(r["voz"][1:, 1:, :].astype(np.float64) - mean).max() <= 8 * eps * scale
    assert np.abs(r["vox"]).max() > 1. and np.abs(r["voy"]).max() > 1. and np.abs(r["voz"]).max() > 1.
    assert np.array_equal(r["qcr"], T(0.5) * (r["ens"] - r["str"]))


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic on the host
def test_derived_math_gives_the_bits_of_the_restatement(tmp_path):
    """tests/derived_host.cpp includes cales_amd/csrc/derived_math.hpp, the functions both kernel forms call, and evaluates all nine quantities in double
    and in float on a random field (interior and ghost cells) of shape (7, 6, 5) with stretched metrics; built under -fsanitize=address,undefined with
    contraction off, as the header demands of a compiler that does not know its pragma"""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "derived_host")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", CSRC, os.path.join(ROOT, "tests", "derived_host.cpp"), "-o", exe])
    n = (7, 6, 5)
    rng = np.random.RandomState(3)
    u, v, w = (np.asfortranarray(rng.randn(*[m + 2 for m in n])) for _ in range(3))
    dxi, dyi = 7. / 3., 11. / 5.
    dzci, dzfi = 1. / (0.05 + rng.rand(n[2] + 2)), 1. / (0.05 + rng.rand(n[2] + 2))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.asarray(n, dtype=np.float64), [dxi, dyi], dzci, dzfi] + [a.ravel(order="F") for a in (u, v, w)]).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(fout).reshape((n[0], n[1], n[2], 9, 2), order="F")
    differ = 0
    for p, T in enumerate((np.float64, np.float32)):
        want = derived_ref(u, v, w, (dxi, dyi), dzci, dzfi, T)
        for q, name in enumerate(NAMES):
            assert np.isfinite(want[name]).all() and np.abs(want[name]).max() > 0.
            assert np.array_equal(got[:, :, :, q, p], want[name].astype(np.float64)), (name, T.__name__, np.abs(got[:, :, :, q, p] - want[name]).max())
            if p == 1:
                differ += int((got[:, :, :, q, 0] != got[:, :, :, q, 1]).sum())
    assert differ > 9 * 100      # (the float results are float's own, not rounded doubles)


# ---------------------------------------------------------------------------------------------- the files of cales_amd/derived.py
class _Stub:
    """what write_visu_3d asks of a host: case, cs, derived_out3d"""
    def __init__(self, case, nranks=1, rank=0):
        self.case, self.cs = case, capi.make_case(case, nranks, rank)
        self.calls = []

    def derived_out3d(self, name, nskip):
        from cales_amd.hotpath import _box_share
        self.calls.append((name, tuple(nskip)))
        ng = [int(x) for x in self.case.ng]
        first, count = _box_share(self.cs, (1, 1, 1), ng, nskip)
        i, j, k = np.meshgrid(*[first[d] + nskip[d] * np.arange(count[d]) for d in range(3)], indexing="ij")
        return np.asfortranarray(capi.DERIVED[name] * 1e6 + i + 100. * j + 10000. * k, dtype=capi.np_real)


def test_log_line_is_the_reference_format():
    from cales_amd.derived import log_line
    l = log_line("vox_fld_0000012.bin", "Vorticity_X", (1, 1, 1), (8, 6, 4), (2, 1, 1), 0.125, 12)
    assert l == " " * 11 + "vox_fld_0000012.bin" + " " * 4 + "Vorticity_X" + "    1    1    1    8    6    4    2    1    1" + "  0.1250000E+000" + "     12"
    assert len(l) == 30 + 15 + 45 + 16 + 7
    assert log_line("a", "b", (1, 1, 1), (2, 2, 2), (1, 1, 1), -1234.56789, 3)[90:106] == " -0.1234568E+004"
    assert log_line("a", "b", (1, 1, 1), (2, 2, 2), (1, 1, 1), 0., 3)[90:106] == "  0.0000000E+000"
    assert log_line("a", "b", (1, 1, 1), (2, 2, 2), (1, 1, 1), 9.99999999e-5, 3)[90:106] == "  0.1000000E-003"


@pytest.mark.parametrize("nskip", [(1, 1, 1), (2, 3, 1)], ids=["dense", "strided"])
def test_write_visu_3d_files(tmp_path, nskip):
    from cales_amd.derived import VARNAMES, write_visu_3d
    g, case = load_golden("tgv_ppp"); case.ng[:] = (8, 6, 4)
    h = _Stub(case)
    write_visu_3d(h, str(tmp_path), 12, 0.125, nskip=nskip)
    write_visu_3d(h, str(tmp_path), 24, 0.25, names=("str", "ens"), nskip=nskip)
    names = [("vox", 12), ("voy", 12), ("voz", 12), ("qcr", 12), ("str", 24), ("ens", 24)]
    assert sorted(os.listdir(str(tmp_path))) == sorted([f"{n}_fld_{s:07d}.bin" for n, s in names] + ["log_visu_3d.out"])
    shape = tuple((m - 1) // s + 1 for m, s in zip((8, 6, 4), nskip))
    i, j, k = np.meshgrid(*[1 + s * np.arange(c) for s, c in zip(nskip, shape)], indexing="ij")
    for n, s in names:
        a = np.fromfile(os.path.join(str(tmp_path), f"{n}_fld_{s:07d}.bin"), dtype=capi.np_real)
        assert a.size == np.prod(shape)
        assert np.array_equal(a.reshape(shape, order="F"), (capi.DERIVED[n] * 1e6 + i + 100. * j + 10000. * k).astype(capi.np_real)), n
    lines = open(os.path.join(str(tmp_path), "log_visu_3d.out")).read().splitlines()
    assert len(lines) == 6
    for (n, s), l in zip(names, lines):
        w = l.split()
        assert w[:2] == [f"{n}_fld_{s:07d}.bin", VARNAMES[n]] and w[2:11] == ["1", "1", "1", "8", "6", "4"] + [str(x) for x in nskip] and int(w[-1]) == s, l
        assert len(l) == 113
    assert [VARNAMES[n] for n, _ in names] == ["Vorticity_X", "Vorticity_Y", "Vorticity_Z", "Q-criterion", "SijSij", "WijWij"]
    with pytest.raises(ValueError):
        write_visu_3d(h, str(tmp_path), 1, 0., names=("vox_edge",))


def test_write_visu_3d_ranks_share_a_file(tmp_path):
    """three ranks, each writing its rows: the file is the one-rank file, the log has one line per file"""
    from cales_amd.derived import write_visu_3d
    g, case = load_golden("tgv_ppp"); case.ng[:] = (8, 6, 4)
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir(); many.mkdir()
    write_visu_3d(_Stub(case), str(one), 5, 1.5, names=("qcr",), nskip=(1, 2, 1))
    for r in (2, 0, 1):
        write_visu_3d(_Stub(case, 3, r), str(many), 5, 1.5, names=("qcr",), nskip=(1, 2, 1))
    assert open(one / "qcr_fld_0000005.bin", "rb").read() == open(many / "qcr_fld_0000005.bin", "rb").read()
    assert open(one / "log_visu_3d.out").read() == open(many / "log_visu_3d.out").read()

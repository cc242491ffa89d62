"""include/cales_pdf.h without a GPU: the header against capi.PDF_SYMBOLS, the two libraries and the Fortran module; the numpy restatement of its bin
rule -- the checker the device tests compare integer counts with, tests/test_gpu_pdf.py -- on hand-made edge cases; and the files of cales_amd/pdfs.py,
read the way their consumer reads them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cales_amd import capi, pdfs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the checker
def bin_of(x, nbins, lo, hi, real=None):
    """The bin rule of include/cales_pdf.h in arrays of `real` (default: the library's precision), the same three operations in the same order:
    s = real(nbins) / (hi - lo); t = (x - lo) * s; -1 where t < 0 (below), nbins where not t < nbins (above), else int(t)."""
    R = real or capi.np_real
    x = np.asarray(x, dtype=R)
    lo, hi = R(lo), R(hi)
    with np.errstate(all="ignore"):
        s = R(nbins) / (hi - lo)
        d = x - lo
        t = d * s
        assert s.dtype == R and t.dtype == R
        below = t < R(0)
        above = ~(t < R(nbins))
        inside = ~(below | above)
        b = np.where(inside, t, R(0)).astype(np.int64)      # (int)t: truncation
    return np.where(below, -1, np.where(above, nbins, b))


def pdf_ref(a, nbins, lo, hi, real=None):
    """counts (nbins, n3), outside (2, n3) of the samples a[:, :, k] (interior cells only)"""
    n3 = a.shape[2]
    counts, outside = np.zeros((nbins, n3), dtype=np.int64, order="F"), np.zeros((2, n3), dtype=np.int64, order="F")
    for k in range(n3):
        b = bin_of(a[:, :, k], nbins, lo, hi, real).ravel()
        outside[0, k], outside[1, k] = (b < 0).sum(), (b >= nbins).sum()
        counts[:, k] = np.bincount(b[(b >= 0) & (b < nbins)], minlength=nbins)
    return counts, outside


def jpdf_ref(a, b, nbins, ra, rb, kplanes, real=None):
    """counts (nbins, nbins, nplanes), first axis a; outside (nplanes): either variable outside. a, b: interior cells; kplanes: 1-based"""
    counts, outside = np.zeros((nbins, nbins, len(kplanes)), dtype=np.int64, order="F"), np.zeros(len(kplanes), dtype=np.int64)
    for q, k in enumerate(kplanes):
        ia, ib = bin_of(a[:, :, k - 1], nbins, ra[0], ra[1], real).ravel(), bin_of(b[:, :, k - 1], nbins, rb[0], rb[1], real).ravel()
        ok = (ia >= 0) & (ia < nbins) & (ib >= 0) & (ib < nbins)
        outside[q] = (~ok).sum()
        counts[:, :, q] = np.bincount(ia[ok] + nbins * ib[ok], minlength=nbins * nbins).reshape((nbins, nbins), order="F")
    return counts, outside


# ---------------------------------------------------------------------------------------------- header, lists, libraries
def declarations(header):
    """the names a header of include/ declares, its comments left out"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(", hdr))


def test_pdf_header_equals_the_symbol_list_and_both_libraries_export_it():
    hdr, declared = declarations("cales_pdf.h")
    assert '#include "cales.h"' in hdr
    assert declared == set(capi.PDF_SYMBOLS) == {"cales_pdf_planes", "cales_jpdf_planes"} and len(capi.PDF_SYMBOLS) == 2
    assert re.search(r"#define\s+CALES_PDF_MAX_BINS\s+4096\b", hdr) and re.search(r"#define\s+CALES_JPDF_MAX_BINS\s+128\b", hdr)
    assert (capi.PDF_MAX_BINS, capi.JPDF_MAX_BINS) == (4096, 128)
    if os.environ.get("CALES_NO_TORCH") != "1":
        import torch  # noqa: F401  (one HIP runtime per process: see capi.lib)
    for so in ("libcales_hip.so", "libcales_hip_sp.so"):
        L = C.CDLL(os.path.join(ROOT, "cales_amd", so))
        for s in capi.PDF_SYMBOLS:
            assert hasattr(L, s), (so, s)
    for s in capi.PDF_SYMBOLS:
        assert getattr(capi.lib(), s).argtypes, s      # bound with argument types by capi.lib()


def test_pdf_symbols_are_a_list_of_their_own():
    assert not set(capi.PDF_SYMBOLS) & set(capi.SYMBOLS)
    assert not set(capi.PDF_SYMBOLS) & set(capi.POST_SYMBOLS)
    for header in ("cales.h", "cales_post.h"):
        hdr, declared = declarations(header)
        assert not declared & set(capi.PDF_SYMBOLS), header
        assert "cales_pdf_planes" not in hdr and "cales_jpdf_planes" not in hdr, header


def test_fortran_module_declares_the_entries():
    txt = open(os.path.join(ROOT, "cales_amd", "fortran", "cales_c.f90")).read()
    for s in capi.PDF_SYMBOLS:
        m = re.search(r"function\s+" + s + r"\s*\(([^)]*)\)\s*bind\(C,\s*name='" + s + r"'\)", txt)
        assert m, s
    assert "integer(c_int64_t) :: counts(*),outside(*)" in txt
    n_args = lambda s: len(re.search(r"function\s+" + s + r"\s*\(([^)]*)\)", txt).group(1).split(","))
    assert n_args("cales_pdf_planes") == 7 and n_args("cales_jpdf_planes") == 12


# ---------------------------------------------------------------------------------------------- the bin rule on edge cases
@pytest.mark.parametrize("real", [np.float64, np.float32], ids=["float64", "float32"])
def test_checker_on_the_edges_of_the_rule(real):
    inf, nan = np.inf, np.nan
    # 4 bins over [1, 3): s = 2 exactly, bin edges at 1, 1.5, 2, 2.5, 3
    x = [1., 3., nan, inf, -inf, 0.99999, 1.5, 1.4999, 2.9999, 2.5, -0., 1e30, -1e30]
    assert bin_of(x, 4, 1., 3., real).tolist() == [0, 4, 4, 4, -1, -1, 1, 0, 3, 3, -1, 4, -1]
    # x == lo is in bin 0 and, where s is exact (a power of two), x == hi is above, whatever the number of bins
    for nbins in (1, 2, 64, 4096):
        assert bin_of([1., 3.], nbins, 1., 3., real).tolist() == [0, nbins]
    # ... where s is rounded, (hi - lo) * s is nbins or the number below it: the rule is the three operations, and x == hi goes where they put it
    for nbins in (1, 2, 7, 64, 100, 4096):
        b = bin_of([-2., 5.], nbins, -2., 5., real).tolist()
        t_hi = (real(5.) - real(-2.)) * (real(nbins) / (real(5.) - real(-2.)))
        assert b[0] == 0 and b[1] == (nbins if not t_hi < nbins else nbins - 1)
        below_hi, below_lo = np.nextafter(real(5.), real(-9.)), np.nextafter(real(-2.), real(-9.))
        b = bin_of([below_lo, below_hi], nbins, -2., 5., real).tolist()
        assert b[0] == -1 and b[1] in (nbins - 1, nbins)      # (a t that rounds up to nbins counts as above: the rule says so)
    # one bin: everything in [lo, hi) is in bin 0
    assert bin_of([0., 0.5, 0.999, 1., -1e-9, nan], 1, 0., 1., real).tolist() == [0, 0, 0, 1, -1, 1]
    # -0. - lo with lo = 0 gives t = -0., which is not < 0: bin 0
    assert bin_of([-0., 0.], 8, 0., 1., real).tolist() == [0, 0]


def test_checker_works_in_the_precision_it_is_given():
    # 1 + 2^-30 is 1 in float32 and above 1 in float64: with lo = 1 + 2^-29 the sample is below in double, and lo itself rounds to 1 in float
    x, lo = 1. + 2. ** -30, 1. + 2. ** -29
    assert bin_of([x], 4, lo, 3., np.float64).tolist() == [-1]
    assert bin_of([x], 4, lo, 3., np.float32).tolist() == [0]


def test_reference_counts_conserve_the_samples():
    rng = np.random.RandomState(0)
    a = rng.randn(9, 7, 5); b = rng.randn(9, 7, 5)
    a[3, 3, 2] = np.nan; b[1, 1, 1] = np.inf
    c, o = pdf_ref(a, 10, -1., 1.)
    assert np.array_equal(c.sum(0) + o.sum(0), np.full(5, 63))
    jc, jo = jpdf_ref(a, b, 6, (-1., 1.), (-50., 50.), [3, 2, 3])
    assert np.array_equal(jc.sum((0, 1)) + jo, np.full(3, 63)) and np.array_equal(jc[:, :, 0], jc[:, :, 2])
    # b's range covers every finite value: the marginal over b is the histogram of a (plane 3) -- but for the sample whose b is infinite (plane 2)
    c6, o6 = pdf_ref(a, 6, -1., 1.)
    assert np.array_equal(jc[:, :, 0].sum(1), c6[:, 2]) and jo[0] == o6[:, 2].sum()
    assert jc[:, :, 1].sum() + jo[1] == 63 and jo[1] == o6[:, 1].sum() + int(0 <= bin_of(a[1, 1, 1], 6, -1., 1.) < 6)


# ---------------------------------------------------------------------------------------------- the files
def synthetic(npdf=6, nz=4, njpdf=3, kplanes=(4, 1), per_plane=False):
    rng = np.random.RandomState(7)
    nv, npl = 5, len(kplanes)
    jr = rng.rand(npl, nv, 2) if per_plane else np.broadcast_to(rng.rand(nv, 2), (npl, nv, 2))
    jr = np.array(jr); jr[:, :, 1] += 1.5
    rg = rng.rand(nv, 2); rg[:, 1] += 1.25
    jp = rng.randint(0, 50000, size=(njpdf, njpdf, npl, nv, nv)).astype(np.int64)
    for a in range(nv):
        jp[:, :, :, a, :a + 1] = 0
    return dict(npdf=npdf, njpdf=njpdf, kplanes=np.asarray(kplanes, dtype=np.int64), ranges=rg, jranges=jr,
                pdf=np.asfortranarray(rng.randint(0, 2 ** 40, size=(npdf, nz, nv)).astype(np.int64)), outside=np.zeros((2, nz, nv), dtype=np.int64),
                jpdf=np.asfortranarray(jp), joutside=np.zeros((npl, nv, nv), dtype=np.int64))


@pytest.mark.parametrize("per_plane", [False, True], ids=["shared_ranges", "ranges_per_plane"])
def test_files_as_their_consumer_reads_them(tmp_path, per_plane):
    c = synthetic(per_plane=per_plane)
    npdf, nz, njpdf, npl = 6, 4, 3, 2
    zc = np.array([-0.05, 0.05, 0.3, 0.7, 0.95, 1.05])      # haloed: zc(0 ... nz+1)
    pdfs.write(str(tmp_path), 1200, c, zc)
    stem = os.path.join(str(tmp_path), "pdfs_fld_0001200")
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(stem) + e for e in ("_pdf.bin", "_pdf_meta.out", "_jpdf.bin", "_jpdf_meta.out"))
    # the 1-D file and its one-line meta file
    raw = np.fromfile(stem + "_pdf.bin", dtype="float64")
    assert raw.size == npdf * nz * 5
    assert np.array_equal(np.reshape(raw, (npdf, nz, 5), order="F"), c["pdf"])
    meta = np.loadtxt(stem + "_pdf_meta.out")
    assert meta.shape == (11,) and int(meta[0]) == npdf
    assert np.array_equal(meta[1:11:2], c["ranges"][:, 0]) and np.array_equal(meta[2:12:2], c["ranges"][:, 1])
    # the joint file: [:, :, plane, a, b]; one meta row per plane
    jraw = np.fromfile(stem + "_jpdf.bin", dtype="float64")
    data = np.reshape(jraw, (njpdf, njpdf, npl, 5, 5), order="F")
    assert np.array_equal(data, c["jpdf"])
    for a in range(5):
        for b in range(a + 1):
            assert not data[:, :, :, a, b].any()
    assert data[:, :, :, 0, 4].any() and data[:, :, :, 2, 3].any()
    jmeta = np.loadtxt(stem + "_jpdf_meta.out")
    assert jmeta.shape == (npl, 13) and (jmeta[:, 0] == njpdf).all()
    assert jmeta[:, 1].tolist() == [4., 1.] and jmeta[:, 2].tolist() == [zc[4], zc[1]]
    assert np.array_equal(jmeta[:, 3:13:2], c["jranges"][:, :, 0]) and np.array_equal(jmeta[:, 4:14:2], c["jranges"][:, :, 1])
    # our own reader
    r = pdfs.read(str(tmp_path), 1200)
    assert r["npdf"] == npdf and r["njpdf"] == njpdf and r["kplanes"].tolist() == [4, 1] and r["zc"].tolist() == [zc[4], zc[1]]
    assert r["pdf"].dtype == np.int64 and np.array_equal(r["pdf"], c["pdf"]) and np.array_equal(r["jpdf"], c["jpdf"])
    assert np.array_equal(r["ranges"], c["ranges"]) and np.array_equal(r["jranges"], c["jranges"])
    # interior heights give the same file
    pdfs.write(str(tmp_path), 1300, c, zc[1:-1])
    assert open(stem + "_jpdf_meta.out").read() == open(os.path.join(str(tmp_path), "pdfs_fld_0001300_jpdf_meta.out")).read()
    with pytest.raises(ValueError):
        pdfs.write(str(tmp_path), 1400, c, zc[:3])


def test_a_single_plane_and_the_sum_of_ranks(tmp_path):
    c = synthetic(kplanes=(2,))
    pdfs.write(str(tmp_path), 7, c, np.arange(4.))
    r = pdfs.read(str(tmp_path), 7)
    assert r["kplanes"].tolist() == [2] and r["zc"].tolist() == [1.] and np.array_equal(r["jpdf"], c["jpdf"])
    both = pdfs.add_ranks([c, c, c])
    for key in ("pdf", "outside", "jpdf", "joutside"):
        assert np.array_equal(both[key], 3 * c[key]) and both[key].flags.f_contiguous
    assert both["npdf"] == c["npdf"] and np.array_equal(both["jranges"], c["jranges"])

"""Host-side mirror of the reference operator interface for the per-step hot path.

`HotPath` owns one `cales_ctx` (one GPU, one HIP stream) and exposes the routines the reference driver
calls inside its time loop, under their reference names and argument meaning
(src/main.f90:417-507: rk, bulk_forcing, bounduvw, fillps, updt_rhs_b, solver, boundp, correc, updatep,
cmpt_sgs; src/main.f90:523-537: chkdt, chkdiv). All arithmetic runs in libcales_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np

from . import capi
from .nml import Case

RKCOEFF = ((32. / 60., 0.), (25. / 60., -17. / 60.), (45. / 60., -25. / 60.))   # src/param.f90:27-29
SMALL = np.finfo(capi.np_real).eps * 10 ** ((6 if capi.SINGLE else 15) // 2)     # src/param.f90:24: epsilon(1._rp)*10**(precision(1._rp)/2)


class CalesError(RuntimeError):
    pass


REAL = capi.np_real      # numpy dtype of rp: float64, or float32 with CALES_PRECISION=single (capi.py)
_COMPLEX = np.result_type(REAL, np.complex64)      # a pair of rp: complex128, or complex64


def _p(a: np.ndarray):
    if a.dtype != REAL or not (a.flags.f_contiguous or a.ndim == 1):
        raise ValueError(f"fields must be Fortran-ordered {np.dtype(REAL).name} arrays")
    return a.ctypes.data_as(C.c_void_p)


def _pc(a: np.ndarray):
    """a Fortran-ordered array of _COMPLEX where the library writes (2, ...) reals"""
    assert a.dtype == _COMPLEX and (a.flags.f_contiguous or a.ndim == 1)
    return a.ctypes.data_as(C.c_void_p)


class _In:
    """An input array in the library's precision (a converted copy when the caller's dtype differs, e.g. float64 fields handed to the
    single-precision build); keeps the copy alive for the duration of the call."""
    def __init__(self, a):
        a = np.asarray(a)
        self.a = a if a.dtype == REAL and (a.flags.f_contiguous or a.ndim == 1) else np.asfortranarray(a, dtype=REAL)
        self.p = self.a.ctypes.data_as(C.c_void_p)


def initgrid(gtype: int, n: int, gr: float, lz: float) -> Dict[str, np.ndarray]:
    """src/initgrid.f90:15 (host helper of the library)."""
    out = [np.zeros(n + 2, dtype=REAL) for _ in range(4)]
    rc = capi.lib().cales_initgrid(int(gtype), int(n), float(gr), float(lz), *[_p(a) for a in out])
    if rc:
        raise CalesError("cales_initgrid failed")
    return dict(dzc=out[0], dzf=out[1], zc=out[2], zf=out[3])


def initflow(case: Case) -> Tuple[np.ndarray, ...]:
    """src/initflow.f90:17, deterministic kinds; returns global haloed u,v,w,p."""
    cs = capi.make_case(case)
    shape = tuple(int(x) + 2 for x in case.ng)
    u, v, w, p = (np.zeros(shape, order="F", dtype=REAL) for _ in range(4))
    rc = capi.lib().cales_initflow(C.byref(cs), case.inivel.encode(), int(case.is_wallturb), _p(u), _p(v), _p(w), _p(p))
    if rc == 2:
        raise CalesError(f"inivel='{case.inivel}' relies on the Fortran RNG stream and is not offered")
    if rc:
        raise CalesError("ERROR: invalid name for initial velocity field")
    return u, v, w, p


def check_case(case: Case, nranks: int = 1) -> None:
    """The a-priori input checks of src/sanity.f90:33-67; raises like the reference aborts."""
    cs = capi.make_case(case, nranks, 0)
    buf = C.create_string_buffer(512)
    if capi.lib().cales_check_case(C.byref(cs), buf, 512):
        raise CalesError("*** Simulation aborted due to errors in the input file *** " + buf.value.decode())


def memory_in_use(handle=None) -> Tuple[int, int]:
    """(bytes, allocations) of device and pinned-host memory held by one context, or with no handle by every context of this process."""
    b, n = C.c_int64(0), C.c_int64(0)
    if capi.lib().cales_memory_in_use(handle, C.byref(b), C.byref(n)):
        raise CalesError("cales_memory_in_use failed")
    return int(b.value), int(n.value)


def _i3(v):
    v = [int(x) for x in v]
    if len(v) != 3:
        raise ValueError("three indices, one per direction")
    return (C.c_int32 * 3)(*v)


def _box_share(cs, lo, hi, nskip) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    first, count = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    L = capi.lib()
    if L.cales_box_share(C.byref(cs), _i3(lo), _i3(hi), _i3(nskip), first, count):
        raise CalesError(L.cales_last_error(None).decode())
    return tuple(first), tuple(count)


def box_share(case: Case, lo, hi, nskip=(1, 1, 1), nranks: int = 1, rank: int = 0) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """cales_box_share (include/cales_post.h; host only): (first, count) of the share of `rank` in the box of the points lo + m nskip <= hi, GLOBAL
    haloed indices 0 ... ng+1. x and z: every point; y: the points in the rows the rank owns (row 0 with the first rank, ng2+1 with the last)."""
    return _box_share(capi.make_case(case, nranks, rank), lo, hi, nskip)


def _derived_id(quantity) -> int:
    return capi.DERIVED[quantity] if isinstance(quantity, str) else int(quantity)


class HotPath:
    def __init__(self, case: Case, nranks: int = 1, rank: int = 0, stream: int | None = None):
        self.case = case
        self.L = capi.lib()
        self.cs = capi.make_case(case, nranks, rank)
        h = C.c_void_p()
        rc = self.L.cales_create(C.byref(self.cs), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc:
            raise CalesError(f"cales_create failed ({rc}): {self.L.cales_last_error(None).decode()}")
        self.h = h
        n = (C.c_int32 * 3)(); lo = (C.c_int32 * 3)()
        self.L.cales_local_size(self.h, n, lo)
        self.n = tuple(n); self.lo = tuple(lo)
        self.shape = tuple(x + 2 for x in self.n)

    # -- plumbing
    def _chk(self, rc: int):
        if rc:
            raise CalesError(self.L.cales_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.cales_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def zeros(self) -> np.ndarray:
        return np.zeros(self.shape, order="F", dtype=REAL)

    def set(self, name: str, a: np.ndarray):
        a = _In(a)
        self._chk(self.L.cales_set_field(self.h, capi.FIELDS[name], a.p))

    def get(self, name: str) -> np.ndarray:
        a = self.zeros()
        self._chk(self.L.cales_get_field(self.h, capi.FIELDS[name], _p(a)))
        return a

    # -- parts of a field (include/cales_post.h): this rank's share, Fortran-ordered, without a copy of the whole field
    def read_box(self, name: str, lo, hi, nskip=(1, 1, 1)) -> np.ndarray:
        """cales_read_box: the points lo + m nskip <= hi of field `name`, GLOBAL haloed indices 0 ... ng+1 (box_share tells where a rank's share starts)."""
        a = np.zeros(_box_share(self.cs, lo, hi, nskip)[1], order="F", dtype=REAL)
        self._chk(self.L.cales_read_box(self.h, capi.FIELDS[name], _i3(lo), _i3(hi), _i3(nskip), _p(a), None))
        return a

    def out2d(self, name: str, inorm: int, islice: int) -> np.ndarray:
        """out2d (src/output.f90:164-189): the interior plane of global index `islice` normal to direction `inorm` (1, 2, 3), shape 1 in that direction."""
        ng = [int(x) for x in self.case.ng]
        lo, hi = [1, 1, 1], list(ng)
        if 1 <= int(inorm) <= 3 and 1 <= int(islice) <= ng[int(inorm) - 1]:      # (anything else: the library refuses it below, nothing is read)
            lo[int(inorm) - 1] = hi[int(inorm) - 1] = int(islice)
            a = np.zeros(_box_share(self.cs, lo, hi, (1, 1, 1))[1], order="F", dtype=REAL)
        else:
            a = np.zeros((1, 1, 1), order="F", dtype=REAL)
        self._chk(self.L.cales_out2d(self.h, capi.FIELDS[name], int(inorm), int(islice), _p(a), None))
        return a

    def out3d(self, name: str, nskip) -> np.ndarray:
        """out3d (src/output.f90:191-242): the interior points 1, 1 + nskip, 1 + 2 nskip ... of every direction."""
        a = np.zeros(_box_share(self.cs, (1, 1, 1), [int(x) for x in self.case.ng], nskip)[1], order="F", dtype=REAL)
        self._chk(self.L.cales_out3d(self.h, capi.FIELDS[name], _i3(nskip), _p(a), None))
        return a

    # -- histograms (include/cales_pdf.h): this rank's counts, int64 and Fortran-ordered; the caller adds the ranks
    def pdf_planes(self, name: str, nbins: int, lo: float, hi: float) -> Tuple[np.ndarray, np.ndarray]:
        """cales_pdf_planes: (counts (nbins, n3), outside (2, n3): below, above) of the interior samples of field `name` on every plane, by the bin rule
        of the header: s = nbins / (hi - lo), t = (x - lo) * s, bin int(t) for 0 <= t < nbins."""
        nbins = int(nbins)
        ok = 1 <= nbins <= capi.PDF_MAX_BINS      # (anything else: the library refuses it below, nothing is written)
        counts = np.zeros((nbins if ok else 1, self.n[2]), order="F", dtype=np.int64)
        outside = np.zeros((2, self.n[2]), order="F", dtype=np.int64)
        self._chk(self.L.cales_pdf_planes(self.h, capi.FIELDS[name], nbins, float(lo), float(hi), counts.ctypes.data_as(C.c_void_p), outside.ctypes.data_as(C.c_void_p)))
        return counts, outside

    def jpdf_planes(self, name_a: str, name_b: str, nbins: int, range_a, range_b, kplanes) -> Tuple[np.ndarray, np.ndarray]:
        """cales_jpdf_planes: (counts (nbins, nbins, nplanes), first axis `name_a`; outside (nplanes): either variable outside its range) of the sample
        pairs at the same index on the planes `kplanes` (global k, 1 ... ng(3); any order, repeats allowed)."""
        nbins = int(nbins)
        kp = np.ascontiguousarray([int(k) for k in kplanes], dtype=np.int32)
        ok = 1 <= nbins <= capi.JPDF_MAX_BINS
        counts = np.zeros((nbins, nbins, kp.size) if ok else (1, 1, max(kp.size, 1)), order="F", dtype=np.int64)
        outside = np.zeros(max(kp.size, 1), dtype=np.int64)
        self._chk(self.L.cales_jpdf_planes(self.h, capi.FIELDS[name_a], capi.FIELDS[name_b], nbins, float(range_a[0]), float(range_a[1]), float(range_b[0]), float(range_b[1]),
                                           int(kp.size), kp.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), outside.ctypes.data_as(C.c_void_p)))
        return counts, outside[:kp.size]

    # -- spectra (include/cales_spectra.h): this rank's sums, Fortran-ordered; normalisation is the caller's (cales_amd/spectra.py)
    def spectra_lines(self, name: str, idir: int, lsum: bool = True):
        """cales_spectra_lines: power (nh, n3) = the sum over the lines of plane k of |DFT of the line|^2, nh = n/2 + 1 modes of the lines along x
        (idir = 1, this rank's rows; the caller adds the ranks) or y (idir = 2, one rank only); with lsum also the complex sum of the lines' DFTs,
        (nh, n3) complex. Unnormalised forward transforms of the interior samples (numpy.fft.rfft)."""
        idir = int(idir)
        n = self.n[idir - 1] if idir in (1, 2) else 1      # (anything else: the library refuses it below, nothing is written)
        nh = (n if n <= capi.SPECTRA_MAX_LINE else 0) // 2 + 1
        power = np.zeros((nh, self.n[2]), order="F", dtype=REAL)
        ls = np.zeros((2, nh, self.n[2]), order="F", dtype=REAL) if lsum else None
        self._chk(self.L.cales_spectra_lines(self.h, capi.FIELDS[name], idir, _p(power), _p(ls) if lsum else None))
        if not lsum:
            return power
        return power, np.asfortranarray(ls[0] + 1j * ls[1])

    def spectra_planes(self, name: str, kplanes) -> np.ndarray:
        """cales_spectra_planes (one rank only): power2 (n1/2+1, n2/2+1, nplanes) = |2-D DFT|^2 of the planes `kplanes` (global k, 1 ... ng(3); any
        order, repeats allowed), mode m along x, and along y the two modes ky = q and n2 - q added where they differ."""
        kp = np.ascontiguousarray([int(k) for k in kplanes], dtype=np.int32)
        ok = self.n[0] <= capi.SPECTRA_MAX_LINE and self.n[1] <= capi.SPECTRA_MAX_LINE
        power2 = np.zeros((self.n[0] // 2 + 1, self.n[1] // 2 + 1, max(kp.size, 1)) if ok else (1, 1, 1), order="F", dtype=REAL)
        self._chk(self.L.cales_spectra_planes(self.h, capi.FIELDS[name], int(kp.size), kp.ctypes.data_as(C.c_void_p), _p(power2)))
        return power2

    # -- cross-spectra (include/cales_cospectra.h): this rank's sums, Fortran-ordered and complex; normalisation is the caller's (cales_amd/cospectra.py)
    def cospectra_lines(self, name_a: str, name_b: str, idir: int, lsum: bool = True):
        """cales_cospectra_lines: cross (nh, n3) complex = the sum over the lines of plane k of DFT(a) conj(DFT(b)), the two fields sampled at the same
        index; nh = n/2 + 1 modes of the lines along x (idir = 1, this rank's rows; the caller adds the ranks) or y (idir = 2, one rank only). The real
        part is the co-spectrum, the imaginary part the quadrature spectrum. With lsum also the complex sums of the lines' DFTs of either field,
        (cross, lsum_a, lsum_b), what spectra_lines returns as lsum."""
        idir = int(idir)
        n = self.n[idir - 1] if idir in (1, 2) else 1      # (anything else: the library refuses it below, nothing is written)
        nh = (n if n <= capi.SPECTRA_MAX_LINE else 0) // 2 + 1
        # (a Fortran-ordered complex array IS the (2, ...) array of reals the library writes: real part, imaginary part)
        cross = np.zeros((nh, self.n[2]), order="F", dtype=_COMPLEX)
        la, lb = (np.zeros((nh, self.n[2]), order="F", dtype=_COMPLEX) for _ in range(2)) if lsum else (None, None)
        self._chk(self.L.cales_cospectra_lines(self.h, capi.FIELDS[name_a], capi.FIELDS[name_b], idir, _pc(cross), _pc(la) if lsum else None, _pc(lb) if lsum else None))
        cplx = lambda a: np.asfortranarray(a, dtype=np.complex128)
        return (cplx(cross), cplx(la), cplx(lb)) if lsum else cplx(cross)

    def cospectra_planes(self, name_a: str, name_b: str, kplanes) -> np.ndarray:
        """cales_cospectra_planes (one rank only): cross2 (n1/2+1, n2/2+1, nplanes) complex = 2-D DFT(a) conj(2-D DFT(b)) of the planes `kplanes` (global
        k, 1 ... ng(3); any order, repeats allowed), mode m along x, and along y the two modes ky = q and n2 - q added where they differ."""
        kp = np.ascontiguousarray([int(k) for k in kplanes], dtype=np.int32)
        ok = self.n[0] <= capi.SPECTRA_MAX_LINE and self.n[1] <= capi.SPECTRA_MAX_LINE
        cross2 = np.zeros((self.n[0] // 2 + 1, self.n[1] // 2 + 1, max(kp.size, 1)) if ok else (1, 1, 1), order="F", dtype=_COMPLEX)
        self._chk(self.L.cales_cospectra_planes(self.h, capi.FIELDS[name_a], capi.FIELDS[name_b], int(kp.size), kp.ctypes.data_as(C.c_void_p), _pc(cross2)))
        return np.asfortranarray(cross2, dtype=np.complex128)

    # -- derived fields (include/cales_derived.h): `quantity` a name of capi.DERIVED (or its number); this rank's share, Fortran-ordered, interior cells only
    def derived_box(self, quantity, lo, hi, nskip=(1, 1, 1)) -> np.ndarray:
        """cales_derived_box: the quantity at the points lo + m nskip <= hi, GLOBAL indices 1 ... ng (box_share tells where a rank's share starts)."""
        a = np.zeros(_box_share(self.cs, lo, hi, nskip)[1], order="F", dtype=REAL)
        self._chk(self.L.cales_derived_box(self.h, _derived_id(quantity), _i3(lo), _i3(hi), _i3(nskip), _p(a), None))
        return a

    def derived_out2d(self, quantity, inorm: int, islice: int) -> np.ndarray:
        """cales_derived_out2d: the quantity on the interior plane of global index `islice` normal to direction `inorm` (1, 2, 3), shape 1 in that direction."""
        ng = [int(x) for x in self.case.ng]
        lo, hi = [1, 1, 1], list(ng)
        if 1 <= int(inorm) <= 3 and 1 <= int(islice) <= ng[int(inorm) - 1]:      # (anything else: the library refuses it below, nothing is read)
            lo[int(inorm) - 1] = hi[int(inorm) - 1] = int(islice)
            a = np.zeros(_box_share(self.cs, lo, hi, (1, 1, 1))[1], order="F", dtype=REAL)
        else:
            a = np.zeros((1, 1, 1), order="F", dtype=REAL)
        self._chk(self.L.cales_derived_out2d(self.h, _derived_id(quantity), int(inorm), int(islice), _p(a), None))
        return a

    def derived_out3d(self, quantity, nskip=(1, 1, 1)) -> np.ndarray:
        """cales_derived_out3d: the quantity at the interior points 1, 1 + nskip, 1 + 2 nskip ... of every direction."""
        a = np.zeros(_box_share(self.cs, (1, 1, 1), [int(x) for x in self.case.ng], nskip)[1], order="F", dtype=REAL)
        self._chk(self.L.cales_derived_out3d(self.h, _derived_id(quantity), _i3(nskip), _p(a), None))
        return a

    def derived_to_pp(self, quantity):
        """cales_derived_to_pp: the quantity into the interior of field pp, which it OVERWRITES (ghost cells untouched): read_box, pdf_planes, jpdf_planes,
        spectra_lines ... on "pp" then work on the derived field."""
        self._chk(self.L.cales_derived_to_pp(self.h, _derived_id(quantity)))

    def upload(self, u, v, w, p):
        a = [_In(x) for x in (u, v, w, p)]
        self._chk(self.L.cales_upload_state(self.h, *[x.p for x in a]))

    def download(self):
        out = [self.zeros() for _ in range(5)]
        self._chk(self.L.cales_download_state(self.h, *[_p(a) for a in out]))
        return out

    def bcvel_planes(self, ivel: int):
        n = self.n
        x = np.zeros((n[1] + 2, n[2] + 2, 2), order="F", dtype=REAL); y = np.zeros((n[0] + 2, n[2] + 2, 2), order="F", dtype=REAL)
        z = np.zeros((n[0] + 2, n[1] + 2, 2), order="F", dtype=REAL)
        self._chk(self.L.cales_get_bcvel(self.h, ivel, _p(x), _p(y), _p(z)))
        return x, y, z

    def sync(self):
        self._chk(self.L.cales_sync(self.h))

    # -- operators (reference names)
    def bounduvw(self, is_updt_wm=True, is_correc=False):
        self._chk(self.L.cales_bounduvw(self.h, int(is_updt_wm), int(is_correc)))

    def boundp(self, field="p", which=0):
        self._chk(self.L.cales_boundp(self.h, capi.FIELDS[field], int(which)))

    def mom(self):
        self._chk(self.L.cales_mom(self.h))

    def rk(self, irk: int, dt: float) -> np.ndarray:
        self._chk(self.L.cales_rk(self.h, int(irk), float(dt)))
        f = np.zeros(3, dtype=REAL)
        self._chk(self.L.cales_get_forcing(self.h, _p(f)))
        return f

    def rk_par(self, rkpar, dt: float) -> np.ndarray:
        """rk(rkpar, ..., dt, ..., f) with the caller's coefficients (src/rk.f90:17)"""
        rp = np.ascontiguousarray(rkpar, dtype=REAL); f = np.zeros(3, dtype=REAL)
        self._chk(self.L.cales_rk_par(self.h, _p(rp), float(dt), _p(f)))
        return f

    def bulk_forcing(self):
        self._chk(self.L.cales_bulk_forcing(self.h))

    def bulk_mean(self, field="u", c_or_f="f") -> float:
        m = capi.c_real(0.)
        self._chk(self.L.cales_bulk_mean(self.h, capi.FIELDS[field], 1 if c_or_f == "f" else 0, C.byref(m)))
        return m.value

    def fillps(self, dtrki: float):
        self._chk(self.L.cales_fillps(self.h, float(dtrki)))

    def updt_rhs_b(self):
        self._chk(self.L.cales_updt_rhs_b(self.h))

    def solver(self):
        self._chk(self.L.cales_solver(self.h))

    def helmholtz_z(self, ivel: int, alpha: float):
        self._chk(self.L.cales_helmholtz_z(self.h, int(ivel), float(alpha)))

    def helmholtz(self, ivel: int, alpha: float):
        """3-D implicit diffusion of one velocity component (impdiff = 1; main.f90:423-491)."""
        self._chk(self.L.cales_helmholtz(self.h, int(ivel), float(alpha)))

    def correc(self, dtrk: float):
        self._chk(self.L.cales_correc(self.h, float(dtrk)))

    def updatep(self, alpha: float = 0.):
        self._chk(self.L.cales_updatep(self.h, float(alpha)))

    def cmpt_sgs(self):
        self._chk(self.L.cales_cmpt_sgs(self.h))

    def chkdt(self) -> float:
        d = capi.c_real(0.)
        self._chk(self.L.cales_chkdt(self.h, C.byref(d)))
        return d.value

    def chkdiv(self) -> Tuple[float, float]:
        a, b = capi.c_real(0.), capi.c_real(0.)
        self._chk(self.L.cales_chkdiv(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stats_chan(self) -> np.ndarray:
        """First block of out1d_single_point_chan (src/output.f90:509-700): 27 plane statistics per z plane, shape (27, n3)."""
        buf = np.zeros((27, self.n[2]), order="F", dtype=REAL)
        self._chk(self.L.cales_out1d_single_point_chan(self.h, _p(buf)))
        return buf

    def out1d(self, field: str, idir: int, use_dzc: bool = False) -> np.ndarray:
        """out1d (src/output.f90:50-163): profile of `field` along idir averaged over the other two directions (this rank's sums)."""
        buf = np.zeros(self.n[idir - 1], dtype=capi.np_real)
        self._chk(self.L.cales_out1d(self.h, capi.FIELDS[field], int(idir), int(use_dzc), _p(buf)))
        return buf

    def out1d_chan(self) -> np.ndarray:
        """out1d_chan (src/output.f90:317-405): (7, n3) um, vm, wm, u2, v2, w2, uw per plane."""
        buf = np.zeros((7, self.n[2]), dtype=capi.np_real, order="F")
        self._chk(self.L.cales_out1d_chan(self.h, _p(buf)))
        return buf

    def out2d_duct(self) -> np.ndarray:
        """out2d_duct (src/output.f90:406-507): (9, n2, n3) um, vm, wm, u2, v2, w2, uv, uw, vw at the cell centres of every (j, k)."""
        buf = np.zeros((9, self.n[1], self.n[2]), dtype=capi.np_real, order="F")
        self._chk(self.L.cales_out2d_duct(self.h, _p(buf)))
        return buf

    def stats_chan_budgets(self):
        """Second and third block of out1d_single_point_chan (src/output.f90:700-1055): (38, n3) budget sums and (6, n3) divergence measures."""
        b = np.zeros((38, self.n[2]), order="F", dtype=REAL); l = np.zeros((6, self.n[2]), order="F", dtype=REAL)
        self._chk(self.L.cales_out1d_chan_budgets(self.h, _p(b), _p(l)))
        return b, l

    def step(self, dt: float):
        """Three RK substeps, src/main.f90:417-508, queued without host synchronisation."""
        self._chk(self.L.cales_step(self.h, float(dt)))

    def dpdl(self) -> np.ndarray:
        d = np.zeros(3, dtype=REAL)
        self._chk(self.L.cales_get_dpdl(self.h, _p(d)))
        return d

    def startup(self):
        """src/main.f90:370-375: ghost cells and eddy viscosity of the initial state."""
        self.bounduvw(True, False); self.boundp("p", 0); self.cmpt_sgs(); self.boundp("visct", 1)

    def describe_plan(self) -> Dict[str, str]:
        """The path the next cales_step takes (struct StepPlan): {'projection': 'in_strain_rate_pass', 'fillps': 'in_x_transform', ...}."""
        buf = C.create_string_buffer(2048)
        rc = self.L.cales_describe_plan(self.h, buf, 2048)
        if rc not in (0, 2):
            self._chk(rc)
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if "=" in kv)

    def calibrate(self, reps: int = 3) -> Dict[str, float]:
        """Read-only / write-only / copy streams over this context's own fields (cales_calibrate): GB/s on THIS box."""
        g = np.zeros(3, dtype=REAL); nb = C.c_int64(0)
        self._chk(self.L.cales_calibrate(self.h, int(reps), _p(g), C.byref(nb)))
        return {"read_GBps": float(g[0]), "write_GBps": float(g[1]), "copy_GBps": float(g[2]), "bytes_per_stream": int(nb.value), "launches": int(reps)}

    # -- measurement
    def profile(self, on: bool):
        self._chk(self.L.cales_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._chk(self.L.cales_profile_reset(self.h))

    def profile_stats(self) -> Dict[str, Tuple[int, float]]:
        out = {}
        for i in range(self.L.cales_profile_count(self.h)):
            name = C.create_string_buffer(64); calls = C.c_int64(0); ms = capi.c_real(0.)
            self.L.cales_profile_get(self.h, i, name, 64, C.byref(calls), C.byref(ms))
            out[name.value.decode()] = (calls.value, ms.value)
        return out

    def memory_in_use(self) -> Tuple[int, int]:
        """(bytes, allocations) this context holds on the device and in pinned host memory right now (cales_memory_in_use)."""
        return memory_in_use(self.h)

    def device_info(self) -> Tuple[str, int]:
        name = C.create_string_buffer(128); b = C.c_int64(0)
        self._chk(self.L.cales_device_info(self.h, name, 128, C.byref(b)))
        return name.value.decode(), b.value

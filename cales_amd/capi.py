"""ctypes binding of libcales_hip.so (C-ABI declared in include/cales.h, include/cales_post.h, include/cales_pdf.h, include/cales_spectra.h, include/cales_cospectra.h and
include/cales_derived.h).

There is no CPU fallback: if the HIP library has not been built, importing the symbols raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# Working precision rp of the reference (src/precision.f90:11-20), a build-time choice there (-D_SINGLE_PRECISION) and a process-wide one
# here: CALES_PRECISION=single loads libcales_hip_sp.so (the same sources built with -DCALES_SINGLE), and every real of the C-ABI --
# fields, case parameters, scalars -- is a float.
PRECISION = os.environ.get("CALES_PRECISION", "double")
if PRECISION not in ("double", "single"):
    raise ValueError("CALES_PRECISION must be 'double' or 'single'")
SINGLE = PRECISION == "single"
c_real = C.c_float if SINGLE else C.c_double
np_real = np.float32 if SINGLE else np.float64
LIB_PATH = os.environ.get("CALES_LIB", os.path.join(_HERE, "libcales_hip_sp.so" if SINGLE else "libcales_hip.so"))   # CALES_LIB: tuning builds only

SGS = {"none": 0, "smag": 1, "dsmag": 2}
SGS_DSMAG_FILTER2D = 3      # CALES_SGS_DSMAG_FILTER2D of include/cales.h: 'dsmag' of a -D_FILTER_2D build of the reference


def filter2d_env() -> bool:
    """CALES_FILTER_2D, the run-time form of the reference's -D_FILTER_2D: set to anything but the empty string or 0."""
    return os.environ.get("CALES_FILTER_2D", "0") not in ("", "0")

# enum cales_sgs_average of include/cales.h, OR-ed onto the two dynamic values: the directions the Germano identity is averaged over (sgs.f90:359-370)
SGS_AVE = {"planes": 0, "volume": 4, "xlines": 8, "local": 64}      # the reference's hard-wired _CHANNEL | -D_DIT | _DUCT without _CHANNEL | _CAVITY without it (CALES_SGS_AVE_LOCAL)


def dsmag_average_env() -> str:
    """CALES_DSMAG_AVERAGE, the run-time form of the reference's _DIT / _CHANNEL / _DUCT / _CAVITY: planes (also unset or empty), volume, xlines or local."""
    return os.environ.get("CALES_DSMAG_AVERAGE", "") or "planes"


FIELDS = dict(u=0, v=1, w=2, p=3, pp=4, visct=5, dudt=6, dvdt=7, dwdt=8, dudto=9, dvdto=10, dwdto=11,
              dudtd=12, dvdtd=13, dwdtd=14)

# every symbol include/cales.h declares (tests/test_capi_symbols.py checks the list against the header)
SYMBOLS = ["cales_real_size", "cales_initgrid", "cales_initflow", "cales_check_case", "cales_create", "cales_destroy", "cales_last_error",
           "cales_sync", "cales_local_size", "cales_upload_state", "cales_download_state", "cales_set_field",
           "cales_get_field", "cales_get_bcvel", "cales_bounduvw", "cales_boundp", "cales_mom", "cales_rk",
           "cales_bulk_forcing", "cales_get_forcing", "cales_bulk_mean", "cales_fillps", "cales_updt_rhs_b",
           "cales_solver", "cales_helmholtz_z", "cales_helmholtz", "cales_correc", "cales_updatep", "cales_cmpt_sgs", "cales_chkdt",
           "cales_chkdiv", "cales_out1d_single_point_chan", "cales_out1d_chan_budgets", "cales_out1d", "cales_out1d_chan", "cales_out2d_duct", "cales_step", "cales_get_dpdl", "cales_profile_enable", "cales_profile_reset",
           "cales_profile_count", "cales_profile_get", "cales_device_info", "cales_comm_buffer_doubles", "cales_set_comm",
           "cales_initflow_slab", "cales_comm_unique_id", "cales_comm_init_rccl", "cales_comm_selftest",
           "cales_device_count", "cales_set_device", "cales_set_comm_overlap", "cales_rk_par", "cales_describe_plan", "cales_calibrate", "cales_memory_in_use"]

# every symbol include/cales_post.h declares, the output side of the C-ABI (planes, boxes and strided samples of a field read from the device); a list of
# its own, as the header is a header of its own (tests/test_box_reads_host.py checks it against that header)
POST_SYMBOLS = ["cales_box_share", "cales_read_box", "cales_out2d", "cales_out3d"]

# every symbol include/cales_pdf.h declares: per-plane histograms of a field and joint histograms of two fields, binned on the device; again a list of
# its own beside a header of its own (tests/test_pdf_host.py checks it against that header)
PDF_SYMBOLS = ["cales_pdf_planes", "cales_jpdf_planes"]
PDF_MAX_BINS, JPDF_MAX_BINS = 4096, 128      # CALES_PDF_MAX_BINS, CALES_JPDF_MAX_BINS

# every symbol include/cales_spectra.h declares: power spectra of a field along x, along y and in x-y planes, transformed on the device; once more a
# list of its own beside a header of its own (tests/test_spectra_host.py checks it against that header)
SPECTRA_SYMBOLS = ["cales_spectra_lines", "cales_spectra_planes"]
SPECTRA_MAX_LINE = 2048      # CALES_SPECTRA_MAX_LINE

# every symbol include/cales_cospectra.h declares: cross-spectra of two fields sampled at the same index, along x, along y and in x-y planes; a sixth
# list beside a sixth header (tests/test_cospectra_host.py checks it against that header)
COSPECTRA_SYMBOLS = ["cales_cospectra_lines", "cales_cospectra_planes"]

# every symbol include/cales_derived.h declares: vorticity, SijSij, WijWij and Q of the stored velocity (the reference's src/post.f90), formed on the device;
# a fifth list beside a fifth header (tests/test_derived_host.py checks it against that header)
DERIVED_SYMBOLS = ["cales_derived_box", "cales_derived_out2d", "cales_derived_out3d", "cales_derived_to_pp"]
DERIVED = dict(vox=0, voy=1, voz=2, str=3, ens=4, qcr=5, vox_edge=6, voy_edge=7, voz_edge=8)      # enum cales_derived


class CalesCase(C.Structure):
    """struct cales_case of include/cales.h."""
    _fields_ = [("ng", C.c_int32 * 3), ("l", c_real * 3), ("gtype", C.c_int32), ("gr", c_real),
                ("visci", c_real), ("cbcvel", C.c_char * 18), ("cbcpre", C.c_char * 6), ("cbcsgs", C.c_char * 6),
                ("bcvel", c_real * 18), ("bcpre", c_real * 6), ("bcsgs", c_real * 6),
                ("bforce", c_real * 3), ("is_forced", C.c_int32 * 3), ("velf", c_real * 3),
                ("sgstype", C.c_int32), ("lwm", C.c_int32 * 6), ("hwm", c_real), ("impdiff", C.c_int32),
                ("nranks", C.c_int32), ("rank", C.c_int32)]


def _chars(a) -> bytes:
    return "".join(np.asarray(a).ravel(order="F").tolist()).encode()


def make_case(case, nranks: int = 1, rank: int = 0) -> CalesCase:
    """cales_amd.nml.Case -> struct cales_case (Fortran storage order kept)."""
    p = CalesCase()
    p.ng[:] = [int(x) for x in case.ng]
    p.l[:] = [float(x) for x in case.l]
    p.gtype, p.gr, p.visci = int(case.gtype), float(case.gr), float(case.visci)
    p.cbcvel, p.cbcpre, p.cbcsgs = _chars(case.cbcvel), _chars(case.cbcpre), _chars(case.cbcsgs)
    p.bcvel[:] = case.bcvel.ravel(order="F").tolist()
    p.bcpre[:] = case.bcpre.ravel(order="F").tolist()
    p.bcsgs[:] = case.bcsgs.ravel(order="F").tolist()
    p.bforce[:] = case.bforce.tolist()
    p.is_forced[:] = [int(x) for x in case.is_forced]
    p.velf[:] = case.velf.tolist()
    if case.sgstype not in SGS:
        raise ValueError("ERROR: unknown SGS model" if case.sgstype != "amd" else "ERROR: AMD model not yet implemented")
    p.sgstype = SGS[case.sgstype]
    f2d = getattr(case, "filter2d", None)
    if case.sgstype == "dsmag" and (filter2d_env() if f2d is None else f2d):      # (the reference ignores the flag for 'none' and 'smag')
        p.sgstype = SGS_DSMAG_FILTER2D
    if case.sgstype == "dsmag":      # (likewise ignored for 'none' and 'smag')
        ave = getattr(case, "dsmag_average", None)
        ave = dsmag_average_env() if ave is None else ave
        if ave not in SGS_AVE:
            raise ValueError(f"ERROR: unknown averaging of the dynamic model {ave!r} (planes, volume, xlines or local)")
        p.sgstype |= SGS_AVE[ave]
    p.lwm[:] = [int(x) for x in case.lwm.ravel(order="F")]
    p.hwm = float(case.hwm)
    p.impdiff = int(case.impdiff)
    p.nranks, p.rank = int(nranks), int(rank)
    return p


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(make -C cales_amd/csrc). The CaLES hot path has no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own HIP/HSA runtime under the same soname (libamdhip64.so.7). A process
        # must hold ONE runtime: whichever is loaded first wins, and torch cannot initialise on top of the system
        # copy. So torch (when installed) is imported before libcales_hip.so is opened; set CALES_NO_TORCH=1 for a
        # torch-free process (e.g. alongside the Fortran driver).
        if os.environ.get("CALES_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        L.cales_real_size.restype = C.c_int; L.cales_real_size.argtypes = []
        if L.cales_real_size() != C.sizeof(c_real):
            raise RuntimeError(f"{LIB_PATH} is built for {8 * L.cales_real_size()}-bit reals, CALES_PRECISION={PRECISION}")
        L.cales_last_error.restype = C.c_char_p
        L.cales_last_error.argtypes = [C.c_void_p]
        L.cales_create.argtypes = [C.POINTER(CalesCase), C.c_void_p, C.POINTER(C.c_void_p)]
        dp = C.c_void_p
        for name, args in {
            "cales_destroy": [C.c_void_p], "cales_sync": [C.c_void_p], "cales_local_size": [C.c_void_p, dp, dp],
            "cales_upload_state": [C.c_void_p, dp, dp, dp, dp], "cales_download_state": [C.c_void_p, dp, dp, dp, dp, dp],
            "cales_set_field": [C.c_void_p, C.c_int, dp], "cales_get_field": [C.c_void_p, C.c_int, dp],
            "cales_get_bcvel": [C.c_void_p, C.c_int, dp, dp, dp],
            "cales_bounduvw": [C.c_void_p, C.c_int, C.c_int], "cales_boundp": [C.c_void_p, C.c_int, C.c_int],
            "cales_mom": [C.c_void_p], "cales_rk": [C.c_void_p, C.c_int, c_real], "cales_bulk_forcing": [C.c_void_p],
            "cales_get_forcing": [C.c_void_p, dp], "cales_bulk_mean": [C.c_void_p, C.c_int, C.c_int, dp],
            "cales_fillps": [C.c_void_p, c_real], "cales_updt_rhs_b": [C.c_void_p], "cales_solver": [C.c_void_p],
            "cales_helmholtz_z": [C.c_void_p, C.c_int, c_real], "cales_helmholtz": [C.c_void_p, C.c_int, c_real], "cales_correc": [C.c_void_p, c_real],
            "cales_updatep": [C.c_void_p, c_real], "cales_cmpt_sgs": [C.c_void_p], "cales_chkdt": [C.c_void_p, dp],
            "cales_chkdiv": [C.c_void_p, dp, dp], "cales_out1d_single_point_chan": [C.c_void_p, C.c_void_p], "cales_out1d_chan_budgets": [C.c_void_p, C.c_void_p, C.c_void_p], "cales_out1d": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p], "cales_out1d_chan": [C.c_void_p, C.c_void_p], "cales_out2d_duct": [C.c_void_p, C.c_void_p], "cales_step": [C.c_void_p, c_real], "cales_get_dpdl": [C.c_void_p, dp],
            "cales_profile_enable": [C.c_void_p, C.c_int], "cales_profile_reset": [C.c_void_p],
            "cales_profile_count": [C.c_void_p], "cales_profile_get": [C.c_void_p, C.c_int, C.c_char_p, C.c_int, dp, dp],
            "cales_device_info": [C.c_void_p, C.c_char_p, C.c_int, dp],
            "cales_initgrid": [C.c_int, C.c_int, c_real, c_real, dp, dp, dp, dp],
            "cales_initflow": [C.POINTER(CalesCase), C.c_char_p, C.c_int, dp, dp, dp, dp],
            "cales_check_case": [C.POINTER(CalesCase), C.c_char_p, C.c_int],
            "cales_comm_buffer_doubles": [C.c_void_p, dp],
            "cales_set_comm": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64],
            "cales_initflow_slab": [C.POINTER(CalesCase), C.c_char_p, C.c_int, dp, dp, dp, dp],
            "cales_comm_unique_id": [C.c_void_p], "cales_comm_init_rccl": [C.c_void_p, C.c_void_p], "cales_comm_selftest": [],
            "cales_device_count": [C.POINTER(C.c_int)], "cales_set_device": [C.c_int],
            "cales_set_comm_overlap": [C.c_void_p, C.c_void_p, C.c_void_p],
            "cales_rk_par": [C.c_void_p, dp, c_real, dp],
            "cales_describe_plan": [C.c_void_p, C.c_char_p, C.c_int], "cales_calibrate": [C.c_void_p, C.c_int, dp, dp],
            "cales_memory_in_use": [C.c_void_p, dp, dp],
        }.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = None if name == "cales_destroy" else C.c_int
        for name, args in {      # include/cales_post.h (POST_SYMBOLS)
            "cales_box_share": [C.POINTER(CalesCase), dp, dp, dp, dp, dp],
            "cales_read_box": [C.c_void_p, C.c_int, dp, dp, dp, dp, dp],
            "cales_out2d": [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp],
            "cales_out3d": [C.c_void_p, C.c_int, dp, dp, dp],
        }.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        for name, args in {      # include/cales_pdf.h (PDF_SYMBOLS)
            "cales_pdf_planes": [C.c_void_p, C.c_int, C.c_int, c_real, c_real, dp, dp],
            "cales_jpdf_planes": [C.c_void_p, C.c_int, C.c_int, C.c_int, c_real, c_real, c_real, c_real, C.c_int, dp, dp, dp],
        }.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        for name, args in {      # include/cales_spectra.h (SPECTRA_SYMBOLS)
            "cales_spectra_lines": [C.c_void_p, C.c_int, C.c_int, dp, dp],
            "cales_spectra_planes": [C.c_void_p, C.c_int, C.c_int, dp, dp],
        }.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        for name, args in {      # include/cales_cospectra.h (COSPECTRA_SYMBOLS)
            "cales_cospectra_lines": [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, dp],
            "cales_cospectra_planes": [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp],
        }.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        for name, args in {      # include/cales_derived.h (DERIVED_SYMBOLS)
            "cales_derived_box": [C.c_void_p, C.c_int, dp, dp, dp, dp, dp],
            "cales_derived_out2d": [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp],
            "cales_derived_out3d": [C.c_void_p, C.c_int, dp, dp, dp],
            "cales_derived_to_pp": [C.c_void_p, C.c_int],
        }.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        _lib = L
    return _lib

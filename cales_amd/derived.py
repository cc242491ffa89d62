"""Vorticity, Q-criterion, SijSij and WijWij as the visualisation files of the reference's write_visu_3d (src/output.f90:274-287).

A case of the reference pastes utils/useful_fortran_blocks/vorticity-inc.f90 and q-criterion-inc.f90 into its out3d.h90 to write, per saved step NNNNNNN,

  vox_fld_NNNNNNN.bin, qcr_fld_NNNNNNN.bin ...   raw reals, Fortran order, the interior points 1, 1 + nskip, ... of every direction
  log_visu_3d.out                                 one line per file, '(A30,A15,9I5,E16.7E3,I7)': file, variable, nmin, nmax, nskip, time, istep

(utils/visualize_fields/gen_xdmf_easy reads the log). There the quantities come from src/post.f90 on the host side of the solver; here from the device
(HotPath.derived_out3d, include/cales_derived.h), one strided sample per quantity, never a whole velocity field. The reference block writes all three vorticity
components under vox_fld_: a slip there; voy_fld_ and voz_fld_ are used here."""
from __future__ import annotations

import os
from typing import Sequence

import numpy as np

from . import capi

# quantity (a name of capi.DERIVED) -> the variable name of the log line
VARNAMES = dict(vox="Vorticity_X", voy="Vorticity_Y", voz="Vorticity_Z", qcr="Q-criterion", str="SijSij", ens="WijWij")
LOG = "log_visu_3d.out"


def _e16_7e3(x: float) -> str:
    """Fortran's E16.7E3: 0.ddddddd x 10^e, seven digits, a three-digit exponent, right-justified in 16 columns"""
    x = float(x)
    if x == 0.:
        body = "0.0000000E+000"
    else:
        mant, ex = f"{abs(x):.6e}".split("e")      # d.dddddd e+-xx, rounded to seven significant digits
        e = int(ex) + 1
        body = ("-" if x < 0. else "") + "0." + mant.replace(".", "") + "E" + ("-" if e < 0 else "+") + f"{abs(e):03d}"
    return body.rjust(16)


def log_line(fname_fld: str, varname: str, nmin, nmax, nskip, time: float, istep: int) -> str:
    """write_log_output (src/output.f90:244-272): a string shorter than its A field is right-justified, a longer one cut"""
    ints = "".join(f"{int(v):5d}" for v in (*nmin, *nmax, *nskip))
    return fname_fld[:30].rjust(30) + varname[:15].rjust(15) + ints + _e16_7e3(time) + f"{int(istep):7d}"


def write_visu_3d(h, datadir: str, istep: int, time: float, names: Sequence[str] = ("vox", "voy", "voz", "qcr"), nskip=(1, 1, 1)) -> None:
    """The files <name>_fld_NNNNNNN.bin of step `istep` and their lines of log_visu_3d.out. `h`: a HotPath, or one rank's SlabHotPath -- every rank calls
    this; a rank writes its rows into the shared file, the first rank appends the log lines."""
    from .hotpath import _box_share
    ng = [int(x) for x in h.case.ng]
    ns = [int(x) for x in nskip]
    for name in names:
        if name not in VARNAMES:
            raise ValueError(f"unknown derived quantity {name!r} ({', '.join(VARNAMES)})")
    first, count = _box_share(h.cs, (1, 1, 1), ng, ns)
    rows = (ng[1] - 1) // ns[1] + 1      # rows of the file; this rank's start at row (first[1] - 1) / nskip
    j0 = (first[1] - 1) // ns[1]
    rank = int(h.cs.rank)
    for name in names:
        a = h.derived_out3d(name, ns)
        fbin = f"{name}_fld_{int(istep):07d}.bin"
        path = os.path.join(datadir, fbin)
        if count[1] == rows:
            a.ravel(order="F").tofile(path)
        elif count[1] > 0:
            size = count[0] * rows * count[2]
            with open(path, "r+b" if os.path.exists(path) else "w+b") as f:
                f.truncate(size * a.itemsize)
                out = np.memmap(f, dtype=a.dtype, mode="r+", shape=(count[0], rows, count[2]), order="F")
                out[:, j0:j0 + count[1], :] = a
                out.flush()
        if rank == 0:
            with open(os.path.join(datadir, LOG), "a") as f:
                f.write(log_line(fbin, VARNAMES[name], (1, 1, 1), ng, ns, time, istep) + "\n")


assert set(VARNAMES) <= set(capi.DERIVED)

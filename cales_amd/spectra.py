"""1-D and 2-D power spectra of u, v, w and p, in the files the reference's utils/spectra-stats.py time-averages.

That script reads, per saved step NNNNNNN of the data directory and for V in u, v, w, p,

  spectra_V_fld_NNNNNNN_1d_x.bin     float64, two blocks of (n1/2+1, nz) in Fortran order: "x0", then "xs"
  spectra_V_fld_NNNNNNN_1d_y.bin     float64, two blocks of (n2/2+1, nz): "y0", then "ys"
  spectra_V_fld_NNNNNNN_2d.bin       float64 (n1/2+1, n2/2+1, nplanes)
  spectra_V_fld_NNNNNNN_kplanes.out  one row per plane: kplane zc(kplane)

No routine of the reference's src/ writes these files. Here the sums come from the device (HotPath.spectra_lines / spectra_planes,
include/cales_spectra.h: unnormalised forward DFTs of the interior samples, no mean removed) and are normalised on the host:

  x0 = 2 power / (n1 n2), power(m, k) = sum_j |F_jk(m)|^2. The consumer's own normalisation: its compute_scales takes irfft(x0, axis=0) / 2 for the
       autocorrelation along x at zero y separation and the first entry of that for the variance -- with this factor it is the plane mean of f^2.
  xs = 2 |lsum / n2|^2 / n1, lsum(m, k) = sum_j F_jk(m): the spectrum of the y-averaged line, normalised like x0 of a single line. The consumer reads
       this block and only averages and saves it; it never says what "xs" is. This is this project's reading of it.
  y0, ys: the same with x and y exchanged.
  2d = power2 / (n1 n2)^2, power2(m, q, p) = |H_k(m, q)|^2 + |H_k(m, n2 - q)|^2 (one term where the two modes are the same). The consumer only averages
       this file, so the normalisation is ours: sum_{m,q} w_m 2d(m, q) is the plane mean of f^2, with w_m = 1 for m = 0 and for m = n1/2 when n1 is
       even, and 2 otherwise.

`collect` gathers one rank's sums, `add_ranks` adds the x parts of several ranks, `write` normalises and writes the files and `read` reads them back.
The y and 2-D parts need whole y lines: one rank only, and `collect` on several ranks gathers x only."""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import numpy as np

VARS = ("u", "v", "w", "p")
NV = len(VARS)


def collect(h, kplanes: Sequence[int]) -> Dict[str, object]:
    """This rank's sums of the four variables: power_x (n1/2+1, nz, 4) and lsum_x (complex, same shape) of the rank's rows; on one rank also
    power_y, lsum_y (n2/2+1, nz, 4) and power2 (n1/2+1, n2/2+1, nplanes, 4) on the planes `kplanes` (global k, 1 ... ng(3)); None on several ranks.
    All float64 / complex128."""
    kp = [int(k) for k in kplanes]
    ng = [int(x) for x in h.case.ng]
    one = int(h.cs.nranks) == 1
    nz, nhx, nhy = h.n[2], ng[0] // 2 + 1, ng[1] // 2 + 1
    out = dict(n1=ng[0], n2=ng[1], kplanes=np.asarray(kp, dtype=np.int64),
               power_x=np.zeros((nhx, nz, NV), order="F"), lsum_x=np.zeros((nhx, nz, NV), order="F", dtype=np.complex128),
               power_y=np.zeros((nhy, nz, NV), order="F") if one else None, lsum_y=np.zeros((nhy, nz, NV), order="F", dtype=np.complex128) if one else None,
               power2=np.zeros((nhx, nhy, len(kp), NV), order="F") if one else None)
    for a, name in enumerate(VARS):
        out["power_x"][:, :, a], out["lsum_x"][:, :, a] = h.spectra_lines(name, 1)
        if one:
            out["power_y"][:, :, a], out["lsum_y"][:, :, a] = h.spectra_lines(name, 2)
            out["power2"][:, :, :, a] = h.spectra_planes(name, kp)
    return out


def add_ranks(parts: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """The x sums of several ranks (each what `collect` returned there) added up; the y and 2-D parts are those of the first part (None on several ranks)."""
    out = dict(parts[0])
    for key in ("power_x", "lsum_x"):
        out[key] = np.asfortranarray(sum(p[key] for p in parts))
    return out


def normalise(collected: Dict[str, object]) -> Dict[str, Optional[np.ndarray]]:
    """x0, xs (n1/2+1, nz, 4); y0, ys (n2/2+1, nz, 4); s2 (n1/2+1, n2/2+1, nplanes, 4) as the module docstring defines them; None where not collected"""
    c = collected
    n1, n2 = int(c["n1"]), int(c["n2"])
    out = dict(x0=2. * c["power_x"] / (n1 * n2), xs=2. * np.abs(c["lsum_x"] / n2) ** 2 / n1, y0=None, ys=None, s2=None)
    if c["power_y"] is not None:
        out.update(y0=2. * c["power_y"] / (n1 * n2), ys=2. * np.abs(c["lsum_y"] / n1) ** 2 / n2, s2=c["power2"] / float(n1 * n2) ** 2)
    return out


def _names(datadir: str, fldnum: int, var: str):
    stem = os.path.join(datadir, f"spectra_{var}_fld_{int(fldnum):07d}")
    return stem + "_1d_x.bin", stem + "_1d_y.bin", stem + "_2d.bin", stem + "_kplanes.out"


def _blocks(a, b) -> np.ndarray:
    return np.concatenate([np.asfortranarray(a, dtype=np.float64).ravel(order="F"), np.asfortranarray(b, dtype=np.float64).ravel(order="F")])


def write(datadir: str, fldnum: int, collected: Dict[str, object], zc) -> None:
    """The files of step `fldnum` for u, v, w, p; the y, 2-D and plane files only where they were collected (one rank). zc: heights of the cell centres,
    haloed (0 ... nz+1, what initgrid returns) or interior (nz values)."""
    s = normalise(collected)
    nz = s["x0"].shape[1]
    zc = np.asarray(zc, dtype=np.float64)
    if zc.size not in (nz, nz + 2):
        raise ValueError("zc must hold nz or nz + 2 values")
    zk = lambda k: zc[k] if zc.size == nz + 2 else zc[k - 1]
    for a, var in enumerate(VARS):
        f_x, f_y, f_2d, f_k = _names(datadir, fldnum, var)
        _blocks(s["x0"][:, :, a], s["xs"][:, :, a]).tofile(f_x)
        if s["y0"] is None:
            continue
        _blocks(s["y0"][:, :, a], s["ys"][:, :, a]).tofile(f_y)
        np.asfortranarray(s["s2"][:, :, :, a], dtype=np.float64).ravel(order="F").tofile(f_2d)
        with open(f_k, "w") as f:
            for k in collected["kplanes"]:
                f.write(f"{int(k)} {float(zk(int(k))):.17e}\n")


def read(datadir: str, fldnum: int, n1: int, n2: int) -> Dict[str, np.ndarray]:
    """What `write` wrote on one rank, for a grid of n1 x n2 points per plane: x0, xs (n1/2+1, nz, 4), y0, ys (n2/2+1, nz, 4), s2 (n1/2+1, n2/2+1,
    nplanes, 4), kplanes and zc (nplanes)."""
    nhx, nhy = int(n1) // 2 + 1, int(n2) // 2 + 1
    per = {k: [] for k in ("x0", "xs", "y0", "ys", "s2")}
    for var in VARS:
        f_x, f_y, f_2d, f_k = _names(datadir, fldnum, var)
        meta = np.atleast_2d(np.loadtxt(f_k))
        rx, ry = np.fromfile(f_x, dtype=np.float64), np.fromfile(f_y, dtype=np.float64)
        nz = rx.size // (2 * nhx)
        if rx.size != 2 * nhx * nz or ry.size != 2 * nhy * nz:
            raise ValueError(f"{f_x} / {f_y}: not two blocks of (n/2+1, nz)")
        per["x0"].append(rx[:nhx * nz].reshape((nhx, nz), order="F")); per["xs"].append(rx[nhx * nz:].reshape((nhx, nz), order="F"))
        per["y0"].append(ry[:nhy * nz].reshape((nhy, nz), order="F")); per["ys"].append(ry[nhy * nz:].reshape((nhy, nz), order="F"))
        per["s2"].append(np.fromfile(f_2d, dtype=np.float64).reshape((nhx, nhy, meta.shape[0]), order="F"))
    out = {k: np.asfortranarray(np.stack(v, axis=-1)) for k, v in per.items()}
    out.update(kplanes=meta[:, 0].astype(np.int64), zc=meta[:, 1].copy())
    return out

"""1-D and 2-D cross-spectra of pairs of fields, in files laid out like those of cales_amd/spectra.py.

Per saved step NNNNNNN of the data directory and for a pair AB of fields (uw, uv, vw, pu, pw by default),

  cospectra_AB_fld_NNNNNNN_1d_x.bin     float64, two blocks of (n1/2+1, nz) in Fortran order: real part (co-spectrum), then imaginary part (quadrature)
  cospectra_AB_fld_NNNNNNN_1d_y.bin     float64, two blocks of (n2/2+1, nz): real part, then imaginary part
  cospectra_AB_fld_NNNNNNN_2d.bin       float64, two blocks of (n1/2+1, n2/2+1, nplanes): real part, then imaginary part
  cospectra_AB_fld_NNNNNNN_kplanes.out  one row per plane: kplane zc(kplane)

No script of the reference's utils/ reads such files (its spectra-stats.py averages power spectra only), so layout and normalisation are this project's,
chosen to match spectra.py. The sums come from the device (HotPath.cospectra_lines / cospectra_planes, include/cales_cospectra.h: unnormalised forward
DFTs of the interior samples of both fields AT THE SAME INDEX, no mean removed) and are normalised on the host:

  x = 2 cross / (n1 n2), cross(m, k) = sum_j F^a_jk(m) conj(F^b_jk(m)): the normalisation of spectra.py's x0, so that irfft(x, n1, axis=0)[0] / 2 is the
      plane mean of a b, and irfft(x) / 2 the cross-correlation along x at zero y separation.
  y: the same with x and y exchanged.
  2d = cross2 / (n1 n2)^2, cross2(m, q, p) = H^a conj(H^b) at (m, q) plus the same at (m, n2 - q) (one term where the two modes are the same):
      sum_{m,q} w_m Re 2d(m, q) is the plane mean of a b, with w_m = 1 for m = 0 and for m = n1/2 when n1 is even, and 2 otherwise.

The line sums of either field (lsum_a, lsum_b, what spectra.py turns into "xs") are collected too: with them the plane means can be taken out of mode 0
afterwards, cross(0, k) - lsum_a(0, k) conj(lsum_b(0, k)) / n2 for the x lines.

STAGGERING. The samples are the stored values: u sits on the x face of its cell, v on the y face, w on the z face, p and the eddy viscosity at the
centre. Two fields that are half a cell apart along the direction of the transform carry a phase exp(I pi m (s_a - s_b) / n) in their cross-spectrum;
`stagger_phase` returns its inverse, and cross * stagger_phase(...) is the cross-spectrum of the two band-limited signals at a common point. Nothing is
corrected in the files. Staggering along z (w against anything at a cell centre in z) cannot be corrected by a phase in x or y and is left alone: such
pairs compare w at the upper face with the other field half a cell below.

`collect` gathers one rank's sums, `add_ranks` adds the x parts of several ranks, `write` normalises and writes the files and `read` reads them back.
The y and 2-D parts need whole y lines: one rank only, and `collect` on several ranks gathers x only."""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

PAIRS = (("u", "w"), ("u", "v"), ("v", "w"), ("p", "u"), ("p", "w"))
_FACE = {"u": 1, "v": 2, "w": 3, "dudt": 1, "dvdt": 2, "dwdt": 3, "dudto": 1, "dvdto": 2, "dwdto": 3, "dudtd": 1, "dvdtd": 2, "dwdtd": 3}      # direction of the face a field sits on


def stagger_phase(name_a: str, name_b: str, idir: int, n: int) -> np.ndarray:
    """exp(-I pi m (s_a - s_b) / n) for m = 0 ... n/2 (1 at m = n/2 of an even n, where the shifted signal is not defined), s = 1 for a field on the
    face in direction `idir` (u and its right-hand sides in x, v in y) and 0 otherwise: what takes the half-cell offset between the two fields out of a
    cross-spectrum along `idir` (1 or 2). Staggering along z is not a phase along x or y and is not touched."""
    if idir not in (1, 2):
        raise ValueError("idir must be 1 or 2")
    n = int(n)
    s = lambda name: 1 if _FACE.get(name, 0) == idir else 0
    m = np.arange(n // 2 + 1)
    ph = np.exp(-1j * np.pi * m * (s(name_a) - s(name_b)) / n)
    if n % 2 == 0:
        ph[-1] = 1.
    return ph


def collect(h, pairs: Sequence[Tuple[str, str]] = PAIRS, kplanes: Sequence[int] = ()) -> Dict[str, object]:
    """This rank's sums of every pair: cross_x (n1/2+1, nz, npairs) complex, lsum_a_x and lsum_b_x (same shape) of the rank's rows; on one rank also
    cross_y, lsum_a_y, lsum_b_y (n2/2+1, nz, npairs) and, where `kplanes` (global k, 1 ... ng(3)) is not empty, cross2 (n1/2+1, n2/2+1, nplanes, npairs);
    None on several ranks. All complex128."""
    pairs = tuple((str(a), str(b)) for a, b in pairs)
    kp = [int(k) for k in kplanes]
    ng = [int(x) for x in h.case.ng]
    one = int(h.cs.nranks) == 1
    nz, nhx, nhy, npr = h.n[2], ng[0] // 2 + 1, ng[1] // 2 + 1, len(pairs)
    z = lambda *shape: np.zeros(shape, order="F", dtype=np.complex128)
    out = dict(n1=ng[0], n2=ng[1], pairs=pairs, kplanes=np.asarray(kp, dtype=np.int64),
               cross_x=z(nhx, nz, npr), lsum_a_x=z(nhx, nz, npr), lsum_b_x=z(nhx, nz, npr),
               cross_y=z(nhy, nz, npr) if one else None, lsum_a_y=z(nhy, nz, npr) if one else None, lsum_b_y=z(nhy, nz, npr) if one else None,
               cross2=z(nhx, nhy, len(kp), npr) if one and kp else None)
    for q, (a, b) in enumerate(pairs):
        out["cross_x"][:, :, q], out["lsum_a_x"][:, :, q], out["lsum_b_x"][:, :, q] = h.cospectra_lines(a, b, 1)
        if one:
            out["cross_y"][:, :, q], out["lsum_a_y"][:, :, q], out["lsum_b_y"][:, :, q] = h.cospectra_lines(a, b, 2)
            if kp:
                out["cross2"][:, :, :, q] = h.cospectra_planes(a, b, kp)
    return out


def add_ranks(parts: Sequence[Dict[str, object]]) -> Dict[str, object]:
    """The x sums of several ranks (each what `collect` returned there) added up; the y and 2-D parts are those of the first part (None on several ranks)."""
    out = dict(parts[0])
    for key in ("cross_x", "lsum_a_x", "lsum_b_x"):
        out[key] = np.asfortranarray(sum(p[key] for p in parts))
    return out


def normalise(collected: Dict[str, object]) -> Dict[str, Optional[np.ndarray]]:
    """x (n1/2+1, nz, npairs), y (n2/2+1, nz, npairs), c2 (n1/2+1, n2/2+1, nplanes, npairs), complex, as the module docstring defines them; None where
    not collected"""
    c = collected
    n1, n2 = int(c["n1"]), int(c["n2"])
    return dict(x=2. * c["cross_x"] / (n1 * n2), y=None if c["cross_y"] is None else 2. * c["cross_y"] / (n1 * n2),
                c2=None if c["cross2"] is None else c["cross2"] / float(n1 * n2) ** 2)


def _names(datadir: str, fldnum: int, pair: Tuple[str, str]):
    stem = os.path.join(datadir, f"cospectra_{pair[0]}{pair[1]}_fld_{int(fldnum):07d}")
    return stem + "_1d_x.bin", stem + "_1d_y.bin", stem + "_2d.bin", stem + "_kplanes.out"


def _blocks(z) -> np.ndarray:
    z = np.asarray(z)
    return np.concatenate([np.asfortranarray(z.real, dtype=np.float64).ravel(order="F"), np.asfortranarray(z.imag, dtype=np.float64).ravel(order="F")])


def _unblocks(path: str, shape) -> np.ndarray:
    raw = np.fromfile(path, dtype=np.float64)
    n = int(np.prod(shape))
    if raw.size != 2 * n:
        raise ValueError(f"{path}: not two blocks of {tuple(shape)}")
    return np.asfortranarray(raw[:n].reshape(shape, order="F") + 1j * raw[n:].reshape(shape, order="F"))


def write(datadir: str, fldnum: int, collected: Dict[str, object], zc) -> None:
    """The files of step `fldnum` for every collected pair; the y file only where it was collected (one rank), the 2-D and plane files only where planes
    were. zc: heights of the cell centres, haloed (0 ... nz+1, what initgrid returns) or interior (nz values)."""
    s = normalise(collected)
    nz = s["x"].shape[1]
    zc = np.asarray(zc, dtype=np.float64)
    if zc.size not in (nz, nz + 2):
        raise ValueError("zc must hold nz or nz + 2 values")
    zk = lambda k: zc[k] if zc.size == nz + 2 else zc[k - 1]
    for q, pair in enumerate(collected["pairs"]):
        f_x, f_y, f_2d, f_k = _names(datadir, fldnum, pair)
        _blocks(s["x"][:, :, q]).tofile(f_x)
        if s["y"] is not None:
            _blocks(s["y"][:, :, q]).tofile(f_y)
        if s["c2"] is not None:
            _blocks(s["c2"][:, :, :, q]).tofile(f_2d)
            with open(f_k, "w") as f:
                for k in collected["kplanes"]:
                    f.write(f"{int(k)} {float(zk(int(k))):.17e}\n")


def read(datadir: str, fldnum: int, n1: int, n2: int, pairs: Sequence[Tuple[str, str]] = PAIRS) -> Dict[str, object]:
    """What `write` wrote on one rank with planes, for a grid of n1 x n2 points per plane: x (n1/2+1, nz, npairs), y (n2/2+1, nz, npairs), c2 (n1/2+1,
    n2/2+1, nplanes, npairs), complex; pairs, kplanes and zc (nplanes)."""
    nhx, nhy = int(n1) // 2 + 1, int(n2) // 2 + 1
    pairs = tuple((str(a), str(b)) for a, b in pairs)
    per = {k: [] for k in ("x", "y", "c2")}
    for pair in pairs:
        f_x, f_y, f_2d, f_k = _names(datadir, fldnum, pair)
        meta = np.atleast_2d(np.loadtxt(f_k))
        nz = os.path.getsize(f_x) // (16 * nhx)
        per["x"].append(_unblocks(f_x, (nhx, nz))); per["y"].append(_unblocks(f_y, (nhy, nz))); per["c2"].append(_unblocks(f_2d, (nhx, nhy, meta.shape[0])))
    out = {k: np.asfortranarray(np.stack(v, axis=-1)) for k, v in per.items()}
    out.update(pairs=pairs, kplanes=meta[:, 0].astype(np.int64), zc=meta[:, 1].copy())
    return out

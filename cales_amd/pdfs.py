"""Per-plane PDFs and joint PDFs of u, v, w, the eddy viscosity and p, in the files the reference's utils/pdf-stats.py time-averages.

That script reads, per saved step NNNNNNN of the data directory,

  pdfs_fld_NNNNNNN_pdf.bin        float64 (npdf, nz, 5), Fortran order: the histogram of each variable on every plane
  pdfs_fld_NNNNNNN_pdf_meta.out   one line: npdf min0 max0 ... min4 max4
  pdfs_fld_NNNNNNN_jpdf.bin       float64 (njpdf, njpdf, nplanes, 5, 5), Fortran order, [:, :, plane, a, b]: first axis variable a, second variable b
  pdfs_fld_NNNNNNN_jpdf_meta.out  one row per plane: njpdf kplane zc(kplane) min0 max0 ... min4 max4

with the variables in the order u, v, w, slot 3, p. The script names slot 3 `ix` and never reads it; the eddy viscosity is written there. It reads the
pairs a < b of the joint file; the blocks with a >= b stay zero. No routine of the reference's src/ writes these files. Here the counts come from the
device (HotPath.pdf_planes / jpdf_planes, include/cales_pdf.h): `collect` gathers one rank's, `add_ranks` adds those of several, `write` writes the four
files and `read` reads them back. (The script reshapes the joint file with npdf, not njpdf: it wants the two equal.)"""
from __future__ import annotations

import os
from typing import Dict, Sequence

import numpy as np

VARS = ("u", "v", "w", "visct", "p")      # the file order; slot 3 is `ix` to the consumer
NV = len(VARS)
_SUMS = ("pdf", "outside", "jpdf", "joutside")


def collect(h, npdf: int, ranges, njpdf: int, kplanes: Sequence[int], jranges) -> Dict[str, np.ndarray]:
    """This rank's counts of the five variables. ranges: five (min, max) pairs; kplanes: global plane indices 1 ... ng(3); jranges: five pairs, or
    (nplanes, 5, 2) with ranges of their own for every plane (the meta file holds a row per plane). Returns pdf (npdf, nz, 5) and outside (2, nz, 5):
    below, above; jpdf (njpdf, njpdf, nplanes, 5, 5) and joutside (nplanes, 5, 5): either variable outside, filled for a < b; all int64."""
    kp = [int(k) for k in kplanes]
    rg = np.asarray(ranges, dtype=np.float64).reshape(NV, 2)
    jr = np.array(np.broadcast_to(np.asarray(jranges, dtype=np.float64), (len(kp), NV, 2)))
    nz = h.n[2]
    out = dict(npdf=int(npdf), njpdf=int(njpdf), kplanes=np.asarray(kp, dtype=np.int64), ranges=rg, jranges=jr,
               pdf=np.zeros((npdf, nz, NV), order="F", dtype=np.int64), outside=np.zeros((2, nz, NV), order="F", dtype=np.int64),
               jpdf=np.zeros((njpdf, njpdf, len(kp), NV, NV), order="F", dtype=np.int64), joutside=np.zeros((len(kp), NV, NV), order="F", dtype=np.int64))
    for a, name in enumerate(VARS):
        out["pdf"][:, :, a], out["outside"][:, :, a] = h.pdf_planes(name, npdf, rg[a, 0], rg[a, 1])
    same = all(np.array_equal(jr[q], jr[0]) for q in range(len(kp)))
    groups = [list(range(len(kp)))] if same else [[q] for q in range(len(kp))]      # planes that share their ranges go in one call
    for a in range(NV):
        for b in range(a + 1, NV):
            for grp in groups:
                r = jr[grp[0]]
                out["jpdf"][:, :, grp, a, b], out["joutside"][grp, a, b] = h.jpdf_planes(VARS[a], VARS[b], njpdf, r[a], r[b], [kp[q] for q in grp])
    return out


def add_ranks(parts: Sequence[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """The counts of several ranks (each what `collect` returned there, with the same arguments) added up."""
    out = dict(parts[0])
    for key in _SUMS:
        out[key] = np.asfortranarray(sum(p[key] for p in parts))
    return out


def _names(datadir: str, fldnum: int):
    stem = os.path.join(datadir, f"pdfs_fld_{int(fldnum):07d}")
    return stem + "_pdf.bin", stem + "_pdf_meta.out", stem + "_jpdf.bin", stem + "_jpdf_meta.out"


def _pairs(r) -> str:
    return " ".join(f"{float(x):.17e}" for x in np.asarray(r).reshape(-1))


def write(datadir: str, fldnum: int, collected: Dict[str, np.ndarray], zc) -> None:
    """The four files of step `fldnum`. zc: heights of the cell centres, haloed (0 ... nz+1, what initgrid returns) or interior (nz values)."""
    c = collected
    nz = c["pdf"].shape[1]
    zc = np.asarray(zc, dtype=np.float64)
    if zc.size not in (nz, nz + 2):
        raise ValueError("zc must hold nz or nz + 2 values")
    zk = lambda k: zc[k] if zc.size == nz + 2 else zc[k - 1]
    f_pdf, f_meta, f_jpdf, f_jmeta = _names(datadir, fldnum)
    np.asfortranarray(c["pdf"], dtype=np.float64).ravel(order="F").tofile(f_pdf)
    with open(f_meta, "w") as f:
        f.write(f"{int(c['npdf'])} {_pairs(c['ranges'])}\n")
    np.asfortranarray(c["jpdf"], dtype=np.float64).ravel(order="F").tofile(f_jpdf)
    with open(f_jmeta, "w") as f:
        for q, k in enumerate(c["kplanes"]):
            f.write(f"{int(c['njpdf'])} {int(k)} {float(zk(int(k))):.17e} {_pairs(c['jranges'][q])}\n")


def read(datadir: str, fldnum: int) -> Dict[str, np.ndarray]:
    """What `write` wrote: npdf, ranges (5, 2), pdf (npdf, nz, 5), njpdf, kplanes, zc (nplanes), jranges (nplanes, 5, 2), jpdf (njpdf, njpdf, nplanes,
    5, 5); the counts as int64."""
    f_pdf, f_meta, f_jpdf, f_jmeta = _names(datadir, fldnum)
    meta = np.loadtxt(f_meta).reshape(-1)
    npdf = int(meta[0])
    raw = np.fromfile(f_pdf, dtype=np.float64)
    jmeta = np.atleast_2d(np.loadtxt(f_jmeta))
    njpdf, nplanes = int(jmeta[0, 0]), jmeta.shape[0]
    jraw = np.fromfile(f_jpdf, dtype=np.float64)
    return dict(npdf=npdf, ranges=meta[1:].reshape(NV, 2), pdf=np.rint(raw).astype(np.int64).reshape((npdf, raw.size // (npdf * NV), NV), order="F"),
                njpdf=njpdf, kplanes=jmeta[:, 1].astype(np.int64), zc=jmeta[:, 2].copy(), jranges=jmeta[:, 3:].reshape(nplanes, NV, 2),
                jpdf=np.rint(jraw).astype(np.int64).reshape((njpdf, njpdf, nplanes, NV, NV), order="F"))

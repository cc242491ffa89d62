"""tests.util.helmholtz_reference: the Helmholtz solve of 3-D implicit diffusion in extended precision (x87 longdouble), the reference the GPU tests
of tests/test_gpu_helmholtz3d.py hold device AND oracle to. CPU only. (1) It reproduces the oracle on every BC set at short lines, at the project's
1e-12; (2) where the transform set is an exact diagonalisation its solution satisfies the discrete equation at least 100 times better than the
oracle's -- which makes it trustworthy without the oracle; (3) the oracle's own error at the line lengths production kernels exist for, as a record
(BASELINE.md 5): it reaches 1e-12 of the solution from 1024-point lines on, which is why those lengths need a reference better than both sides."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import (LD, OPEN_SETS, helmholtz_exact_kinds, helmholtz_operator, helmholtz_reference, helmholtz_unknowns, load_golden, open_case)

ALPHA = -0.21


def _couette(ng):
    g, case = load_golden("couette_imp3d_ops")
    case.ng[:] = ng
    return case


def _cavity(ng):
    g, case = load_golden("cavity_nnn")
    case.ng[:] = ng; case.impdiff = 1; case.lwm[:] = 0; case.sgstype = "none"; case.bcvel[:] = 0.
    return case


def _solve_both(case, ivel, seed=1):
    """random r.h.s. in +-0.5 with the boundary terms added: (r, oracle's x, reference's x) on the unknowns, and the oracle"""
    o = Oracle(case, nthreads=8)
    nn = helmholtz_unknowns(case, o, ivel)
    rng = np.random.RandomState(seed + ivel)
    q = o.zeros(); q[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1] = rng.rand(*nn) - 0.5
    o.updt_rhs_b_vel(ivel, ALPHA, q)
    x = helmholtz_reference(case, o, ivel, ALPHA, q)
    r = q[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1].copy()
    o.solver_helmholtz(ivel, ALPHA, q)
    assert x.dtype == np.longdouble and x.shape == tuple(nn)
    return r, q[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1].copy(), x, o


FREE_SLIP = (("DD", "NN"), ("DD", "NN"))
# (id, x set, y set, case): the sets as open_case takes them, for the cases that have none of their own the pairs they come with
SHORT = ([(f"open-{i}", xs, ys, lambda xs=xs, ys=ys, ng=ng: open_case(xs, ys, ng)) for i, (xs, ys, ng) in enumerate(OPEN_SETS)] +
         [("cavity-32x16x12", ("DD", "DD"), ("DD", "DD"), lambda: _cavity((32, 16, 12))), ("cavity-20x36x10", ("DD", "DD"), ("DD", "DD"), lambda: _cavity((20, 36, 10))),
          ("couette-32x16x12", None, None, lambda: _couette((32, 16, 12))), ("couette-48x40x9", None, None, lambda: _couette((48, 40, 9))),
          ("free-slip-64x32x12", *FREE_SLIP, lambda: open_case(*FREE_SLIP, (64, 32, 12))), ("free-slip-18x20x7", *FREE_SLIP, lambda: open_case(*FREE_SLIP, (18, 20, 7)))])
LONGER = [("couette-96x48x8", None, None, lambda: _couette((96, 48, 8))), ("couette-2048x16x4", None, None, lambda: _couette((2048, 16, 4))),
          ("cavity-128x64x8", ("DD", "DD"), ("DD", "DD"), lambda: _cavity((128, 64, 8)))]


def _exact(xs, ys, ivel):
    """the transform set of the component is an exact diagonalisation: no NN or ND pair along it"""
    own = (xs, ys, None)[ivel - 1]
    return own is None or own[0] not in ("NN", "ND")


@pytest.mark.imp3d_open
@pytest.mark.parametrize("make,ivel", [pytest.param(mk, iv, id=f"{i}-{'uvw'[iv - 1]}") for i, xs, ys, mk in SHORT for iv in (1, 2, 3)])
def test_oracle_agrees_with_the_reference_at_short_lines(make, ivel):
    """every BC set of OPEN_SETS, the no-slip cavity, the periodic couette case and a free-slip box at lines of 64 points and less: 1e-12 max|x|
    ("Poisson / Helmholtz solve"). The reference follows the algorithm, the two inexact face-centred sets included."""
    r, xo, x, o = _solve_both(make(), ivel)
    err = float(np.abs(xo - x).max() / np.abs(x).max())
    print("oracle - reference", err)
    assert err < 1e-12


@pytest.mark.imp3d_open
@pytest.mark.parametrize("make,ivel", [pytest.param(mk, iv, id=f"{i}-{'uvw'[iv - 1]}") for i, xs, ys, mk in SHORT + LONGER for iv in (1, 2, 3) if _exact(xs, ys, iv)])
def test_reference_satisfies_the_discrete_equation(make, ivel):
    """(1 + alpha L_h) x - r in extended precision for the reference's solution and for the oracle's, same input, where the transform set is exact (PP,
    every cell-centred pair, face-centred DD and DN): the reference's residual is at least 100 times smaller. Extended precision carries 2^11 times
    the digits; 100 leaves a factor of 20 for the longer summations."""
    case = make()
    r, xo, x, o = _solve_both(case, ivel)
    assert helmholtz_exact_kinds(o, ivel)      # (NN / ND along the component are no exact inverses in the reference, test_helmholtz_3d_identity_open_x: held to the oracle above)
    rr = r.astype(LD); scale = np.abs(rr).max()
    res_ref = float(np.abs(helmholtz_operator(case, o, ivel, ALPHA, x) - rr).max() / scale)
    res_ora = float(np.abs(helmholtz_operator(case, o, ivel, ALPHA, xo.astype(LD)) - rr).max() / scale)
    print("residual: reference %.2e oracle %.2e" % (res_ref, res_ora))
    assert res_ora < 1e-9      # (the operator here is the oracle's: 1.6e-10 at 2048-cell rows, whose 1/h^2 is 1e6)
    assert 100. * res_ref <= res_ora, (res_ref, res_ora)


PRODUCTION = [(96, 48, 8), (64, 32, 129), (32, 768, 4), (32, 16, 1024), (16, 1024, 4), (2048, 16, 4), (1536, 16, 4)]


@pytest.mark.parametrize("ivel", [1, 3])
@pytest.mark.parametrize("ng", PRODUCTION)
def test_oracle_error_at_production_lengths(ng, ivel):
    """The record: the oracle's error against the reference, relative to max|x|, on the periodic couette case, u | w. Measured: 96 x 48 x 8
    1.2e-15 | 3.1e-15, 64 x 32 x 129 3.4e-15 | 8.9e-15, 32 x 768 x 4 1.9e-15 | 7.3e-14, 32 x 16 x 1024 1.5e-13 | 2.6e-13, 16 x 1024 x 4 2.2e-15 | 3.4e-13,
    2048 x 16 x 4 5.7e-15 | 1.4e-12, 1536 x 16 x 4 6.3e-15 | 1.2e-12 (u stays small because the moving walls' boundary terms dominate its solution). What
    grows with the line is not the transforms' round-off but the FP64 eigenvalues -2 (1 - cos theta) of initsolver.f90:66-98: fed those, the reference
    agrees with the oracle to 2e-15 at 2048 x 16 x 4. Asserted only against the weaker of the project's two bars (1e-11, the pressure
    solve's at production lengths)."""
    r, xo, x, o = _solve_both(_couette(ng), ivel)
    err = float(np.abs(xo - x).max() / np.abs(x).max())
    print("oracle error", ng, "ivel", ivel, "%.2e" % err)
    assert err < 1e-11

"""k_wallmodel at its launch edges. All wall-model faces of a bounduvw share one launch of 64 x 4 blocks that spans the largest face; blocks beyond a
smaller face return, and the two tangential components of a face have different index ranges (0..na x 1..nb against 1..na x 0..nb, wmodel.f90:139-170,
190-221, 241-271). The golden cases' faces of 8-12 cells fit in one block column. Here: a box with six wall-model faces, both stress laws and six moving
walls, at sizes that put a face's first index at 63, 65, 67 and 131 points, on x-normal and z-normal faces, with faces of very different size in one launch
-- against the CPU restatement, which the reference-made vectors pin branch by branch (tests/test_oracle_golden.py: faces in x, the laminar law, the
wall velocities, one-sided models)."""
import numpy as np
import pytest

from tests.util import F, load_golden, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-13
SIZES = [(62, 6, 5), (64, 6, 5), (66, 8, 6), (130, 4, 4), (4, 66, 5), (4, 130, 4)]
# the tangential components of a face with normal idir, in the order of the reference's two loops
TANGENTIAL = {1: (2, 3), 2: (1, 3), 3: (1, 2)}


def _box(ng):
    """all walls, uniform grid of 0.1-wide cells, hwm = 0.17 (between the second and the third cell centre: index_wm = 3 / n - 2, no tie), the log law and the
    laminar law on three faces each -- one of each per direction --, every wall moving with its own two tangential velocities"""
    g, case = load_golden("cavity_smag_wm6")
    case.ng[:] = ng; case.l[:] = [0.1 * x for x in ng]; case.gtype = 1; case.gr = 0.; case.hwm = 0.17
    case.lwm[:, 0] = (1, -1); case.lwm[:, 1] = (-1, 1); case.lwm[:, 2] = (1, -1)
    case.bcvel[:] = 0.
    for d in range(3):
        for side in range(2):
            for q, iv in enumerate(TANGENTIAL[d + 1]):
                case.bcvel[side, d, iv - 1] = (-1.) ** (side + q) * 0.05 * (1 + q + 2 * side + 4 * d)
    return case


def _written(ng, idir, iv):
    """the entries of component iv's plane at a face with normal idir that the wall-model loops assign (the same on both sides)"""
    na, nb = (ng[1] if idir == 1 else ng[0]), (ng[1] if idir == 3 else ng[2])
    m = np.zeros((na + 2, nb + 2), dtype=bool)
    if iv == TANGENTIAL[idir][0]:
        m[0:na + 1, 1:nb + 1] = True
    elif iv == TANGENTIAL[idir][1]:
        m[1:na + 1, 0:nb + 1] = True
    return m


@pytest.mark.parametrize("ng", SIZES, ids=lambda v: "x".join(str(x) for x in v))
def test_wall_model_planes_at_block_edges(ng):
    from cales_amd.hotpath import HotPath, check_case
    from oracle.oracle import Oracle
    case = _box(ng)
    check_case(case)
    assert len({case.bcvel[s, d, iv - 1] for d in range(3) for s in range(2) for iv in TANGENTIAL[d + 1]}) == 12
    o = Oracle(case)
    iw = o.index_wm()
    assert all(iw[0, d] == 3 and iw[1, d] == ng[d] - 2 for d in range(3)), iw
    rng = np.random.RandomState(2026)
    shape = tuple(x + 2 for x in ng)
    raw = [F(rng.rand(*shape) - 0.5) for _ in range(4)]
    u, v, w = (a.copy(order="F") for a in raw[:3])
    o.bounduvw(u, v, w, True, False)
    h = HotPath(case)
    h.upload(*raw)
    h.bounduvw(True, False)
    for iv, nm in ((1, "bcu"), (2, "bcv"), (3, "bcw")):
        for idir, (a, ref) in enumerate(zip(h.bcvel_planes(iv), o.bcvel_planes(iv)), start=1):
            err = np.abs(a - ref).max()
            print(f"{nm}.{'xyz'[idir - 1]}: max |diff| = {err:.3e} of {np.abs(ref).max():.3e}")
            assert err <= 1e-12 * max(1., np.abs(ref).max()), (nm, idir, err)
            # what the loops leave alone: the ghost corners, row 0 of the second component, row and column 0 / n + 1, the normal component's planes
            keep = ~_written(ng, idir, iv)
            assert np.array_equal(a[keep], ref[keep]), (nm, idir)
            assert np.isfinite(ref).all() and (iv == idir or np.abs(ref[_written(ng, idir, iv)]).min() > 0.)
    for k, ref in zip("uvw", (u, v, w)):
        err = relerr(h.get(k), ref)
        print(f"{k} after bounduvw: {err:.3e}")
        assert err < TOL, k
    # the strain rates of the subgrid model see ghost cells extrapolated from the interior at these faces (extrapolate(...,lwm), sgs.f90:683-766) and the van
    # Driest damping the stress-carrying ones: the eddy viscosity of the same fields, at the bars of the stage-by-stage test
    visct = o.zeros()
    o.cmpt_sgs(u, v, w, visct)
    h.upload(u, v, w, raw[3]); h.cmpt_sgs()
    err = relerr(h.get("visct")[1:-1, 1:-1, 1:-1], visct[1:-1, 1:-1, 1:-1])
    print(f"visct interior: {err:.3e}")
    assert err < TOL
    h.set("visct", visct); h.boundp("visct", 1)
    o.boundp(visct, 1)
    assert relerr(h.get("visct"), visct) < TOL
    h.close(); o.close()

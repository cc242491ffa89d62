"""The one-launch ghost-cell kernel of the periodic BC sets (k_bc_merged: x and y periodic, any pointwise z condition) against the reference's order, one
launch per direction (CALES_UNMERGED_BC), on RANDOM fields with random ghost cells -- the comparison test_all_directions_ghost_cell_kernel_equals_the_sequence
(tests/test_gpu_golden.py) makes for k_bc_all, at shapes chosen for where the kernel's 64 x 4 blocks and its three regions (z planes, x columns with the
lanes along y, y rows) can go wrong."""
import numpy as np
import pytest

from tests.util import F, load_golden

pytestmark = pytest.mark.gpu

SHAPES = [("tgv_ppp", (16, 12, 10)),       # periodic z: both ends from one rule, corners through all three wraps
          ("chan_dsmag", (72, 8, 6)),      # n1 + 2 > 64: two blocks along x; face-centred Dirichlet top plane
          ("chan_smag", (8, 70, 6)),       # n2 + 2 > 64 > n1 + 2: region 1 runs its lanes along y over two blocks
          ("chan_dsmag", (16, 8, 20))]     # n3 + 2 > n2 + 2: the grid's second extent comes from z
FIELDS = ("u", "v", "w", "p", "visct", "pp")


@pytest.mark.parametrize("is_correc", [False, True], ids=["impose", "is_correc"])
@pytest.mark.parametrize("name,ng", SHAPES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in SHAPES])
def test_one_launch_periodic_kernel_equals_the_sequence(name, ng, is_correc, monkeypatch):
    """bounduvw (both values of is_correc) and boundp of p, visct and pp: every cell of every field, ghost cells and the cells neither form may touch
    included, to 4e-16 max(1, max|b|) -- the bar of the k_bc_all test: both forms evaluate the same one or two operations per ghost cell."""
    from cales_amd.hotpath import HotPath
    g, case = load_golden(name); case.ng[:] = ng
    rng = np.random.RandomState(11)
    shape = tuple(x + 2 for x in ng)
    f0 = [F(rng.rand(*shape) - 0.5) for _ in range(5)]
    out = {}
    for mode in ("one_launch", "by_direction"):
        if mode == "by_direction":
            monkeypatch.setenv("CALES_UNMERGED_BC", "1")
        h = HotPath(case)
        assert h.describe_plan()["ghost_cells"] == mode
        h.upload(*f0[:4]); h.set("visct", f0[4]); h.set("pp", f0[3])
        h.bounduvw(True, is_correc); h.boundp("p", 0); h.boundp("visct", 1); h.boundp("pp", 0)
        out[mode] = [h.get(k) for k in FIELDS]
        h.close()
    for nm, a, b in zip(FIELDS, out["one_launch"], out["by_direction"]):
        err = np.abs(a - b).max()
        print(nm, err)
        assert err <= 4e-16 * max(1., np.abs(b).max()), (nm, err)

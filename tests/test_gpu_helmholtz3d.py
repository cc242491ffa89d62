"""cales_helmholtz (3-D implicit diffusion, impdiff = 1) on the kernels production grids take: the radix-8 and odd-radix transforms, k_fft_y16, the
Neumann radix-8 kinds of free-slip walls, k_dst1 behind its LDS attribute, every M of the z tile, u, v and w on different tiles with one table, the
persistent 1024-plane tile. Every row is the smallest grid that reaches the kernel it names, and asserts the path by name (helmholtz_u/v/w of
cales_describe_plan) BEFORE it solves: without the kernel the name fails, not the number.

The bar. The CPU oracle is itself at 1e-12 of the solution from 1024-point lines on (tests/test_helmholtz_reference.py), so device and
oracle are both measured against the extended-precision solve of the same system (tests.util.helmholtz_reference) on the same input:
e_gpu <= max(1e-12, 4 e_oracle), both relative to max|x_ref|. 1e-12 is the project's bar for this operator; the second term only matters where a correct
FP64 evaluation of the algorithm is above it, and 4 is the room one such evaluation gets over another with a different summation order. The direct
device-oracle difference is printed, not asserted."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.test_gpu_vs_oracle import _hot
from tests.util import helmholtz_reference, helmholtz_unknowns, load_golden, open_case

pytestmark = pytest.mark.gpu

ALPHA = -0.21
R8, R8R, Y16, MIX, FACE = "radix8", "radix8_register_ends", "radix8_16_per_thread", "mixed_radix", "face_centred"


def _couette(ng):
    g, case = load_golden("couette_imp3d_ops")
    case.ng[:] = ng
    return case


def _cavity(ng):      # as in test_helmholtz_3d_with_walls
    g, case = load_golden("cavity_nnn")
    case.ng[:] = ng; case.impdiff = 1
    case.lwm[:] = 0; case.sgstype = "none"; case.bcvel[:] = 0.
    return case


def _free_slip(ng):
    return open_case(("DD", "NN"), ("DD", "NN"), ng)


def _pp(xk, yk, zu, zw=None):
    """periodic x and y: one transform pair for the three components, the tile of u and v | of w"""
    return {iv: f"x:PP/{xk},y:PP/{yk},z:{zu if iv < 3 else (zw or zu)}" for iv in (1, 2, 3)}


def _walls(xpair, ypair, xk, yk, z, zw=None):
    """x and y pairs (normal, tangential) with the kernel each tangential direction takes; the normal one is face-centred"""
    face = {"DD": "DDf", "NN": "NNf", "DN": "DNf"}
    out = {}
    for iv in (1, 2, 3):
        x = f"{face[xpair[0]]}/{FACE}" if iv == 1 else f"{xpair[1]}/{xk}"
        y = f"{face[ypair[0]]}/{FACE}" if iv == 2 else f"{ypair[1]}/{yk}"
        out[iv] = f"x:{x},y:{y},z:{z if iv < 3 else (zw or z)}"
    return out


T2, T4, T8, T16 = "lds_tile_m2", "lds_tile_m4", "lds_tile_m8", "lds_tile_m16"
NOSLIP = (("DD", "DD"), ("DD", "DD"))
SLIP = (("DD", "NN"), ("DD", "NN"))
# (id, case, components, names per component, environment)
ROWS = [
    # periodic x and y (the couette case, its own wall values kept)
    ("pp-32x16x12", lambda: _couette((32, 16, 12)), (1, 2, 3), _pp(R8, R8R, T2), {}),                       # the anchor the suite has today
    ("pp-96x48x8", lambda: _couette((96, 48, 8)), (1, 2, 3), _pp("radix8x3", "radix8x3", T2), {}),
    ("pp-160x72x6", lambda: _couette((160, 72, 6)), (1, 2, 3), _pp("radix8x5", "radix8x9", T2), {}),
    ("pp-144x80x6", lambda: _couette((144, 80, 6)), (1, 2, 3), _pp("radix8x9", "radix8x5", T2), {}),
    ("pp-2048x16x4", lambda: _couette((2048, 16, 4)), (1, 2, 3), _pp(R8, R8R, T2), {}),                     # 1024-point radix-8 rows
    ("pp-1536x16x4", lambda: _couette((1536, 16, 4)), (1, 2, 3), _pp("radix8x3", R8R, T2), {}),             # 768-point rows
    ("pp-16x1024x4", lambda: _couette((16, 1024, 4)), (1, 2, 3), _pp(MIX, Y16, T2), {}),                    # k_fft_y16, periodic
    ("pp-32x768x4", lambda: _couette((32, 768, 4)), (1, 2, 3), _pp(R8, "radix8x3", T2), {}),                # 768-point odd y lines, LDS above 64 KB
    ("pp-64x32x129", lambda: _couette((64, 32, 129)), (1, 2, 3), _pp(R8, R8R, T4, T2), {}),                 # u, v: 129 planes, w: 128 -- one table
    ("pp-32x16x513", lambda: _couette((32, 16, 513)), (1, 2, 3), _pp(R8, R8R, T16, T8), {}),
    ("pp-64x32x24-march", lambda: _couette((64, 32, 24)), (1, 2, 3), _pp(R8, R8R, "thomas_march"), {"CALES_GAUSSEL_MARCH": "1"}),
    # no-slip walls: k_dst1 along the component, the generic Dirichlet-Dirichlet transform across it
    ("walls-128x64x8", lambda: _cavity((128, 64, 8)), (1, 2, 3), _walls(*NOSLIP, MIX, MIX, T2), {}),
    ("walls-100x36x6", lambda: _cavity((100, 36, 6)), (1, 2, 3), _walls(*NOSLIP, MIX, MIX, T2), {}),
    ("walls-1024x16x4", lambda: _cavity((1024, 16, 4)), (1, 2), _walls(*NOSLIP, MIX, MIX, T2), {}),         # k_dst1 on 2048 points: 65.6 KB of LDS
    ("walls-16x1024x4", lambda: _cavity((16, 1024, 4)), (1, 2), _walls(*NOSLIP, MIX, MIX, T2), {}),
    ("walls-32x16x1024", lambda: _cavity((32, 16, 1024)), (1, 2, 3), _walls(*NOSLIP, MIX, MIX, "lds_tile_persistent", T16), {}),
    # free-slip box: Neumann radix-8 across the component
    ("slip-64x32x12", lambda: _free_slip((64, 32, 12)), (1, 2, 3), _walls(*SLIP, R8, R8, T2), {}),
    ("slip-96x48x8", lambda: _free_slip((96, 48, 8)), (1, 2, 3), _walls(*SLIP, "radix8x3", "radix8x3", T2), {}),
    ("slip-32x256x4", lambda: _free_slip((32, 256, 4)), (1, 2, 3), _walls(*SLIP, R8, Y16, T2), {}),         # k_fft_y16, Neumann, 256 points
    ("slip-1536x16x4", lambda: _free_slip((1536, 16, 4)), (1, 2, 3), _walls(*SLIP, "radix8x3", R8, T2), {}),   # 768-point Neumann rows
    # real x modes and periodic y: k_gaussel_herm with a Helmholtz scale
    ("slipx-64x32x12", lambda: open_case(("DD", "NN"), None, (64, 32, 12)), (1, 2, 3),
     {1: f"x:DDf/{FACE},y:PP/{R8R},z:thomas_hermitian", 2: f"x:NN/{R8},y:PP/{R8R},z:thomas_hermitian", 3: f"x:NN/{R8},y:PP/{R8R},z:thomas_hermitian"}, {}),
    # open boundaries: the generic x transform of kind 1 (REDFT10/01 along u) and the DCT-IV rows feeding radix-8 y
    ("open-ND-32x64x10", lambda: open_case(("ND", "ND"), None, (32, 64, 10)), (1, 2, 3),
     {1: f"x:NN/{MIX},y:PP/{R8R},z:thomas_hermitian", 2: f"x:ND/dct4,y:PP/{R8R},z:thomas_hermitian", 3: f"x:ND/dct4,y:PP/{R8R},z:thomas_hermitian"}, {}),
    ("open-DN-64x32x10", lambda: open_case(("DN", "NN"), None, (64, 32, 10)), (1, 2, 3),
     {1: f"x:DNf/{FACE},y:PP/{R8R},z:thomas_hermitian", 2: f"x:NN/{MIX},y:PP/{R8R},z:thomas_hermitian", 3: f"x:NN/{MIX},y:PP/{R8R},z:thomas_hermitian"}, {}),
]
OPEN = ("slip", "open")      # outside the reference's own limits for 3-D implicit diffusion: CALES_IMP3D_OPEN (the marker)
PARAMS = [pytest.param(row, iv, id=f"{row[0]}-{'uvw'[iv - 1]}", marks=[pytest.mark.imp3d_open] if row[0].startswith(OPEN) else [])
          for row in ROWS for iv in row[2]]


@pytest.mark.parametrize("row,ivel", PARAMS)
def test_helmholtz_3d_production_kernels(row, ivel, monkeypatch):
    """the body of test_helmholtz_3d_open_boundaries, device and oracle each against the extended-precision reference (the module's docstring)"""
    rid, make, _, names, env = row
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = make()
    ng = tuple(int(x) for x in case.ng)
    o = Oracle(case, nthreads=8); h = _hot(case)
    key = "helmholtz_" + "uvw"[ivel - 1]
    got_name = h.describe_plan().get(key)
    print(rid, key, got_name)
    assert got_name == names[ivel], (rid, ivel, got_name)
    nn = helmholtz_unknowns(case, o, ivel)
    rng = np.random.RandomState(30 + ivel)
    rhs = o.zeros(); rhs[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1] = rng.rand(*nn) - 0.5
    ref = rhs.copy(order="F"); o.updt_rhs_b_vel(ivel, ALPHA, ref)
    x = helmholtz_reference(case, o, ivel, ALPHA, ref)      # the boundary terms are no part of the solve: the r.h.s. after them
    o.solver_helmholtz(ivel, ALPHA, ref)
    h.set("uvw"[ivel - 1], rhs); h.helmholtz(ivel, ALPHA)
    got = h.get("uvw"[ivel - 1])
    a = got[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1]; b = ref[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1]
    scale = np.abs(x).max()
    e_gpu, e_oracle = float(np.abs(a - x).max() / scale), float(np.abs(b - x).max() / scale)
    print(rid, ng, "ivel", ivel, "e_gpu %.2e e_oracle %.2e gpu-oracle %.2e" % (e_gpu, e_oracle, np.abs(a - b).max() / np.abs(b).max()))
    assert h.describe_plan().get(key) == got_name
    h.close()
    assert e_gpu <= max(1e-12, 4. * e_oracle), (rid, ivel, e_gpu, e_oracle)


T_U = "x:PP/radix8x3,y:PP/radix8x3,z:" + T2
STEPS = [((96, 48, 12), "x:PP/radix8x3,y:PP/radix8x3,", {"helmholtz_u": T_U, "helmholtz_v": T_U, "helmholtz_w": T_U}),
         # 130 | 129 planes: u, v and w all on the four-planes-per-lane tile
         ((64, 32, 130), f"x:PP/{R8},y:PP/{R8R},", {k: f"x:PP/{R8},y:PP/{R8R},z:{T4}" for k in ("helmholtz_u", "helmholtz_v", "helmholtz_w")}),
         # 129 | 128 planes: w on another tile than u and v, the table they share rebuilt by every solve
         ((64, 32, 129), f"x:PP/{R8},y:PP/{R8R},", {"helmholtz_u": f"x:PP/{R8},y:PP/{R8R},z:{T4}", "helmholtz_v": f"x:PP/{R8},y:PP/{R8R},z:{T4}", "helmholtz_w": f"x:PP/{R8},y:PP/{R8R},z:{T2}"})]


@pytest.mark.parametrize("ng,solver,plan", STEPS)
def test_time_steps_imp3d_at_production_kernels(ng, solver, plan):
    """two steps against the oracle, body and bars of test_time_steps_at_odd_radix_lines (velocity 1e-9, mean-free pressure 1e-8), the plan keys asserted"""
    from tests.test_gpu_lines359 import test_time_steps_at_odd_radix_lines
    test_time_steps_at_odd_radix_lines("couette_imp3d_ops", ng, plan, solver)


@pytest.mark.parametrize("P", [2, 4])
def test_slab_ranks_imp3d_radix8(P):
    """emulated ranks against the single-rank run, 1e-10 (tests/test_gpu_decomp.py): Helmholtz solves with radix-8 transforms in both directions"""
    from tests.test_gpu_decomp import test_slab_ranks_match_single_rank
    test_slab_ranks_match_single_rank("couette_imp3d_ops", (64, 32, 16), P)


def test_slab_ranks_imp3d_radix8_pipelined_exchange(monkeypatch):
    """... and the k-chunked exchange on the second stream, which a Helmholtz solve takes only with radix-8 in both directions (event-ordered emulation)"""
    from tests.test_gpu_decomp import test_slab_ranks_overlapped_event_ordered
    test_slab_ranks_overlapped_event_ordered("couette_imp3d_ops", (64, 32, 16), 2, monkeypatch)

"""The x and y transform passes (k_solver.hip: XPass / YPass, filled by x_pass / y_pass at set-up, launched by fft_x / fft_y): every instantiation of
k_fft_x8, k_fft_y8r, k_fft_y8, k_fft_y16, the Stockham kernels, k_fft_x4, k_fft_y4 and k_dst1 on the smallest grid that reaches it, held to the commit
before the pass records bit for bit: the plan string and a SHA-256 of the bytes of the result (tests/golden/transform_passes/digests.json, written by
gen_digests.py beside it with that commit's library; it runs the functions of this file). No tolerance: the same instructions run in the same
geometry.

Kinds of case. solve: pp after solver() of a seeded compatible right-hand side (made as tests/test_gpu_lines359._solve makes it). step: u, v, w, p after
one cales_step from the perturbed initial flow, with fillps inside the forward x transform (asserted first). helm: the component after
helmholtz(iv, -0.21) of the right-hand side of tests/test_gpu_helmholtz3d (rows of its ROWS, by id) or of an open_case of tests/util.OPEN_SETS, per
component. ranks: tgv_dsmag_ppp on two loopback ranks (tests/test_gpu_solver_schedule.tgv_run), u, v, w, p, visct per rank."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.util import GOLD, load_golden, open_case

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(GOLD, "transform_passes", "digests.json")
ALPHA = -0.21
SWITCHES = ("CALES_FFT_GENERIC", "CALES_FFT_NO_ODD_RADIX", "CALES_IMP3D_OPEN")

# (kind, what, grid or None, environment)
CASES = [
    # k_fft_x8 without fillps: PP and NN | ODD | 768-point rows (LDS above 64 KB)
    ("solve", "chan_smag", (64, 16, 6), {}), ("solve", "cavity_nnn", (64, 32, 6), {}),      # (the second: k_fft_y8<., 1> too)
    ("solve", "chan_smag", (96, 48, 6), {}), ("solve", "cavity_nnn", (96, 48, 8), {}),
    ("solve", "chan_smag", (1536, 16, 4), {}), ("solve", "cavity_nnn", (1536, 16, 4), {}),
    # k_fft_x8<0, ., 1, .>: fillps inside the transform
    ("step", "chan_smag", (64, 16, 16), {}), ("step", "chan_smag", (96, 48, 8), {}), ("step", "cavity_nnn", (64, 32, 8), {}), ("step", "cavity_nnn", (96, 48, 8), {}),
    # k_fft_y8r, and at 512 points behind its attribute (82 KB)
    ("solve", "chan_smag", (16, 16, 6), {}), ("solve", "tgv_ppp", (32, 512, 4), {}),
    # k_fft_y8<., ., 1>: 768-point lines of both kinds (66 KB)
    ("solve", "chan_smag", (16, 768, 4), {}), ("solve", "duct_smag_wm", (32, 768, 4), {}),
    # k_fft_y16: NN 256, NN 512, PP 1024, NN 1024
    ("solve", "cavity_nnn", (32, 256, 4), {}), ("solve", "cavity_nnn", (16, 512, 4), {}), ("solve", "chan_smag", (16, 1024, 4), {}), ("solve", "cavity_nnn", (32, 1024, 4), {}),
    # Stockham k_fft_x / k_fft_y (the Dirichlet-Dirichlet kind in y: the u of walls-128x64x8 below -- no pressure of the goldens has it)
    ("solve", "chan_smag", (60, 90, 10), {}), ("solve", "chan_smag", (96, 48, 6), {"CALES_FFT_NO_ODD_RADIX": "1"}), ("solve", "chan_smag", (64, 16, 6), {"CALES_FFT_GENERIC": "1"}),
    # k_fft_x4, k_dst1<0 | 1 | 2> (walls-1024x16x4: behind its attribute), k_fft_y4 (the y sets of tests/util.OPEN_SETS)
    ("helm", "open-ND-32x64x10", None, {}), ("helm", "open-DN-64x32x10", None, {}), ("helm", "walls-128x64x8", None, {}), ("helm", "slip-64x32x12", None, {}),
    ("helm", "slipx-64x32x12", None, {}), ("helm", "walls-1024x16x4", None, {}),
    ("helm", "openy-DN-NN", (12, 16, 10), {}), ("helm", "openy-ND-DN", (12, 24, 10), {}),
    ("solve", "devchan_nd", (16, 8, 600), {}),
    # two ranks, loopback: in order and with the chunked exchange on the second stream
    ("ranks", "in_order", (32, 48, 16), {}), ("ranks", "second_stream", (32, 48, 16), {}),
]
OPENY = {"openy-DN-NN": ("DN", "NN"), "openy-ND-DN": ("ND", "DN")}


def case_id(kind, what, ng, env):
    return "-".join([kind, what] + (["%dx%dx%d" % tuple(ng)] if ng else []) + [k[6:].lower() for k in sorted(env)])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()


def _solve(name, ng):
    from oracle.oracle import Oracle
    from tests.test_gpu_vs_oracle import _hot
    g, case = load_golden(name)
    case.ng[:] = ng
    if case.lwm.any() and ng[2] == 4:      # see tests/test_gpu_lines359._solve
        case.hwm = 0.3
    o = Oracle(case, nthreads=8); h = _hot(case)
    plan = h.describe_plan()["solver"]
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    dzf = o.grid()["dzf"][1:-1]
    rhs[1:-1, 1:-1, 1:-1] -= (rhs[1:-1, 1:-1, 1:-1] * dzf).sum() / (dzf.sum() * ng[0] * ng[1])
    h.set("pp", rhs); h.solver()
    out = {"solver": plan, "pp": _sha(h.get("pp"))}
    h.close()
    return out


def _step(name, ng):
    from cales_amd.hotpath import initflow
    from tests.test_gpu_vs_oracle import _hot
    g, case = load_golden(name)
    case.ng[:] = ng
    h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(1)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    pl = h.describe_plan()
    assert pl["fillps"].startswith("in_x_transform"), pl
    h.step(0.5 * h.chkdt())
    out = {"solver": pl["solver"]}
    out.update({k: _sha(a) for k, a in zip("uvwp", h.download())})
    h.close()
    return out


def _helm(rid, ng):
    from oracle.oracle import Oracle
    from tests.test_gpu_helmholtz3d import ROWS
    from tests.test_gpu_vs_oracle import _hot
    from tests.util import helmholtz_unknowns
    if rid in OPENY:
        case, comps = open_case(None, OPENY[rid], ng), (1, 2, 3)
    else:
        row = [r for r in ROWS if r[0] == rid][0]
        case, comps = row[1](), row[2]
    o = Oracle(case, nthreads=8); h = _hot(case)
    out = {"solver": h.describe_plan()["solver"]}
    for iv in comps:
        nm = "uvw"[iv - 1]
        out["helmholtz_" + nm] = h.describe_plan()["helmholtz_" + nm]
        nn = helmholtz_unknowns(case, o, iv)
        rng = np.random.RandomState(30 + iv)
        rhs = o.zeros(); rhs[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1] = rng.rand(*nn) - 0.5
        h.set(nm, rhs); h.helmholtz(iv, ALPHA)
        out[nm] = _sha(h.get(nm))
    h.close()
    return out


def _ranks(order, ng):
    from tests.test_gpu_solver_schedule import tgv_run
    out = {}
    for r, x in enumerate(tgv_run(ng, 2, order == "second_stream")):
        out["rank%d_plan" % r] = x[5]
        out.update({"rank%d_%s" % (r, nm): _sha(x[q]) for q, nm in enumerate(("u", "v", "w", "p", "visct"))})
    return out


def run_case(kind, what, ng, env):
    """the plan strings and digests of one case, with the switches of env set for the context's lifetime"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    if kind == "helm" and what.startswith(("slip", "open")):      # beyond the reference's limits for 3-D implicit diffusion (tests/conftest.py: imp3d_open)
        os.environ["CALES_IMP3D_OPEN"] = "1"
    try:
        return {"solve": _solve, "step": _step, "helm": _helm, "ranks": _ranks}[kind](what, ng)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("kind,what,ng,env", CASES, ids=[case_id(*c) for c in CASES])
def test_transform_passes_give_the_bits_of_the_commit_before(kind, what, ng, env):
    want = json.load(open(DIGESTS))[case_id(kind, what, ng, env)]
    got = run_case(kind, what, ng, env)
    print(case_id(kind, what, ng, env), got)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], (k, got[k], want[k])

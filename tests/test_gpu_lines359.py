"""x rows and y lines of 3, 5, 9 times 2^p points (ng(1)/2 and ng(2) from 48 to 1024) in the radix-8 register kernels: the odd factor as a first
radix-3 / radix-5 stage (two radix-3 stages for 9) in front of the radix-8 / 4 / 2 body. With them comes the plan of a step that power-of-two
rows have: fillps inside the forward x transform, wrapped x ghost columns, the folded projection, the packed mode column. Every comparison here is
one the suite already makes at power-of-two lengths, at the same bar; each case also asserts the path it took by name
(cales_describe_plan), which is what fails without these kernels."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.test_gpu_vs_oracle import _hot
from tests.util import F, load_golden, relerr

pytestmark = pytest.mark.gpu

R8, R8R, MIX = "radix8", "radix8_register_ends", "mixed_radix"
# (case, grid, x kernel, y kernel): every odd factor in x and in y, both kinds, the smallest and the largest p
SOLVES = [("chan_smag", (96, 48, 6), "PP/radix8x3", "PP/radix8x3"), ("chan_smag", (160, 72, 6), "PP/radix8x5", "PP/radix8x9"),
          ("chan_smag", (144, 80, 6), "PP/radix8x9", "PP/radix8x5"), ("chan_smag", (1536, 16, 4), "PP/radix8x3", "PP/" + R8R),
          ("chan_smag", (1280, 16, 4), "PP/radix8x5", "PP/" + R8R), ("chan_smag", (1152, 16, 4), "PP/radix8x9", "PP/" + R8R),
          ("chan_smag", (16, 768, 4), "PP/" + MIX, "PP/radix8x3"), ("chan_smag", (16, 640, 4), "PP/" + MIX, "PP/radix8x5"),
          ("chan_smag", (16, 576, 4), "PP/" + MIX, "PP/radix8x9"), ("chan_smag", (192, 96, 40), "PP/radix8x3", "PP/radix8x3"),      # z tile with the packed column
          ("duct_smag_wm", (96, 48, 12), "PP/radix8x3", "NN/radix8x3"), ("duct_smag_wm", (64, 80, 12), "PP/" + R8, "NN/radix8x5"),
          ("duct_smag_wm", (64, 72, 12), "PP/" + R8, "NN/radix8x9"), ("duct_smag_wm", (32, 768, 4), "PP/" + R8, "NN/radix8x3"),
          ("duct_smag_wm", (32, 640, 4), "PP/" + R8, "NN/radix8x5"),
          ("cavity_nnn", (96, 48, 8), "NN/radix8x3", "NN/radix8x3"), ("cavity_nnn", (160, 144, 8), "NN/radix8x5", "NN/radix8x9"),
          ("cavity_nnn", (144, 160, 8), "NN/radix8x9", "NN/radix8x5"), ("cavity_nnn", (1536, 16, 4), "NN/radix8x3", "NN/" + R8),
          ("cavity_nnn", (64, 576, 4), "NN/" + R8, "NN/radix8x9"),
          ("tgv_ppp", (96, 48, 16), "PP/radix8x3", "PP/radix8x3")]      # periodic z


def _solve(name, ng, xk, yk):
    """the body of test_poisson_solve (1e-11 on pp - mean(pp)) with the plan string asserted"""
    g, case = load_golden(name)
    case.ng[:] = ng
    if case.lwm.any() and ng[2] == 4:      # the duct's wall model plays no part in the solve, but its sampling height must lie above zc(1) = l(3)/8 (sanity.f90:224-231)
        case.hwm = 0.3
    o = Oracle(case, nthreads=8); h = _hot(case)
    sol = h.describe_plan()["solver"]
    assert sol.startswith(f"x:{xk},y:{yk},z:"), sol
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    dzf = o.grid()["dzf"][1:-1]
    rhs[1:-1, 1:-1, 1:-1] -= (rhs[1:-1, 1:-1, 1:-1] * dzf).sum() / (dzf.sum() * ng[0] * ng[1])     # compatible r.h.s.
    ref = rhs.copy(order="F"); o.solver(ref)
    h.set("pp", rhs); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    err = np.abs((a - a.mean()) - (b - b.mean())).max()
    print(name, ng, sol, "err/bar", err / (1e-11 * np.abs(b - b.mean()).max() + 1e-14 * abs(b.mean())))
    assert err < 1e-11 * np.abs(b - b.mean()).max() + 1e-14 * abs(b.mean()), (ng, err)
    h.close()


@pytest.mark.parametrize("name,ng,xk,yk", SOLVES)
def test_poisson_solve_odd_radix_lines(name, ng, xk, yk):
    _solve(name, ng, xk, yk)


@pytest.mark.parametrize("name,ng,xk,yk", [("chan_smag", (96, 48, 6), "PP/" + MIX, "PP/" + MIX), ("duct_smag_wm", (64, 80, 12), "PP/" + R8, "NN/" + MIX),
                                           ("cavity_nnn", (144, 160, 8), "NN/" + MIX, "NN/" + MIX)])
def test_poisson_solve_odd_radix_switched_off(name, ng, xk, yk, monkeypatch):
    """CALES_FFT_NO_ODD_RADIX: these lengths on the Stockham kernels, as before -- same bar"""
    monkeypatch.setenv("CALES_FFT_NO_ODD_RADIX", "1")
    _solve(name, ng, xk, yk)


@pytest.mark.parametrize("name,ng", [("chan_smag", (192, 48, 40)), ("chan_smag", (96, 128, 100)), ("chan_smag", (128, 96, 24)), ("duct_smag_wm", (192, 80, 24))])
def test_nyquist_packing_agrees_at_odd_radix_lines(name, ng, monkeypatch):
    """the body of test_nyquist_packing_agrees: modes 0 and n1/2 in one column against columns of their own, 1e-12; a direction counts as radix-8 with either family"""
    g, case = load_golden(name)
    case.ng[:] = ng
    rng = np.random.RandomState(11)
    rhs = np.zeros(tuple(x + 2 for x in ng), order="F"); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    rhs[1:-1, 1:-1, 1:-1] += (1. + 0.5 * np.cos(np.pi * np.arange(ng[0])))[:, None, None] * rng.rand(1, ng[1], ng[2])
    out = []
    for packed in (True, False):
        if not packed:
            monkeypatch.setenv("CALES_NO_NYQUIST_PACKING", "1")
        h = _hot(case)
        sol = h.describe_plan()["solver"]
        assert ("one_column" in sol) == packed, sol
        assert "radix8x" in sol and "mixed_radix" not in sol, sol
        h.set("pp", rhs); h.solver()
        a = h.get("pp")[1:-1, 1:-1, 1:-1]; out.append(a - a.mean()); h.close()
    print(name, ng, "err/bar", np.abs(out[0] - out[1]).max() / (1e-12 * np.abs(out[1]).max()))
    assert np.abs(out[0] - out[1]).max() < 1e-12 * np.abs(out[1]).max()


WRAPPED = {"x_ghost_columns": "wrapped", "fillps": "in_x_transform"}
STEPS = [("chan_dsmag", (192, 20, 12), dict(WRAPPED, projection="in_strain_rate_pass"), "x:PP/radix8x3,"),      # three x tiles
         ("chan_dsmag", (320, 12, 10), dict(WRAPPED, projection="in_strain_rate_pass"), "x:PP/radix8x5,"),      # five
         ("chan_smag", (96, 48, 12), {"fillps": "in_x_transform"}, "x:PP/radix8x3,y:PP/radix8x3,"),
         ("tgv_ppp", (96, 48, 16), {"fillps": "in_x_transform", "projection": "in_next_momentum_pass"}, "x:PP/radix8x3,y:PP/radix8x3,"),
         ("cavity_nnn", (96, 80, 12), {"fillps": "in_x_transform", "projection": "in_next_momentum_pass"}, "x:NN/radix8x3,y:NN/radix8x5,"),
         # the shipped wall-modelled channel at its own grid: fillps in the transform, but x ghost columns maintained and the correction in its own pass
         ("chan_smag_wm", (192, 72, 48), {"fillps": "in_x_transform", "x_ghost_columns": "maintained", "projection": "own_pass"}, "x:PP/radix8x3,y:PP/radix8x9,"),
         ("duct_smag_wm", (64, 80, 80), {"fillps": "in_x_transform"}, "x:PP/radix8,y:NN/radix8x5,")]


@pytest.mark.parametrize("name,ng,plan,solver", STEPS)
def test_time_steps_at_odd_radix_lines(name, ng, plan, solver):
    """the body and bars of test_time_steps (velocity 1e-9, pressure mean-free 1e-8, eddy viscosity 1e-7), two steps, with the plan the steps read"""
    from cales_amd.hotpath import initflow
    nsteps = 2
    g, case = load_golden(name)
    case.ng[:] = ng
    o = Oracle(case, nthreads=8); h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(1)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    assert abs(h.chkdt() / (2 * dt) - 1) < 1e-12
    for _ in range(nsteps):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    pl = h.describe_plan()
    assert pl["solver"].startswith(solver), pl
    for k, val in plan.items():
        assert pl[k].startswith(val), (k, pl)
    gu, gv, gw, gp, gvis = h.download()
    errs = [relerr(a, b) for a, b in ((gu, u), (gv, v), (gw, w))]
    ep = relerr(gp[1:-1, 1:-1, 1:-1] - gp[1:-1, 1:-1, 1:-1].mean(), p[1:-1, 1:-1, 1:-1] - p[1:-1, 1:-1, 1:-1].mean())
    print(name, ng, "u v w", errs, "p", ep, "visct", relerr(gvis, visct))
    for e, nm in zip(errs, "uvw"):
        assert e < 1e-9, nm
    assert ep < 1e-8
    assert relerr(gvis, visct) < 1e-7
    dg, do = h.chkdiv(), o.chkdiv(u, v, w)
    assert dg[1] < 20. * do[1] + 1e-14 and (dg[1] < 1e-11 or do[1] > 1e-11)
    h.close()


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "separate"])
def test_folded_strain_pass_against_reference_made_state_at_a_192_cell_row(folded, monkeypatch):
    """the body of test_folded_strain_pass_against_reference_made_state on the reference-made state at a row of three 64-cell tiles
    (tests/golden/lines, gen_golden_lines.py): same counters, same bars, x lines in the radix-3-first kernel"""
    if not folded:
        monkeypatch.setenv("CALES_UNFOLDED_CORREC", "1")
    g, case = load_golden("lines/chan_dsmag_x192")
    h = _hot(case)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    h.profile(True)
    h.step(float(g["dt"]))
    u, v, w, p, visct = h.download()
    h.profile(False); st = h.profile_stats()
    nfold, ncorr = st.get("correc_strain_filter_uvw", (0, 0.))[0], st.get("correc_updatep", (0, 0.))[0]
    assert (nfold, ncorr) == ((3, 0) if folded else (0, 3)), st
    pl = h.describe_plan()
    assert pl["solver"].startswith("x:PP/radix8x3,"), pl
    assert pl["projection"] == ("in_strain_rate_pass" if folded else "own_pass(correc+updatep)"), pl
    assert pl["x_ghost_columns"] == "wrapped" and pl["fillps"] == "in_x_transform" and pl["sgs"] == "dsmag_tiles(pair_fields)", pl
    assert pl["bulk_forcing"] == "in_correction(means_in_x_transform)", pl
    for a, k in zip((u, v, w), "uvw"):
        assert relerr(a, g["r3_s7_" + k]) < 1e-10, k
    pg = g["r3_s8_p"]
    assert relerr(p - p[1:-1, 1:-1, 1:-1].mean(), pg - pg[1:-1, 1:-1, 1:-1].mean()) < 1e-9
    assert relerr(visct, g["r3_s9_visct"]) < 1e-8
    assert np.abs(h.dpdl() - g["dpdl"]).max() < 1e-9 * max(1., np.abs(g["dpdl"]).max())
    assert h.chkdiv()[1] < 1e-12
    h.close()


@pytest.mark.parametrize("P", [2, 3])
def test_slab_ranks_at_a_192_cell_row(P):
    """emulated ranks on one GPU against the single-rank run, 1e-10 (tests/test_gpu_decomp.py): the mode-block layout with 96 packed mode columns"""
    from tests.test_gpu_decomp import test_slab_ranks_match_single_rank
    test_slab_ranks_match_single_rank("chan_dsmag", (192, 24, 16), P)


@pytest.mark.parametrize("P", [2, 3])
def test_slab_ranks_pipelined_exchange_at_a_192_cell_row(P, monkeypatch):
    """... and with the k-chunked exchange on the second stream, which both radix-8 families take (event-ordered emulation)"""
    from tests.test_gpu_decomp import test_slab_ranks_overlapped_event_ordered
    test_slab_ranks_overlapped_event_ordered("chan_dsmag", (192, 24, 16), P, monkeypatch)


def test_single_precision_odd_radix_lines():
    """the single-precision library at the bars of tests/test_gpu_single.py"""
    from tests.test_gpu_single import _check, _worker
    _check(_worker(["chan_dsmag:192x48x32:1", "cavity_nnn:96x80x16:1"]))

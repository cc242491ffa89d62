"""HIP path vs the CPU oracle on seeded inputs at sizes the oracle finishes in seconds: Poisson solve for
power-of-two and mixed-radix (2,3,5) line lengths and the three z closures, several full time steps of
each model, plus size-independent properties at a larger size (projection => div ~ 0, bulk velocity held)."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import DT_FACTORS, OPEN_SETS, F, load_golden, relerr
from tests.util import open_case as _open_case      # (tests/test_helmholtz_reference.py runs the same cases on the CPU)

pytestmark = pytest.mark.gpu


def _hot(case):
    from cales_amd.hotpath import HotPath
    if case.sgstype == "none" and case.cbcvel[0, 0, 0] != "P":      # see tests/test_gpu_golden.py
        case.cbcsgs[:, 0] = "D"
    return HotPath(case)


@pytest.mark.parametrize("name,ng", [("chan_smag", (32, 16, 12)), ("chan_smag", (48, 40, 24)), ("chan_smag", (64, 128, 8)),
                                     ("chan_smag", (512, 64, 6)), ("chan_smag", (60, 90, 10)), ("chan_smag", (2048, 16, 4)),
                                     ("tgv_ppp", (32, 32, 16)), ("tgv_ppp", (24, 20, 18)), ("halfchan_imp1d", (16, 1024, 4)),
                                     ("duct_smag_wm", (32, 64, 16)), ("duct_smag_wm", (24, 30, 12)), ("duct_smag_wm", (128, 256, 8)),
                                     ("cavity_nnn", (32, 16, 12)), ("cavity_nnn", (20, 36, 10)), ("cavity_nnn", (256, 128, 6)),
                                     # line lengths with factors 7, 11, 13 (direct-DFT butterflies)
                                     ("chan_smag", (28, 22, 10)), ("cavity_nnn", (52, 14, 8)), ("duct_smag_wm", (44, 26, 12)),
                                     # other prime factors (17, 19, 23, 37): run-time radix stage
                                     ("chan_smag", (34, 38, 10)), ("cavity_nnn", (46, 74, 8)), ("duct_smag_wm", (38, 34, 12)),
                                     # deep z: the in-LDS tridiagonal tile with 2, 4, 8, 16 planes per lane, partial last chunks; 512 planes of 129 / 513 complex modes: the persistent
                                     # form on the whole tiles, the classic one on the two columns left over
                                     ("chan_smag", (16, 8, 100)), ("chan_smag", (16, 8, 130)), ("cavity_nnn", (40, 8, 300)),
                                     ("chan_smag", (16, 4, 512)), ("chan_smag", (256, 8, 512)), ("chan_smag", (1024, 4, 512)), ("duct_smag_wm", (16, 8, 514)), ("chan_smag", (8, 4, 1024)),
                                     # 513..1024 planes of real x modes (16 planes per lane, one matrix per column): full, partial and nearly empty last chunks; odd column counts;
                                     # 1024 planes in whole 16-column tiles take the persistent form (k_gaussel_tile_p): one tile per block, and two (64 x 1024 x 1024)
                                     ("cavity_nnn", (16, 8, 1024)), ("cavity_nnn", (64, 4, 1024)), ("cavity_nnn", (64, 1024, 1024)), ("cavity_nnn", (40, 4, 700)), ("cavity_nnn", (24, 6, 520)), ("devchan_nd", (16, 8, 600)), ("cavity_nnn", (18, 4, 1000)),
                                     # periodic y lines of 16 ... 512 points: every first radix of the register-ended transform (8-2, 8-4, 8-8, 2-8-8, 4-8-8, 8-8-8)
                                     ("chan_smag", (16, 16, 6)), ("chan_smag", (16, 32, 6)), ("tgv_ppp", (16, 64, 8)), ("chan_smag", (16, 256, 4)), ("tgv_ppp", (32, 512, 4))])
def test_poisson_solve(name, ng):
    g, case = load_golden(name)
    case.ng[:] = ng
    o = Oracle(case, nthreads=8); h = _hot(case)
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    dzf = o.grid()["dzf"][1:-1]
    rhs[1:-1, 1:-1, 1:-1] -= (rhs[1:-1, 1:-1, 1:-1] * dzf).sum() / (dzf.sum() * ng[0] * ng[1])     # compatible r.h.s.
    ref = rhs.copy(order="F"); o.solver(ref)
    h.set("pp", rhs); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    # 1e-11 on pp - mean(pp); the round-off-defined zero mode (solver.f90:165) can be huge for periodic z
    err = np.abs((a - a.mean()) - (b - b.mean())).max()
    assert err < 1e-11 * np.abs(b - b.mean()).max() + 1e-14 * abs(b.mean()), (ng, err)
    h.close()


@pytest.mark.parametrize("name,ng", [("chan_smag", (64, 128, 8)), ("tgv_ppp", (32, 32, 16)), ("cavity_nnn", (256, 128, 6)), ("duct_smag_wm", (128, 256, 8)), ("chan_smag", (512, 64, 6))])
def test_poisson_solve_generic_transforms(name, ng, monkeypatch):
    """CALES_FFT_GENERIC: the mixed-radix Stockham kernels also for power-of-two lines (which otherwise take the radix-8 register kernels), same bar."""
    monkeypatch.setenv("CALES_FFT_GENERIC", "1")
    test_poisson_solve(name, ng)


@pytest.mark.parametrize("name,ng", [("chan_smag", (32, 16, 24)), ("cavity_nnn", (24, 20, 70)), ("halfchan_imp1d", (16, 16, 200)), ("cavity_nnn", (24, 20, 700))])
def test_tridiagonal_paths_agree(name, ng, monkeypatch):
    """the in-LDS substructured sweep (default on one rank) against the marching Thomas sweep (CALES_GAUSSEL_MARCH)"""
    g, case = load_golden(name)
    case.ng[:] = ng
    rng = np.random.RandomState(5)
    rhs = np.zeros(tuple(x + 2 for x in ng), order="F"); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    out = []
    for march in (False, True):
        if march:
            monkeypatch.setenv("CALES_GAUSSEL_MARCH", "1")
        h = _hot(case); h.set("pp", rhs); h.solver()
        a = h.get("pp")[1:-1, 1:-1, 1:-1]; out.append(a - a.mean()); h.close()
    assert np.abs(out[0] - out[1]).max() < 1e-11 * np.abs(out[1]).max()


@pytest.mark.parametrize("name,ng", [("chan_smag", (64, 16, 6)), ("chan_smag", (64, 32, 100)), ("chan_dsmag", (128, 64, 130)), ("chan_smag", (64, 16, 300)), ("chan_smag", (64, 16, 512)),
                                     ("chan_smag", (128, 16, 700)), ("chan_smag", (64, 16, 1024)), ("chan_smag", (512, 1024, 4)), ("halfchan_imp1d", (64, 64, 40)),
                                     # Neumann y (ducts): no pairing of rows, Re = mode 0 and Im = mode n1/2; the staged y kernel (32, 128 points) and k_fft_y16 (256)
                                     ("duct_smag_wm", (64, 32, 40)), ("duct_dsmag", (128, 128, 130)), ("duct_smag_wm", (128, 256, 24)), ("duct_dsmag_wm", (64, 16, 300))])
def test_nyquist_packing_agrees(name, ng, monkeypatch):
    """periodic x, periodic or Neumann y: the real x modes 0 and n1/2 sharing column 0 of the spectrum (default; k_gaussel_nyq separates them in the z solve by the
    Hermitian pairing of the y rows / by real and imaginary part) against columns of their own (CALES_NO_NYQUIST_PACKING) -- every chunking of the z tile, y lines of every first radix"""
    g, case = load_golden(name)
    case.ng[:] = ng
    rng = np.random.RandomState(11)
    rhs = np.zeros(tuple(x + 2 for x in ng), order="F"); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    # (content in the two packed modes in particular: a constant and the alternating row, modulated in y and z)
    rhs[1:-1, 1:-1, 1:-1] += (1. + 0.5 * np.cos(np.pi * np.arange(ng[0])))[:, None, None] * rng.rand(1, ng[1], ng[2])
    out = []
    for packed in (True, False):
        if not packed:
            monkeypatch.setenv("CALES_NO_NYQUIST_PACKING", "1")
        h = _hot(case)
        assert ("one_column" in h.describe_plan()["solver"]) == packed
        h.set("pp", rhs); h.solver()
        a = h.get("pp")[1:-1, 1:-1, 1:-1]; out.append(a - a.mean()); h.close()
    assert np.abs(out[0] - out[1]).max() < 1e-12 * np.abs(out[1]).max()


@pytest.mark.parametrize("name,ng,nsteps", [("tgv_ppp", (32, 24, 16), 5), ("chan_smag_wm", (32, 16, 16), 5), ("chan_dsmag", (32, 16, 16), 5),
                                            ("halfchan_imp1d", (16, 16, 16), 3), ("chan_smag", (24, 20, 12), 10),
                                            # tile kernels: partial tiles in x and y, several x tiles, k chunks, wall-modelled z faces
                                            ("chan_dsmag", (80, 20, 12), 3), ("tgv_dsmag_ppp", (72, 16, 40), 3), ("chan_dsmag_wm", (128, 30, 70), 2), ("chan_smag_wm", (96, 18, 40), 3),
                                            ("duct_smag_wm", (16, 24, 24), 4), ("cavity_nnn", (16, 16, 16), 5),
                                            # dynamic model in ducts: tile passes with the wall rule along y; partial y tiles, several x tiles, wall-model and no-slip walls
                                            ("duct_dsmag_wm", (80, 20, 24), 3), ("duct_dsmag", (72, 18, 20), 3), ("duct_dsmag", (16, 8, 12), 4), ("cavity_dsmag", (16, 16, 12), 3), ("devchan_nd", (32, 16, 16), 4), ("devchan_nd", (40, 18, 12), 3),
                                            # wall-model sampling height inside the first cell (index_wm = 1 / n): the wall model reads the ghost cells
                                            # of the last bounduvw, which have to survive the double-buffered velocity update
                                            ("duct_smag_wm", (16, 8, 24), 3), ("duct_smag_wm_imp1d", (50, 8, 76), 2), ("chan_smag_wm", (32, 16, 8), 3),
                                            # 3-D implicit diffusion (impdiff = 1): Helmholtz solves of u,v,w through the FFT solver
                                            ("couette_imp3d_ops", (16, 16, 16), 4), ("couette_imp3d_ops", (32, 20, 24), 3),
                                            # power-of-two rows with periodic x: cales_step leaves the x ghost columns alone until it returns and its kernels
                                            # wrap around (one full tile, two tiles, a row shorter than a tile; all ghost cells are compared at the end)
                                            ("chan_dsmag", (64, 20, 12), 3), ("chan_dsmag", (128, 12, 20), 2), ("chan_smag", (64, 18, 12), 3), ("chan_smag", (128, 10, 16), 2),
                                            ("chan_smag", (16, 12, 10), 3), ("tgv_dsmag_ppp", (64, 16, 24), 3), ("duct_dsmag", (64, 18, 20), 2), ("tgv_ppp", (128, 8, 8), 3),
                                            # static Smagorinsky duct WITHOUT wall model, power-of-two rows: the step leaves the x ghost columns alone and the
                                            # shear of the y walls (k_wall_shear_y) has to wrap around like every other reader; one and two x tiles
                                            ("duct_smag", (64, 16, 20), 3), ("duct_smag", (128, 12, 16), 2), ("duct_smag", (24, 18, 12), 3),
                                            # BASELINE configs[0] at its own size in FP64
                                            ("tgv_ppp", (64, 64, 64), 3)])
def test_time_steps(name, ng, nsteps, factors=None):
    """u,v,w <= 1e-9, p (mean removed) <= 1e-8 after the steps; divmax same order of magnitude. `factors` (not parametrized: for callers
    such as tests/test_gpu_variable_dt.py): step n is made with factors[n] * dt instead of dt"""
    from cales_amd.hotpath import initflow
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
    for n in range(nsteps):
        dtn = dt if factors is None else factors[n] * dt
        h.step(dtn); o.step(dtn, u, v, w, p, pp, visct)
    gu, gv, gw, gp, gvis = h.download()
    for a, b, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(a, b) < 1e-9, nm
    assert relerr(gp[1:-1, 1:-1, 1:-1] - gp[1:-1, 1:-1, 1:-1].mean(), p[1:-1, 1:-1, 1:-1] - p[1:-1, 1:-1, 1:-1].mean()) < 1e-8
    assert relerr(gvis, visct) < 1e-7
    dg, do = h.chkdiv(), o.chkdiv(u, v, w)
    # divergence after projection: round-off level, not worse than a decade above the oracle's (a smaller one is fine).
    # Triply periodic boxes whose n3 is not a power of two are the exception: initgrid's default-real arithmetic
    # (initgrid.f90:63) leaves dzf non-uniform at 1e-7, the singular Poisson problem is then incompatible and the reference
    # algorithm itself (restated by the oracle) stops at ~1e-9.
    assert dg[1] < 20. * do[1] + 1e-14 and (dg[1] < 1e-11 or do[1] > 1e-11)
    h.close()


# halfchan_imp1d (w has a Dirichlet top: n3 - 1 unknowns) at the n3 where the planes-per-lane rule of the in-LDS tile and its "do n3 planes fit" test switch:
# 128: 2 planes per lane for u, v and w; 129: 4 for u, v -- w's 128 unknowns take 2, whose tile cannot hold 129 planes: the shared-pivot column kernels;
# 130: 4 for all three; 257: 8 for u, v, the column kernels for w
HZ_GRIDS = [(16, 8, 128), (16, 8, 129), (16, 8, 130), (16, 8, 257)]


@pytest.mark.parametrize("name,ng", [("halfchan_imp1d", (16, 16, 16)), ("duct_smag_wm_imp1d", (16, 12, 12)), ("duct_smag_wm_imp1d", (64, 16, 20))] +
                                    [("halfchan_imp1d", ng) for ng in HZ_GRIDS])
def test_z_implicit_steps_with_a_changing_time_step(name, ng):
    """The z-only Helmholtz sweeps keep the coefficient tables of the (component, alpha) pairs they have seen (four per component; three alphas per step while
    dt stays): seven steps with five different time steps -- hits, misses and evictions -- against the oracle, which scales a, b, c anew for every sweep
    (main.f90:432-437)."""
    from cales_amd.hotpath import initflow
    g, case = load_golden(name); case.ng[:] = ng
    o = Oracle(case, nthreads=8); h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(4)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    for fac in DT_FACTORS:
        h.step(fac * dt); o.step(fac * dt, u, v, w, p, pp, visct)
    gu, gv, gw, gp, gvis = h.download()
    for a, b, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(a, b) < 1e-9, nm
    assert relerr(gvis, visct) < 1e-7
    h.close()


@pytest.mark.parametrize("alpha", [-1e-5, -1e-2])
@pytest.mark.parametrize("ivel", [1, 2, 3])
@pytest.mark.parametrize("ng", HZ_GRIDS)
def test_helmholtz_z_forms_against_the_oracle(ng, ivel, alpha):
    """cales_helmholtz_z in every form the z-only sweeps take (the in-LDS tile with 2, 4, 8 planes per lane; the shared-pivot column kernel where w's n3 planes
    do not fit its tile) against the oracle's updt_rhs_b_velz + solver_gaussel_z on the unknown planes, 1e-12 of the field maximum (the bar of the golden
    stage test of this operator; on the CPU the oracle and a LAPACK banded solve of these systems differ by 4.2e-15 at most). Then the table cache of the
    sweeps: the same alpha again (a hit), five other alphas (four slots per component: an eviction) and the first once more -- bit-identical each time."""
    g, case = load_golden("halfchan_imp1d"); case.ng[:] = ng
    o = Oracle(case, nthreads=8); h = _hot(case)
    k = "uvw"[ivel - 1]
    nz = ng[2] - (1 if ivel == 3 and case.cbcvel[1, 2, 2] == "D" else 0)
    rng = np.random.RandomState(100 * ivel + ng[2])
    q0 = o.zeros(); q0[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    ref = q0.copy(order="F"); o.updt_rhs_b_velz(ivel, alpha, ref); o.solver_gaussel_z(ivel, alpha, ref)

    def sweep(al):
        h.set(k, q0); h.helmholtz_z(ivel, al)
        return h.get(k)
    first = sweep(alpha)
    err = relerr(first[1:-1, 1:-1, 1:nz + 1], ref[1:-1, 1:-1, 1:nz + 1])
    print(ng, ivel, alpha, "relerr", err)
    assert err < 1e-12, (ng, ivel, alpha, err)
    assert np.array_equal(sweep(alpha), first), "table hit"
    for m in (2., 3., 5., 7., 11.):
        sweep(m * alpha)
    assert np.array_equal(sweep(alpha), first), "after an eviction"
    h.close()


@pytest.mark.parametrize("name,ng,nsteps", [("chan_dsmag", (32, 16, 16), 3), ("chan_smag", (64, 18, 12), 2), ("tgv_ppp", (32, 24, 16), 3)])
def test_time_steps_with_x_ghosts_kept(name, ng, nsteps, monkeypatch):
    """CALES_XGHOSTS_IN_STEP: every ghost-cell operator of cales_step fills the x ghost columns and the kernels read them (the form the operator-level
    entries always use) instead of wrapping around."""
    monkeypatch.setenv("CALES_XGHOSTS_IN_STEP", "1")
    test_time_steps(name, ng, nsteps)


_BOOL_SWITCHES = ["CALES_UNFUSED_RK", "CALES_UNFUSED_CORREC", "CALES_UNFOLDED_CORREC", "CALES_UNFOLDED_MOM", "CALES_LAZY_PROJECTION", "CALES_UNFUSED_FORCING", "CALES_UNFUSED_FILLPS", "CALES_UNFUSED_MEAN", "CALES_KEEP_LAST_RHS",
                  "CALES_GAUSSEL_MARCH", "CALES_NO_NYQUIST_PACKING", "CALES_DSMAG_XGHOSTS", "CALES_WIDE_OFFSETS",
                  "CALES_UNMERGED_BC", "CALES_XGHOSTS_IN_STEP",
                  "CALES_FFT_GENERIC", "CALES_HELMHOLTZ_Z_PER_COLUMN", "CALES_UNFUSED_IMP_RHS",
                  "CALES_DSMAG_REFERENCE_SEQUENCE", "CALES_SMAG_REFERENCE_SEQUENCE"]


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("name,ng", [("chan_dsmag", (32, 16, 16)), ("tgv_dsmag_ppp", (32, 16, 16)), ("chan_smag_wm", (32, 16, 12)), ("duct_smag_wm_imp1d", (16, 12, 12)),
                                     ("chan_smag", (64, 12, 10))])
def test_time_steps_with_switch_combinations(name, ng, seed, monkeypatch):
    """The run-time switches select alternative code paths one at a time in the other tests; here three to six of them at once, drawn with a fixed
    seed (the space of combinations cannot be enumerated: this samples it), against the oracle after two steps."""
    rng = np.random.RandomState(1000 + seed)
    chosen = rng.choice(_BOOL_SWITCHES, size=rng.randint(3, 7), replace=False)
    for k in chosen:
        monkeypatch.setenv(str(k), "1")
    if rng.rand() < 0.5:
        monkeypatch.setenv("CALES_KCHUNK", str(rng.randint(3, 9)))
    test_time_steps(name, ng, 2)


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("name,ng,hwm", [("chan_smag_wm", (32, 16, 12), None), ("chan_smag_wm", (64, 16, 12), None), ("chan_dsmag_wm", (32, 16, 16), None),
                                         ("duct_smag_wm", (16, 24, 24), None), ("duct_smag_wm", (16, 8, 24), "first_cell"), ("duct_dsmag_wm", (16, 24, 20), None)])
def test_deferred_forcing_with_wall_model_equals_the_separate_pass(name, ng, hwm, P, monkeypatch):
    """Two things cales_step does with a wall model, against the reference's full sequence: (1) the bounduvw between bulk_forcing and fillps leaves the wall-model
    update and the tangential ghost cells of the wall-model faces alone -- the bounduvw after correc rewrites both before anything has read them (main.f90:492-501;
    not when the sampling height lies inside the first cell, "first_cell": the second update then interpolates with the ghost cell the first one set, and nothing
    is skipped); (2) with that update gone nothing samples the velocity between bulk_forcing and correc, so the forcing increment is added by the correction pass
    (one whole-field pass less). Against CALES_UNFUSED_FORCING (mom.f90:311-335 as its own kernel, the skip still on) and against CALES_UNMERGED_BC (every ghost-cell
    launch and both wall-model updates of the reference, no deferral) to round-off, from an initial field at HALF the target bulk velocity so that the first
    increment is of order one. One rank and two slabs."""
    from cales_amd.hotpath import HotPath, initflow
    g, case = load_golden(name)
    case.ng[:] = ng
    # ("first_cell": with eight cells across the duct's 2 x 2 section the default sampling height lies inside the first cell -- index_wm = 1 / n, the
    #  interpolation reaches the ghost cells of the last bounduvw)
    u0 = [0.5 * a for a in initflow(case)[:3]] + [initflow(case)[3]]
    rng = np.random.RandomState(3)
    for a in u0[:3]:
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)

    def run():
        if P == 1:
            h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.25 * h.chkdt()
            for _ in range(3):
                h.step(dt)
            out = h.download(); h.close()
            return out
        from cales_amd.decomp import run_loopback

        def body(h, r):
            h.upload_global(*u0); h.startup(); dt = 0.25 * h.chkdt()
            for _ in range(3):
                h.step(dt)
            return h.download()
        res = run_loopback(case, P, body)
        return [np.concatenate([res[r][q][:, 1:-1, :] for r in range(P)], axis=1) for q in range(5)]
    a = run()
    monkeypatch.setenv("CALES_UNFUSED_FORCING", "1")
    b = run()
    monkeypatch.delenv("CALES_UNFUSED_FORCING"); monkeypatch.setenv("CALES_UNMERGED_BC", "1")
    c_ = run()
    for other, what in ((b, "separate forcing pass"), (c_, "full reference sequence")):
        for x, y, nm in zip(a, other, "uvwps"):
            assert relerr(x, y) < (1e-12 if nm in "uvw" else 1e-10), (what, nm)


@pytest.mark.parametrize("name,ng", [("chan_dsmag", (32, 16, 16)), ("chan_dsmag", (64, 20, 12)), ("duct_dsmag", (16, 12, 12))])
def test_time_steps_dsmag_with_inhomogeneous_sgs_bc_values(name, ng, monkeypatch):
    """Non-zero boundary VALUES of the eddy viscosity (bcsgs, src/param.f90:66; boundp(visct) with cbcsgs = 'D': ghost = 2 bc - visct(1)): the dynamic
    model's tile path then writes visct = max(|S| <LM>/<MM>, 0) as a field (k_dsmag_final) instead of keeping |S| and the plane coefficients -- the lazy
    form needs ghost values that scale with their plane. The only trigger of that form since the CALES_DSMAG_EAGER switch went (round 5)."""
    g, case = load_golden(name)
    orig = load_golden

    def patched(nm):
        g2, c2 = orig(nm); c2.bcsgs[:, 2] = (2e-4, 3e-4)
        return g2, c2
    monkeypatch.setattr("tests.test_gpu_vs_oracle.load_golden", patched)
    test_time_steps(name, ng, 2)


def _two_steps(case, ng, seed=7):
    from cales_amd.hotpath import initflow
    rng = np.random.RandomState(seed)
    o = Oracle(case, nthreads=8); h = _hot(case)
    u, v, w, p = initflow(case)
    for x in (u, v, w):
        x[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    for _ in range(2):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    gu, gv, gw, gp, _ = h.download()
    h.close()
    return (gu, gv, gw, gp), (u, v, w, p)


# triply periodic boxes whose n3 is not a power of two: the two sizes the fuzzers flagged (tools/fuzz_sizes.py, tools/fuzz_tiny.py) and two more
TRIPERIODIC_ODD = [(10, 6, 12), (46, 74, 15), (24, 20, 18), (16, 12, 9)]


@pytest.mark.parametrize("ng", TRIPERIODIC_ODD)
def test_triperiodic_reference_null_mode(ng, monkeypatch):
    """CALES_KEEP_NULL_MODE=1 is the reference-identical path of singular pressure problems: the zero-eigenvalue column goes through
    gaussel_periodic / dgtsv_homebrewed in the reference's own operation order, one rounding per operation (k_null_column), +eps pivots
    included. On these grids the reference's pressure is C + p' with C = 1e4..1e6 (a numerator of 1e-8 over a pivot of +-eps: the sign hangs on
    the last bit of the sequential elimination). The device reproduces C (1e-4; every other order of operations gives another constant, even
    another sign) and p' to the accuracy to which the reference algorithm defines it: 100 eps |C| / range(p'), the bound two CPU evaluations of
    the same algorithm with different transforms meet (tests/test_oracle_solver.py::test_triperiodic_reference_solution_is_defined_only_to_eps_times_its_constant).
    Two time steps then agree to 1e-8 of the velocity scale (the same sensitivity times dt / dx), where well-posed cases reach 1e-12."""
    from tests.util import perturbed_tgv_rhs
    monkeypatch.setenv("CALES_KEEP_NULL_MODE", "1")
    g, case = load_golden("tgv_ppp"); case.ng[:] = ng
    o = Oracle(case, nthreads=8); h = _hot(case)
    pp = perturbed_tgv_rhs(o, case)[0]
    ref = pp.copy(order="F"); o.solver(ref)
    h.set("pp", pp); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    h.close()
    C = b.mean(); unit = np.finfo(float).eps * abs(C) / np.ptp(b - C)
    assert abs(C) > 1e4 and abs(a.mean() - C) < 1e-4 * abs(C), (a.mean(), C)
    d = np.abs((a - a.mean()) - (b - C)).max() / np.abs(b - C).max()
    assert d < 100. * unit, (d, unit)
    # the null column itself (plane means): the reference's round-off pattern C (p2 - 1) along z is reproduced, not just its mean
    za, zb = a.mean(axis=(0, 1)), b.mean(axis=(0, 1))
    assert np.abs((za - za.mean()) - (zb - zb.mean())).max() < 20. * np.finfo(float).eps * abs(C)
    (gu, gv, gw, gp), (u, v, w, p) = _two_steps(case, ng)
    for x, y, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(x, y) < 1e-8, (nm, relerr(x, y))
    ma, mb = gp[1:-1, 1:-1, 1:-1].mean(), p[1:-1, 1:-1, 1:-1].mean()
    assert abs(ma - mb) < 1e-3 * abs(mb), (ma, mb)      # six solves later the accumulated constant still agrees


def test_triperiodic_reference_null_mode_well_posed(monkeypatch):
    """... and where the grid arithmetic is exact (n3 a power of two) the same switch meets the ordinary bar."""
    monkeypatch.setenv("CALES_KEEP_NULL_MODE", "1")
    g, case = load_golden("tgv_ppp"); case.ng[:] = (16, 16, 16)
    (gu, gv, gw, gp), (u, v, w, p) = _two_steps(case, (16, 16, 16))
    for x, y in ((gu, u), (gv, v), (gw, w)):
        assert relerr(x, y) < 1e-13
    assert relerr(gp - gp[1:-1, 1:-1, 1:-1].mean(), p - p[1:-1, 1:-1, 1:-1].mean()) < 1e-12


@pytest.mark.parametrize("ng", TRIPERIODIC_ODD[:2])
def test_triperiodic_default_pins_the_null_mode(ng):
    """The default takes the member p(n3) = 0 of the singular column instead: no round-off-defined constant, and a pressure whose accuracy does
    not depend on one. Measured here: the device's mean pressure stays O(1) where the reference algorithm's (the oracle's) is >= 1e3; the
    velocities of the two differ by no more than the reference's own sensitivity to its constant (1e-8 of the velocity scale, see above); the
    device's divergence after projection is not worse than the oracle's."""
    g, case = load_golden("tgv_ppp"); case.ng[:] = ng
    (gu, gv, gw, gp), (u, v, w, p) = _two_steps(case, ng)
    assert abs(gp[1:-1, 1:-1, 1:-1].mean()) < 1. and abs(p[1:-1, 1:-1, 1:-1].mean()) > 1e3
    errs = [relerr(a, b) for a, b in ((gu, u), (gv, v), (gw, w))]
    assert max(errs) < 1e-8, errs
    o = Oracle(case, nthreads=4)
    assert o.chkdiv(gu, gv, gw)[1] <= 2. * o.chkdiv(u, v, w)[1] + 1e-14


@pytest.mark.parametrize("ng", [(74, 52, 26), (20, 58, 12), (76, 46, 19), (46, 74, 15), (16, 32, 48)])
@pytest.mark.parametrize("keep", [0, 1], ids=["pinned", "reference_null_mode"])
def test_triperiodic_within_the_reference_algorithms_own_sensitivity(ng, keep, monkeypatch):
    """Sizes the size fuzzer flagged at 1e-8..3e-8 (n3 not a power of two). The yardstick is the reference algorithm itself: how far ITS two-step
    result moves when the initial field moves by one unit in the last place (tests/util.py one_ulp_sensitivity; 2e-8 at 74x52x26, 1e-15 for
    well-posed boxes, tests/test_oracle_solver.py) plus the digits its round-off-defined pressure constant costs (tests/util.py triperiodic_bounds).
    The device -- default member p(n3) = 0 and CALES_KEEP_NULL_MODE alike -- stays within that, and its divergence after projection is not worse
    than the oracle's."""
    from tests.util import one_ulp_sensitivity
    if keep:
        monkeypatch.setenv("CALES_KEEP_NULL_MODE", "1")
    g, case = load_golden("tgv_ppp"); case.ng[:] = ng
    sens, (u, v, w, p, dt) = one_ulp_sensitivity(case, 2, seed=3)
    from cales_amd.hotpath import initflow
    h = _hot(case)
    u0, v0, w0, p0 = initflow(case)
    rng = np.random.RandomState(3)
    for a in (u0, v0, w0):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    h.upload(u0, v0, w0, p0); h.startup()
    for _ in range(2):
        h.step(dt)
    gu, gv, gw, gp, gvis = h.download()
    # (16x32x48: the algorithm is insensitive to the last place of its input there, 1e-15, but its constant is 4e5 -- the second term of the bound:
    #  the digits such a constant costs, relative to the 0.01 of the w component of this flow)
    from tests.util import triperiodic_bounds
    bounds = triperiodic_bounds(case, (u, v, w), p, dt, 2, sens)
    for a, b, bd, nm in ((gu, u, bounds[0], "u"), (gv, v, bounds[1], "v"), (gw, w, bounds[2], "w")):
        assert relerr(a, b) < bd, (nm, relerr(a, b), bd, sens)
    assert max(bounds) < 1e-5
    o = Oracle(case, nthreads=4)
    assert h.chkdiv()[1] <= 2. * o.chkdiv(u, v, w)[1] + 1e-14
    h.close()


def test_projection_properties_at_size():
    """256x128x128 wall-modelled channel (BASELINE.json configs[1]): 3 steps, divergence ~ round-off, bulk velocity held."""
    import bench
    from cales_amd.hotpath import initflow
    g, case = load_golden("chan_smag_wm")
    case.ng[:] = (256, 128, 128)
    h = _hot(case)
    h.upload(*initflow(case)); h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(3):
        h.step(dt)
    divtot, divmax = h.chkdiv()
    assert divmax < 5e-12 and np.isfinite(divtot)
    assert abs(h.bulk_mean("u", "f") - 1.0) < 1e-12
    h.close()


def test_bench_config_properties_full_size():
    """BASELINE.json's metric configuration itself (512^3 channel, dynamic Smagorinsky, bulk forcing; bench.py's case file):
    after two steps the projected field is divergence-free to round-off, the bulk velocity is held, the eddy viscosity is
    finite and non-negative; the Poisson solve satisfies L_h(solve(r)) = r on sampled planes."""
    import bench
    from cales_amd.hotpath import HotPath, initflow
    case = bench.channel_case((512, 512, 512), "dsmag")
    h = HotPath(case)
    h.upload(*initflow(case)); h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    divtot, divmax = h.chkdiv()
    assert divmax < 1e-11 and np.isfinite(divtot)
    assert abs(h.bulk_mean("u", "f") - 1.0) < 1e-12
    visct = h.get("visct")[1:-1, 1:-1, 1:-1]
    assert visct.min() >= 0. and np.isfinite(visct).all()
    del visct
    # discrete Laplacian of the solution == right-hand side (interior planes of a few y rows; x periodic, z Neumann handled by the ghost cells)
    rng = np.random.RandomState(7)
    rhs = np.zeros((514, 514, 514), order="F"); rhs[1:-1, 1:-1, 1:-1] = rng.rand(512, 512, 512) - 0.5
    from oracle.oracle import Oracle
    small = bench.channel_case((8, 8, 512), "dsmag"); dzf = Oracle(small).grid()["dzf"][1:-1]; dzc = Oracle(small).grid()["dzc"]
    rhs[1:-1, 1:-1, 1:-1] -= (rhs[1:-1, 1:-1, 1:-1] * dzf).sum() / (dzf.sum() * 512 * 512)
    h.set("pp", rhs); h.solver(); h.boundp("pp", 0)
    p = h.get("pp")
    dxi, dyi = 512 / case.l[0], 512 / case.l[1]
    for j in (1, 200, 512):
        c = p[1:-1, j, 1:-1]
        lap = ((p[2:, j, 1:-1] - 2 * c + p[:-2, j, 1:-1]) * dxi ** 2 + (p[1:-1, j + 1, 1:-1] - 2 * c + p[1:-1, j - 1, 1:-1]) * dyi ** 2 +
               ((p[1:-1, j, 2:] - c) / dzc[1:-1] - (c - p[1:-1, j, :-2]) / dzc[:-2]) / dzf)
        assert np.abs(lap - rhs[1:-1, j, 1:-1]).max() < 1e-9 * np.abs(lap).max()
    h.close()


@pytest.mark.parametrize("bx", ["ND", "DN", "DD"])
@pytest.mark.parametrize("ng", [(32, 16, 12), (20, 36, 10), (128, 64, 8), (52, 14, 8)])
def test_poisson_solve_open_x(bx, ng):
    """Pressure Dirichlet on one or both x faces (inflow/outflow, examples/dns/developing_duct): RODFT10/01, REDFT11, RODFT11
    in x (fft.f90:192-245) with Neumann-Neumann y and z."""
    g, case = load_golden("cavity_nnn")
    case.ng[:] = ng
    for side in (0, 1):
        case.cbcpre[side, 0] = bx[side]
        case.cbcvel[side, 0, :] = "N" if bx[side] == "D" else "D"       # sanity.f90:150-170: velocity N where the pressure is D
        case.bcvel[side, 0, :] = 0.
    o = Oracle(case, nthreads=8); h = _hot(case)
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    ref = rhs.copy(order="F"); o.solver(ref)
    h.set("pp", rhs); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    assert np.abs(a - b).max() < 1e-11 * np.abs(b).max(), (bx, ng)      # non-singular: no mean to remove
    h.close()


def test_time_steps_inflow_outflow_duct():
    """examples/dns/developing_duct BCs (inflow u = 1 at x = 0, outflow with Dirichlet pressure at x = l, walls in y and z):
    REDFT11 in x, REDFT10/01 in y; several steps against the oracle."""
    from cales_amd.hotpath import initflow
    g, case = load_golden("cavity_nnn")
    case.ng[:] = (32, 16, 12)
    case.cbcpre[:, 0] = ["N", "D"]
    case.cbcvel[0, 0, :] = "D"; case.cbcvel[1, 0, :] = "N"
    case.bcvel[:] = 0.; case.bcvel[0, 0, 0] = 1.                     # u = 1 on the inflow face, lid at rest
    o = Oracle(case, nthreads=8); h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(5)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*case.ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    assert abs(h.chkdt() / (2 * dt) - 1) < 1e-12
    for _ in range(4):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    gu, gv, gw, gp, _ = h.download()
    for a, b, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(a, b) < 1e-9, nm
    assert relerr(gp[1:-1, 1:-1, 1:-1], p[1:-1, 1:-1, 1:-1]) < 1e-8            # Dirichlet pressure: no free constant
    assert h.chkdiv()[1] < 1e-11
    h.close()


@pytest.mark.parametrize("bx", ["ND", "NN", "DN", "DD"])
@pytest.mark.parametrize("ng", [(32, 16, 12), (20, 30, 10), (64, 128, 8), (28, 22, 10)])
def test_poisson_solve_open_x_periodic_y(bx, ng):
    """examples/dns/developing_channel: non-periodic x with PERIODIC y -- the pairs of real x modes have different eigenvalues
    and are separated through the Hermitian symmetry of their y spectra (k_gaussel_herm)."""
    g, case = load_golden("chan_smag")
    case.ng[:] = ng
    for side in (0, 1):
        case.cbcpre[side, 0] = bx[side]
        case.cbcvel[side, 0, :] = "N" if bx[side] == "D" else "D"
        case.bcvel[side, 0, :] = 0.
    case.cbcsgs[:, 0] = "D"                                     # sanity.f90:191-203
    case.is_forced[:] = False; case.sgstype = "none"; case.lwm[:] = 0
    o = Oracle(case, nthreads=8); h = _hot(case)
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    if bx == "NN":
        dzf = o.grid()["dzf"][1:-1]
        rhs[1:-1, 1:-1, 1:-1] -= (rhs[1:-1, 1:-1, 1:-1] * dzf).sum() / (dzf.sum() * ng[0] * ng[1])     # singular problem: compatible r.h.s.
    ref = rhs.copy(order="F"); o.solver(ref)
    h.set("pp", rhs); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    if bx == "NN":
        a = a - a.mean(); b = b - b.mean()
    assert np.abs(a - b).max() < 1e-11 * np.abs(b).max(), (bx, ng)
    h.close()


@pytest.mark.parametrize("by", ["DD", "ND", "DN"])
@pytest.mark.parametrize("bx", ["NN", "DD", "ND", "PP"])
@pytest.mark.parametrize("ng", [(32, 16, 12), (20, 36, 10), (64, 128, 8), (28, 22, 10)])
def test_poisson_solve_open_y(bx, by, ng):
    """Pressure Dirichlet on one or both y faces (RODFT10/01: the Neumann-Neumann kernel on sign-alternated rows, reversed eigenvalues;
    REDFT11 / RODFT11: k_fft_y4) combined with Neumann or open x faces; also three steps of such a box against the oracle."""
    g, case = load_golden("cavity_nnn")
    case.ng[:] = ng
    for d, pair in ((0, bx), (1, by)):
        for side in (0, 1):
            case.cbcpre[side, d] = pair[side]
            case.cbcvel[side, d, :] = "P" if pair[side] == "P" else ("N" if pair[side] == "D" else "D")
            case.cbcsgs[side, d] = "P" if pair[side] == "P" else "D"
            case.bcvel[side, d, :] = 0.
    o = Oracle(case, nthreads=8); h = _hot(case)
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    ref = rhs.copy(order="F"); o.solver(ref)
    h.set("pp", rhs); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    assert np.abs(a - b).max() < 1e-11 * np.abs(b).max(), (bx, ng)
    # a few time steps from a smooth divergence-free-ish start
    from cales_amd.hotpath import initflow
    u, v, w, p = initflow(case)
    for q in (u, v, w):
        q[1:-1, 1:-1, 1:-1] += 0.05 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.25 * o.chkdt(visct, u, v, w)
    for _ in range(3):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    gu, gv, gw, gp, _ = h.download()
    for x, y, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(x, y) < 1e-9, nm
    assert relerr(gp[1:-1, 1:-1, 1:-1], p[1:-1, 1:-1, 1:-1]) < 1e-8
    h.close()


@pytest.mark.parametrize("bxy", [("NN", "NN"), ("DD", "NN"), ("ND", "DD"), ("NN", "DD")])
@pytest.mark.parametrize("ng", [(32, 16, 12), (20, 36, 10), (28, 22, 16)])
def test_poisson_solve_walls_xy_periodic_z(bxy, ng):
    """A duct along z: non-periodic x and y with PERIODIC z (cyclic tridiagonal closure, solver.f90:124-133, on the real x modes)."""
    g, case = load_golden("cavity_nnn")
    case.ng[:] = ng
    for d, pair in ((0, bxy[0]), (1, bxy[1])):
        for side in (0, 1):
            case.cbcpre[side, d] = pair[side]
            case.cbcvel[side, d, :] = "N" if pair[side] == "D" else "D"
            case.bcvel[side, d, :] = 0.
    case.cbcpre[:, 2] = "P"; case.cbcvel[:, 2, :] = "P"; case.cbcsgs[:, 2] = "P"; case.bcvel[:, 2, :] = 0.
    case.gtype = 1; case.gr = 0.                                       # periodic z: uniform grid
    o = Oracle(case, nthreads=8); h = _hot(case)
    rng = np.random.RandomState(sum(ng))
    rhs = o.zeros(); rhs[1:-1, 1:-1, 1:-1] = rng.rand(*ng) - 0.5
    singular = bxy == ("NN", "NN")
    if singular:
        rhs[1:-1, 1:-1, 1:-1] -= rhs[1:-1, 1:-1, 1:-1].mean()
    ref = rhs.copy(order="F"); o.solver(ref)
    h.set("pp", rhs); h.solver()
    a = h.get("pp")[1:-1, 1:-1, 1:-1]; b = ref[1:-1, 1:-1, 1:-1]
    if singular:
        a = a - a.mean(); b = b - b.mean()
    assert np.abs(a - b).max() < 1e-11 * np.abs(b).max() + (1e-14 * abs(ref[1:-1, 1:-1, 1:-1].mean()) if singular else 0.), (bxy, ng)
    h.close()


@pytest.mark.parametrize("name,ng", [("chan_dsmag", (32, 16, 12)), ("chan_smag_wm", (40, 18, 20)), ("cavity_nnn", (20, 36, 10)), ("tgv_ppp", (24, 20, 18))])
def test_plane_statistics(name, ng):
    """cales_out1d_single_point_chan (27 plane sums of output.f90:509-700) against the oracle's restatement after two steps."""
    from cales_amd.hotpath import initflow
    g, case = load_golden(name)
    case.ng[:] = ng
    o = Oracle(case, nthreads=8); h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(3)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.05 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    gu, gv, gw, gp, gvis = h.download()
    ref = o.stats_chan(*(F(a) for a in (gu, gv, gw, gp, gvis)))
    got = h.stats_chan()
    # sums of signed terms: relative to the largest plane value of the statistic, plus the round-off of plane sums that cancel to ~0
    tol = 1e-12 * np.abs(ref).max(axis=1, keepdims=True) + 1e-13
    assert (np.abs(got - ref) <= tol).all(), np.argwhere(np.abs(got - ref) > tol)[:5]
    h.close()


@pytest.mark.parametrize("name,ng", [("chan_dsmag", (32, 16, 12)), ("chan_smag_wm", (40, 18, 20)), ("cavity_nnn", (20, 36, 10))])
def test_plane_budgets_and_leakage(name, ng):
    """cales_out1d_chan_budgets (38 + 6 plane measures of output.f90:700-1055) against the numpy restatement oracle/stats_np.py"""
    from cales_amd.hotpath import initflow
    from oracle import stats_np
    g, case = load_golden(name)
    case.ng[:] = ng
    o = Oracle(case); h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(4)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.05 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    gu, gv, gw, gp, _ = h.download()
    gr = o.grid(); dx, dy = float(case.l[0]) / ng[0], float(case.l[1]) / ng[1]
    rb = stats_np.budget_terms(gu, gv, gw, gp, dx, dy, gr["dzc"], gr["dzf"], float(case.l[0]), float(case.l[1]))
    rl = stats_np.leakage_terms(gu, gv, gw, dx, dy, gr["dzf"], float(case.l[0]), float(case.l[1]))
    bud, leak = h.stats_chan_budgets()
    for got, ref in ((bud, rb), (leak, rl)):
        tol = 1e-12 * np.abs(ref).max(axis=1, keepdims=True) + 1e-12 * max(np.abs(gu).max() * ng[0] / float(case.l[0]), 1.) ** 2
        assert (np.abs(got - ref) <= tol).all(), np.argwhere(np.abs(got - ref) > tol)[:5]
    h.close()


@pytest.mark.parametrize("name,ng", [("cavity_nnn", (32, 16, 12)), ("cavity_nnn", (20, 36, 10)), ("duct_smag_wm", (16, 24, 20))])
@pytest.mark.parametrize("ivel", [1, 2, 3])
def test_helmholtz_3d_with_walls(name, ng, ivel):
    """cales_helmholtz (3-D implicit diffusion) in boxes with no-slip walls in x and/or y: RODFT00 along the component, RODFT10/01
    across it (k_dst1, generic kernels), against the oracle's generalised o_solver_helmholtz (operator-identity tested on the CPU)."""
    g, case = load_golden(name)
    case.ng[:] = ng; case.impdiff = 1
    case.lwm[:] = 0; case.sgstype = "none"; case.bcvel[:] = 0.
    if name.startswith("duct"):
        case.cbcsgs[:] = np.where(case.cbcvel[:, :, 0] == "P", "P", "D")
    o = Oracle(case, nthreads=4); h = _hot(case)
    nn = list(ng); 
    if case.cbcvel[0, ivel - 1, ivel - 1] == "D":
        nn[ivel - 1] -= 1
    rng = np.random.RandomState(20 + ivel)
    rhs = o.zeros(); rhs[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1] = rng.rand(*nn) - 0.5
    alpha = -0.21
    ref = rhs.copy(order="F"); o.solver_helmholtz(ivel, alpha, ref)
    h.set("uvw"[ivel - 1], rhs); h.helmholtz(ivel, alpha)
    got = h.get("uvw"[ivel - 1])
    a = got[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1]; b = ref[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1]
    assert np.abs(a - b).max() < 1e-12 * np.abs(b).max(), (name, ng, ivel)
    h.close()


@pytest.mark.imp3d_open
@pytest.mark.parametrize("xset,yset,ng", OPEN_SETS)
@pytest.mark.parametrize("ivel", [1, 2, 3])
def test_helmholtz_3d_open_boundaries(xset, yset, ng, ivel):
    """cales_helmholtz with open boundaries / inflow profiles / moving side walls in x and y: every BC pair of find_fft (fft.f90:192-245) for
    the component's own direction (face-centred: REDFT00, RODFT00, REDFT10/01, RODFT01/10) and across it (the pressure's kinds), with the
    boundary terms of the x and y faces (bc_rhs / updt_rhs_b, bound.f90:501-603), against the oracle's restatement of the same."""
    case = _open_case(xset, yset, ng)
    o = Oracle(case, nthreads=4); h = _hot(case)
    nn = list(ng)
    for d in range(2):
        if d == ivel - 1 and case.cbcvel[0, d, ivel - 1] == "D" and case.cbcvel[1, d, ivel - 1] == "D":
            nn[d] -= 1
    if ivel == 3:
        nn[2] -= 1
    rng = np.random.RandomState(30 + ivel)
    rhs = o.zeros(); rhs[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1] = rng.rand(*nn) - 0.5
    alpha = -0.21
    ref = rhs.copy(order="F"); o.updt_rhs_b_vel(ivel, alpha, ref); o.solver_helmholtz(ivel, alpha, ref)
    h.set("uvw"[ivel - 1], rhs); h.helmholtz(ivel, alpha)
    got = h.get("uvw"[ivel - 1])
    a = got[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1]; b = ref[1:nn[0] + 1, 1:nn[1] + 1, 1:nn[2] + 1]
    assert np.abs(a - b).max() < 1e-12 * np.abs(b).max(), (xset, yset, ng, ivel)
    h.close()


@pytest.mark.imp3d_open
@pytest.mark.parametrize("xset,yset,ng", [OPEN_SETS[0], OPEN_SETS[1], OPEN_SETS[4], OPEN_SETS[7]])
def test_time_steps_imp3d_open(xset, yset, ng):
    """Three steps of an inflow / outflow box with 3-D implicit diffusion (impdiff = 1): momentum split, boundary terms of the inflow faces,
    Helmholtz solves with the open-boundary transform kinds, pressure solve (REDFT11 / RODFT11), against the oracle."""
    case = _open_case(xset, yset, ng)
    o = Oracle(case, nthreads=8); h = _hot(case)
    rng = np.random.RandomState(4)
    u, v, w, p = (o.zeros() for _ in range(4))
    for a, m in ((u, 0.7), (v, 0.3), (w, 0.)):
        a[1:-1, 1:-1, 1:-1] = m + 0.05 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.4 * o.chkdt(visct, u, v, w)
    for _ in range(3):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    gu, gv, gw, gp, _ = h.download()
    for a, b, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(a, b) < 1e-9, nm
    assert relerr(gp[1:-1, 1:-1, 1:-1], p[1:-1, 1:-1, 1:-1]) < 1e-8
    h.close()


@pytest.mark.parametrize("name,ng,sgs", [("cavity_nnn", (32, 16, 12), "none"), ("cavity_nnn", (20, 36, 10), "none"), ("duct_smag_wm", (16, 24, 20), "smag")])
def test_time_steps_imp3d_with_walls(name, ng, sgs):
    """Three steps with 3-D implicit diffusion (impdiff = 1) in a lid-driven cavity and a duct without wall model: momentum split,
    Helmholtz solves of u,v,w with the wall transform kinds, boundary r.h.s. of the moving lid, full-Laplacian pressure update."""
    from cales_amd.hotpath import initflow
    g, case = load_golden(name)
    case.ng[:] = ng; case.impdiff = 1; case.lwm[:] = 0; case.sgstype = sgs
    if name.startswith("duct"):
        case.cbcsgs[:] = np.where(case.cbcvel[:, :, 0] == "P", "P", "D")
    o = Oracle(case, nthreads=8); h = _hot(case)
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(2)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    for _ in range(3):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    gu, gv, gw, gp, _ = h.download()
    for a, b, nm in ((gu, u, "u"), (gv, v, "v"), (gw, w, "w")):
        assert relerr(a, b) < 1e-9, nm
    a = gp[1:-1, 1:-1, 1:-1]; b = p[1:-1, 1:-1, 1:-1]
    assert relerr(a - a.mean(), b - b.mean()) < 1e-8
    assert h.chkdiv()[1] < 1e-11
    h.close()


def _laplacian_identity(h, case, grid, rng, planes, tol=1e-9):
    """L_h(solve(r)) == r on the sampled y rows, for Neumann or periodic pressure BCs (ghost cells from boundp)."""
    n1, n2, n3 = (int(x) for x in case.ng)
    rhs = np.zeros((n1 + 2, n2 + 2, n3 + 2), order="F")
    rhs[1:-1, 1:-1, 1:-1] = rng.rand(n1, n2, n3) - 0.5
    dzf, dzc = grid["dzf"][1:-1], grid["dzc"]
    rhs[1:-1, 1:-1, 1:-1] -= (rhs[1:-1, 1:-1, 1:-1] * dzf).sum() / (dzf.sum() * n1 * n2)      # compatible r.h.s. (singular problem)
    h.set("pp", rhs); h.solver(); h.boundp("pp", 0)
    p = h.get("pp")
    dxi, dyi = n1 / case.l[0], n2 / case.l[1]
    for j in planes:
        c = p[1:-1, j, 1:-1]
        lap = ((p[2:, j, 1:-1] - 2 * c + p[:-2, j, 1:-1]) * dxi ** 2 + (p[1:-1, j + 1, 1:-1] - 2 * c + p[1:-1, j - 1, 1:-1]) * dyi ** 2 +
               ((p[1:-1, j, 2:] - c) / dzc[1:-1] - (c - p[1:-1, j, :-2]) / dzc[:-2]) / dzf)
        assert np.abs(lap - rhs[1:-1, j, 1:-1]).max() < tol * np.abs(lap).max(), j


@pytest.mark.parametrize("key,nsteps", [("c2", 10), ("c4", 3), ("c3", 2)])
def test_baseline_configs_by_value_at_full_size(key, nsteps):
    """BASELINE.json configs[1], [3] and [2] at their FULL sizes, BY VALUE: the case files bench.py times (256 x 128 x 128 wall-modelled channel with the static
    model, 512 x 256 x 256 wall-modelled duct with z-implicit diffusion, 512^3 channel with the dynamic model -- the headline run itself), a perturbed initial
    field, whole time steps on the device against the oracle (OpenMP team of 16: 512^3 takes it ~10 s per step and ~45 GB of host memory): u, v, w <= 1e-9,
    p (mean removed) <= 1e-8, eddy viscosity <= 1e-7 of each field's maximum, ghost cells included. configs[4] (1024^3: 8.6 GB per field)
    stays with the size-independent properties of test_c5_cavity_full_size."""
    import bench
    from cales_amd.hotpath import HotPath
    case = bench.channel_case((512, 512, 512), "dsmag") if key == "c3" else bench.load_case(bench.CONFIGS[key]["file"], bench.CONFIGS[key]["impdiff"])
    ng = tuple(int(x) for x in case.ng)
    o = Oracle(case, nthreads=16, team_sums=True)
    u, v, w, p = o.initflow(case.inivel, case.is_wallturb)
    rng = np.random.RandomState(5)
    for a in (u, v, w):
        for k in range(ng[2]):      # plane by plane: no second copy of a 1 GB field
            a[1:-1, 1:-1, k + 1] += 0.02 * (rng.rand(ng[0], ng[1]) - 0.5)
    h = HotPath(case)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    assert abs(h.chkdt() / (2 * dt) - 1) < 1e-12
    for _ in range(nsteps):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    errs = {nm: relerr(h.get(nm), b) for nm, b in (("u", u), ("v", v), ("w", w))}
    gp = h.get("p")[1:-1, 1:-1, 1:-1]; pi = p[1:-1, 1:-1, 1:-1]
    errs["p"] = relerr(gp - gp.mean(), pi - pi.mean())
    del gp, pi
    errs["visct"] = relerr(h.get("visct"), visct)
    dg, do = h.chkdiv(), o.chkdiv(u, v, w)
    print(key, ng, nsteps, "steps:", " ".join(f"{k} {e:.1e}" for k, e in errs.items()), f"divmax {dg[1]:.1e} (oracle {do[1]:.1e})")
    assert max(errs["u"], errs["v"], errs["w"]) < 1e-9 and errs["p"] < 1e-8 and errs["visct"] < 1e-7, errs
    assert dg[1] < 20. * do[1] + 1e-14 and dg[1] < 1e-11
    h.close(); o.close()


def test_c4_duct_full_size():
    """BASELINE.json configs[3] at FULL size on one GPU: square duct 512x256x256, wall model on the four walls, z-implicit
    (Crank-Nicolson) viscous terms -> Helmholtz sweeps + DCT Poisson solve. Size-independent properties after three steps (the
    reference's own abort rules, main.f90:523-544: finite divergence, divmax below its bound), bulk velocity held by the forcing,
    eddy viscosity finite and non-negative, and L_h(solve(r)) = r for the Neumann-Neumann (y, z) solve on sampled rows."""
    from cales_amd.hotpath import initflow
    g, case = load_golden("duct_smag_wm_imp1d")
    case.ng[:] = (512, 256, 256)
    h = _hot(case)
    h.upload(*initflow(case)); h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(3):
        h.step(dt)
    divtot, divmax = h.chkdiv()
    assert divmax < 1e-11 and np.isfinite(divtot)
    assert abs(h.bulk_mean("u", "f") - 1.0) < 1e-12
    visct = h.get("visct")[1:-1, 1:-1, 1:-1]
    assert visct.min() >= 0. and np.isfinite(visct).all()
    del visct
    small = case.copy(); small.ng[:] = (8, 8, 256)
    _laplacian_identity(h, case, Oracle(small).grid(), np.random.RandomState(11), (1, 100, 256))
    h.close()


def test_c5_cavity_full_size():
    """BASELINE.json configs[4] on one GPU at FULL size: lid-driven cavity 1024^3, all-Neumann pressure (DCT in x and y), fields of 8.6 GB
    (64-bit offset kernels, 16 planes per lane in the tridiagonal tile). The initial field of this case is zero (inivel = 'zer'), so one
    host array of 8.6 GB is uploaded four times: the test needs ~20 GB of host memory and FAILS, rather than shrinking, on a box with less.
    Two steps: divergence at round-off, finite fields, L_h(solve(r)) = r on sampled rows."""
    free_gb = int(open("/proc/meminfo").read().split("MemAvailable:")[1].split()[0]) / 2 ** 20
    n3 = 1024
    g, case = load_golden("cavity_nnn")
    case.ng[:] = (1024, 1024, n3)
    print(f"cavity 1024x1024x{n3} (host MemAvailable {free_gb:.0f} GB)")
    assert case.inivel == "zer"
    assert free_gb > 20., f"the full-size cavity needs ~20 GB of host memory, this box has {free_gb:.0f} GB available"
    h = _hot(case)
    z = h.zeros()
    for k in "uvwp":
        h.set(k, z)
    del z
    h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    divtot, divmax = h.chkdiv()
    assert divmax < 1e-11 and np.isfinite(divtot)
    small = case.copy(); small.ng[:] = (8, 8, n3)
    _laplacian_identity(h, case, Oracle(small).grid(), np.random.RandomState(13), (1, 500, 1024))
    uu = h.get("u")
    assert np.isfinite(uu).all() and np.abs(uu[1:-1, 1:-1, -1] + uu[1:-1, 1:-1, -2] - 2.).max() < 1e-13      # lid: u = 1 at the top wall
    h.close()


@pytest.mark.parametrize("wide", [False, True], ids=["offsets32", "offsets64"])
def test_cavity_1024_wide_whole_steps_by_value(wide, monkeypatch):
    """The last by-value hole of VERDICT r05 (item 6): WHOLE STEPS of a 1024-wide cavity against the oracle -- BASELINE.json configs[4]'s case at
    1024 x 1024 x 32 (its full 1024-point DCT-II/III lines in x and y, src/fft.f90:323-493; k_bc_all on its x faces; the momentum pass with the projection
    folded in, src/correc.f90:44-67), lid velocity plus a random perturbation so that every term is exercised, two steps: u, v, w <= 1e-9, p (mean removed)
    <= 1e-8 of each field's maximum, ghost cells included. Once with the 64-bit offset instantiations the 8.6-GB fields of the 1024^3 run take
    (CALES_WIDE_OFFSETS)."""
    if wide:
        monkeypatch.setenv("CALES_WIDE_OFFSETS", "1")
    g, case = load_golden("cavity_nnn")
    case.ng[:] = (1024, 1024, 32)
    ng = tuple(int(x) for x in case.ng)
    o = Oracle(case, nthreads=16, team_sums=True)
    u, v, w, p = o.initflow(case.inivel, case.is_wallturb)
    rng = np.random.RandomState(17)
    for a in (u, v, w):
        for k in range(ng[2]):
            a[1:-1, 1:-1, k + 1] += 0.05 * (rng.rand(ng[0], ng[1]) - 0.5)
    h = _hot(case)
    h.upload(u, v, w, p); h.startup()
    visct, pp = o.zeros(), o.zeros()
    o.bounduvw(u, v, w, True, False); o.boundp(p, 0); o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)
    dt = 0.5 * o.chkdt(visct, u, v, w)
    assert abs(h.chkdt() / (2 * dt) - 1) < 1e-12
    pl = h.describe_plan()
    assert pl["solver"] == "x:NN/radix8,y:NN/radix8,z:lds_tile" and pl["projection"].startswith("in_next_momentum_pass"), pl
    for _ in range(2):
        h.step(dt); o.step(dt, u, v, w, p, pp, visct)
    errs = {nm: relerr(h.get(nm), b) for nm, b in (("u", u), ("v", v), ("w", w))}
    gp = h.get("p")[1:-1, 1:-1, 1:-1]; pi = p[1:-1, 1:-1, 1:-1]
    errs["p"] = relerr(gp - gp.mean(), pi - pi.mean())
    dg, do = h.chkdiv(), o.chkdiv(u, v, w)
    print("cavity", ng, "2 steps:", " ".join(f"{k} {e:.1e}" for k, e in errs.items()), f"divmax {dg[1]:.1e} (oracle {do[1]:.1e})")
    assert max(errs["u"], errs["v"], errs["w"]) < 1e-9 and errs["p"] < 1e-8, errs
    assert dg[1] < 20. * do[1] + 1e-14 and dg[1] < 1e-10
    h.close(); o.close()


@pytest.mark.parametrize("name,ng", [("chan_smag", (512, 512, 8)), ("cavity_nnn", (1024, 512, 4)), ("cavity_nnn", (512, 1024, 4)),
                                     ("duct_smag_wm", (512, 256, 16)), ("chan_smag", (1024, 1024, 2))])
def test_poisson_solve_production_lengths(name, ng):
    """The production line lengths (512- and 1024-point r2c/c2c FFTs and DCTs in x and y) against the oracle itself on thin slabs,
    so the large transforms are checked by value and not only through the operator identity."""
    test_poisson_solve(name, ng)

"""HIP hot path (through the C-ABI) against the golden vectors produced by the reference's own
compiled operators. Same stage-by-stage replay as tests/test_oracle_golden.py: every operator is fed
the golden input of its stage. FP64 tolerance 1e-13 relative (L-inf, scaled by the field maximum);
the kernels keep the reference's expression order but are compiled with FMA contraction."""
import os

import numpy as np
import pytest

from tests.util import RK, F, load_golden, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-13
DEVICE_CASES = ["tgv_ppp", "tgv_dsmag_ppp", "chan_smag_wm", "chan_smag", "chan_dsmag", "chan_dsmag_wm", "halfchan_imp1d",
                "duct_smag_wm", "duct_smag_wm_imp1d", "cavity_nnn", "devchan_nd",
                "duct_dsmag_wm", "duct_dsmag", "cavity_dsmag",    # PP, NN (DCT) and ND (DCT-IV, inflow/outflow) pressure transforms
                # the wall model beyond the shipped examples (wmodel.f90:65-335): faces in x, the laminar law, moving walls, a model on one side of a direction
                "cavity_smag_wm6", "cavity_dsmag_wm_mixed", "cavity_smag_wm_lam", "chan_smag_wm_mov", "halfchan_smag_wm_imp1d", "halfchan_dsmag_wm"]


def _hot(case):
    from cales_amd.hotpath import HotPath
    # examples/dns/developing_channel ships cbcsgs(:,1) = 'N','N', which the reference's own sanity.f90:191-203 rejects for a
    # DN velocity; with sgstype = 'none' the entry only touches the ghost cells of an identically zero visct
    if case.sgstype == "none" and case.cbcvel[0, 0, 0] != "P":
        case.cbcsgs[:, 0] = "D"
    return HotPath(case)


WALLED_DSMAG = ["cavity_dsmag", "cavity_dsmag_wm_mixed"]    # walls in x: the kernel-per-loop sequence is the only path (ducts, y walls, go through the tile passes)


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_startup_and_substeps(name, general_sgs=False):
    g, case = load_golden(name)
    h = _hot(case)
    imp = case.impdiff
    # the kernel-per-loop sequences keep the reference's expression order (only the plane sums associate differently) and are
    # held to the single-operator tolerance; the tile passes re-associate the filter sums
    general_sgs = general_sgs or name in WALLED_DSMAG
    tol_sgs0, tol_sgs = (TOL, TOL) if (case.sgstype != "dsmag" or general_sgs) else (1e-11, 1e-10)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp"))
    h.bounduvw(True, False); h.boundp("p", 0)
    for k in "uvwp":
        assert relerr(h.get(k), g["s0_" + k]) < TOL, ("s0", k)
    h.upload(*(F(g["s0_" + k]) for k in "uvwp"))
    h.cmpt_sgs()
    assert relerr(h.get("visct")[1:-1, 1:-1, 1:-1], g["s0_visct_nobc"][1:-1, 1:-1, 1:-1]) < tol_sgs0
    h.set("visct", F(g["s0_visct_nobc"])); h.boundp("visct", 1)
    assert relerr(h.get("visct"), g["s0_visct"]) < TOL
    if np.any(case.lwm != 0):
        for iv, nm in ((1, "bcu"), (2, "bcv"), (3, "bcw")):
            for a, d in zip(h.bcvel_planes(iv), "xyz"):
                ref = g[f"s0_{nm}_{d}"]
                assert np.abs(a - ref).max() <= 1e-12 * max(1., np.abs(ref).max()), (nm, d)
    h.set("visct", F(g["s0_visct"]))
    assert abs(h.chkdt() / float(g["dt_cfl"]) - 1) < 1e-13
    h.mom()
    for fld, k in (("dudt", "dudt"), ("dvdt", "dvdt"), ("dwdt", "dwdt")) + ((("dudtd", "dudtd"), ("dvdtd", "dvdtd"), ("dwdtd", "dwdtd")) if imp else ()):
        assert relerr(h.get(fld)[1:-1, 1:-1, 1:-1], g["m_" + k]) < TOL, k
    assert abs(h.bulk_mean("u", "f") - float(g["mean_u_f"])) <= 1e-13 * max(1, abs(float(g["mean_u_f"])))
    d0 = h.chkdiv()
    assert abs(d0[1] / g["div0"][1] - 1) < 1e-12 and abs(d0[0] - g["div0"][0]) < 1e-11 * max(1, abs(g["div0"][0]))

    dt = float(g["dt"])
    prev = dict(u=g["s0_u"], v=g["s0_v"], w=g["s0_w"], p=g["s0_p"], visct=g["s0_visct"])
    for irk in (1, 2, 3):
        K = f"r{irk}_"
        dtrk = (RK[irk - 1][0] + RK[irk - 1][1]) * dt; dtrki = dtrk ** (-1)
        alpha = -.5 * case.visc * dtrk if imp else 0.
        h.upload(F(prev["u"]), F(prev["v"]), F(prev["w"]), F(prev["p"])); h.set("visct", F(prev["visct"]))
        f = h.rk(irk, dt); h.bulk_forcing()
        assert np.abs(f - g[K + "s1_f"]).max() < 1e-13
        for k in "uvw":
            assert relerr(h.get(k)[1:-1, 1:-1, 1:-1], g[K + "s1_" + k][1:-1, 1:-1, 1:-1]) < TOL, (K, "s1", k)
        nxt, sfx = "s1", ""
        if imp == 2:
            for k in "uvw":
                h.set(k, F(g[K + "s1_" + k]))
            for iv in (1, 2, 3):
                h.helmholtz_z(iv, alpha)
            for k in "uvw":   # made by the reference's own gaussel + tridmatrix (solver_gaussel_z = a transposition around them, solver.f90:182-233)
                assert relerr(h.get(k)[1:-1, 1:-1, 1:-1], g[K + "s1b_" + k][1:-1, 1:-1, 1:-1]) < 1e-12, (K, "s1b", k)
            nxt, sfx = "s1b", ""
        for k in "uvw":
            h.set(k, F(g[K + nxt + "_" + k + sfx]))
        h.bounduvw(True, False)
        for k in "uvw":
            assert relerr(h.get(k), g[K + "s2_" + k]) < TOL, (K, "s2", k)
        h.fillps(dtrki); h.updt_rhs_b()
        assert relerr(h.get("pp")[1:-1, 1:-1, 1:-1], g[K + "s3_pp"][1:-1, 1:-1, 1:-1]) < TOL
        # Poisson solve: golden output came from the oracle; the reference's own chkdiv certified it (r?_div)
        h.set("pp", F(g[K + "s3_pp"])); h.solver(); h.boundp("pp", 0)
        a, b = h.get("pp"), g[K + "s5_pp"]
        a = a - a[1:-1, 1:-1, 1:-1].mean(); b = b - b[1:-1, 1:-1, 1:-1].mean()
        assert relerr(a, b) < 1e-11, (K, "s5")
        h.set("pp", F(g[K + "s5_pp"]))
        for k in "uvw":
            h.set(k, F(g[K + "s2_" + k]))
        h.correc(dtrk)
        if irk == 1:
            for k in "uvw":
                assert relerr(h.get(k), g[K + "s6_" + k]) < TOL, (K, "s6", k)
        h.bounduvw(True, True)
        for k in "uvw":
            assert relerr(h.get(k), g[K + "s7_" + k]) < TOL, (K, "s7", k)
        dv = h.chkdiv()
        assert dv[1] < 1e-12, "divergence after projection"
        h.set("p", F(prev["p"])); h.updatep(alpha); h.boundp("p", 0)
        assert relerr(h.get("p"), g[K + "s8_p"]) < TOL
        h.set("visct", F(prev["visct"]))
        for k in "uvw":
            h.set(k, F(g[K + "s7_" + k]))
        h.cmpt_sgs(); h.boundp("visct", 1)
        assert relerr(h.get("visct"), g[K + "s9_visct"]) < tol_sgs, (K, "s9")
        prev = dict(u=g[K + "s7_u"], v=g[K + "s7_v"], w=g[K + "s7_w"], p=g[K + "s8_p"], visct=g[K + "s9_visct"])
    h.close()


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_fused_step_matches_operator_sequence(name):
    """cales_step (one call, no host sync) == the golden end-of-step state, up to the growth of round-off
    through three substeps (1e-10) and with p compared after removing its mean (singular mode, solver.f90:165)."""
    g, case = load_golden(name)
    h = _hot(case)
    # start-up as the driver does it (main.f90:370-375): besides the ghost cells it fills the wall-model planes
    # bcu/bcv/bcw, which the z-implicit boundary r.h.s. of the first substep reads (main.f90:425)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    h.step(float(g["dt"]))
    u, v, w, p, visct = h.download()
    for a, k in zip((u, v, w), "uvw"):
        assert relerr(a, g["r3_s7_" + k]) < 1e-10, k
    pg = g["r3_s8_p"]
    assert relerr(p - p[1:-1, 1:-1, 1:-1].mean(), pg - pg[1:-1, 1:-1, 1:-1].mean()) < 1e-9
    assert relerr(visct, g["r3_s9_visct"]) < 1e-8
    assert np.abs(h.dpdl() - g["dpdl"]).max() < 1e-9 * max(1., np.abs(g["dpdl"]).max())
    dv = h.chkdiv()
    assert dv[1] < 1e-12 and abs(dv[1]) < 10 * max(g["r3_div"][1], 1e-16) * 10
    h.close()


@pytest.mark.parametrize("keep_x", [False, True], ids=["wrap", "xghosts"])
@pytest.mark.parametrize("name", ["chan_dsmag_p2", "chan_smag_p2", "duct_dsmag_p2", "tgv_ppp_p2", "chan_dsmag_x64", "chan_dsmag_x128", "tgv_dsmag_ppp_x64",
                                  "chan_smag_wm_x64", "duct_smag_wm_x64", "duct_smag_wm_imp1d_x64",
                                  "chan_nosgs_x64", "cavity_nnn_x64", "halfchan_imp1d_x64", "duct_dsmag_x64", "tgv_ppp_x64",
                                  "chan_smag_fy_x64", "chan_dsmag_fxy_x64", "tgv_fyz_x64",      # (forcing in y and z, a body force)
                                  "chan_smag_wm_mov_x64", "cavity_smag_wm6_x64", "halfchan_dsmag_wm_x64"])      # (moving walls, wall-model faces in x, the laminar law on one wall)
def test_fused_step_at_power_of_two_rows(name, keep_x, monkeypatch):
    """Reference-made end-of-step states at power-of-two row lengths: radix-8 transforms, fillps inside the forward x pass, the x ghost columns left
    alone until the step returns (and, with CALES_XGHOSTS_IN_STEP, updated by every ghost-cell operator as at the operator level)."""
    if keep_x:
        monkeypatch.setenv("CALES_XGHOSTS_IN_STEP", "1")
    test_fused_step_matches_operator_sequence(name)


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "separate"])
@pytest.mark.parametrize("name", ["chan_dsmag_x64", "chan_dsmag_x128", "tgv_dsmag_ppp_x64"])
def test_folded_strain_pass_against_reference_made_state(name, folded, monkeypatch):
    """Reference-made end-of-step states (src/sgs.f90:153-380 + src/correc.f90:44-67 + src/updatep.f90:30-47 through the compiled modules,
    gen_golden.py END_ONLY) at rows of 64 cells, the only row lengths at which the dynamic model's strain-rate pass takes the projection on load
    (k_corr_strain_tile, the dominant kernel of the 512^3 bench: api.hip `fold_correc` asks for whole 64-cell tiles in x). The profile counters
    say which kernels ran: the folded pass in every substep and no correction pass of its own -- or, with CALES_UNFOLDED_CORREC, the opposite."""
    if not folded:
        monkeypatch.setenv("CALES_UNFOLDED_CORREC", "1")
    g, case = load_golden(name)
    h = _hot(case)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    h.profile(True)
    h.step(float(g["dt"]))
    u, v, w, p, visct = h.download()
    h.profile(False); st = h.profile_stats()
    nfold, ncorr = st.get("correc_strain_filter_uvw", (0, 0.))[0], st.get("correc_updatep", (0, 0.))[0]
    assert (nfold, ncorr) == ((3, 0) if folded else (0, 3)), st
    # ... and the plan the step read (cales_describe_plan, struct StepPlan) names the same path
    pl = h.describe_plan()
    assert pl["projection"] == ("in_strain_rate_pass" if folded else "own_pass(correc+updatep)"), pl
    assert pl["x_ghost_columns"] == "wrapped" and pl["fillps"] == "in_x_transform" and pl["sgs"] == "dsmag_tiles(pair_fields)", pl
    assert pl["bulk_forcing"] == ("in_correction(means_in_x_transform)" if name.startswith("chan") else "none"), pl
    for a, k in zip((u, v, w), "uvw"):
        assert relerr(a, g["r3_s7_" + k]) < 1e-10, k
    pg = g["r3_s8_p"]
    assert relerr(p - p[1:-1, 1:-1, 1:-1].mean(), pg - pg[1:-1, 1:-1, 1:-1].mean()) < 1e-9
    assert relerr(visct, g["r3_s9_visct"]) < 1e-8
    assert np.abs(h.dpdl() - g["dpdl"]).max() < 1e-9 * max(1., np.abs(g["dpdl"]).max())
    assert h.chkdiv()[1] < 1e-12
    h.close()


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "separate"])
@pytest.mark.parametrize("name", ["chan_nosgs_x64", "cavity_nnn_x64", "halfchan_imp1d_x64", "tgv_ppp_x64"])
def test_folded_momentum_pass_against_reference_made_state(name, folded, monkeypatch):
    """No subgrid model: the projection of substeps 1 and 2 is applied by the next momentum pass (k_momrk<.., CORR>), the ghost cells through the corrected
    view. Held to end-of-step states made by the reference's compiled modules at 64-cell rows (gen_golden.py END_ONLY): a forced DNS channel, a cavity,
    a half channel with z-implicit diffusion (velocity only folded), the triply periodic box. The counters say what ran: ONE correction pass per step
    (the third substep's) with the fold, three without (CALES_UNFOLDED_MOM)."""
    if not folded:
        monkeypatch.setenv("CALES_UNFOLDED_MOM", "1")
    g, case = load_golden(name)
    h = _hot(case)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    h.profile(True)
    h.step(float(g["dt"]))
    u, v, w, p, visct = h.download()
    h.profile(False); st = h.profile_stats()
    ncorr = st.get("correc_updatep", (0, 0.))[0] + st.get("correc", (0, 0.))[0]
    assert ncorr == (1 if folded else 3), st
    pl = h.describe_plan()      # the plan the step read (struct StepPlan) names the same path
    assert pl["projection"] == ("in_next_momentum_pass(substeps_1_2)" if folded else "own_pass(correc+updatep)"), pl
    assert pl["sgs"] == "none" and pl["visct_ghost_cells"] == "zero_field", pl
    if name == "halfchan_imp1d_x64":
        assert pl["implicit_rhs"] == "in_helmholtz_sweep", pl
    for a, k in zip((u, v, w), "uvw"):
        assert relerr(a, g["r3_s7_" + k]) < 1e-10, k
    pg = g["r3_s8_p"]
    assert relerr(p - p[1:-1, 1:-1, 1:-1].mean(), pg - pg[1:-1, 1:-1, 1:-1].mean()) < 1e-9
    assert np.abs(h.dpdl() - g["dpdl"]).max() < 1e-9 * max(1., np.abs(g["dpdl"]).max())
    assert h.chkdiv()[1] < 1e-12
    h.close()


@pytest.mark.parametrize("name", ["chan_dsmag", "duct_smag_wm_imp1d"])
def test_wide_offset_kernels(name, monkeypatch):
    """Fields of 4 GB and more (e.g. the 1024^3 cavity) use the size_t instantiations of the tile kernels; force them
    here on a small case and hold them to the same end-of-step tolerances."""
    monkeypatch.setenv("CALES_WIDE_OFFSETS", "1")
    test_fused_step_matches_operator_sequence(name)


@pytest.mark.parametrize("env", ["CALES_DSMAG_REFERENCE_SEQUENCE", "CALES_UNFUSED_RK", "CALES_UNFUSED_CORREC", "CALES_UNFUSED_FORCING", "CALES_UNFUSED_FILLPS", "CALES_UNFUSED_MEAN", "CALES_GAUSSEL_MARCH", "CALES_NO_NYQUIST_PACKING", "CALES_KEEP_LAST_RHS",
                                 "CALES_UNMERGED_BC"])
@pytest.mark.parametrize("name", ["chan_dsmag", "chan_dsmag_wm", "tgv_dsmag_ppp", "duct_smag_wm_imp1d", "duct_dsmag_wm"])
def test_unfused_paths(name, env, monkeypatch):
    """The kernel-per-loop forms behind the operator-level entries (general dsmag sequence, mom + rk_update, correc +
    updatep, bulk forcing and fillps as passes of their own, marching tridiagonal sweep) stay selectable and are held to the same
    end-of-step tolerances."""
    monkeypatch.setenv(env, "1")
    test_fused_step_matches_operator_sequence(name)


SWITCH_CASES = [
    # per-column pivots / separate implicit r.h.s. passes in the z-implicit step
    ({"CALES_HELMHOLTZ_Z_PER_COLUMN": "1"}, ["duct_smag_wm_imp1d", "halfchan_imp1d"]),
    ({"CALES_UNFUSED_IMP_RHS": "1"}, ["duct_smag_wm_imp1d", "halfchan_imp1d"]),
    # ghost columns of the dynamic model's scratch fields filled instead of wrapped
    ({"CALES_DSMAG_XGHOSTS": "1"}, ["chan_dsmag", "chan_dsmag_wm", "tgv_dsmag_ppp", "duct_dsmag_wm"]),
    # k chunks of the marching tile kernels: forced length (with its three-plane prologues inside the field) and the block-count threshold
    ({"CALES_KCHUNK": "3"}, ["chan_dsmag", "chan_dsmag_wm", "chan_smag_wm", "duct_dsmag_wm", "duct_smag_wm_imp1d"]),
    ({"CALES_KCHUNK": "5"}, ["chan_smag_wm", "duct_smag_wm"]),
    ({"CALES_TILE_MIN_BLOCKS": "1000000"}, ["chan_dsmag", "duct_smag_wm_imp1d"]),
    ({"CALES_TILE_MIN_BLOCKS": "1"}, ["chan_dsmag", "duct_smag_wm_imp1d"]),
    # dynamic model inside cales_step: the projection as a pass of its own (k_correc_cell) instead of inside the strain-rate pass. The folded form needs
    # rows that are whole 64-cell tiles (api.hip `fold_correc`), so of the golden cases only chan_dsmag_x64 / tgv_dsmag_ppp_x64 take it by default
    # (test_folded_strain_pass_against_reference_made_state asserts which kernels ran); on the shorter rows here the switch only has to be harmless
    ({"CALES_UNFOLDED_CORREC": "1"}, ["chan_dsmag", "chan_dsmag_p2", "tgv_dsmag_ppp", "chan_dsmag_x64"]),
    # no subgrid model inside cales_step: the projection of every substep as a pass of its own instead of inside the next momentum pass (the default for
    # explicit diffusion with every direction periodic or between no-slip walls)
    ({"CALES_UNFOLDED_MOM": "1"}, ["tgv_ppp", "tgv_ppp_p2", "cavity_nnn"]),
]


@pytest.mark.parametrize("envs,name", [(e, n) for e, names in SWITCH_CASES for n in names],
                         ids=lambda v: "+".join(f"{k[6:]}={x}" for k, x in v.items()) if isinstance(v, dict) else v)
def test_remaining_switches(envs, name, monkeypatch):
    """Every run-time switch of DESIGN.md's table that selects an alternative code path is exercised against the reference-made goldens
    (end-of-step state) -- a path in the product library that no test runs is either dead or a latent fault."""
    for k, v in envs.items():
        monkeypatch.setenv(k, v)
    test_fused_step_matches_operator_sequence(name)
    if "CALES_KCHUNK" in envs:
        test_startup_and_substeps(name)      # stage by stage at 1e-13 as well


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_unmerged_bc_operator_level(name, monkeypatch):
    """The one-launch ghost-cell kernel (x, y periodic: every ghost cell = the z operation on the wrapped interior cell) is the default
    where it applies; the direction-by-direction sequence of bound.f90:158-199 behind CALES_UNMERGED_BC must give the same ghost cells,
    corners included: both are held to the reference's planes stage by stage."""
    monkeypatch.setenv("CALES_UNMERGED_BC", "1")
    test_startup_and_substeps(name)


@pytest.mark.parametrize("name", ["chan_smag", "chan_smag_wm", "duct_smag_wm", "cavity_smag_wm6", "cavity_smag_wm_lam", "chan_smag_wm_mov", "halfchan_smag_wm_imp1d"])
def test_smag_reference_sequence(name, monkeypatch):
    """Static Smagorinsky through the kernel-per-loop sequence (the path ducts and cavities take)."""
    monkeypatch.setenv("CALES_SMAG_REFERENCE_SEQUENCE", "1")
    test_startup_and_substeps(name, general_sgs=True)


@pytest.mark.parametrize("name", ["chan_dsmag", "chan_dsmag_wm", "tgv_dsmag_ppp", "duct_dsmag_wm", "duct_dsmag", "cavity_dsmag_wm_mixed"])
def test_dsmag_reference_sequence(name, monkeypatch):
    """Dynamic Smagorinsky through the kernel-per-loop sequence of sgs.f90:153-380, operator by operator at 1e-13.
    (Not halfchan_dsmag_wm: the 1e-13 stands for plane sums in another association, and on that case the reference's own algorithm -- the CPU restatement,
    bit-identical to the golden vectors -- moves the start-up eddy viscosity by 3.8e-12 of its maximum when every input moves by one unit in the last
    place, against 1e-15 to 6e-14 on the cases listed: a model coefficient that is the quotient of two plane sums that cancel, in plane 12. The sequence gave
    3.3e-13 there. The case is held at the bars of the tile passes by test_startup_and_substeps and test_unmerged_bc_operator_level.)"""
    monkeypatch.setenv("CALES_DSMAG_REFERENCE_SEQUENCE", "1")
    test_startup_and_substeps(name, general_sgs=True)


def test_imp3d_operators():
    """3-D implicit diffusion (impdiff = 1) against the reference built with -D_IMPDIFF: momentum split, two RK substeps,
    pressure update with the full Laplacian, time-step bound (same stages as tests/test_oracle_golden.py)."""
    g, case = load_golden("couette_imp3d_ops")
    h = _hot(case)
    h.upload(*(F(g["s0_" + k]) for k in "uvwp")); h.set("visct", F(g["s0_visct"]))
    h.mom()
    for k in ("dudt", "dvdt", "dwdt", "dudtd", "dvdtd", "dwdtd"):
        assert relerr(h.get(k)[1:-1, 1:-1, 1:-1], g["m_" + k][1:-1, 1:-1, 1:-1] if g["m_" + k].shape == h.zeros().shape else g["m_" + k]) < TOL, k
    for env in (None, "CALES_UNFUSED_RK"):
        import os
        if env:      # the switches are read when a context is created
            os.environ[env] = "1"; h.close(); h = _hot(case)
        try:
            h.upload(*(F(g["s0_" + k]) for k in "uvwp")); h.set("visct", F(g["s0_visct"]))
            for k in ("dudto", "dvdto", "dwdto"):
                h.set(k, h.zeros())
            # the golden calls rk twice with no bounduvw in between; the fused kernel writes the new velocity into a second
            # set of buffers and leaves their ghost cells undefined (include/cales.h), so only the in-place form can follow it
            for irk in ((1, 2) if env else (1,)):
                h.rk(irk, float(g["dt"]))
                for k in "uvw":
                    assert relerr(h.get(k)[1:-1, 1:-1, 1:-1], g[f"r{irk}_s1_{k}"][1:-1, 1:-1, 1:-1]) < TOL, (env, irk, k)
        finally:
            if env:
                del os.environ[env]
    assert abs(h.chkdt() / float(g["dt_cfl"]) - 1) < 1e-13
    h.set("p", F(g["s0_p"])); h.set("pp", F(g["upd_pp"]))
    h.updatep(float(g["upd_alpha"]))
    assert relerr(h.get("p")[1:-1, 1:-1, 1:-1], g["upd_p"][1:-1, 1:-1, 1:-1]) < TOL
    h.close()


@pytest.mark.parametrize("name", ["chan_smag", "tgv_ppp"])
def test_rk_with_caller_coefficients(name):
    """cales_rk_par(rkpar, dt) = the reference's rk(rkpar, ...) signature (rk.f90:17): with rkcoeff(:, irk) of param.f90:27-29 it is
    the golden substep; the forcing comes back through f_out."""
    g, case = load_golden(name)
    h = _hot(case)
    h.upload(*(F(g["s0_" + k]) for k in "uvwp")); h.set("visct", F(g["s0_visct"]))
    f = h.rk_par(RK[0], float(g["dt"]))
    assert np.abs(f - g["r1_s1_f"]).max() < 1e-13
    h.bulk_forcing()
    for k in "uvw":
        assert relerr(h.get(k)[1:-1, 1:-1, 1:-1], g["r1_s1_" + k][1:-1, 1:-1, 1:-1]) < TOL, k
    h.close()


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_plane_statistics_against_reference(name):
    """cales_out1d_single_point_chan / cales_out1d_chan_budgets on the golden end-of-step state against the output of the reference's own
    out1d_single_point_chan (src/output.f90:509-1061, compiled from its lines by oracle/ref/Makefile): 27 + 38 + 6 columns per plane.
    The device sums planes in two deterministic levels, the reference in one loop: 1e-12 of each column's largest entry (measured ≤ 1e-14)."""
    g, case = load_golden(name)
    h = _hot(case)
    h.upload(*(F(g[k]) for k in ("r3_s7_u", "r3_s7_v", "r3_s7_w", "r3_s8_p"))); h.set("visct", F(g["r3_s9_visct"]))
    st = h.stats_chan(); bud, leak = h.stats_chan_budgets()
    for got, ref, nm in ((st, g["st_chan"], "single-point"), (bud, g["st_budget"], "budget"), (leak, g["st_leak"], "leakage")):
        scale = np.abs(ref).max(axis=1, keepdims=True)
        # columns that vanish by cancellation (mean w, mean vorticity of a periodic box ...) are held to 1e-14 of the block's largest column
        assert (np.abs(got - ref) <= 1e-12 * scale + 1e-14 * np.abs(ref).max()).all(), (nm, np.abs(got - ref).max(axis=1) / np.maximum(scale[:, 0], 1e-300))
    h.close()


@pytest.mark.parametrize("name", ["tgv_ppp", "chan_smag_wm", "chan_dsmag", "duct_smag_wm", "duct_smag_wm_imp1d", "duct_dsmag", "cavity_nnn", "devchan_nd", "halfchan_imp1d",
                                  "chan_dsmag_p2", "chan_smag_p2", "duct_dsmag_p2", "tgv_ppp_p2"])
def test_profiles_and_duct_statistics(name):
    """cales_out1d, cales_out1d_chan, cales_out2d_duct (src/output.f90:50-163, 317-507) on the end-of-step state of the golden cases: against what
    the reference's own routines print (8 significant digits, tests/golden/outstats.npz) and against the oracle to 1e-13 of each column's scale
    (fixed summation order on the device, another association than the reference's loops)."""
    from oracle.oracle import Oracle
    from tests.test_oracle_golden import outstats_of, printed_equal
    g, case, G, (u, v, w) = outstats_of(name, None)
    h = _hot(case); o = Oracle(case)
    for k, a in zip("uvw", (u, v, w)):
        h.set(k, a)
    vmax = max(np.abs(a).max() for a in (u, v, w)); fl = 1e-13 * max(vmax, vmax ** 2)
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-13 * np.abs(b).max() + fl
    for key, (idir, fld, dzc) in dict(u_z=(3, "u", 0), v_y=(2, "v", 0), w_x=(1, "w", 1), w_z=(3, "w", 1), u_y=(2, "u", 0)).items():
        mine = h.out1d(fld, idir, bool(dzc))
        fa = dict(u=u, v=v, w=w)[fld]
        printed_equal(mine, G[f"{name}__out1d_{key}"][1], key, floor=1e-13 * np.abs(fa).max())
        assert np.abs(mine - o.out1d(idir, fa, bool(dzc))).max() <= 1e-13 * np.abs(fa).max(), key
    ch = h.out1d_chan()
    printed_equal(ch.T, G[name + "__out1d_chan"][:, 1:], "out1d_chan", floor=fl)
    oc = o.out1d_chan(u, v, w)
    assert all(close(ch[q], oc[q]) for q in range(7))
    n2, n3 = int(case.ng[1]), int(case.ng[2])
    du = h.out2d_duct()
    printed_equal(du.reshape(9, n2 * n3, order="F").T, G[name + "__out2d_duct"][:, 2:], "out2d_duct", floor=fl)
    od = o.out2d_duct(u, v, w)
    assert all(close(du[q], od[q]) for q in range(9))
    h.close()


def test_profiles_on_slabs_add_up():
    """Several ranks: every rank returns the sums over its rows; added (profiles along x and z, the seven plane sums) or laid side by side
    (profile along y, the duct maps) they are the one-rank result."""
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import initflow
    g, case = load_golden("duct_smag_wm"); case.ng[:] = (16, 24, 12); case.hwm = 0.3
    h = _hot(case); u, v, w, p = initflow(case); h.upload(u, v, w, p); h.startup()
    ref = dict(z=h.out1d("u", 3), y=h.out1d("u", 2), x=h.out1d("w", 1, True), chan=h.out1d_chan(), duct=h.out2d_duct()); h.close()

    def body(hh, r):
        hh.upload_initial(); hh.startup()
        return dict(z=hh.out1d("u", 3), y=hh.out1d("u", 2), x=hh.out1d("w", 1, True), chan=hh.out1d_chan(), duct=hh.out2d_duct())
    res = run_loopback(case, 3, body)
    tol = lambda a, b: np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
    assert tol(sum(r["z"] for r in res), ref["z"]) and tol(sum(r["x"] for r in res), ref["x"]) and tol(sum(r["chan"] for r in res), ref["chan"])
    assert tol(np.concatenate([r["y"] for r in res]), ref["y"]) and tol(np.concatenate([r["duct"] for r in res], axis=1), ref["duct"])


@pytest.mark.parametrize("name,ng,nsteps,kchunk", [("chan_dsmag", (64, 20, 12), 3, None), ("chan_dsmag", (128, 30, 23), 2, "5"), ("tgv_dsmag_ppp", (64, 16, 24), 2, None),
                                                   ("chan_dsmag", (64, 8, 40), 2, "7"), ("chan_dsmag", (192, 12, 16), 2, None)])
def test_folded_projection_equals_the_separate_pass(name, ng, nsteps, kchunk, monkeypatch):
    """cales_step on one rank, dynamic model, x and y periodic with whole 64-cell tiles in x: the velocity correction and the pressure update are done by
    the strain-rate pass of cmpt_sgs (k_corr_strain_tile: corrected velocity on load, the z ghost planes by their boundary rule, p += pp) instead of
    k_correc_cell. Same operations on the same values -- the two forms agree to round-off of the strain-rate block's association (1e-13 on every field,
    ghost cells included; 1e-9 on the eddy viscosity, whose plane coefficients are quotients of sums); partial y tiles, k chunks that end inside the
    field, z walls and z periodic."""
    from cales_amd.hotpath import HotPath, initflow
    if kchunk:
        monkeypatch.setenv("CALES_KCHUNK", kchunk)
    out = {}
    for mode in ("fold", "separate"):
        if mode == "separate":
            monkeypatch.setenv("CALES_UNFOLDED_CORREC", "1")
        g, case = load_golden(name); case.ng[:] = ng
        h = HotPath(case); u, v, w, p = initflow(case)
        rng = np.random.RandomState(1)
        for a in (u, v, w):
            a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
        h.upload(u, v, w, p); h.startup(); dt = 0.5 * h.chkdt()
        for _ in range(nsteps):
            h.step(dt)
        out[mode] = h.download() + [h.get("pp")]
        st = h.profile_stats() if False else None
        h.close()
    for nm, a, b in zip(("u", "v", "w", "p", "visct", "pp"), out["fold"], out["separate"]):
        assert relerr(a, b) < (1e-9 if nm == "visct" else 1e-12), nm


def _nosgs_case(name, ng):
    g, case = load_golden({"chan_nosgs": "chan_smag", "chan_nosgs_imp1d": "chan_smag", "halfchan_nosgs": "halfchan_imp1d"}.get(name, name)); case.ng[:] = ng
    if name in ("chan_nosgs", "chan_nosgs_imp1d"):      # DNS channel: bulk forcing in x, z walls, no subgrid model
        case.sgstype = "none"
    if name == "halfchan_nosgs":      # open channel: no-slip bottom, free-slip top (Neumann u, v; w = 0), bulk forcing, explicit diffusion
        case.impdiff = 0
    if name == "chan_nosgs_imp1d":      # DNS channel with z-implicit diffusion: the velocity correction folds, the pressure update keeps its pass
        case.impdiff = 2
    return case


@pytest.mark.parametrize("name,ng,nsteps,kchunk", [("tgv_ppp", (64, 16, 24), 3, None), ("tgv_ppp", (32, 24, 16), 2, "5"), ("tgv_ppp", (24, 10, 9), 2, None),
                                                   ("cavity_nnn", (32, 24, 20), 3, None), ("cavity_nnn", (70, 14, 9), 2, "4"), ("cavity_nnn", (128, 8, 12), 2, None),
                                                   ("chan_nosgs", (64, 16, 16), 3, None), ("chan_nosgs", (128, 12, 10), 2, "3"), ("chan_nosgs", (48, 20, 12), 2, None),
                                                   ("chan_nosgs_imp1d", (64, 16, 16), 3, None), ("chan_nosgs_imp1d", (48, 12, 10), 2, "3"), ("halfchan_imp1d", (64, 12, 16), 2, None),
                                                   ("halfchan_imp1d", (24, 10, 12), 3, "unmerged"),
                                                   ("halfchan_nosgs", (64, 12, 16), 3, None), ("halfchan_nosgs", (40, 16, 13), 2, "4"), ("halfchan_nosgs", (32, 8, 10), 2, "unmerged"),
                                                   # the ghost cells direction by direction (k_set_bc) instead of the one-launch kernel
                                                   ("tgv_ppp", (64, 16, 24), 2, "unmerged"), ("chan_nosgs", (64, 16, 16), 2, "unmerged")])
def test_projection_folded_into_the_momentum_pass_equals_the_separate_pass(name, ng, nsteps, kchunk, monkeypatch):
    """cales_step without subgrid model (explicit diffusion, one rank, every direction periodic or between no-slip walls): the projection and pressure update of
    substeps 1 and 2 are applied by the momentum pass of the next substep while it loads its planes (k_momrk<.., CORR = 1>), the ghost cells of the projected
    velocity come from the ghost-cell kernels' corrected view. Same operations on the same values as k_correc_cell + bounduvw + boundp: all fields agree to
    round-off, ghost cells included -- triply periodic, all walls (x ghost columns maintained), a forced channel (x ghost columns left alone inside the step),
    partial tiles in x and y, k chunks that end inside the field."""
    from cales_amd.hotpath import HotPath, initflow
    if kchunk == "unmerged":
        monkeypatch.setenv("CALES_UNMERGED_BC", "1")
    elif kchunk:
        monkeypatch.setenv("CALES_KCHUNK", kchunk)
    # the third substep's projection: completed inside the step (the default below 4M cells per rank) or left to the next step's first momentum pass and,
    # after the last step, to the download (CALES_LAZY_PROJECTION: the default of large grids)
    lazy = (ng[0] + ng[1] + nsteps) % 2 == 0
    if lazy:
        monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    out = {}
    for mode in ("fold", "separate"):
        if mode == "separate":
            monkeypatch.setenv("CALES_UNFOLDED_MOM", "1")
        case = _nosgs_case(name, ng)
        h = HotPath(case); u, v, w, p = initflow(case)
        rng = np.random.RandomState(2)
        for a in (u, v, w):
            a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)
        h.upload(u, v, w, p); h.startup(); dt = 0.5 * h.chkdt()
        h.profile(True)
        for _ in range(nsteps):
            h.step(dt)
        out[mode] = h.download() + [h.get("pp"), h.chkdiv()[1], h.dpdl()]
        h.profile(False); st = h.profile_stats()
        ncorr = st.get("correc_updatep", (0, 0.))[0] + st.get("correc", (0, 0.))[0]      # (z-implicit diffusion, folded: the completion corrects the velocity only)
        # the fold is what ran: no correction pass inside the steps (the last projection is completed by the download above), three per step otherwise
        assert ncorr == ((1 if lazy else nsteps) if mode == "fold" else 3 * nsteps), (mode, lazy, ncorr)
        h.close()
    for nm, a, b in zip(("u", "v", "w", "p", "visct", "pp"), out["fold"], out["separate"]):
        assert relerr(a, b) < 1e-12, nm
    assert out["fold"][6] < 2. * out["separate"][6] + 1e-12 and np.abs(np.asarray(out["fold"][7]) - np.asarray(out["separate"][7])).max() < 1e-12 * max(1., np.abs(np.asarray(out["separate"][7])).max())


def test_pending_projection_is_completed_by_every_entry_that_looks(monkeypatch):
    """CALES_LAZY_PROJECTION (the default of large one-rank grids): cales_step returns with the third substep's projection pending. cales_sync completes it
    (one correction pass, once), a second sync does nothing more, the next step consumes a pending projection in its first momentum pass without any
    correction pass, and chkdiv -- which reads the velocity -- sees a divergence-free field right after a step."""
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    case = _nosgs_case("cavity_nnn", (32, 16, 12))
    h = HotPath(case); h.upload(*initflow(case)); h.startup(); dt = 0.5 * h.chkdt()
    ncorr = lambda: h.profile_stats().get("correc_updatep", (0, 0.))[0]
    h.profile(True)
    h.step(dt); assert ncorr() == 0
    h.sync(); assert ncorr() == 1
    h.sync(); assert ncorr() == 1
    h.step(dt); h.step(dt); h.step(dt); assert ncorr() == 1      # three steps, each consuming its predecessor's projection
    assert h.chkdiv()[1] < 1e-12 and ncorr() == 2
    h.profile(False); h.close()


# ---- every entry of include/cales.h that takes a context, against a projection left pending by cales_step (api.hip ENTER / finish_pending) ----
# entries that read or write no field (or are the consumer itself): they do not have to complete a pending projection
_NO_FIELD_ENTRIES = {"cales_destroy", "cales_last_error", "cales_local_size", "cales_get_forcing", "cales_get_dpdl", "cales_get_bcvel", "cales_step", "cales_describe_plan",
                     "cales_profile_enable", "cales_profile_reset", "cales_profile_count", "cales_profile_get", "cales_device_info",
                     "cales_comm_buffer_doubles", "cales_set_comm", "cales_set_comm_overlap", "cales_comm_init_rccl", "cales_memory_in_use"}


def _entry_calls(h, dt):
    """name -> a call of that entry with valid arguments on the context `h` (an explicit or z-implicit case without subgrid model)"""
    import ctypes as C
    from cales_amd import capi
    L, H = h.L, h.h
    z = lambda: h.zeros()
    r1 = capi.c_real(0.)
    n = h.n
    st = np.zeros((27, n[2]), order="F"); bud = np.zeros((38, n[2]), order="F"); lk = np.zeros((6, n[2]), order="F")
    o1 = np.zeros(n[2]); oc = np.zeros((7, n[2]), order="F"); od = np.zeros((9, n[1], n[2]), order="F")
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rk = np.array([32. / 60., 0.]); f3 = np.zeros(3)
    fld = [z() for _ in range(5)]
    return {
        "cales_sync": lambda: L.cales_sync(H),
        "cales_upload_state": lambda: L.cales_upload_state(H, *[P(a) for a in fld[:4]]),
        "cales_download_state": lambda: L.cales_download_state(H, *[P(a) for a in fld]),
        "cales_set_field": lambda: L.cales_set_field(H, capi.FIELDS["p"], P(fld[0])),
        "cales_get_field": lambda: L.cales_get_field(H, capi.FIELDS["u"], P(fld[0])),
        "cales_bounduvw": lambda: L.cales_bounduvw(H, 1, 0),
        "cales_boundp": lambda: L.cales_boundp(H, capi.FIELDS["p"], 0),
        "cales_mom": lambda: L.cales_mom(H),
        "cales_rk": lambda: L.cales_rk(H, 1, dt),
        "cales_rk_par": lambda: L.cales_rk_par(H, P(rk), dt, P(f3)),
        "cales_bulk_forcing": lambda: L.cales_bulk_forcing(H),
        "cales_bulk_mean": lambda: L.cales_bulk_mean(H, capi.FIELDS["u"], 1, C.byref(r1)),
        "cales_fillps": lambda: L.cales_fillps(H, 1. / dt),
        "cales_updt_rhs_b": lambda: L.cales_updt_rhs_b(H),
        "cales_solver": lambda: L.cales_solver(H),
        "cales_helmholtz_z": lambda: L.cales_helmholtz_z(H, 1, -1e-4),
        "cales_helmholtz": lambda: L.cales_helmholtz(H, 1, -1e-4),      # (refused without 3-D implicit diffusion -- AFTER the pending projection was completed)
        "cales_correc": lambda: L.cales_correc(H, dt),
        "cales_updatep": lambda: L.cales_updatep(H, 0.),
        "cales_cmpt_sgs": lambda: L.cales_cmpt_sgs(H),
        "cales_chkdt": lambda: L.cales_chkdt(H, C.byref(r1)),
        "cales_chkdiv": lambda: L.cales_chkdiv(H, C.byref(r1), C.byref(capi.c_real(0.))),
        "cales_out1d_single_point_chan": lambda: L.cales_out1d_single_point_chan(H, P(st)),
        "cales_out1d_chan_budgets": lambda: L.cales_out1d_chan_budgets(H, P(bud), P(lk)),
        "cales_out1d": lambda: L.cales_out1d(H, capi.FIELDS["u"], 3, 0, P(o1)),
        "cales_out1d_chan": lambda: L.cales_out1d_chan(H, P(oc)),
        "cales_out2d_duct": lambda: L.cales_out2d_duct(H, P(od)),
        "cales_calibrate": lambda: L.cales_calibrate(H, 1, P(f3), None),
    }


def _header_ctx_entries():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cales.h")).read()
    return sorted(set(re.findall(r"\b(cales_[a-z_0-9]+)\s*\(\s*(?:const\s+)?cales_ctx\s*\*", hdr)))


@pytest.mark.parametrize("first", ["chkdt", "chkdiv", "get_field", "stats", "cmpt_sgs"])
@pytest.mark.parametrize("name,ng", [("chan_dsmag", (64, 16, 12)), ("chan_smag", (64, 18, 12)), ("tgv_dsmag_ppp", (64, 16, 16))])
def test_x_ghost_columns_are_refreshed_for_the_first_reader(name, ng, first, monkeypatch):
    """cales_step with periodic x leaves the x ghost columns alone (its kernels wrap around) and, since round 5, returns with them STALE: the next cales_step
    does not read them, every other entry of include/cales.h brings them up to date before it does anything else (finish_pending, pend_xrefresh). Whatever
    entry comes first after the steps -- a reduction that reads u(n1+1), a download, the plane statistics, an operator -- must see what the eager form
    (CALES_EAGER_PROJECTION, refresh inside the step) sees: same scalars, same fields, ghost cells included, to the last bit."""
    from cales_amd.hotpath import HotPath, initflow
    g, case = load_golden(name); case.ng[:] = ng
    u0 = initflow(case)
    rng = np.random.RandomState(2)
    for a in u0[:3]:
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*ng) - 0.5)

    def run():
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.4 * h.chkdt()
        for _ in range(3):
            h.step(dt)
        out = {}
        if first == "chkdt": out["chkdt"] = h.chkdt()
        elif first == "chkdiv": out["chkdiv"] = h.chkdiv()
        elif first == "get_field": out["w"] = h.get("w")
        elif first == "stats": out["stats"] = h.stats_chan()
        else: h.cmpt_sgs()
        out["fields"] = h.download(); out["dt2"] = h.chkdt(); out["div"] = h.chkdiv()
        h.close()
        return out
    lazy = run()
    monkeypatch.setenv("CALES_EAGER_PROJECTION", "1")
    eager = run()
    for k in lazy:
        if k == "fields":
            for a, b, nm in zip(lazy[k], eager[k], "uvwps"):
                assert np.array_equal(a, b), nm
        else:
            assert np.array_equal(np.asarray(lazy[k]), np.asarray(eager[k])), k


@pytest.mark.parametrize("name", ["cavity_nnn", "chan_nosgs_imp1d"])
def test_every_entry_sees_the_projected_state(name, monkeypatch):
    """The pending-projection contract, mechanically (the state protected is src/main.f90:498-504): after a cales_step that leaves its
    last projection to its successor, EVERY entry of include/cales.h that takes a context and reads or writes a field completes the projection before it
    does anything else -- enumerated from the header, so an entry added later fails here until it is classified. Detected by the profile counters (one
    correction pass appears), and by value: the velocity the entry leaves behind is divergence-free where the entry does not change it."""
    from cales_amd.hotpath import HotPath, initflow
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    case = _nosgs_case(name, (32, 16, 12))
    entries = _header_ctx_entries()
    assert "cales_sync" in entries and "cales_get_field" in entries and len(entries) > 40, entries
    probe = HotPath(case); table = _entry_calls(probe, 1e-3); probe.close()
    unclassified = [e for e in entries if e not in table and e not in _NO_FIELD_ENTRIES]
    assert not unclassified, f"entries of include/cales.h without a rule for a pending projection: {unclassified}"
    u0 = initflow(case)
    for e in entries:
        if e in _NO_FIELD_ENTRIES:
            continue
        h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.5 * h.chkdt()
        ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))
        h.profile(True)
        h.step(dt)
        assert ncorr() == 0, (e, "the step was expected to leave its last projection pending")
        rc = _entry_calls(h, dt)[e]()
        assert ncorr() >= 1, (e, "did not complete the pending projection")
        # (the two Helmholtz entries refuse a case without the matching implicit diffusion -- after the pending projection was completed)
        assert rc == 0 or e == "cales_helmholtz" or (e == "cales_helmholtz_z" and case.impdiff != 2), (e, h.L.cales_last_error(h.h))
        if e in ("cales_sync", "cales_get_field", "cales_download_state", "cales_chkdt", "cales_bulk_mean", "cales_boundp", "cales_out1d", "cales_out1d_chan", "cales_helmholtz"):
            n1 = ncorr()
            assert h.chkdiv()[1] < 1e-12, e      # what the entry saw was the projected velocity
            assert ncorr() == n1, e              # ... and nothing was pending any more
        h.profile(False); h.close()
    # the entries that deliberately do not complete it leave it pending (and the next step still consumes it)
    h = HotPath(case); h.upload(*u0); h.startup(); dt = 0.5 * h.chkdt()
    ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))
    h.profile(True); h.step(dt)
    h.dpdl(); f = np.zeros(3); h._chk(h.L.cales_get_forcing(h.h, f.ctypes.data_as(__import__("ctypes").c_void_p))); h.bcvel_planes(1)
    assert ncorr() == 0
    h.step(dt); assert ncorr() == 0
    assert h.chkdiv()[1] < 1e-12 and ncorr() == 1
    h.profile(False); h.close()


@pytest.mark.parametrize("is_correc", [False, True], ids=["impose", "is_correc"])
@pytest.mark.parametrize("name,ng", [("duct_smag_wm", (16, 12, 10)), ("duct_dsmag", (24, 10, 12)), ("cavity_nnn", (12, 10, 14)), ("halfchan_imp1d", (16, 12, 10)),
                                     ("devchan_nd", (14, 8, 10)), ("chan_smag_wm", (16, 8, 12)), ("cavity_dsmag", (10, 12, 8)),
                                     # wall-model faces in x, on one side of a direction, under moving walls
                                     ("cavity_smag_wm6", (12, 10, 14)), ("cavity_dsmag_wm_mixed", (10, 12, 8)), ("chan_smag_wm_mov", (16, 8, 12)), ("halfchan_dsmag_wm", (16, 12, 10))])
def test_all_directions_ghost_cell_kernel_equals_the_sequence(name, ng, is_correc, monkeypatch):
    """k_bc_all (every direction of a bounduvw / boundp in one launch: the closed form Z(Y(X(stored))) of bound.f90:158-199) against the reference's
    order, one launch per direction (CALES_UNMERGED_BC), on RANDOM fields -- ghost cells included, so that every corner and edge cell and every cell a
    direction leaves alone is told apart -- for ducts (with and without wall model), cavities, a half channel (free-slip top), inflow / outflow (Neumann on
    face-centred data: not served, both runs take the sequence) and a wall-modelled channel (the periodic kernel + the wall-model faces)."""
    g, case = load_golden(name); case.ng[:] = ng
    rng = np.random.RandomState(11)
    shape = tuple(x + 2 for x in ng)
    f0 = [F(rng.rand(*shape) - 0.5) for _ in range(5)]
    out = {}
    for mode in ("all", "sequence"):
        if mode == "sequence":
            monkeypatch.setenv("CALES_UNMERGED_BC", "1")
        h = _hot(case)
        h.upload(*f0[:4]); h.set("visct", f0[4]); h.set("pp", f0[3])
        h.bounduvw(True, is_correc); h.boundp("p", 0); h.boundp("visct", 1); h.boundp("pp", 0)
        out[mode] = [h.get(k) for k in ("u", "v", "w", "p", "visct", "pp")]
        h.close()
    for nm, a, b in zip(("u", "v", "w", "p", "visct", "pp"), out["all"], out["sequence"]):
        assert np.abs(a - b).max() <= 4e-16 * max(1., np.abs(b).max()), (nm, np.abs(a - b).max())


@pytest.mark.parametrize("name,env,expect", [
    ("chan_dsmag_x64", {}, {"projection": "in_strain_rate_pass", "x_ghost_columns": "wrapped", "fillps": "in_x_transform", "ghost_cells": "one_launch",
                            "sgs": "dsmag_tiles(pair_fields)", "solver": "x:PP/radix8,y:PP/radix8_register_ends,z:lds_tile,modes_0_and_n1/2:one_column", "exchanges": "none"}),
    ("chan_dsmag_x64", {"CALES_NO_NYQUIST_PACKING": "1"}, {"solver": "x:PP/radix8,y:PP/radix8_register_ends,z:lds_tile"}),
    ("chan_dsmag_x64", {"CALES_UNMERGED_BC": "1"}, {"projection": "own_pass(correc+updatep)", "ghost_cells": "by_direction", "sgs": "dsmag_tiles"}),
    ("chan_dsmag", {}, {"projection": "own_pass(correc+updatep)", "x_ghost_columns": "maintained", "fillps": "own_pass", "solver": "x:PP/mixed_radix,y:PP/mixed_radix,z:lds_tile"}),
    ("chan_dsmag", {"CALES_DSMAG_REFERENCE_SEQUENCE": "1", "CALES_GAUSSEL_MARCH": "1"}, {"sgs": "dsmag_reference_sequence", "solver": "x:PP/mixed_radix,y:PP/mixed_radix,z:thomas_march"}),
    ("chan_smag_wm_x64", {}, {"projection": "own_pass(correc+updatep)", "sgs": "smag_rows", "x_ghost_columns": "maintained"}),
    ("chan_smag_wm_x64", {"CALES_UNFUSED_FORCING": "1"}, {"bulk_forcing": "own_pass"}),
    ("duct_smag_wm_imp1d_x64", {}, {"implicit_rhs": "in_helmholtz_sweep", "bulk_forcing": "in_helmholtz_sweep", "solver": "x:PP/radix8,y:NN/mixed_radix,z:lds_tile"}),
    ("cavity_nnn_x64", {}, {"projection": "in_next_momentum_pass(substeps_1_2)", "solver": "x:NN/radix8,y:NN/radix8,z:lds_tile", "sgs": "none", "visct_ghost_cells": "zero_field"}),
    ("cavity_nnn_x64", {"CALES_LAZY_PROJECTION": "1"}, {"projection": "in_next_momentum_pass(all_substeps)"}),
    ("cavity_dsmag", {}, {"sgs": "dsmag_reference_sequence", "projection": "own_pass(correc+updatep)"}),
    ("tgv_ppp_x64", {"CALES_UNFOLDED_MOM": "1", "CALES_KEEP_NULL_MODE": "1"}, {"projection": "own_pass(correc+updatep)", "solver": "x:PP/radix8,y:PP/radix8_register_ends,z:lds_tile_periodic,null_mode:reference_order"}),
    # wall models beyond the shipped examples. Faces in x: the first wall-model update of a substep is kept (make_plan), the sequence is the only form
    # (sgs_setup: xw); faces in z alone, one law per wall or one wall only: skipped, the row form and the tiles (pair fields: x and y periodic, the normal
    # velocity prescribed at both z ends -- the free-slip top of the half channel is_wall for the filters as in the reference)
    ("cavity_smag_wm6_x64", {}, {"first_wall_model_update": "kept", "sgs": "smag_reference_sequence", "bulk_forcing": "none"}),
    ("chan_smag_wm_mov_x64", {}, {"first_wall_model_update": "skipped", "sgs": "smag_rows"}),
    ("halfchan_dsmag_wm_x64", {}, {"first_wall_model_update": "skipped", "sgs": "dsmag_tiles(pair_fields)"}),
])
def test_step_plan_is_a_value(name, env, expect, monkeypatch):
    """The path of a step is a VALUE (struct StepPlan, api.hip make_plan): computed from the case, the switches and the context's state, read by step_body,
    printed by cales_describe_plan. Held here against the cases whose goldens pin each path (the sequence protected: src/main.f90:417-508), before and
    after a step (the plan describes the NEXT step and must not change by taking one), and across a change of the state it was made from."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, case = load_golden(name)
    h = _hot(case)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    pl = h.describe_plan()
    for k, v in expect.items():
        assert pl.get(k) == v, (k, pl)
    assert pl["ranks"] == "1"
    if "first_wall_model_update" in pl and case.impdiff == 0 and not env and np.any(case.is_forced):      # the deferred forcing needs the first wall-model update to be dead work
        assert pl["bulk_forcing"] == ("in_correction(means_in_x_transform)" if pl["first_wall_model_update"] == "skipped" else "own_pass"), pl
    h.step(float(g["dt"]))
    assert h.describe_plan() == pl
    if pl["sgs"] == "none" and pl["projection"].startswith("in_next_momentum_pass"):
        # an eddy viscosity set by hand: the momentum pass reads it again, the fold that assumes a zero field is off, and the plan says so
        h.set("visct", h.zeros() + 1e-5)
        pl2 = h.describe_plan()
        assert pl2["projection"] == "own_pass(correc+updatep)" and pl2["visct_ghost_cells"] == "updated", pl2
        h.step(float(g["dt"])); assert h.chkdiv()[1] < 1e-11
    h.close()

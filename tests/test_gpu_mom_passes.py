"""The fused momentum pass (k_momrk.hip: momrk_kernel picks one of 64 instantiations -- IMP 0/1/2 x offset type x NOS x RD x WR, and the two CORR forms x offset
type x RD x WR -- op_momrk launches it under the name momrk_kernel spells) held to the CPU oracle BY VALUE on grids whose tile seams lie inside the field: 64-lane
tiles in x (a tile two lanes short, a whole one, a second tile of two cells, three tiles: the band map), 10-row tiles in y (one, one and two rows, two whole
ones, three), k chunks whose last prologue and prefetch clamp at n3 + 1, two planes.

1. Operator level (test_substeps_at_tile_seams): cales_rk of the substeps 1, 2, 3, each fed the oracle's state of its stage, against o_rk -- the new velocity, the
   r.h.s. the pass STORED (read back after the swap, against o_mom of the same input; with implicit diffusion the diffusive part too) and the forcing, interior
   cells, 1e-13 of the field's maximum (the bar of the operator tests of tests/test_gpu_golden.py and of test_forcing_operators). Seven case families span IMP x NOS,
   both offset types. test_lazy_eddy_viscosity_at_tile_seams: the dynamic model's lazy form, visct = |S| cs(k) scaled while the pass loads its planes.
2. Whole steps (test_steps_reach_the_forms_of_cales_step): the forms only cales_step launches -- the third substep's WR = 0, the projection applied on load
   (CORR = 1, 2), wrapped x columns, a first substep with a pending projection (CALES_LAZY_PROJECTION) -- against the oracle's step at the bars of
   test_time_steps (u, v, w 1e-9, p without its mean 1e-8: BASELINE.md 5), and where the projection is folded against the same library with CALES_UNFOLDED_MOM
   on the same device, all fields with their ghost cells to 1e-12 (the bar tools/fuzz_fold_mom.py holds the pair to).
3. The table is held to what it claims (test_each_row_reaches_the_instantiation_it_claims): with CALES_TEST_BAD_LAUNCH set to an instantiation's name the row that
   claims it fails naming it -- the runtime refuses that launch for its block size, nothing runs. test_every_instantiation_is_claimed_or_unreachable: the 64
   names, each claimed by a row or listed in UNREACHABLE with the reason.

Every by-value case prints its largest error over its bar (pytest -s); profiles/mom_pass_table.md has the figures of one MI355X. The one near a bar: the stored
r.h.s. of u of halfchan_imp1d, 5.0e-14 to 7.9e-14 on every grid with or without a seam -- a box of unit length, advective fluxes of 127 and more per face against
a sum of 1.8 -- where every other family stays below 1e-14."""
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import RK, perturbed_start, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-13
SWITCHES = ("CALES_WIDE_OFFSETS", "CALES_KCHUNK", "CALES_LAZY_PROJECTION", "CALES_UNFOLDED_MOM", "CALES_TEST_BAD_LAUNCH")
WIDE, KCHUNK4, LAZY = {"CALES_WIDE_OFFSETS": "1"}, {"CALES_KCHUNK": "4"}, {"CALES_LAZY_PROJECTION": "1"}


def kname(imp, wide, nos, rd, wr, corr=0):
    """the instantiation as momrk_kernel spells it"""
    return "k_momrk<%d, %s, %d, %d, %d, %d>" % (imp, "size_t" if wide else "unsigned", nos, rd, wr, corr)


ALL = [kname(imp, wide, nos, rd, wr) for imp in (0, 1, 2) for wide in (0, 1) for nos in (0, 1) for rd in (0, 1) for wr in (0, 1)] + \
      [kname(imp, wide, 1, rd, wr, corr) for imp, corr in ((0, 1), (2, 2)) for wide in (0, 1) for rd in (0, 1) for wr in (0, 1)]
# (RD, WR) = (0, 0), a first substep whose r.h.s. nobody keeps: the entries of the C-ABI that take a substep alone (cales_rk, cales_rk_par) always store the
# r.h.s. (RkOpts::store_rhs defaults to true), and inside cales_step the one substep that drops it is the third, whose weight f2 of the old r.h.s. is not zero
_NO_RD_NO_WR = "RD = 0 with WR = 0: operator calls always store the r.h.s., and the only substep of cales_step that drops it reads the old one"
UNREACHABLE = {**{kname(imp, wide, nos, 0, 0): _NO_RD_NO_WR for imp in (0, 1, 2) for wide in (0, 1) for nos in (0, 1)},
               **{kname(imp, wide, 1, 0, 0, corr): _NO_RD_NO_WR for imp, corr in ((0, 1), (2, 2)) for wide in (0, 1)}}


def _duct_imp3d(case):      # (as test_time_steps_imp3d_with_walls sets it up: no wall model, no-slip walls, static Smagorinsky)
    case.impdiff = 1; case.lwm[:] = 0; case.sgstype = "smag"
    case.cbcsgs[:] = np.where(case.cbcvel[:, :, 0] == "P", "P", "D")


def _cavity_imp3d(case):
    case.impdiff = 1


# family: (golden, edit of the Case, IMP, NOS)
FAMILIES = {"chan_smag": ("chan_smag", None, 0, 0),                      # stretched z grid
            "tgv_ppp": ("tgv_ppp", None, 0, 1),
            "cavity_nnn": ("cavity_nnn", None, 0, 1),                    # walls on all six faces
            "cavity_nnn_imp3d": ("cavity_nnn", _cavity_imp3d, 1, 1),
            "duct_smag_imp3d": ("duct_smag_wm", _duct_imp3d, 1, 0),
            "halfchan_imp1d": ("halfchan_imp1d", None, 2, 1),
            "duct_smag_wm_imp1d": ("duct_smag_wm_imp1d", None, 2, 0),    # wall model: k_copy_ghosts runs too
            "chan_nosgs_x64": ("chan_nosgs_x64", None, 0, 1)}            # DNS channel with bulk forcing (the steps below)


def _case(fam, ng):
    from tests.test_gpu_filter2d import _shaped_case
    golden, edit, imp, nos = FAMILIES[fam]
    case = _shaped_case(golden, ng)      # (wall model: the sampling height inside the coarser grid)
    if np.any(case.lwm != 0):      # ... and below the last cell centre: with two planes 1.6 cells is above it (sanity.f90:224-231), the mid-height is not
        case.hwm = min(float(case.hwm), 0.5 * min(float(case.l[d]) for d in range(3) if case.lwm[:, d].any()))
    if edit:
        edit(case)
    assert int(case.impdiff) == imp and (case.sgstype == "none") == bool(nos), (fam, case.impdiff, case.sgstype)
    return case


def _hot(case):
    from cales_amd.hotpath import HotPath
    return HotPath(case)


class _switches:
    """the switches of a row, set for the lifetime of its contexts (run_case of tests/test_gpu_sgs_passes.py)"""

    def __init__(self, env, bad_launch=None):
        self.env = dict(env)
        if bad_launch:
            self.env["CALES_TEST_BAD_LAUNCH"] = bad_launch

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _rest_of_substep(o, case, dtrk, f, u, v, w, p, pp, visct):
    """main.f90:423-507 on the oracle (the body of tests/util.oracle_forcing_of_substeps behind its o.rk): the next cales_rk starts from the state the reference sequence gives"""
    alpha = 0.
    o.bulk_forcing(f, u, v, w)
    if case.impdiff:
        alpha = -.5 * case.visc * dtrk
        for iv, q in ((1, u), (2, v), (3, w)):
            if case.impdiff == 2:
                o.updt_rhs_b_velz(iv, alpha, q); o.solver_gaussel_z(iv, alpha, q)
            else:
                o.updt_rhs_b_vel(iv, alpha, q); o.solver_helmholtz(iv, alpha, q)
    o.bounduvw(u, v, w, True, False)
    o.fillps(1. / dtrk, u, v, w, pp); o.updt_rhs_b_p(pp); o.solver(pp); o.boundp(pp, 0)
    o.correc(dtrk, pp, u, v, w); o.bounduvw(u, v, w, True, True)
    o.updatep(alpha, pp, p); o.boundp(p, 0)
    o.cmpt_sgs(u, v, w, visct); o.boundp(visct, 1)


def _inner(a):
    return a[1:-1, 1:-1, 1:-1]


RHS = ("dudto", "dvdto", "dwdto")      # where the r.h.s. a substep stored sits after the swap of rk.f90:98-100
RHSD = ("dudtd", "dvdtd", "dwdtd")


# ------------------------------------------------------------------ 1. operator level
# one x tile two lanes short (lanes 62, 63 clamped, the right halo is the ghost column) and exactly one y tile | a whole x tile, a second y tile of two rows |
# a second x tile of two cells: seams at i = 64|65 and j = 10|11, two whole y tiles | three x tiles (the band map with a padded grid; the last of two cells),
# three y tiles (the last of two rows) -- and with chunks of 4, 4 and 1 planes, the last chunk's prologue and prefetch clamped at n3 + 1 | two planes
OP_GRIDS = [((62, 10, 5), {}), ((64, 12, 6), {}), ((66, 20, 5), {}), ((130, 22, 9), {}), ((130, 22, 9), KCHUNK4), ((64, 10, 2), {}),
            ((66, 20, 5), WIDE), ((130, 22, 9), WIDE)]
OP_FAMILIES = ("chan_smag", "tgv_ppp", "cavity_nnn", "cavity_nnn_imp3d", "duct_smag_imp3d", "halfchan_imp1d", "duct_smag_wm_imp1d")
OP_ROWS = [(fam, ng, env) for fam in OP_FAMILIES for ng, env in OP_GRIDS]


def row_id(fam, ng, env):
    return "-".join([fam, "%dx%dx%d" % tuple(ng)] + ["%s=%s" % (k[6:].lower(), env[k]) for k in sorted(env)])


def op_claims(fam, ng, env):
    _, _, imp, nos = FAMILIES[fam]
    wide = int("CALES_WIDE_OFFSETS" in env)
    return (kname(imp, wide, nos, 0, 1), kname(imp, wide, nos, 1, 1))


def run_substeps(fam, ng, env, bad_launch=None):
    """the three substeps of one row; returns the largest error of each compared quantity"""
    case = _case(fam, ng)
    _, _, imp, nos = FAMILIES[fam]
    with _switches(env, bad_launch):
        o = Oracle(case, nthreads=8); h = _hot(case)
        try:
            assert h.describe_plan()["momentum"] == "fused_mom_rk"
            (u, v, w, p, visct, pp, dt), raw = perturbed_start(case, o)
            h.upload(*raw); h.startup()
            worst = {}
            for irk in (1, 2, 3):
                dtrk = (RK[irk - 1][0] + RK[irk - 1][1]) * dt
                h.upload(u, v, w, p)
                if not nos:      # (no subgrid model: the eddy viscosity stays the zeros it was created with, which is what selects NOS = 1)
                    h.set("visct", visct)
                rhs = o.mom(u, v, w, visct)
                hf = h.rk(irk, dt)
                f = o.rk(irk, dt, p, visct, u, v, w)
                ef = np.abs(hf - f).max() / max(1., np.abs(f).max())
                assert ef < TOL, (irk, "forcing", hf, f)
                assert all(hf[d] == 0. for d in range(3) if not case.is_forced[d]) and all(f[d] != 0. for d in range(3) if case.is_forced[d])
                errs = {"forcing": ef}
                for k, b in zip("uvw", (u, v, w)):
                    errs[k] = relerr(_inner(h.get(k)), _inner(b))
                for k, b in zip(RHS + (RHSD if imp else ()), rhs):
                    errs[k] = relerr(_inner(h.get(k)), b)
                for k in sorted(errs):
                    worst[k] = max(worst.get(k, 0.), errs[k])
                    assert errs[k] < TOL, (irk, k, errs[k])
                _rest_of_substep(o, case, dtrk, f, u, v, w, p, pp, visct)
            return worst
        finally:
            h.close(); o.close()


@pytest.mark.parametrize("fam,ng,env", OP_ROWS, ids=[row_id(*r) for r in OP_ROWS])
def test_substeps_at_tile_seams(fam, ng, env):
    worst = run_substeps(fam, ng, env)
    k = max(worst, key=worst.get)
    print("substeps", row_id(fam, ng, env), "largest error / bar %.3f (%s)" % (worst[k] / TOL, k), " ".join("%s %.1e" % (q, worst[q]) for q in sorted(worst)))


@pytest.mark.parametrize("ng", [(66, 20, 6), (130, 22, 9)], ids=lambda ng: "%dx%dx%d" % tuple(ng))
def test_lazy_eddy_viscosity_at_tile_seams(ng):
    """chan_dsmag: after cmpt_sgs the field holds |S| and the momentum pass multiplies by cs(k) while loading (MomRkArgs::cs), as long as nobody reads visct. The
    oracle's rk is fed the eddy viscosity a SECOND, identical context returned after the same cmpt_sgs: the dynamic model's deliberate re-association
    (1e-11 / 1e-10) stays out of the comparison and the bar at 1e-13. That the first context never scaled the field itself is held by making
    that launch (k_scale_planes, materialize_visct) invalid for it: the case would fail naming it."""
    from tests.test_gpu_filter2d import _shaped_case
    case = _shaped_case("chan_dsmag", ng)
    o = Oracle(case, nthreads=8)
    with _switches({}, bad_launch="k_scale_planes"):
        h = _hot(case)
    with _switches({}):
        h2 = _hot(case)
    try:
        assert h.describe_plan()["momentum"] == "fused_mom_rk" and h.describe_plan()["sgs"].startswith("dsmag_tiles"), h.describe_plan()
        (u, v, w, p, visct, pp, dt), raw = perturbed_start(case, o)
        for x in (h, h2):      # (the ghost-cell update of a field that only WRITES it keeps the lazy form: the rule is linear and homogeneous, cs(0) and cs(n3 + 1) follow it)
            x.upload(u, v, w, p); x.cmpt_sgs(); x.boundp("visct", 1)
        vis = h2.get("visct")
        # not all zeros, and another field on every plane the clip of cs(k) (sgs.f90:359-379) leaves one on -- at least two of them
        planes = np.abs(_inner(vis)).max(axis=(0, 1)); live = planes[planes > 0.]
        assert np.isfinite(vis).all() and len(live) >= 2 and len(set(live.tolist())) == len(live), planes
        rhs = o.mom(u, v, w, vis)
        hf = h.rk(1, dt); f = o.rk(1, dt, p, vis, u, v, w)
        errs = {"forcing": np.abs(hf - f).max() / max(1., np.abs(f).max())}
        for k, b in zip("uvw", (u, v, w)):
            errs[k] = relerr(_inner(h.get(k)), _inner(b))
        for k, b in zip(RHS, rhs):
            errs[k] = relerr(_inner(h.get(k)), b)
        k = max(errs, key=errs.get)
        print("lazy visct chan_dsmag %dx%dx%d" % tuple(ng), "largest error / bar %.3f (%s)" % (errs[k] / TOL, k), " ".join("%s %.1e" % (q, errs[q]) for q in sorted(errs)))
        for k in sorted(errs):
            assert errs[k] < TOL, (k, errs[k])
    finally:
        h.close(); h2.close(); o.close()


# ------------------------------------------------------------------ 2. the forms only cales_step reaches
# two x tiles | a last x tile of 32 cells: with wrapped x columns the lane right of the last cell loads the first column | three x tiles: the band map together with
# CORR, the 3 * 2^p transform plan
STEP_GRIDS = [(128, 22, 6), (96, 22, 5), (192, 12, 5)]
FOLD_FAMILIES = ("chan_nosgs_x64", "tgv_ppp", "cavity_nnn", "halfchan_imp1d")
# (kind, family, grid, switches). fold: the projection rides in the next momentum pass -- against the oracle and against CALES_UNFOLDED_MOM. The size_t forms of
# both: one lazy row per CORR (two steps of a lazy row launch all three (RD, WR) of its CORR form). oracle: the families whose projection stays a pass of its
# own, for the third substep's WR = 0 of their IMP x NOS, both offset types
STEP_ROWS = [("fold", fam, ng, env) for fam in FOLD_FAMILIES for ng in STEP_GRIDS for env in ({}, LAZY)] + \
            [("fold", "tgv_ppp", (96, 22, 5), {**LAZY, **WIDE}), ("fold", "halfchan_imp1d", (192, 12, 5), {**LAZY, **WIDE})] + \
            [("oracle", fam, (66, 20, 6), env) for fam in ("chan_smag", "cavity_nnn_imp3d", "duct_smag_imp3d", "duct_smag_wm_imp1d") for env in ({}, WIDE)]


def step_id(kind, fam, ng, env):
    return kind + "-" + row_id(fam, ng, env)


def step_claims(kind, fam, ng, env):
    _, _, imp, nos = FAMILIES[fam]
    wide = int("CALES_WIDE_OFFSETS" in env)
    plain = tuple(kname(imp, wide, nos, rd, wr) for rd, wr in ((0, 1), (1, 1), (1, 0)))      # no pending projection: the oracle rows, and the CALES_UNFOLDED_MOM run of the others
    if kind == "oracle":
        return plain
    corr = 2 if imp == 2 else 1
    return plain + tuple(kname(imp, wide, 1, rd, wr, corr) for rd, wr in ((1, 1), (1, 0)) + (((0, 1),) if "CALES_LAZY_PROJECTION" in env else ()))


def _two_steps(case, raw, dt):
    h = _hot(case)
    try:
        h.upload(*raw); h.startup()
        plan = h.describe_plan()      # (the plan of the steps is known once the start-up has run the first cmpt_sgs)
        assert abs(h.chkdt() / (2 * dt) - 1) < 1e-12
        for _ in range(2):
            h.step(dt)
        return plan, h.download() + [h.get("pp")]
    finally:
        h.close()


def run_steps(kind, fam, ng, env, bad_launch=None):
    case = _case(fam, ng)
    o = Oracle(case, nthreads=8)
    try:
        (u, v, w, p, visct, pp, dt), raw = perturbed_start(case, o)
        with _switches(env, bad_launch):
            plan, got = _two_steps(case, raw, dt)
        assert plan["momentum"] == "fused_mom_rk", plan
        if kind == "fold":
            assert plan["projection"] == "in_next_momentum_pass(" + ("all_substeps" if "CALES_LAZY_PROJECTION" in env else "substeps_1_2") + ")", plan
        for _ in range(2):
            o.step(dt, u, v, w, p, pp, visct)
        errs = {k: relerr(a, b) / 1e-9 for k, a, b in zip("uvw", got, (u, v, w))}
        errs["p"] = relerr(_inner(got[3]) - _inner(got[3]).mean(), _inner(p) - _inner(p).mean()) / 1e-8
        k = max(errs, key=errs.get)
        print("steps", step_id(kind, fam, ng, env), "against the oracle: largest error / bar %.3g (%s)" % (errs[k], k), " ".join("%s %.1e" % (q, errs[q]) for q in sorted(errs)))
        for k in sorted(errs):
            assert errs[k] < 1., (k, errs[k])
        if kind == "fold":
            with _switches({**env, "CALES_UNFOLDED_MOM": "1"}, bad_launch):
                plan2, ref = _two_steps(case, raw, dt)
            assert not plan2["projection"].startswith("in_next_momentum_pass"), plan2
            # (pp of the triply periodic box: its round-off-defined constant moves the last digits, the velocity and p do not see it -- tools/fuzz_fold_mom.py)
            errs = {k: relerr(a, b) / (1e-10 if (k == "pp" and fam == "tgv_ppp") else 1e-12) for k, a, b in zip(("u", "v", "w", "p", "visct", "pp"), got, ref)}
            k = max(errs, key=errs.get)
            print("steps", step_id(kind, fam, ng, env), "against CALES_UNFOLDED_MOM: largest error / bar %.3g (%s)" % (errs[k], k), " ".join("%s %.1e" % (q, errs[q]) for q in sorted(errs)))
            for k in sorted(errs):
                assert errs[k] < 1., (k, errs[k])
    finally:
        o.close()


@pytest.mark.parametrize("kind,fam,ng,env", STEP_ROWS, ids=[step_id(*r) for r in STEP_ROWS])
def test_steps_reach_the_forms_of_cales_step(kind, fam, ng, env):
    run_steps(kind, fam, ng, env)


# ------------------------------------------------------------------ 3. the table is held to what it claims
CLAIMS = {}      # instantiation -> the first row that claims it
for _r in OP_ROWS:
    for _k in op_claims(*_r):
        CLAIMS.setdefault(_k, (run_substeps, _r, row_id(*_r)))
for _r in STEP_ROWS:
    for _k in step_claims(*_r):
        CLAIMS.setdefault(_k, (run_steps, _r, step_id(*_r)))


def test_every_instantiation_is_claimed_or_unreachable():
    assert len(ALL) == 64 and len(set(ALL)) == 64
    assert not set(CLAIMS) & set(UNREACHABLE)
    assert set(CLAIMS) | set(UNREACHABLE) == set(ALL), sorted(set(ALL) - set(CLAIMS) - set(UNREACHABLE))
    assert all(not (a != b and a in b) for a in ALL for b in ALL)      # (the hook matches substrings: no name may hide in another)
    print("k_momrk: %d instantiations claimed, %d unreachable" % (len(CLAIMS), len(UNREACHABLE)))


@pytest.mark.parametrize("kernel", sorted(CLAIMS), ids=lambda k: k.replace(" ", ""))
def test_each_row_reaches_the_instantiation_it_claims(kernel):
    """with that one kernel made unlaunchable the row fails, and the message names it"""
    from cales_amd.hotpath import CalesError
    run, row, _ = CLAIMS[kernel]
    with pytest.raises(CalesError) as e:
        run(*row, bad_launch=kernel)
    assert "kernel launch failed" in str(e.value) and kernel in str(e.value), e.value

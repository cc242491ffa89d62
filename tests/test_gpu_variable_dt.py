"""Whole steps through cales_step against the CPU oracle under a time step that changes at EVERY step (DT_FACTORS of tests/util.py: seven steps, five
different dt), as a production run changes it at every icheck block. Since the step carries dt-dependent state between operators, substeps and steps
-- the pending projection {dtrk, fmask, p_done, xskip} a step leaves to its successor's first momentum pass or to finish_pending, the corrected ghost-cell
view (BcCall::view_dtrk), the projection inside the strain-rate pass (SgsFold::dtrk), the deferred forcing increment that rides with either, step_dt of
cales_get_dpdl, the ghost rows the folded projection scales on slabs (tests/test_gpu_decomp.py), the alpha of the 3-D Helmholtz solves -- a factor taken
from the wrong step cannot be seen at a constant dt. tests/test_variable_dt_oracle.py shows on the oracle alone that each such mistake costs 3e-6 .. 1e-1
of the field maximum under this schedule, three decades and more above the bars here, which are those of BASELINE.md 5: u, v, w 1e-9, p (mean removed)
1e-8, visct 1e-7, divmax < 20 x oracle + 1e-14, dpdl and the last substep's forcing 1e-9 max(1, |.|), forced bulk means within 1e-10 of the oracle's,
chkdt 1e-7 relative (the loosest bar among its inputs).

Measured on an MI355X, the largest over all rows (printed per row as `WORST`): u, v, w 8.0e-14, p 1.3e-12, visct 1.2e-13, dpdl 6.5e-13, the last forcing
1.2e-14, chkdt 9.7e-14 -- chkdt sits six decades below its bar, which stays where its inputs put it. One row stands apart: tgv_dsmag_ppp 64 x 16 x 24 with
2.3e-10, 3.1e-9, 5.5e-10 and chkdt 1.2e-11. That is the triply periodic box whose n3 is no power of two (dzf not exactly uniform, the singular pressure
problem incompatible, a mean pressure of -1e6 that takes the digits: test_time_steps, triperiodic_bounds), not the schedule: seven steps at a constant
dt give 4.3e-10, 7.8e-9, 1.6e-9 there, and 64 x 16 x 32 gives 4e-15 either way. A build whose next momentum pass took the CURRENT step's dtrk for the
pending projection failed the five all_substeps rows without reads by 4.7e-5 (cavity) .. 2.0e-3 (channel) in u, v, w; nothing fails on the library as it is.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import (DT_FACTORS, VARIABLE_DT_COMBINATION_GRIDS, VARIABLE_DT_IDS, VARIABLE_DT_PARAMS, relerr, steps_under_schedule, variable_dt_case)

pytestmark = pytest.mark.gpu


def _hot(case):
    from cales_amd.hotpath import HotPath
    if case.sgstype == "none" and case.cbcvel[0, 0, 0] != "P":      # see tests/test_gpu_golden.py
        case.cbcsgs[:, 0] = "D"
    return HotPath(case)


def _plan_says(pl, expect):
    for k, v in expect.items():
        assert (pl.get(k, "").startswith(v[:-1]) and k in pl) if v.endswith("*") else pl.get(k) == v, (k, v, pl)


def _against_the_oracle(case, h, o, state, worst, tag):
    """the fields and forced bulk means after the schedule, each printed before it is held to its bar"""
    u, v, w, p, visct = state
    gu, gv, gw, gp, gvis = h.download()
    errs = [relerr(a, b) for a, b in ((gu, u), (gv, v), (gw, w))]
    ep = relerr(gp[1:-1, 1:-1, 1:-1] - gp[1:-1, 1:-1, 1:-1].mean(), p[1:-1, 1:-1, 1:-1] - p[1:-1, 1:-1, 1:-1].mean())
    ev = relerr(gvis, visct) if np.abs(visct).max() > 0. else float(np.abs(gvis).max())
    print(tag, "relerr u, v, w", errs, "p", ep, "visct", ev, "dpdl", worst["dpdl"], "forcing", worst["forcing"], "chkdt", worst["chkdt"], "divmax (device, oracle)", worst["div"])
    print("WORST", tag, " ".join(f"{x:.2e}" for x in (max(errs), ep, ev, worst["dpdl"], worst["forcing"], worst["chkdt"])))
    for e, nm in zip(errs, "uvw"):
        assert e < 1e-9, (nm, e)
    assert ep < 1e-8, ep
    assert ev < 1e-7, ev
    for d, (fld, b, wgt) in enumerate((("u", u, "f"), ("v", v, "f"), ("w", w, "c"))):
        if case.is_forced[d]:
            m, mo = h.bulk_mean(fld, wgt), o.bulk_mean(b, wgt)
            print(tag, "bulk mean of", fld, m, "oracle", mo)
            assert abs(m - mo) < 1e-10, (fld, m, mo)


@pytest.mark.parametrize("name,ng,fset,edits,expect,env,reads", VARIABLE_DT_PARAMS, ids=VARIABLE_DT_IDS)
def test_steps_with_a_changing_time_step(name, ng, fset, edits, expect, env, reads, monkeypatch):
    """Every projection path of the plan (asserted through cales_describe_plan), with nothing between two steps (`reads` False: what a step left to its
    successor meets another dt) and with the production loop's block between them (chkdt, chkdiv, dpdl, the last forcing, each against the oracle's value for
    that step). Where the third substep's projection is the next step's (all_substeps) the profile scopes show that no stand-alone correction ran before the
    first read, and that each block of reads completed exactly one."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = variable_dt_case(name, ng, fset, edits)
    tag = " ".join(str(x) for x in (name, ng, fset, edits, env, "reads" if reads else "no reads"))
    o = Oracle(case, nthreads=8); h = _hot(case)
    ncorr = lambda: sum(h.profile_stats().get(k, (0, 0.))[0] for k in ("correc_updatep", "correc"))      # noqa: E731
    lazy, nblocks = [False], [0]

    def hook(n, what):
        if what == "started":      # (the plan depends on the state the start-up leaves: visct = 0 for good without a model)
            pl = h.describe_plan()
            print("PLAN", tag, pl)
            _plan_says(pl, expect)
            lazy[0] = pl["projection"] == "in_next_momentum_pass(all_substeps)"
            if lazy[0]:
                h.profile(True)
        elif not lazy[0]:
            return
        elif what == "stepped":
            assert ncorr() == nblocks[0], (n, "a step completed its own last projection", ncorr())
        else:
            nblocks[0] += 1
            assert ncorr() == nblocks[0], (n, "one completion per block of reads", ncorr())
    state, dt0, worst = steps_under_schedule(case, o, h, reads, hook=hook, tag=tag)
    if lazy[0]:
        assert nblocks[0] == (len(DT_FACTORS) if reads else 1)
        h.profile(False)
    assert lazy[0] == ("CALES_LAZY_PROJECTION" in env and "in_next_momentum_pass" in expect.get("projection", ""))
    _against_the_oracle(case, h, o, state, worst, tag)
    h.close(); o.close()


def test_a_field_set_by_hand_between_two_steps(monkeypatch):
    """step_body's path 'the conditions changed between two steps': the channel without a model, every projection left to the next momentum pass, no reads;
    after the third step u is read (which completes the pending projection) and set again, and the schedule goes on -- the result is the oracle's as before."""
    monkeypatch.setenv("CALES_LAZY_PROJECTION", "1")
    case = variable_dt_case("chan_nosgs_x64", (64, 24, 16), "B", {})
    o = Oracle(case, nthreads=8); h = _hot(case)

    def hook(n, what):
        if what == "started":
            _plan_says(h.describe_plan(), {"projection": "in_next_momentum_pass(all_substeps)"})
        if n == 2 and what == "stepped":
            h.set("u", h.get("u"))
    tag = "chan_nosgs_x64 u set by hand after step 3"
    state, dt0, worst = steps_under_schedule(case, o, h, False, hook=hook, tag=tag)
    _against_the_oracle(case, h, o, state, worst, tag)
    h.close(); o.close()


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("name,ng", VARIABLE_DT_COMBINATION_GRIDS)
def test_switch_combinations_with_a_changing_time_step(name, ng, seed, monkeypatch):
    """The draw of test_time_steps_with_switch_combinations (the same switches, the seeds 1000 + seed), seven steps under the schedule."""
    import tests.test_gpu_vs_oracle as V
    rng = np.random.RandomState(1000 + seed)
    chosen = rng.choice(V._BOOL_SWITCHES, size=rng.randint(3, 7), replace=False)
    for k in chosen:
        monkeypatch.setenv(str(k), "1")
    if rng.rand() < 0.5:
        monkeypatch.setenv("CALES_KCHUNK", str(rng.randint(3, 9)))
    V.test_time_steps(name, ng, len(DT_FACTORS), factors=DT_FACTORS)

"""The cases of tests/test_gpu_variable_dt.py on the CPU restatement ALONE, under the schedule DT_FACTORS of tests/util.py (seven steps, five different time
steps): (1) o.step handles a changing dt exactly as the operator sequence does, bit for bit; (2) a factor taken from the step before is no no-op -- the
three mistakes a step that carries dt-dependent state over a step boundary can make, each run on the oracle from the second step on, move u, v, w by far
more than the 1e-9 the device is held to; (3) dpdl of a step is -sum(f) / dt of THAT step; (4) the oracle's dynamic coefficient without averaging
(Case.dsmag_average = 'local'), which one row needs, is the -D_CAVITY reference's.

relerr against the unmutated run after the seven steps, the largest of u, v, w, then p with the mean removed (measured; the floors asserted are 1e-5 for
the four rows marked *, 1e-6 -- three decades above the device's bar -- for every other row):

  case, grid, forcing set          | stale dtrk in the 3rd correc | stale dt in the 1st rk | stale dtrki in the 1st fillps
  cavity_dsmag 16x16x12            | 1.3e-04, 2.7e-07             | 3.7e-02, 6.8e-03       | 9.9e-05, 7.6e-06
  cavity_nnn 16x16x16              | 2.9e-04, 2.1e-06             | 3.6e-02, 1.2e-02       | 2.3e-04, 1.8e-05
  chan_dsmag 128x12x20 B           | 1.4e-04, 3.9e-05             | 4.7e-02, 4.8e-02       | 1.7e-05, 6.5e-04
  chan_dsmag 32x16x16 B            | 3.7e-04, 3.1e-04             | 6.2e-02, 6.9e-02       | 1.9e-04, 9.5e-04
  chan_dsmag 32x16x16              | 7.1e-04, 2.2e-04             | 7.3e-02, 6.7e-02       | 1.8e-04, 8.1e-04
  chan_dsmag 64x20x12 B local      | 3.3e-04, 1.6e-04             | 6.8e-02, 6.8e-02       | 1.6e-04, 1.1e-03
 *chan_dsmag 64x20x12 B            | 4.0e-04, 2.0e-04             | 7.2e-02, 7.4e-02       | 1.3e-04, 1.1e-03
  chan_dsmag 80x20x12 B            | 3.3e-04, 1.4e-04             | 6.2e-02, 7.2e-02       | 9.3e-05, 1.0e-03
  chan_dsmag_wm 64x16x12 B         | 4.7e-04, 2.4e-04             | 8.0e-02, 7.4e-02       | 1.1e-04, 1.3e-03
  chan_nosgs_x64 64x24x16 A        | 3.9e-04, 2.0e-04             | 6.8e-02, 8.3e-02       | 6.9e-05, 1.2e-03
  chan_nosgs_x64 64x24x16 B        | 3.1e-04, 1.6e-04             | 5.5e-02, 7.1e-02       | 6.9e-05, 8.7e-04
  chan_smag 24x20x12 B             | 4.3e-04, 3.5e-04             | 7.4e-02, 5.3e-02       | 1.3e-04, 9.7e-04
  chan_smag 64x12x10               | 7.2e-04, 1.8e-04             | 8.2e-02, 6.7e-02       | 1.5e-04, 1.4e-03
 *chan_smag 64x18x12 B             | 3.9e-04, 1.9e-04             | 7.4e-02, 7.3e-02       | 1.3e-04, 1.1e-03
  chan_smag_wm 32x16x12            | 8.5e-04, 2.9e-04             | 8.1e-02, 6.2e-02       | 2.0e-04, 1.0e-03
 *chan_smag_wm 32x16x16 B          | 4.2e-04, 3.5e-04             | 8.2e-02, 6.5e-02       | 2.1e-04, 1.0e-03
  couette_imp3d_ops 16x16x16       | 7.1e-04, 3.4e-04             | 9.8e-02, 6.2e-02       | 5.4e-04, 2.5e-03
  devchan_nd 32x16x16              | 3.0e-03, 7.5e-03             | 2.4e-01, 4.7e-02       | 4.5e-03, 1.7e-02
  duct_dsmag 64x18x20              | 4.6e-04, 8.3e-05             | 5.4e-02, 6.5e-02       | 3.8e-05, 7.6e-04
  duct_smag_wm 16x24x24            | 6.0e-05, 6.7e-06             | 1.8e-02, 2.0e-02       | 6.5e-06, 1.3e-04
  tgv_dsmag_ppp 64x16x24 D         | 6.4e-05, 1.9e-06             | 1.8e-02, 6.4e-03       | 3.3e-06, 4.0e-05
 *tgv_ppp 32x24x16 D               | 2.1e-04, 2.9e-05             | 2.6e-02, 1.4e-02       | 1.4e-05, 1.7e-04
  tgv_ppp 64x16x16 D               | 6.0e-05, 1.9e-06             | 1.8e-02, 6.6e-03       | 3.6e-06, 4.1e-05
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.util import (DT_FACTORS, STALE_FACTORS, VARIABLE_DT_COMBINATION_GRIDS, VARIABLE_DT_ROWS, F, forcing_id, load_golden, oracle_forcing_of_substeps,
                        perturbed_start, relerr, variable_dt_case)

# one row per (case, grid, forcing set, edits): the switches select forms of the device code, not other cases
ROWS = sorted({(name, ng, fset, tuple(edits.items())) for name, ng, fset, edits, _, _, _ in VARIABLE_DT_ROWS} |
              {(name, ng, None, ()) for name, ng in VARIABLE_DT_COMBINATION_GRIDS}, key=str)
MEASURED = {("chan_dsmag", (64, 20, 12)), ("chan_smag", (64, 18, 12)), ("tgv_ppp", (32, 24, 16)), ("chan_smag_wm", (32, 16, 16))}      # floor 1e-5
_cache = {}


def _row_id(v):
    return forcing_id(v) if not (isinstance(v, tuple) and (not v or isinstance(v[0], tuple))) else "-".join(str(x[1]) for x in v) or "plain"


def _run(name, ng, fset, edits, how):
    """how: 'step' (o.step), 'operators' (the sequence of o_step), or one of STALE_FACTORS (the sequence with that factor from the step before, from the
    second step on); returns (u, v, w, p, visct), the dt of every step, o.step's dpdl / the substeps' forcing of every step"""
    key = (name, ng, fset, edits, how)
    if key not in _cache:
        case = variable_dt_case(name, ng, fset, dict(edits))
        o = Oracle(case, nthreads=4)
        (u, v, w, p, visct, pp, dt0), _ = perturbed_start(case, o)
        dts = [fac * dt0 for fac in DT_FACTORS]; per_step = []
        for n, dt in enumerate(dts):
            if how == "step":
                per_step.append(o.step(dt, u, v, w, p, pp, visct).copy())
            else:
                stale = how if (how in STALE_FACTORS and n > 0) else None
                per_step.append(oracle_forcing_of_substeps(o, case, dt, u, v, w, p, pp, visct, stale=stale, dt_stale=dts[n - 1] if stale else None))
        o.close()
        _cache[key] = ((u, v, w, p, visct), dts, per_step)
    return _cache[key]


@pytest.mark.parametrize("name,ng,fset,edits", ROWS, ids=_row_id)
def test_step_is_the_operator_sequence_under_the_schedule(name, ng, fset, edits):
    a, _, _ = _run(name, ng, fset, edits, "step"); b, _, _ = _run(name, ng, fset, edits, "operators")
    assert all(np.isfinite(x).all() for x in a)
    for x, y, nm in zip(a, b, ("u", "v", "w", "p", "visct")):
        assert np.array_equal(x, y), nm


@pytest.mark.parametrize("name,ng,fset,edits", ROWS, ids=_row_id)
def test_stale_factors_are_no_no_ops(name, ng, fset, edits):
    base, _, _ = _run(name, ng, fset, edits, "operators")
    floor = 1e-5 if (name, ng) in MEASURED and not edits else 1e-6
    inner = lambda q: q[1:-1, 1:-1, 1:-1] - q[1:-1, 1:-1, 1:-1].mean()      # noqa: E731
    got = []
    for how in STALE_FACTORS:
        other, _, _ = _run(name, ng, fset, edits, how)
        got.append((max(relerr(other[i], base[i]) for i in range(3)), relerr(inner(other[3]), inner(base[3]))))
    print("TABLE", name, forcing_id(ng), fset, _row_id(edits), " | ".join(f"{e:.1e}, {ep:.1e}" for e, ep in got))
    for how, (e, ep) in zip(STALE_FACTORS, got):
        assert e >= floor, (how, e, floor)


@pytest.mark.parametrize("name,ng,fset,edits", [r for r in ROWS if r[2] is not None or r[0].startswith("chan")], ids=_row_id)
def test_dpdl_is_the_forcing_over_the_time_step_of_its_own_step(name, ng, fset, edits):
    """The check of test_forced_steps, at every step of the schedule: o.step's dpdl = -sum(f) / dt_n to 1e-12 max(1, |.|). With the step before's dt
    instead it is off by the ratio of the two steps, 14 % of its size at the least under DT_FACTORS."""
    _, dts, dpdls = _run(name, ng, fset, edits, "step"); _, _, fss = _run(name, ng, fset, edits, "operators")
    assert any(np.abs(d).max() > 0. for d in dpdls), "nothing forced"
    for n, (dt, dpdl, fs) in enumerate(zip(dts, dpdls, fss)):
        assert np.abs(-sum(fs) / dt - dpdl).max() <= 1e-12 * max(1., np.abs(dpdl).max()), n
        if n > 0 and dts[n - 1] != dt:
            wrong = -sum(fs) / dts[n - 1]
            off = np.abs(wrong - dpdl).max() / np.abs(dpdl).max()
            assert abs(off - abs(dt / dts[n - 1] - 1.)) < 1e-9 and off > 0.14, (n, off)


@pytest.mark.parametrize("stem", ["local_chan_dsmag", "local_chan_dsmag_wm", "local_tgv_dsmag_ppp"])
def test_oracle_coefficient_without_averaging_is_the_references(stem):
    """cmpt_sgs of the oracle with Case.dsmag_average = 'local' on the start-up state of the goldens made by the reference built with -D_CAVITY
    (tests/golden/local): 1e-11 of the field maximum, the bar the device's first call is held to on the same vectors (tests/test_gpu_dsmag_local.py: the
    reference's own cmpt_sgs moves by 1e-14 .. 1e-13 under a relative 1e-15 of u, v, w). Without the flag the field differs by more than 0.1 of its maximum."""
    g, case = load_golden("local/" + stem)
    want = g["s0_visct_nobc"][1:-1, 1:-1, 1:-1]
    out = []
    for ave in ("local", None):
        case.dsmag_average = ave
        o = Oracle(case, nthreads=4); visct = o.zeros()
        o.cmpt_sgs(F(g["s0_u"]), F(g["s0_v"]), F(g["s0_w"]), visct); o.close()
        out.append(visct[1:-1, 1:-1, 1:-1])
    err = relerr(out[0], want)
    print(stem, "relerr of the local coefficient", err)
    assert err < 1e-11, err
    assert np.abs(out[1] - want).max() > 0.1 * np.abs(want).max()

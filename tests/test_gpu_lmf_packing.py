"""Dynamic model's last pass on one rank: the remainder x tile packed into full waves (k_lmf_tile<.., PACK>, cales_amd/csrc/lmf_pack.hpp).

The pass works on tiles of 62 output columns; a row of n1 cells leaves rem = n1 mod 62 live columns for the last tile, and S stretches of rem + 2 lanes
-- one every P lanes, P = rem + 2 rounded up to a multiple of four, S = 64 / P, each on a y tile of its own -- share one wave in a launch of their own
behind the launch of the full tiles. Every cell's contribution is computed by the same instructions from the same inputs, and every y tile's block sum
by the same additions in the same order (stretches start on a multiple of four lanes, as the kernel's sums of four need), in the slot it has in the one
launch: the packed and the unpacked form (CALES_LMF_UNPACKED_REMAINDER: the one launch and the kernels of before) give the same bits.

Which form a call took is read off the launch check's hook (CALES_TEST_BAD_LAUNCH, tests/test_gpu_launch_check.py), as tests/test_gpu_dsmag_five.py does.

Shapes, each the smallest that reaches its case: (128, 24, 10) -- rem 4, S = 8, one packed block with three live segments and five dead ones;
(64, 16, 20) -- rem 2, S = 16, two live segments, seven k chunks, between z walls and with z periodic; (512, 32, 12) -- the headline's own map, rem 16,
S = 3, four y tiles: the second packed block has one live and two dead segments. (1024, 8, 6): rem 32, S = 1 -- not packed."""
import numpy as np
import pytest

from tests.util import F, load_golden, relerr

pytestmark = pytest.mark.gpu

PACKED_STEP = "k_lmf_tile<unsigned, 0, 1, 10>"      # five components, inside the step
PACKED_START = "k_lmf_tile<unsigned, 0, 1, 9>"      # six components: start-up and operator-level cmpt_sgs
UNPACKED = "CALES_LMF_UNPACKED_REMAINDER"
PLAN = ("in_strain_rate_pass", "dsmag_tiles(pair_fields)")


def _case(name, ng):
    g, case = load_golden(name); case.ng[:] = ng
    return case


def _start(case, seed=1):
    from cales_amd.hotpath import initflow
    u, v, w, p = initflow(case)
    rng = np.random.RandomState(seed)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*case.ng) - 0.5)
    return u, v, w, p


def _run(case, start, nsteps=3):
    from cales_amd.hotpath import HotPath
    h = HotPath(case); h.upload(*start); h.startup(); dt = 0.5 * h.chkdt()
    plan = h.describe_plan()
    for _ in range(nsteps):
        h.step(dt)
    out = h.download()
    h.close()
    return out, plan


def _fails_at(case, start, kernel, monkeypatch):
    """'startup' / 'step' / None: where a run fails with `kernel` made unlaunchable (the message must name it)"""
    from cales_amd.hotpath import CalesError, HotPath
    monkeypatch.setenv("CALES_TEST_BAD_LAUNCH", kernel)
    where = "startup"
    try:
        h = HotPath(case); h.upload(*start)
        try:
            h.startup(); where = "step"
            h.step(0.5 * h.chkdt()); where = None
        except CalesError as e:
            assert "kernel launch failed" in str(e) and kernel in str(e), e
        h.close()
    finally:
        monkeypatch.delenv("CALES_TEST_BAD_LAUNCH")
    return where


SHAPES = [("chan_dsmag_x128", (128, 24, 10)), ("chan_dsmag_x64", (64, 16, 20)), ("tgv_dsmag_ppp_x64", (64, 16, 20)), ("chan_dsmag_x128", (512, 32, 12))]
IDS = ["x128_three_live_segments", "x64_seven_chunks_z_walls", "x64_seven_chunks_z_periodic", "x512_headline_map_dead_segments"]


@pytest.mark.parametrize("name,ng", SHAPES, ids=IDS)
def test_packed_against_unpacked_by_value(name, ng, monkeypatch):
    """Three steps at 0.5 dt_cfl from the deterministic start plus a seeded perturbation: the step launches the packed in-step instantiation and start-up
    the packed six-component one -- neither with the switch set --, the plan is the headline's in both, and u, v, w, p and the eddy viscosity of the two
    forms agree to 1e-12 of each field's maximum (the bar test_five_components_against_six_by_value sets for a round-off level change in this pass) --
    and, since every block sum is formed by the unpacked tile's own additions, to the bit."""
    case = _case(name, ng); start = _start(case)
    assert _fails_at(case, start, PACKED_STEP, monkeypatch) == "step"
    assert _fails_at(case, start, PACKED_START, monkeypatch) == "startup"
    packed, plan_p = _run(case, start)
    monkeypatch.setenv(UNPACKED, "1")
    assert _fails_at(case, start, PACKED_STEP, monkeypatch) is None
    assert _fails_at(case, start, PACKED_START, monkeypatch) is None
    plain, plan_u = _run(case, start)
    assert plan_p == plan_u and (plan_p["projection"], plan_p["sgs"]) == PLAN, (plan_p, plan_u)
    errs = {nm: relerr(a, b) for nm, a, b in zip(("u", "v", "w", "p", "visct"), packed, plain)}
    for nm, e in errs.items():
        print(f"packed against unpacked, {ng}, {nm}: {e:.3e}")
    assert np.abs(packed[4]).max() > 0.
    for nm, e in errs.items():
        assert e < 1e-12, (nm, e)
    for nm, a, b in zip(("u", "v", "w", "p", "visct"), packed, plain):
        assert np.array_equal(a, b), nm


def test_a_row_length_with_one_segment_per_wave_is_not_packed(monkeypatch):
    """1024 cells per row: rem = 32, S = 1 -- the one launch as before: neither packed instantiation is launched, by start-up or by a step."""
    case = _case("chan_dsmag_x128", (1024, 8, 6)); start = _start(case)
    from cales_amd.hotpath import HotPath
    h = HotPath(case); plan = h.describe_plan(); h.close()
    assert plan["sgs"] == PLAN[1], plan
    assert _fails_at(case, start, PACKED_STEP, monkeypatch) is None
    assert _fails_at(case, start, PACKED_START, monkeypatch) is None


def test_the_packed_launch_opens_no_scope(monkeypatch):
    """Per-kernel timers on: the timer scopes of a step are the same with and without the switch (both launches sit inside the one scope of the pass), and
    the pass opens its scope once per substep."""
    from cales_amd.hotpath import HotPath
    case = _case("chan_dsmag_x128", (128, 24, 10)); start = _start(case)
    scopes = {}
    for unpacked in (False, True):
        if unpacked:
            monkeypatch.setenv(UNPACKED, "1")
        h = HotPath(case); h.upload(*start); h.startup(); dt = 0.5 * h.chkdt()
        h.step(dt)
        h.profile(True); h.step(dt); h.sync(); h.profile(False)
        st = h.profile_stats(); h.close()
        assert st["lij_mij_filter_contract"][0] == 3, st
        scopes[unpacked] = {k: v[0] for k, v in st.items()}
    assert scopes[False] == scopes[True], scopes


def test_cmpt_sgs_at_operator_level_packed_against_unpacked(monkeypatch):
    """A random, non-solenoidal velocity on 64 x 12 x 10 and one operator-level cmpt_sgs: the call launches the packed six-component instantiation (not with
    the switch set), and the eddy viscosity of the two forms agrees to 1e-12 of its maximum -- and to the bit."""
    from cales_amd.hotpath import CalesError, HotPath
    case = _case("chan_dsmag_x64", (64, 12, 10))
    rng = np.random.RandomState(5)
    shape = tuple(x + 2 for x in case.ng)
    fld = [F(rng.rand(*shape) - 0.5) for _ in range(4)]

    def visct(bad=None):
        if bad:
            monkeypatch.setenv("CALES_TEST_BAD_LAUNCH", bad)
        try:
            h = HotPath(case); h.upload(*fld)
            h.bounduvw(True, False)
            try:
                h.cmpt_sgs(); out = h.get("visct")
            except CalesError as e:
                assert "kernel launch failed" in str(e) and bad in str(e), e
                out = None
            h.close()
        finally:
            if bad:
                monkeypatch.delenv("CALES_TEST_BAD_LAUNCH")
        return out

    assert visct(PACKED_START) is None
    packed = visct()
    monkeypatch.setenv(UNPACKED, "1")
    assert visct(PACKED_START) is not None
    plain = visct()
    e = relerr(packed, plain)
    print(f"operator-level cmpt_sgs, packed against unpacked, visct: {e:.3e}")
    assert np.abs(plain).max() > 0. and e < 1e-12, e
    assert np.array_equal(packed, plain)

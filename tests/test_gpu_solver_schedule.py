"""The schedule of the FFT solves (k_solver.hip, SolveSched: chunks of the exchange, launch geometry, made at set-up and when the communication hooks
change): the chunked exchange on the second stream and the in-order one are the same sequence and give the same bits, a step allocates nothing, and
cales_describe_plan prints what the commit before the schedule record printed (tests/golden/solver_schedule/plans.json, written there by
gen_plans.py, which runs the functions of this file).

Shapes. Lines of 32 x 24 points (ng(1)/2 = 16 on k_fft_x8; ng(2) = 24 = 3 * 2^3) were meant to chunk, but the radix-8 y kernels take lines of
3 * 2^p points from 48 points on only (solver_setup, odd_of), so a 24-point line stays with k_fft_y and its solve in order whatever the hooks: those four
shapes are kept and hold one chunk each, and the same four with ng(2) = 48 = 3 * 2^4 chunk as intended -- two chunks, four chunks, n3 = 6 too small to
chunk while the second stream exists (the in-order exchange beside a second stream), two chunks with the mode columns padded on the last of three
ranks. The chunk count is read off the profile: a solve makes 2 nch exchanges, a step three solves."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.util import GOLD, load_golden

pytestmark = pytest.mark.gpu

PLANS = os.path.join(GOLD, "solver_schedule", "plans.json")
# ng, ranks, chunks of the exchange with the second stream
SHAPES = [((32, 24, 16), 2, 1), ((32, 24, 32), 2, 1), ((32, 24, 6), 2, 1), ((32, 24, 18), 3, 1),
          ((32, 48, 16), 2, 2), ((32, 48, 32), 2, 4), ((32, 48, 6), 2, 1), ((32, 48, 18), 3, 2)]
NSTEPS = 3
_runs = {}


def _plan_string(h):
    buf = C.create_string_buffer(2048)
    assert h.L.cales_describe_plan(h.h, buf, 2048) in (0, 2)
    return buf.value.decode()


def _key(name, ng, P, overlap):
    return "%s_%dx%dx%d_ranks%d_%s" % ((name,) + tuple(ng) + (P, "second_stream" if overlap else "in_order"))


def tgv_run(ng, P, overlap):
    """tgv_dsmag_ppp (unforced: no partial sums whose block partition differs) on P loopback ranks, three steps; per rank u, v, w, p, the eddy viscosity,
    the plan string and the exchanges of the solves per step. Run once per (shape, order) and shared."""
    from cales_amd.decomp import run_loopback
    k = (ng, P, overlap)
    if k in _runs:
        return _runs[k]
    g, case = load_golden("tgv_dsmag_ppp")
    case.ng[:] = ng
    env = {"CALES_OVERLAP": "1", "CALES_LOOPBACK_EVENTS": "1"} if overlap else {}      # (event-ordered copies: a kernel that did not wait for its chunk reads stale data)
    old = {q: os.environ.get(q) for q in ("CALES_OVERLAP", "CALES_LOOPBACK_EVENTS", "CALES_NO_OVERLAP")}
    for q in old:
        os.environ.pop(q, None)
    os.environ.update(env)
    try:
        def body(h, r):
            h.upload_initial(); h.startup()
            dt = 0.5 * h.chkdt()
            plan = _plan_string(h)
            h.profile(True)
            for _ in range(NSTEPS):
                h.step(dt)
            h.profile(False)
            return h.download() + [plan, h.profile_stats()["alltoall"][0] // NSTEPS]
        _runs[k] = run_loopback(case, P, body)
    finally:
        for q, v in old.items():
            os.environ.pop(q, None)
            if v is not None:
                os.environ[q] = v
    return _runs[k]


def memory_run(P, overlap):
    """chan_dsmag at (64, 16, 16), forced in x, the fused fillps forming the bulk means: (bytes, allocations) right before the first step and after two,
    and the plan string, per rank"""
    g, case = load_golden("chan_dsmag")
    case.ng[:] = (64, 16, 16)

    def body(h, r):
        h.upload_initial() if P > 1 else h.upload(*_initial(case))
        h.startup()
        dt = 0.5 * h.chkdt()
        plan = _plan_string(h)
        assert h.describe_plan()["bulk_forcing"] == "in_correction(means_in_x_transform)"
        before = h.memory_in_use()
        h.step(dt); h.step(dt); h.sync()
        return before, h.memory_in_use(), plan
    if P == 1:
        from cales_amd.hotpath import HotPath
        h = HotPath(case)
        out = [body(h, 0)]
        h.close()
        return out
    from cales_amd.decomp import run_loopback
    old = os.environ.get("CALES_OVERLAP")
    if overlap:
        os.environ["CALES_OVERLAP"] = "1"
    try:
        return run_loopback(case, P, body)      # (SlabHotPath calls cales_set_comm and cales_set_comm_overlap when it is made)
    finally:
        os.environ.pop("CALES_OVERLAP", None)
        if old is not None:
            os.environ["CALES_OVERLAP"] = old


def _initial(case):
    from cales_amd.hotpath import initflow
    return initflow(case)


@pytest.mark.parametrize("ng,P,nch", SHAPES)
def test_chunked_and_in_order_solves_agree_to_the_bit(ng, P, nch):
    """Every row and every column is transformed by the same instructions whichever way the spectrum travels: == on every field of every rank. (Measured on
    the commit before the schedule record, which had the two forms side by side: equal there too, profiles/solver_schedule_refactor.md.)"""
    a, b = tgv_run(ng, P, True), tgv_run(ng, P, False)
    for r in range(P):
        print(ng, "rank", r, "exchanges per step: second stream", a[r][6], "in order", b[r][6])
        assert a[r][6] == 3 * 2 * nch and b[r][6] == 3 * 2
        for q, nm in enumerate(("u", "v", "w", "p", "visct")):
            print("   ", nm, "largest difference", np.abs(a[r][q] - b[r][q]).max())
            assert np.array_equal(a[r][q], b[r][q]), (r, nm)


@pytest.mark.parametrize("P,overlap", [(1, False), (2, True)])
def test_a_step_allocates_nothing(P, overlap):
    """The partial sums of the bulk means are sized with the pressure's schedule (solver_setup, solver_comm_changed), not by the first solve that needs them."""
    for r, (before, after, plan) in enumerate(memory_run(P, overlap)):
        print("rank", r, "bytes, allocations before the first step", before, "after two", after)
        assert before == after


def test_plan_strings_are_those_of_the_commit_before():
    want = json.load(open(PLANS))
    for ng, P, nch in SHAPES:
        for overlap in (True, False):
            assert [x[5] for x in tgv_run(ng, P, overlap)] == want[_key("tgv_dsmag_ppp", ng, P, overlap)], (ng, P, overlap)
    for P, overlap in ((1, False), (2, True)):
        assert [x[2] for x in memory_run(P, overlap)] == want[_key("chan_dsmag", (64, 16, 16), P, overlap)], P

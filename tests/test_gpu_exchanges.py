"""The contract of the exchanges between y slabs (struct StageLayout and struct Comm): what the hosts of a decomposed run see of them -- every
hook call of start-up, two steps, chkdt and chkdiv, per rank and in order, with all its integer arguments -- next to the size of the staging buffers, the
plan string and the fields that come out, bit for bit. tests/golden/exchanges/traces.json is the library's own behaviour before the exchanges were given
one layout record and one path each (tests/golden/exchanges/gen_traces.py wrote it); no row, message or offset may move, so everything is compared with `==`.
The recording wrapper also holds every range to the region of the staging buffers the layout gives it."""
import functools
import hashlib
import json
import os

import pytest

from tests.util import GOLD

pytestmark = pytest.mark.gpu

# key -> (golden case, grid, ranks, switches, plan entries that prove the path)
CASES = {
    # second and third rows through the companion fields, batched in order
    "a": ("chan_dsmag", (64, 32, 24), 4, {}, {"projection": "in_strain_rate_pass(ghost_rows_local)", "exchanges": "in_order"}),
    # three rows per slab: the one-row form (row 2 of pp through its companion, one exchange for both)
    "b": ("chan_dsmag", (64, 24, 16), 8, {}, {"projection": "in_strain_rate_pass", "exchanges": "in_order"}),
    # thirteen scratch fields of the dynamic model in one batch (plain fields, the projection a pass of its own)
    "c": ("chan_dsmag", (64, 32, 24), 4, {"CALES_DSMAG_XGHOSTS": "1"}, {"projection": "own_pass(correc+updatep)", "x_ghost_columns": "maintained", "exchanges": "in_order"}),
    # the second stream: halo rows of the scratch fields and the k-chunks of the solve
    "d": ("duct_dsmag_wm", (32, 32, 32), 2, {"CALES_OVERLAP": "1"}, {"exchanges": "second_stream"}),
    # static Smagorinsky between y walls on four slabs: the wall-shear planes borrow the head of A
    "e": ("duct_smag_wm", (16, 32, 24), 4, {}, {"exchanges": "in_order"}),
    # no model: the rows that leave are read through the corrected view
    "f": ("chan_nosgs", (32, 24, 12), 3, {}, {"projection": "in_next_momentum_pass(substeps_1_2)", "exchanges": "in_order"}),
}
SWITCHES = ("CALES_DSMAG_XGHOSTS", "CALES_OVERLAP", "CALES_NO_OVERLAP", "CALES_LOOPBACK_EVENTS")
MAXPLANES = 16      # StageLayout::MAXPLANES


def layout(h, ng, P):
    """StageLayout of rank h, restated from the grid alone: (reals of a row plane, halo region, all-to-all capacity, offset of the tail, total)"""
    from cales_amd import capi
    line = 32 if capi.SINGLE else 16
    n1, n2l, n3 = ng[0], ng[1] // P, ng[2]
    s1 = (n1 + 3 + line - 1) // line * line
    plane = s1 * (n3 + 2)
    cw = (n1 // 2 + 1 + P - 1) // P      # mode columns per rank, in whole lines where that adds 6 % or less (k_solver.hip, solver_setup)
    cw8 = (cw + 7) // 8 * 8
    if 100 * (cw8 - cw) <= 6 * cw and cw8 * ng[1] * n3 <= s1 * (n2l + 2) * (n3 + 2):
        cw = cw8
    a2a = 2 * P * n3 * n2l * cw
    tail = max(a2a, 2 * 2 * MAXPLANES * plane)      # (the halo term counts twice the region the offsets use: StageLayout::HALO_SIZED_FOR)
    return plane, 2 * MAXPLANES * plane, a2a, tail, tail + 4096 + 2 * n3 + 2 + 2


def _record(h, r, ng, P, out):
    import ctypes as C
    plane, halo, a2a, tail, total = layout(h, ng, P)
    assert h.nbuf == total, (h.nbuf, total)
    own = int(h.stream.cuda_stream)
    trace, phase = [], [None]
    inner = {m: getattr(h.comm, m) for m in ("halo", "halo_s", "alltoall", "alltoall_part", "allreduce")}

    def halo_ok(slo, shi, rlo, rhi, n):
        assert n >= 1 and n % plane == 0 and n <= MAXPLANES * plane, (n, plane)
        for off in (slo, shi, rlo, rhi):
            assert 0 <= off and off + n <= halo <= tail, (off, n, halo, tail)

    def halo_(slo, shi, rlo, rhi, n):
        halo_ok(slo, shi, rlo, rhi, n)
        trace.append([phase[0], "halo", int(slo), int(shi), int(rlo), int(rhi), int(n)])
        return inner["halo"](slo, shi, rlo, rhi, n)

    def halo_s(slo, shi, rlo, rhi, n, st):
        halo_ok(slo, shi, rlo, rhi, n)
        trace.append([phase[0], "halo_s", int(slo), int(shi), int(rlo), int(rhi), int(n), int(st or 0) == own])
        return inner["halo_s"](slo, shi, rlo, rhi, n, st)

    def alltoall(d, n):
        assert n >= 1 and P * n <= a2a, (n, a2a)
        trace.append([phase[0], "alltoall", int(d), int(n)])
        return inner["alltoall"](d, n)

    def alltoall_part(d, stride, off, n, st):
        assert n >= 1 and 0 <= off and off + n <= stride and P * stride <= a2a, (stride, off, n, a2a)
        trace.append([phase[0], "alltoall_part", int(d), int(stride), int(off), int(n), int(st or 0) == own])
        return inner["alltoall_part"](d, stride, off, n, st)

    def allreduce(off, n, op):
        assert n >= 1 and ((tail <= off and off + n <= total) or (off == 0 and n <= tail)), (off, n, tail, total)
        trace.append([phase[0], "allreduce", int(off), int(n), int(op)])
        return inner["allreduce"](off, n, op)

    h.upload_initial()
    for m, f in (("halo", halo_), ("halo_s", halo_s), ("alltoall", alltoall), ("alltoall_part", alltoall_part), ("allreduce", allreduce)):
        setattr(h.comm, m, f)
    phase[0] = "startup"; h.startup()
    phase[0] = "chkdt0"; dt = 0.5 * h.chkdt()
    buf = C.create_string_buffer(4096)
    assert h.L.cales_describe_plan(h.h, buf, 4096) == 0
    phase[0] = "step1"; h.step(dt)
    phase[0] = "step2"; h.step(dt)
    phase[0] = "chkdt"; h.chkdt()
    phase[0] = "chkdiv"; h.chkdiv()
    phase[0] = "download"
    fields = h.download()
    for m, f in inner.items():
        setattr(h.comm, m, f)
    out[r] = {"nbuf": int(h.nbuf), "plan": buf.value.decode(), "trace": trace,
              "sha256": {nm: hashlib.sha256(a.tobytes(order="F")).hexdigest() for nm, a in zip(("u", "v", "w", "p", "visct"), fields)}}


@functools.lru_cache(maxsize=None)
def run(key):
    """[{nbuf, plan, trace, sha256} of rank r] of one case -- computed once, shared by the tests below"""
    from cales_amd.decomp import run_loopback
    from tests.test_gpu_decomp import _case
    from tests.test_gpu_golden import _nosgs_case
    name, ng, P, env, _ = CASES[key]
    case = _nosgs_case(name, ng) if name == "chan_nosgs" else _case(name, ng)
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        out = [None] * P
        run_loopback(case, P, lambda h, r: _record(h, r, ng, P, out))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return out


def _gold():
    with open(os.path.join(GOLD, "exchanges", "traces.json")) as f:
        return json.load(f)


def _plane(key):
    from cales_amd import capi
    ng, line = CASES[key][1], 32 if capi.SINGLE else 16
    return (ng[0] + 3 + line - 1) // line * line * (ng[2] + 2)


@pytest.mark.parametrize("key", sorted(CASES))
def test_exchanges_as_recorded(key):
    """Every hook call in its order with every argument, the size of the staging buffers, the plan string and the fields: the recorded ones on every rank."""
    got, gold = run(key), _gold()[key]
    assert len(got) == len(gold)
    for r, (a, b) in enumerate(zip(got, gold)):
        print(key, "rank", r, "nbuf", a["nbuf"], "calls", len(a["trace"]), a["plan"])
        assert a["nbuf"] == b["nbuf"], (r, a["nbuf"], b["nbuf"])
        assert a["plan"] == b["plan"], (r, a["plan"], b["plan"])
        assert json.loads(json.dumps(a["trace"])) == b["trace"], (r, [x for x, y in zip(a["trace"], b["trace"]) if x != y][:3], len(a["trace"]), len(b["trace"]))
        assert a["sha256"] == b["sha256"], (r, a["sha256"], b["sha256"])


@pytest.mark.parametrize("key", sorted(CASES))
def test_case_takes_its_path(key):
    """The plan entries and the calls that show the case ran what it is there for."""
    name, ng, P, env, want = CASES[key]
    plane = _plane(key)
    for r, a in enumerate(run(key)):
        plan = dict(kv.split("=", 1) for kv in a["plan"].split(";"))
        for k, v in want.items():
            assert plan[k] == v, (r, k, plan)
        step = [t for t in a["trace"] if t[0] == "step2"]
        names = {t[1] for t in step}
        halos = [t[6] // plane for t in step if t[1] == "halo"]
        if key == "a":      # per substep: u, v, w and their second rows (6 planes), pp with its second and third rows (3)
            assert halos == [6, 3] * 3, (r, halos)
        if key == "b":      # ... the prediction, pp with row 2 in its companion, and the batch of the dynamic model's scratch fields
            assert halos == [3, 2, 11] * 3, (r, halos)
        if key == "c":      # thirteen plain fields in the batch of cmpt_sgs: the sixteen planes of a block hold them, one exchange per substep
            assert halos.count(13) == 3, (r, halos)
        if key == "d":
            assert {"halo_s", "alltoall_part"} <= names and "alltoall" not in names, (r, sorted(names))
            assert all(not t[-1] for t in step if t[1] in ("halo_s", "alltoall_part")), r      # (the second stream, not the context's own)
        if key == "e":      # both y walls' shear planes, summed over the slabs at the head of A
            assert ["step2", "allreduce", 0, 2 * plane, 0] in step, (r, [t for t in step if t[1] == "allreduce"])
        if key == "f":
            assert halos and "halo_s" not in names, (r, sorted(names))

"""The contract of the scalar reductions and plane statistics (struct RedLayout): what the hosts of a decomposed run see of them --
the all-reduce callbacks, in their order, with their counts and operations -- and what every entry returns, bit for bit. The literals below and
tests/golden/reductions/*.npz are the library's own behaviour before its reductions were given one layout record
(tests/golden/reductions/gen_reductions.py wrote both); nothing in the arithmetic or its order may move, so the values are compared with `==`."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests.util import GOLD, load_golden

pytestmark = pytest.mark.gpu

# key -> (golden case, grid, Case.dsmag_average). (24, 20, 12): rows that are no whole tiles, n3 a multiple of nothing the kernels use
CASES = {"chan_smag": ("chan_smag", (24, 20, 12), None), "chan_dsmag": ("chan_dsmag", (64, 16, 16), None),
         "chan_dsmag_volume": ("chan_dsmag", (64, 16, 16), "volume")}
PHASES = ("startup", "chkdt", "step", "chkdt_after", "chkdiv", "bulk_mean_u")

# (count, op) of every all-reduce callback, per phase, on EACH of two ranks; op: 0 sum, 1 max
SEQUENCES = {
    "chan_smag": {"startup": [], "chkdt": [(2, 1)], "step": [(1, 0)] * 3, "chkdt_after": [(2, 1)], "chkdiv": [(1, 0), (1, 1)], "bulk_mean_u": [(1, 0)]},
    "chan_dsmag": {"startup": [(32, 0)], "chkdt": [(2, 1)], "step": [(1, 0), (32, 0)] * 3, "chkdt_after": [(2, 1)], "chkdiv": [(1, 0), (1, 1)], "bulk_mean_u": [(1, 0)]},
    "chan_dsmag_volume": {"startup": [(32, 0)], "chkdt": [(2, 1)], "step": [(1, 0), (32, 0)] * 3, "chkdt_after": [(2, 1)], "chkdiv": [(1, 0), (1, 1)], "bulk_mean_u": [(1, 0)]},
}


def make_case(key):
    name, ng, ave = CASES[key]
    g, case = load_golden(name)
    case.ng[:] = ng
    if ave is not None:
        case.dsmag_average = ave
    return case


def _entries(h, dt_of_step):
    """every reduction and statistics entry of one context, after a step"""
    from cales_amd.hotpath import REAL, _p
    out = {}
    out["chkdt"] = np.array(h.chkdt())
    out["chkdiv"] = np.array(h.chkdiv())
    out["bulk_mean"] = np.array([h.bulk_mean("u", "f"), h.bulk_mean("v", "f"), h.bulk_mean("w", "c"), h.bulk_mean("p", "c")])
    f = np.zeros(3, dtype=REAL); h._chk(h.L.cales_get_forcing(h.h, _p(f)))
    out["forcing"] = f
    out["dpdl"] = h.dpdl()
    out["stats_chan"] = h.stats_chan()
    out["budget"], out["leak"] = h.stats_chan_budgets()
    for idir in (1, 2, 3):
        out[f"out1d_{idir}"] = h.out1d("u", idir)
    out["out1d_chan"] = h.out1d_chan()
    out["out2d_duct"] = h.out2d_duct()
    out["dt"] = np.array(dt_of_step)
    return out


def _body(h, r, seq, slab):
    """start-up, one step and the entries; on slabs with every all-reduce callback recorded per phase, its range held to the staging buffer"""
    phase = [None]
    if slab:
        inner = h.comm.allreduce

        def recorded(off, count, op):
            assert 0 <= off and count >= 1 and off + count <= h.nbuf, (phase[0], off, count, h.nbuf)
            seq[r][phase[0]].append((int(count), int(op)))
            return inner(off, count, op)
        h.comm.allreduce = recorded
        h.upload_initial()
    else:
        from cales_amd.hotpath import initflow
        h.upload(*initflow(h.case))
    phase[0] = "startup"; h.startup()
    phase[0] = "chkdt"; dt = 0.5 * h.chkdt()
    phase[0] = "step"; h.step(dt); h.sync()
    phase[0] = "chkdt_after"; h.chkdt()
    phase[0] = "chkdiv"; h.chkdiv()
    phase[0] = "bulk_mean_u"; h.bulk_mean("u", "f")
    phase[0] = "entries"
    return _entries(h, dt)


@functools.lru_cache(maxsize=None)
def run(key, nranks):
    """([entries of rank r], [{phase: [(count, op), ...]} of rank r]) -- computed once, shared by the tests below"""
    case = make_case(key)
    seq = [{p: [] for p in PHASES + ("entries",)} for _ in range(nranks)]
    if nranks == 1:
        from tests.test_gpu_vs_oracle import _hot
        h = _hot(case)
        vals = [_body(h, 0, seq, False)]
        h.close()
    else:
        from cales_amd.decomp import run_loopback
        vals = run_loopback(case, nranks, lambda h, r: _body(h, r, seq, True))
    return vals, seq


@pytest.mark.parametrize("key", sorted(CASES))
def test_collective_sequence(key):
    """Two loopback ranks: the all-reduce callbacks of start-up, a step, chkdt, chkdiv and bulk_mean -- number, order, count and op -- are the
    recorded ones on both ranks (the offsets are the layout's business: only that every range lies inside the staging buffer, asserted in the callback)."""
    vals, seq = run(key, 2)
    for r in range(2):
        got = {p: seq[r][p] for p in PHASES}
        print(key, "rank", r, got, "entries:", seq[r]["entries"])
        assert got == SEQUENCES[key], (r, got)


@pytest.mark.parametrize("nranks", [1, 2])
@pytest.mark.parametrize("key", sorted(CASES))
def test_results_bit_for_bit(key, nranks):
    """chkdt, chkdiv, the bulk means, forcing and dpdl after a step, the plane statistics, budgets, leakage, the profiles and the duct
    statistics: equal to the stored values of the same library before the refactor, every bit (NaN nowhere: `==` on whole arrays)."""
    vals, seq = run(key, nranks)
    gold = np.load(os.path.join(GOLD, "reductions", key + ".npz"))
    for r in range(nranks):
        for name, got in vals[r].items():
            ref = gold[f"p{nranks}_r{r}_{name}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (r, name, got.shape, ref.shape)
            assert np.array_equal(got, ref), (r, name, np.abs(got - ref).max())


def test_two_ranks_without_hooks_and_with():
    """nranks = 2 and no hooks registered: chkdiv reports that, whatever the layout says about where its results live. Registering the hooks moves
    the results and the plane sums into the staging buffer and allocates nothing; both ranks then agree on chkdiv."""
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import CalesError, HotPath
    case = make_case("chan_dsmag")
    bare = []
    for r in range(2):
        h = HotPath(case, nranks=2, rank=r)
        bare.append(h.memory_in_use())
        with pytest.raises(CalesError, match="no communication hooks registered"):
            h.chkdiv()
        with pytest.raises(CalesError, match="no communication hooks registered"):      # ... and so does a step, at its first exchange
            h.step(1e-3)
        h.close()

    def body(h, r):
        with_hooks = h.memory_in_use()
        h._chk(h.L.cales_set_comm(h.h, h._cb[0], h._cb[1], h._cb[2], None, C.c_void_p(h.A.data_ptr()), C.c_void_p(h.B.data_ptr()), C.c_int64(h.nbuf)))
        again = h.memory_in_use()
        h.upload_initial(); h.startup()
        return with_hooks, again, h.chkdiv()
    out = run_loopback(case, 2, body)
    for r in range(2):
        assert out[r][0] == bare[r] and out[r][1] == bare[r], (r, bare[r], out[r][:2])
    assert out[0][2] == out[1][2]

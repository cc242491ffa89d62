"""The context owns its device memory ("who owns device memory"): everything cales_create and the lazy paths behind it allocate --
fields, companions, pair fields, the solver's tables, the tables a first Helmholtz solve makes, the scratch of the statistics, the result buffers of
the profile calls -- is counted by cales_memory_in_use and given back by cales_destroy, on whole, failed and half-built contexts alike. Every test
takes the totals of the process first and asserts that they are back at exactly that balance, bytes and allocation count, at its end."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests.util import load_golden, open_case

pytestmark = pytest.mark.gpu


def _baseline():
    from cales_amd.hotpath import memory_in_use
    gc.collect()      # (a context an earlier test dropped without close() goes now, not in the middle of this test)
    return memory_in_use()


def _field_bytes(ng):
    """(ntot + LINE_REALS) * sizeof(real): one haloed field in the library's layout (rows padded to whole 128-B lines)"""
    from cales_amd import capi
    rsz = C.sizeof(capi.c_real); line = 128 // rsz
    s1 = (ng[0] + 3 + line - 1) // line * line
    return (s1 * (ng[1] + 2) * (ng[2] + 2) + line) * rsz


def _fields_held(case, pair=False):
    """fields a context of this case cannot do without: u, v, w, p, pp, visct, the two r.h.s. sets of rk (a third with implicit diffusion), two scratch
    fields of the solver, the second velocity buffers; |S| and three (six) work fields of the static (dynamic) model; the dynamic model's two filtered
    velocities and alph2, and |S|Sij as three pair fields (two fields each) or as sij / mij"""
    n = 6 + (9 if case.impdiff else 6) + 2 + 3
    if case.sgstype == "smag":
        n += 1 + 3
    if case.sgstype == "dsmag":
        n += 1 + 6 + 6 + 1 + (6 if pair else 12)
    return n


def _golden_case(name, ng=None):
    g, case = load_golden(name)
    if ng is not None:
        case.ng[:] = ng
    return case


def _couette():
    return _golden_case("couette_imp3d_ops", (32, 16, 12))


def _open_y():      # inflow / outflow along y: the pressure and the tangential components take the DCT-IV / DST-IV kernels and their weights
    case = open_case(None, ("DN", "NN"), (12, 16, 10))
    case.through_flow = True
    return case


def _initial(case):
    from cales_amd.hotpath import initflow
    ng = tuple(int(x) for x in case.ng)
    if getattr(case, "through_flow", False):      # the open box (its inivel is 'zer')
        rng = np.random.RandomState(4)
        out = [np.zeros(tuple(x + 2 for x in ng), order="F") for _ in range(4)]
        for a, m in zip(out[:3], (0.3, 0.7, 0.)):
            a[1:-1, 1:-1, 1:-1] = m + 0.05 * (rng.rand(*ng) - 0.5)
        return out
    return initflow(case)


def _hot(case):
    from tests.test_gpu_vs_oracle import _hot as hot
    return hot(case)


def _drive(h, case, channel):
    """every entry that allocates on first use or per call"""
    h.upload(*_initial(case)); h.startup()
    dt = 0.5 * h.chkdt()
    h.step(dt); h.chkdt(); h.chkdiv(); h.describe_plan(); h.calibrate(1)
    for idir in (1, 2, 3):
        h.out1d("u", idir)
    h.out1d_chan(); h.out2d_duct()
    if channel:
        h.stats_chan(); h.stats_chan_budgets()


CASES = [
    # id, case, |S|Sij as pair fields, channel statistics, environment
    pytest.param(lambda: _golden_case("tgv_ppp", (64, 16, 16)), False, False, {}, id="tgv_ppp"),                      # no model, tile z solve
    pytest.param(lambda: _golden_case("chan_smag", (24, 20, 12)), False, True, {}, id="chan_smag"),                   # rows that are no whole tiles; d_del
    pytest.param(lambda: _golden_case("chan_dsmag", (64, 16, 16)), True, True, {}, id="chan_dsmag"),                  # pair fields; d_cs
    pytest.param(lambda: _golden_case("cavity_dsmag", (24, 20, 12)), False, False, {}, id="cavity_dsmag"),            # sij / mij
    pytest.param(lambda: _golden_case("duct_smag_wm"), False, False, {}, id="duct_smag_wm"),                          # wall-model planes
    pytest.param(lambda: _golden_case("halfchan_imp1d"), False, True, {}, id="halfchan_imp1d"),                       # z-implicit: tab_hz, d_scaled
    pytest.param(_couette, False, True, {}, id="couette_imp3d"),                                                       # the lazy tables of velocity_path
    pytest.param(_open_y, False, False, {}, id="open_y_imp3d_dct4", marks=pytest.mark.imp3d_open),                     # ... with DCT-IV weights
    pytest.param(lambda: _golden_case("tgv_ppp", (64, 16, 16)), False, False, {"CALES_KEEP_NULL_MODE": "1"}, id="tgv_ppp_null_mode"),      # d_nullw
]


@pytest.mark.parametrize("make,pair,channel,env", CASES)
def test_destroy_returns_what_the_context_took(make, pair, channel, env, monkeypatch):
    from cales_amd.hotpath import memory_in_use
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    base = _baseline()
    case = make()
    h = _hot(case)
    created = h.memory_in_use()
    _drive(h, case, channel)
    own = h.memory_in_use()
    print("bytes, allocations after create", created, "after use", own, "process", memory_in_use())
    assert own[0] > 0 and own[1] > 0
    assert own[0] >= created[0] and own[1] >= created[1]
    assert own[0] >= _fields_held(case, pair) * _field_bytes([int(x) for x in case.ng]), (own, _fields_held(case, pair))
    tot = memory_in_use()
    assert (tot[0] - base[0], tot[1] - base[1]) == own
    h.close()
    assert memory_in_use() == base


def test_two_contexts_alive_at_once():
    from cales_amd.hotpath import memory_in_use
    base = _baseline()
    ca, cb = _golden_case("chan_dsmag", (64, 16, 16)), _golden_case("chan_smag", (24, 20, 12))
    a = _hot(ca); _drive(a, ca, True)
    b = _hot(cb); _drive(b, cb, True)
    ma, mb, tot = a.memory_in_use(), b.memory_in_use(), memory_in_use()
    assert ma[0] > mb[0] > 0
    assert (tot[0] - base[0], tot[1] - base[1]) == (ma[0] + mb[0], ma[1] + mb[1])
    a.close()
    tot = memory_in_use()
    assert (tot[0] - base[0], tot[1] - base[1]) == mb and b.memory_in_use() == mb
    b.close()
    assert memory_in_use() == base


def test_same_case_same_use_same_totals():
    from cales_amd.hotpath import memory_in_use
    base = _baseline()
    seen = []
    for _ in range(2):
        case = _golden_case("chan_dsmag", (64, 16, 16))
        h = _hot(case)
        created = h.memory_in_use()
        _drive(h, case, True)
        seen.append((created, h.memory_in_use()))
        h.close()
    assert seen[0] == seen[1], seen
    assert memory_in_use() == base


def test_several_slabs_and_a_second_set_comm():
    """companion fields, cales_set_comm (the plane sums of the dynamic model move into the staging buffer) -- twice on one rank, same buffers"""
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import memory_in_use
    base = _baseline()
    case = _golden_case("chan_dsmag", (64, 16, 16))

    def body(h, r):
        before = h.memory_in_use()
        if r == 0:
            h._chk(h.L.cales_set_comm(h.h, h._cb[0], h._cb[1], h._cb[2], None, C.c_void_p(h.A.data_ptr()), C.c_void_p(h.B.data_ptr()), C.c_int64(h.nbuf)))
            assert h.memory_in_use() == before
        h.upload_initial(); h.startup()
        dt = 0.5 * h.chkdt()
        h.step(dt); h.chkdiv()
        return before, h.memory_in_use(), h.describe_plan()["projection"]
    out = run_loopback(case, 2, body)
    for before, after, projection in out:
        print("bytes, allocations after create", before, "after a step", after, projection)
        assert after[0] >= before[0] > 0
        assert before[0] >= (_fields_held(case, True) + 3 + 3 + 1) * _field_bytes((64, 8, 16))      # a companion behind u, v, w (both sets), a second one behind pp
    assert out[0][1] == out[1][1]
    assert memory_in_use() == base


def test_failed_creation_and_failed_upload_leave_nothing(monkeypatch):
    """a context that fails half-way through cales_create (every launch invalid: the first set-up kernel of the solver fails it, with the fields, the BC
    planes and part of the solver's tables allocated) and one that fails at its first use (the upload's repack kernel) and is closed afterwards"""
    from cales_amd.hotpath import CalesError, HotPath, initflow
    from cales_amd.hotpath import memory_in_use
    base = _baseline()
    monkeypatch.setenv("CALES_TEST_BAD_LAUNCH", "k_")
    for name, ng in (("chan_dsmag", (64, 16, 16)), ("chan_smag", (32, 16, 12))):
        with pytest.raises(CalesError, match="kernel launch failed.*k_"):
            HotPath(_golden_case(name, ng))
        assert memory_in_use() == base
    monkeypatch.setenv("CALES_TEST_BAD_LAUNCH", "k_repack")
    case = _golden_case("chan_smag", (32, 16, 12))
    h = HotPath(case)
    assert h.memory_in_use()[0] > 0
    with pytest.raises(CalesError, match="kernel launch failed.*k_repack"):
        h.upload(*initflow(case))
    h.close()
    assert memory_in_use() == base


def test_failed_profile_call_releases_its_buffer(monkeypatch):
    from cales_amd.hotpath import CalesError
    from cales_amd.hotpath import memory_in_use
    base = _baseline()
    monkeypatch.setenv("CALES_TEST_BAD_LAUNCH", "k_out1d")
    case = _golden_case("chan_smag", (24, 20, 12))
    h = _hot(case)
    h.upload(*_initial(case)); h.startup()
    before = h.memory_in_use()
    with pytest.raises(CalesError, match="kernel launch failed.*k_out1d"):
        h.out1d("u", 3)
    assert h.memory_in_use() == before
    h.close()
    assert memory_in_use() == base

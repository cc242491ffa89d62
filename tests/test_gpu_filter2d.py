"""The dynamic model with the reference's 2-D test filter (-D_FILTER_2D: filter2d, src/sgs.f90:824-848, called at 236-247 and 316-327; alph2 = 2.52
everywhere, 817-821) as a run-time choice: cales_case.sgstype = 3, in Python Case.filter2d or the environment variable CALES_FILTER_2D.

The yardstick is the reference itself built with the flag (tests/golden/filter2d, gen_golden_filter2d.py): the same cases, edits and keys as the goldens
of the 3-D filter, so the replay functions of tests/test_gpu_golden.py run on them UNCHANGED with the variable set -- their tolerances are the existing
ones. The eddy viscosity of these files differs from the 3-D filter's by 30-100 % of its maximum: none of the replays can pass without the feature."""
import os
import re

import numpy as np
import pytest

from tests import test_gpu_golden as G
from tests.util import F, load_golden, relerr

pytestmark = pytest.mark.gpu

TILES = ["chan_dsmag", "chan_dsmag_wm", "tgv_dsmag_ppp"]      # x periodic, nothing at the y faces, z between walls (no-slip / wall-modelled) or periodic: the tile passes
SEQUENCE = ["duct_dsmag", "duct_dsmag_wm", "cavity_dsmag"]    # walls or wall-model faces in x or y: the kernel-per-loop sequence
END = ["chan_dsmag_x64", "chan_dsmag_x128", "tgv_dsmag_ppp_x64", "duct_dsmag_x64"]


@pytest.fixture
def flag(monkeypatch):
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    monkeypatch.delenv("CALES_DSMAG_REFERENCE_SEQUENCE", raising=False)
    return monkeypatch


@pytest.mark.parametrize("name", TILES + SEQUENCE)
def test_stage_replay_default_path(name, flag):
    """Every operator of the start-up and of three substeps against the flag build's stage vectors; cmpt_sgs at the tile tolerances (1e-11, 1e-10) where
    the tile passes serve the case, at the single-operator 1e-13 where the sequence does."""
    G.test_startup_and_substeps("filter2d/" + name, general_sgs=name in SEQUENCE)


@pytest.mark.parametrize("name", TILES + SEQUENCE)
def test_stage_replay_reference_sequence(name, flag):
    """... and with the sequence selected for all six: every operator at 1e-13."""
    flag.setenv("CALES_DSMAG_REFERENCE_SEQUENCE", "1")
    G.test_startup_and_substeps("filter2d/" + name, general_sgs=True)


@pytest.mark.parametrize("name", TILES + SEQUENCE + END)
def test_whole_step(name, flag):
    """cales_step against the flag build's end-of-step state: u, v, w 1e-10, p 1e-9, visct 1e-8, divmax < 1e-12 (the existing bounds)."""
    G.test_fused_step_matches_operator_sequence("filter2d/" + name)


@pytest.mark.parametrize("name", TILES + SEQUENCE + END)
def test_plan_names_the_form(name, flag):
    g, case = load_golden("filter2d/" + name)
    h = G._hot(case)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    pl = h.describe_plan()
    tiles = name.startswith(("chan", "tgv"))
    assert pl["sgs"] == ("dsmag_tiles(filter2d)" if tiles else "dsmag_reference_sequence(filter2d)"), pl
    assert pl["projection"] == "own_pass(correc+updatep)", pl      # (not folded into the strain-rate pass under the flag)
    h.step(float(g["dt"]))
    assert h.describe_plan() == pl
    h.close()
    if tiles:
        flag.setenv("CALES_DSMAG_REFERENCE_SEQUENCE", "1")
        h = G._hot(case)
        assert h.describe_plan()["sgs"] == "dsmag_reference_sequence(filter2d)"
        h.close()


def test_without_the_flag_nothing_changes(monkeypatch):
    """The field set to False wins over the variable, and the 3-D filter's plan strings are what they were."""
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    g, case = load_golden("chan_dsmag_x64")
    h = G._hot(case.copy(filter2d=False))
    pl = h.describe_plan()
    assert pl["sgs"] == "dsmag_tiles(pair_fields)" and pl["projection"] == "in_strain_rate_pass", pl
    h.close()


def _shaped_case(name, ng):
    g, case = load_golden(name)
    case.ng[:] = ng
    if np.any(case.lwm != 0):      # the sampling height stays above the first cell of the shrunk grid (as tools/fuzz_switches.py keeps it)
        case.hwm = max(float(case.hwm), 1.6 * max(float(case.l[d]) / ng[d] for d in range(3) if case.lwm[:, d].any()))
    if case.inivel == "hcp":
        case.inivel = "poi"
    return case


def _fields(case, seed):
    """The start of tools/fuzz_switches.py: the case's initial field (divergence-free) plus 2 % noise."""
    from cales_amd.hotpath import initflow
    rng = np.random.RandomState(seed)
    u, v, w, p = initflow(case)
    for a in (u, v, w):
        a[1:-1, 1:-1, 1:-1] += 0.02 * (rng.rand(*(int(x) for x in case.ng)) - 0.5)
    return u, v, w, p


def _visct_of_one_call(case, fields, monkeypatch, sequence):
    if sequence:
        monkeypatch.setenv("CALES_DSMAG_REFERENCE_SEQUENCE", "1")
    else:
        monkeypatch.delenv("CALES_DSMAG_REFERENCE_SEQUENCE", raising=False)
    h = G._hot(case)
    h.upload(*(F(a) for a in fields)); h.bounduvw(True, False); h.boundp("p", 0)
    h.cmpt_sgs()
    out, form = h.get("visct")[1:-1, 1:-1, 1:-1].copy(), h.describe_plan()["sgs"]
    h.close()
    return out, form


# 64x16x12: one tile | 126x20x9: partial last x tile of both passes (64- and 62-wide), odd n3, three y tiles of the last pass | 192x12x10: three x tiles |
# 64x16x16, z periodic: the wrap of the ring across the ends. Channels with no-slip and with wall-modelled z faces; the periodic box has no faces to model.
@pytest.mark.parametrize("name,ng", [("chan_dsmag", (64, 16, 12)), ("chan_dsmag_wm", (64, 16, 12)), ("chan_dsmag", (126, 20, 9)), ("chan_dsmag_wm", (126, 20, 9)),
                                     ("chan_dsmag", (192, 12, 10)), ("chan_dsmag_wm", (192, 12, 10)), ("tgv_dsmag_ppp", (64, 16, 16))])
def test_tile_form_equals_the_sequence(name, ng, flag):
    """One cmpt_sgs of the two forms on the same field, interior eddy viscosity. Bound 1e-11 of the field maximum -- the bound the stage replay holds a
    single cmpt_sgs of the tile passes to against the sequence's result (tests/test_gpu_golden.py, tol_sgs0): the forms share every input and differ in
    the association of the filter sums (a few units in the last place per filtered value) and of the plane sums of n1 n2 <= 2520 products, whose
    cancellation in <Mij Lij> costs two to three digits on such fields."""
    case = _shaped_case(name, ng)
    fields = _fields(case, 3)
    tile, form_t = _visct_of_one_call(case, fields, flag, sequence=False)
    seq, form_s = _visct_of_one_call(case, fields, flag, sequence=True)
    assert (form_t, form_s) == ("dsmag_tiles(filter2d)", "dsmag_reference_sequence(filter2d)")
    live = int((np.abs(seq).reshape(-1, ng[2]).max(axis=0) > 0.).sum())
    err = relerr(tile, seq)
    print(f"{name} {ng}: planes with a coefficient {live} of {ng[2]}, tile against sequence {err:.2e}")
    assert np.isfinite(seq).all() and live >= 2      # (a field whose every plane is clipped would compare zeros)
    assert err < 1e-11


def test_several_k_chunks(flag):
    """The last pass in chunks of five planes: the |S|Sij rows in flight and the ring are started inside the field, not only at a wall."""
    flag.setenv("CALES_KCHUNK", "5")
    case = _shaped_case("chan_dsmag", (64, 16, 12))
    fields = _fields(case, 5)
    tile, _ = _visct_of_one_call(case, fields, flag, sequence=False)
    seq, _ = _visct_of_one_call(case, fields, flag, sequence=True)
    assert relerr(tile, seq) < 1e-11


@pytest.mark.parametrize("sequence", [False, True], ids=["tiles", "sequence"])
def test_the_flag_is_not_a_no_op(sequence, monkeypatch):
    case = _shaped_case("chan_dsmag", (64, 16, 12))
    fields = _fields(case, 3)
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    on, form_on = _visct_of_one_call(case, fields, monkeypatch, sequence)
    monkeypatch.delenv("CALES_FILTER_2D")
    off, form_off = _visct_of_one_call(case, fields, monkeypatch, sequence)
    assert "filter2d" in form_on and "filter2d" not in form_off
    assert relerr(on, off) > 1e-3


def test_slabs_equal_one_rank(flag):
    """Two emulated slabs against one rank, two steps, under the flag: the ghost rows of the tile form travel through the same calls as the 3-D filter's."""
    from tests.test_gpu_decomp import _case, _slabs_against_single_rank
    _slabs_against_single_rank(_case("chan_dsmag", (64, 16, 12)), 2, 2)


def test_fortran_host_reads_the_variable(tmp_path):
    """`cales` with CALES_FILTER_2D=1 writes the checkpoint of the Python host with Case.filter2d = True (same library, same sequence: the same bits, as
    tests/test_gpu_fortran_host.py holds the two hosts to), and another one than without the variable."""
    from cales_amd.hotpath import HotPath, initflow
    from cales_amd.nml import parse_text
    from tests import test_gpu_fortran_host as FH
    if not os.path.exists(FH.EXE):
        pytest.skip("Fortran host not built (amdflang absent)")
    text = FH._nml("chan_dsmag", nstep=4, icheck=2, iout0d=2, iout1d=0, iout2d=0, iout3d=0, isave=100000)
    text = re.sub(r"stop_type\(1:3\) = .*", "stop_type(1:3) = T, F, F", text)
    env = {k: v for k, v in os.environ.items() if k != "CALES_FILTER_2D"}
    assert "*** Fim ***" in FH._run(str(tmp_path / "on"), text, env=dict(env, CALES_FILTER_2D="1"))
    assert "*** Fim ***" in FH._run(str(tmp_path / "off"), text, env=env)
    case = parse_text(text); case.filter2d = True
    ng = tuple(int(x) for x in case.ng)
    on, t_on, istep = FH._read_fld(os.path.join(tmp_path, "on", "fld.bin"), ng)
    off, _, _ = FH._read_fld(os.path.join(tmp_path, "off", "fld.bin"), ng)
    assert istep == 4
    h = HotPath(case)
    assert h.describe_plan()["sgs"] == "dsmag_tiles(filter2d)"
    h.upload(*initflow(case)); h.startup()
    dt = min(case.cfl * h.chkdt(), case.dtmax)
    for s in range(1, 5):
        h.step(dt)
        if s % 2 == 0:
            dt = min(case.cfl * h.chkdt(), case.dtmax)
    py = h.download()[:4]
    h.close()
    for a, b in zip(on, py):
        assert np.array_equal(a, b[1:-1, 1:-1, 1:-1])
    assert not np.array_equal(on[0], off[0])      # (another eddy viscosity has acted on u for four steps)

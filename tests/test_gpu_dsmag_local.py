"""The dynamic model WITHOUT averaging of the Germano identity (src/sgs.f90:368-377, the reference's _CAVITY): visct = max(|S| MijLij / MijMij, 0) cell
by cell -- the flag CALES_SGS_AVE_LOCAL on cales_case.sgstype, in Python Case.dsmag_average = 'local' or the environment variable CALES_DSMAG_AVERAGE.

The yardstick is the reference itself built with -D_CAVITY (tests/golden/local, gen_golden_local.py): the same cases, edits and keys as the plane-averaged
goldens, so the replay functions of tests/test_gpu_golden.py run on them UNCHANGED with the variable set. cmpt_sgs is held to the 1e-11 (first call) /
1e-10 (substeps) of tests/test_gpu_dsmag_average.py: on the golden states the reference's own cmpt_sgs moves by 1e-14 .. 1e-13 of the field maximum under
a relative 1e-15 of u, v, w (2e-15 .. 5e-14 when it averages over planes), and an error of the feature is of order one."""
import os
import re

import numpy as np
import pytest

from tests import test_gpu_golden as G
from tests.test_gpu_dsmag_average import _env, _plan, _sgs_errors, _visct_of_one_call
from tests.test_gpu_filter2d import _fields, _shaped_case
from tests.util import F, load_golden, relerr

pytestmark = pytest.mark.gpu

# (file stem under tests/golden/local, plane filter)
STAGES = [("local_cavity_dsmag", 0), ("local_cavity_dsmag_wm_mixed", 0), ("local_tgv_dsmag_ppp", 0), ("local_chan_dsmag", 0), ("local_chan_dsmag_wm", 0),
          ("local_duct_dsmag", 0), ("local_f2d_chan_dsmag", 1)]
END = [("local_tgv_dsmag_ppp_x64", 0), ("local_chan_dsmag_x64", 0)]
IDS = lambda cases: [c[0] for c in cases]      # noqa: E731


@pytest.mark.parametrize("sequence", [False, True], ids=["default_path", "reference_sequence"])
@pytest.mark.parametrize("stem,f2d", STAGES, ids=IDS(STAGES))
def test_stage_replay(stem, f2d, sequence, monkeypatch):
    """Every operator of the start-up and of three substeps against the stage vectors of the reference built with -D_CAVITY: cmpt_sgs at 1e-11 / 1e-10,
    every other operator at the 1e-13 the replay function has."""
    _env(monkeypatch, "local", f2d, sequence)
    errs, form = _sgs_errors("local/" + stem)
    print(f"cmpt_sgs {stem} [{form}]: first call {errs[0]:.2e}, substeps {errs[1]:.2e} {errs[2]:.2e} {errs[3]:.2e}")
    G.test_startup_and_substeps("local/" + stem, general_sgs=False)
    assert errs[0] < 1e-11 and max(errs[1:]) < 1e-10


@pytest.mark.parametrize("stem,f2d", STAGES + END, ids=IDS(STAGES + END))
def test_whole_step(stem, f2d, monkeypatch):
    """cales_step against the end-of-step state of that build: u, v, w 1e-10, p 1e-9, visct 1e-8, divmax < 1e-12 (the existing bounds)."""
    _env(monkeypatch, "local", f2d)
    G.test_fused_step_matches_operator_sequence("local/" + stem)


@pytest.mark.parametrize("name", ["chan_dsmag", "cavity_dsmag"])
@pytest.mark.parametrize("sequence", [False, True], ids=["default_path", "reference_sequence"])
def test_the_word_is_taken_and_is_not_a_no_op(name, sequence, monkeypatch):
    """Before the feature the word `local` is refused (ValueError: unknown averaging). With it, one cmpt_sgs on the golden's start-up state gives the
    -D_CAVITY reference's field, which differs from the plane-averaged one by more than 0.1 of its maximum."""
    g, case = load_golden("local/local_" + name)
    fields = [F(g["s0_" + k]) for k in "uvwp"]

    def one(ave):
        _env(monkeypatch, ave, 0, sequence)
        h = G._hot(case)
        h.upload(*fields); h.cmpt_sgs()
        out = h.get("visct")[1:-1, 1:-1, 1:-1].copy()
        h.close()
        return out
    on, off = one("local"), one("planes")
    want = g["s0_visct_nobc"][1:-1, 1:-1, 1:-1]
    assert np.isfinite(on).all() and relerr(on, want) < 1e-11
    assert np.abs(on - off).max() > 0.1 * np.abs(on).max()
    assert np.abs(want - off).max() > 0.1 * np.abs(want).max()


@pytest.mark.parametrize("stem,f2d", STAGES + END, ids=IDS(STAGES + END))
def test_plan_names_the_averaging_and_the_form(stem, f2d, monkeypatch):
    _env(monkeypatch, "local", f2d)
    g, case = load_golden("local/" + stem)
    pl = _plan(case)
    assert pl["sgs_average"] == "local", pl
    _env(monkeypatch, "planes", f2d)
    planes = _plan(case)
    assert "sgs_average" not in planes, planes
    if f2d:      # the plane filter and local together: the sequence (k_lmf_plane_tile has no local form)
        assert pl["sgs"] == "dsmag_reference_sequence(filter2d)" and planes["sgs"] == "dsmag_tiles(filter2d)", (pl, planes)
    elif "cavity" in stem:      # walls in x: the sequence, under either average
        assert pl["sgs"] == planes["sgs"] == "dsmag_reference_sequence", (pl, planes)
    else:      # x periodic, z walls or periodic: the tile form of the plane average, and the projection where it was
        assert pl["sgs"] == planes["sgs"] and pl["sgs"].startswith("dsmag_tiles"), (pl, planes)
        assert pl["projection"] == planes["projection"], (pl, planes)
    if stem == "local_chan_dsmag_x64":
        assert pl["sgs"] == "dsmag_tiles(pair_fields)" and pl["projection"] == "in_strain_rate_pass", pl
    _env(monkeypatch, "local", f2d, True)
    assert _plan(case)["sgs"].startswith("dsmag_reference_sequence")      # CALES_DSMAG_REFERENCE_SEQUENCE=1 forces the sequence, as before


def test_planes_keep_every_plan_string(monkeypatch):
    """Without the flag the plan of the headline class is what it was, byte for byte, without a new key -- also when the variable names another average
    and the field says planes."""
    g, case = load_golden("chan_dsmag_x64")
    _env(monkeypatch, "planes")
    base = _plan(case)
    assert base == {**base, "sgs": "dsmag_tiles(pair_fields)", "projection": "in_strain_rate_pass"} and "sgs_average" not in base, base
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "local")
    assert _plan(case.copy(dsmag_average="planes")) == base
    on = _plan(case)
    assert {k: v for k, v in on.items() if k != "sgs_average"} == base and on["sgs_average"] == "local"


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("name", ["chan_dsmag_x64", "duct_dsmag"])
def test_slabs_equal_one_rank(name, P, monkeypatch):
    """P emulated slabs against one rank, two steps, at 64 x 16 x 12: nothing of the local coefficient travels and nothing is reduced (the bound of
    tests/test_gpu_dsmag_average.py test_slabs_equal_one_rank: 1e-10 on u, v, w and visct), on a field whose eddy viscosity is not zero."""
    from cales_amd.hotpath import HotPath, initflow
    from tests.test_gpu_decomp import _case, _slabs_against_single_rank
    _env(monkeypatch, "local")
    case = _case(name, (64, 16, 12))
    h = HotPath(case)
    assert h.describe_plan()["sgs_average"] == "local" and h.describe_plan()["sgs"].startswith("dsmag_tiles")
    h.upload(*initflow(case)); h.startup()
    start = h.get("visct")[1:-1, 1:-1, 1:-1]
    h.close()
    assert np.isfinite(start).all() and start.max() > 0.
    _slabs_against_single_rank(case, P, 2)


def test_fortran_host_reads_the_variable(tmp_path):
    """`cales` with CALES_DSMAG_AVERAGE=local prints the plan with sgs_average=local and writes the checkpoint of the Python host with
    Case.dsmag_average = 'local' (same library, same sequence: the same bits, as tests/test_gpu_fortran_host.py holds the two hosts to)."""
    from cales_amd.hotpath import HotPath, initflow
    from cales_amd.nml import parse_text
    from tests import test_gpu_fortran_host as FH
    if not os.path.exists(FH.EXE):
        pytest.skip("Fortran host not built (amdflang absent)")
    text = FH._nml("chan_dsmag", nstep=4, icheck=2, iout0d=2, iout1d=0, iout2d=0, iout3d=0, isave=100000)
    text = re.sub(r"stop_type\(1:3\) = .*", "stop_type(1:3) = T, F, F", text)
    env = {k: v for k, v in os.environ.items() if k not in ("CALES_DSMAG_AVERAGE", "CALES_FILTER_2D", "CALES_DSMAG_REFERENCE_SEQUENCE")}
    out_on = FH._run(str(tmp_path / "on"), text, env=dict(env, CALES_DSMAG_AVERAGE="local"))
    assert "*** Fim ***" in out_on and "sgs_average=local" in out_on
    case = parse_text(text); case.dsmag_average = "local"; case.filter2d = False
    ng = tuple(int(x) for x in case.ng)
    on, _, istep = FH._read_fld(os.path.join(tmp_path, "on", "fld.bin"), ng)
    assert istep == 4
    h = HotPath(case)
    assert h.describe_plan()["sgs_average"] == "local"
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


# The bar of "tile form equals the sequence". Under plane and volume averaging the project holds one cmpt_sgs of the tile passes to 1e-11 of the field maximum
# against the sequence's (tests/test_gpu_filter2d.py, tests/test_gpu_dsmag_average.py). Without averaging the field of these noisy states is spiky -- cells
# with a small MijMij, the maximum many times the 99th percentile -- and a pointwise ratio answers the round-off differences of its operands more strongly
# than a ratio of plane sums. How much more is measured on the REFERENCE, never on the device: `tests/golden/gen_golden_local.py --noise-seeds` runs one
# cmpt_sgs of the -D_CAVITY build and one of the default build on these very fields, each again with u, v, w changed by a relative 1e-14, and prints both
# responses in the relerr metric and their ratio A, local over planes. The bar per shape is 1e-11 max(1, A), for the seed of 1..12 with the smallest A:
#   shape                      seed    local      planes      A       bar
#   chan_dsmag 64x16x12          3    7.94e-14   8.47e-14    0.9    1e-11
#   chan_dsmag_wm 64x16x12       3    1.53e-13   8.26e-14    1.9    1.9e-11
#   chan_dsmag 126x20x9          9    4.83e-12   3.79e-14  127.4    1.274e-9
#   tgv_dsmag_ppp 64x16x16       7    6.98e-13   9.82e-13    0.7    1e-11
#   duct_dsmag 64x12x12          8    2.62e-14   2.23e-14    1.2    1.2e-11
# (126x20x9: A between 127 and 866 over the twelve seeds, every other shape between 0.7 and 10.4.)
TILE_SHAPES = [("chan_dsmag", (64, 16, 12), 0, 3, 0.9),        # one tile
               ("chan_dsmag_wm", (64, 16, 12), 0, 3, 1.9),     # wall-model z faces
               ("chan_dsmag", (126, 20, 9), 0, 9, 127.4),      # partial last x tile of the 62- and 64-wide passes, three y tiles, odd n3
               ("tgv_dsmag_ppp", (64, 16, 16), 0, 7, 0.7),     # periodic z wrap
               ("duct_dsmag", (64, 12, 12), 0, 8, 1.2),        # y walls: the YW instantiation
               ("chan_dsmag", (64, 16, 12), 5, 3, 0.9)]        # chunks of five planes: several chunks


@pytest.mark.parametrize("name,ng,kchunk,seed,A", TILE_SHAPES)
def test_tile_form_equals_the_sequence(name, ng, kchunk, seed, A, monkeypatch):
    """One cmpt_sgs of each form on the same noisy field, interior eddy viscosity, below 1e-11 max(1, A) of the field maximum (table above)."""
    case = _shaped_case(name, ng)
    fields = _fields(case, seed)
    more = {"CALES_KCHUNK": str(kchunk)} if kchunk else {}
    _env(monkeypatch, "local", 0, False, **more)
    tile, form_t, _ = _visct_of_one_call(case, fields)
    _env(monkeypatch, "local", 0, True, **more)
    seq, form_s, _ = _visct_of_one_call(case, fields)
    assert form_t.startswith("dsmag_tiles") and form_s == "dsmag_reference_sequence", (form_t, form_s)
    err = relerr(tile, seq)
    live = float((seq != 0.).mean())
    print(f"{name} {ng} kchunk={kchunk} seed={seed}: tile against sequence {err:.2e} (bar {1e-11 * max(1., A):.3e}), max {np.abs(seq).max():.3e}, {live:.2f} of the cells non-zero")
    assert np.isfinite(seq).all() and np.isfinite(tile).all() and np.abs(seq).max() > 0. and np.abs(tile).max() > 0.
    assert err < 1e-11 * max(1., A)

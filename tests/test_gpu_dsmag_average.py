"""The directions the dynamic model averages the Germano identity over (src/sgs.f90:359-370: the reference's build switches _DIT / _CHANNEL / _DUCT) as a
run-time choice: flags on cales_case.sgstype, in Python Case.dsmag_average or the environment variable CALES_DSMAG_AVERAGE.

The yardstick is the reference itself built for each averaging (tests/golden/average, gen_golden_average.py): the same cases, edits and keys as the
plane-averaged goldens, so the replay functions of tests/test_gpu_golden.py run on them UNCHANGED with the variable set. cmpt_sgs is held to the
replay's 1e-11 (first call) / 1e-10 (substeps) in every averaging case, the kernel-per-loop sequence included: the averaging sum re-associates up to
64 x 16 x 16 products whose cancellation already costs digits -- what those two bounds were set for -- and an error of the feature is of order one.
The eddy viscosity of these files differs from the plane-averaged one by 0.3 to 1800 times its maximum: no replay can pass without the feature."""
import os
import re

import numpy as np
import pytest

from tests import test_gpu_golden as G
from tests.test_gpu_filter2d import _fields, _shaped_case
from tests.util import F, load_golden, relerr

pytestmark = pytest.mark.gpu

# (file stem under tests/golden/average, averaging, plane filter)
STAGES = [("volume_tgv_dsmag_ppp", "volume", 0), ("volume_chan_dsmag", "volume", 0), ("volume_chan_dsmag_wm", "volume", 0), ("volume_duct_dsmag", "volume", 0),
          ("volume_cavity_dsmag", "volume", 0), ("volume_f2d_tgv_dsmag_ppp", "volume", 1), ("volume_f2d_chan_dsmag", "volume", 1),
          ("xlines_duct_dsmag", "xlines", 0), ("xlines_duct_dsmag_wm", "xlines", 0), ("xlines_tgv_dsmag_ppp", "xlines", 0), ("xlines_f2d_duct_dsmag", "xlines", 1)]
END = [("volume_tgv_dsmag_ppp_x64", "volume", 0), ("volume_chan_dsmag_x64", "volume", 0), ("xlines_duct_dsmag_x64", "xlines", 0)]
IDS = lambda cases: [c[0] for c in cases]      # noqa: E731


def _env(mp, ave, f2d=0, sequence=False, **more):
    for k in ("CALES_DSMAG_AVERAGE", "CALES_FILTER_2D", "CALES_DSMAG_REFERENCE_SEQUENCE", "CALES_KCHUNK"):
        mp.delenv(k, raising=False)
    if ave != "planes":
        mp.setenv("CALES_DSMAG_AVERAGE", ave)
    if f2d:
        mp.setenv("CALES_FILTER_2D", "1")
    if sequence:
        mp.setenv("CALES_DSMAG_REFERENCE_SEQUENCE", "1")
    for k, v in more.items():
        mp.setenv(k, v)


def _sgs_errors(name):
    """The errors of the four cmpt_sgs calls of the stage replay (tests/test_gpu_golden.py:45-47,110-114), measured the way it measures them."""
    g, case = load_golden(name)
    h = G._hot(case)
    h.upload(*(F(g["s0_" + k]) for k in "uvwp"))
    h.cmpt_sgs()
    errs = [relerr(h.get("visct")[1:-1, 1:-1, 1:-1], g["s0_visct_nobc"][1:-1, 1:-1, 1:-1])]
    prev = g["s0_visct"]
    for irk in (1, 2, 3):
        K = f"r{irk}_"
        h.upload(*(F(g[K + "s7_" + k]) for k in "uvw"), F(g[K + "s8_p"])); h.set("visct", F(prev))
        h.cmpt_sgs(); h.boundp("visct", 1)
        errs.append(relerr(h.get("visct"), g[K + "s9_visct"]))
        prev = g[K + "s9_visct"]
    form = h.describe_plan()["sgs"]
    h.close()
    return errs, form


@pytest.mark.parametrize("sequence", [False, True], ids=["default_path", "reference_sequence"])
@pytest.mark.parametrize("stem,ave,f2d", STAGES, ids=IDS(STAGES))
def test_stage_replay(stem, ave, f2d, sequence, monkeypatch):
    """Every operator of the start-up and of three substeps against the stage vectors of the reference built for the averaging: cmpt_sgs at 1e-11 / 1e-10,
    every other operator at the 1e-13 the replay function has."""
    _env(monkeypatch, ave, f2d, sequence)
    errs, form = _sgs_errors("average/" + stem)
    print(f"cmpt_sgs {stem} [{form}]: first call {errs[0]:.2e}, substeps {errs[1]:.2e} {errs[2]:.2e} {errs[3]:.2e}")
    G.test_startup_and_substeps("average/" + stem, general_sgs=False)
    assert errs[0] < 1e-11 and max(errs[1:]) < 1e-10


@pytest.mark.parametrize("stem,ave,f2d", STAGES + END, ids=IDS(STAGES + END))
def test_whole_step(stem, ave, f2d, monkeypatch):
    """cales_step against the end-of-step state of that build: u, v, w 1e-10, p 1e-9, visct 1e-8, divmax < 1e-12 (the existing bounds)."""
    _env(monkeypatch, ave, f2d)
    G.test_fused_step_matches_operator_sequence("average/" + stem)


def _plan(case):
    h = G._hot(case)
    pl = h.describe_plan()
    h.close()
    return pl


@pytest.mark.parametrize("stem,ave,f2d", STAGES + END, ids=IDS(STAGES + END))
def test_plan_names_the_averaging(stem, ave, f2d, monkeypatch):
    _env(monkeypatch, ave, f2d)
    g, case = load_golden("average/" + stem)
    pl = _plan(case)
    assert pl["sgs_average"] == {"volume": "volume", "xlines": "x_lines"}[ave], pl
    _env(monkeypatch, "planes", f2d)
    planes = _plan(case)
    assert "sgs_average" not in planes, planes
    if ave == "volume":      # the same form, the same projection, every other key: one key more and nothing else
        assert {k: v for k, v in pl.items() if k != "sgs_average"} == planes
    else:
        assert pl["sgs"] == ("dsmag_reference_sequence(filter2d)" if f2d else "dsmag_reference_sequence"), pl
    if stem == "volume_chan_dsmag_x64":
        assert pl["sgs"] == "dsmag_tiles(pair_fields)" and pl["projection"] == "in_strain_rate_pass", pl


def test_planes_keep_every_plan_string(monkeypatch):
    """No flag, the word `planes` and the empty variable are today's meaning: the plan of the headline class, byte for byte without a new key."""
    g, case = load_golden("chan_dsmag_x64")
    _env(monkeypatch, "planes")
    base = _plan(case)
    assert "sgs_average" not in base and base["sgs"] == "dsmag_tiles(pair_fields)" and base["projection"] == "in_strain_rate_pass", base
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "")
    assert _plan(case) == base
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "volume")
    assert _plan(case.copy(dsmag_average="planes")) == base      # the field, when set, decides


def _visct_of_one_call(case, fields):
    h = G._hot(case)
    h.upload(*(F(a) for a in fields)); h.bounduvw(True, False); h.boundp("p", 0)
    h.cmpt_sgs()
    out, form, cfl = h.get("visct")[1:-1, 1:-1, 1:-1].copy(), h.describe_plan()["sgs"], h.chkdt()
    h.close()
    return out, form, cfl


# The seed of the noise under volume averaging. On white noise the one coefficient of the domain is the small remainder of plane sums of both signs, and
# for about half of the seeds it is negative: the clip zeroes the whole field, in the reference too, and two zero fields compare equal whatever the kernels
# do. The seeds are therefore picked by the REFERENCE built with -D_DIT, run on these very fields on the CPU (`tests/golden/gen_golden_average.py
# --noise-seeds` prints the list) -- never by what the device gives: per shape the seed of 1..12 with the largest coefficient, i.e. the least cancellation
# between the planes. The tests assert a non-zero field themselves, so a bad seed fails instead of passing. The reference's interior maximum of visct:
#   seed 3 (the plane-averaged tests' seed)   0 for every 3-D-filter shape below; 4.5e-8 with the plane filter
#   seed 4    chan_dsmag 64x16x12  3.53e-6 | chan_dsmag_wm 64x16x12  2.72e-6          seed 9    chan_dsmag 126x20x9  3.07e-6 | chan_dsmag_wm 126x20x9  2.89e-6
#   seed 12   tgv_dsmag_ppp 64x16x16  3.66e-6                                         seed 11   chan_dsmag 64x16x12 with the plane filter  7.19e-7
SEED_CHAN = 4      # chan_dsmag at 64x16x12 with the 3-D filter, wherever a test below needs a live volume coefficient


# 64x16x12: one tile | 126x20x9: partial last x tile of both passes (64- and 62-wide), odd n3, three y tiles of the last pass | 64x16x16, z periodic: the
# wrap across the ends | the plane filter's last pass | the last pass in chunks of five planes: partial sums of several chunks per plane
@pytest.mark.parametrize("name,ng,f2d,kchunk,seed", [("chan_dsmag", (64, 16, 12), 0, 0, SEED_CHAN), ("chan_dsmag_wm", (64, 16, 12), 0, 0, 4),
                                                     ("chan_dsmag", (126, 20, 9), 0, 0, 9), ("chan_dsmag_wm", (126, 20, 9), 0, 0, 9),
                                                     ("tgv_dsmag_ppp", (64, 16, 16), 0, 0, 12), ("chan_dsmag", (64, 16, 12), 1, 0, 11),
                                                     ("chan_dsmag", (64, 16, 12), 0, 5, SEED_CHAN)])
def test_tile_form_equals_the_sequence_under_volume(name, ng, f2d, kchunk, seed, monkeypatch):
    """One cmpt_sgs of the two forms on the same field, interior eddy viscosity, below 1e-11 of the field maximum (the bound of a single cmpt_sgs of the
    tile passes against the sequence's result, tests/test_gpu_filter2d.py): both forms hand k_volume_fold plane sums that differ by their association."""
    case = _shaped_case(name, ng)
    fields = _fields(case, seed)
    more = {"CALES_KCHUNK": str(kchunk)} if kchunk else {}
    _env(monkeypatch, "volume", f2d, False, **more)
    tile, form_t, _ = _visct_of_one_call(case, fields)
    _env(monkeypatch, "volume", f2d, True, **more)
    seq, form_s, _ = _visct_of_one_call(case, fields)
    assert form_t.startswith("dsmag_tiles") and form_s.startswith("dsmag_reference_sequence"), (form_t, form_s)
    err = relerr(tile, seq)
    print(f"{name} {ng} f2d={f2d} kchunk={kchunk} seed={seed}: tile against sequence {err:.2e}, max {np.abs(seq).max():.3e}")
    assert np.isfinite(seq).all() and np.isfinite(tile).all() and np.abs(seq).max() > 0. and np.abs(tile).max() > 0.
    assert err < 1e-11


def test_lazy_and_materialised_forms_agree_under_volume(monkeypatch):
    """Homogeneous sgs boundary values: the tile form leaves |S| in visct and the coefficient in cs(k) (k_dsmag_coef; k_scale_planes when the field is
    downloaded). One non-zero boundary value -- it reaches ghost cells only, and only through boundp -- switches that off: k_dsmag_final writes the
    product. The interior fields differ by the rounding of |S| (lm/mm) against (|S| lm)/mm: two roundings each, below 1e-14 of the maximum; and the time
    step limit chkdt reads behind the lazy form is that of the sequence's field to the bound of the tile comparison."""
    case = _shaped_case("chan_dsmag", (64, 16, 12))
    fields = _fields(case, SEED_CHAN)
    _env(monkeypatch, "volume")
    lazy, form, cfl_lazy = _visct_of_one_call(case, fields)
    eager_case = case.copy(); eager_case.bcsgs[0, 2] = 1e-30
    eager, form_e, _ = _visct_of_one_call(eager_case, fields)
    assert form == form_e == "dsmag_tiles(pair_fields)" and np.abs(lazy).max() > 0.
    assert relerr(lazy, eager) < 1e-14
    _env(monkeypatch, "volume", 0, True)
    seq, _, cfl_seq = _visct_of_one_call(case, fields)
    assert abs(cfl_lazy / cfl_seq - 1.) < 1e-11


def _lines_all_zero_or_all_positive(inner):
    lo, hi = inner.min(axis=0), inner.max(axis=0)
    return bool(((hi == 0.) | (lo > 0.)).all()), int((hi > 0.).sum())


@pytest.mark.parametrize("f2d", [0, 1], ids=["filter3d", "filter2d"])
def test_x_lines_are_constant_along_x(f2d, monkeypatch):
    """visct = |S| c(j, k) with c >= 0: visct/|S| cannot be formed from outside, the exact consequence can -- a line (j, k) is all zero or all positive
    (|S| > 0 in every cell of a noisy field). 64 x 12 x 12: three blocks of four lines per plane row, several lines per wave's block."""
    case = _shaped_case("duct_dsmag", (64, 12, 12))
    fields = _fields(case, 3)
    _env(monkeypatch, "xlines", f2d)
    lines, form, _ = _visct_of_one_call(case, fields)
    ok, live = _lines_all_zero_or_all_positive(lines)
    print(f"duct_dsmag 64x12x12 f2d={f2d}: {live} of 144 lines carry a coefficient")
    assert form.startswith("dsmag_reference_sequence") and np.isfinite(lines).all()
    assert ok and live > 0
    _env(monkeypatch, "planes", f2d, True)
    planes, _, _ = _visct_of_one_call(case, fields)
    assert relerr(lines, planes) > 1e-3


def test_x_lines_rows_longer_than_a_wave_and_partial_segments(monkeypatch):
    """Rows of 150 cells (two whole segments of 64 and one of 22 cells) and 6 x 7 lines (the last block has two waves with a line and two without):
    the same exact property, and the result is not the plane-averaged one."""
    case = _shaped_case("duct_dsmag", (150, 6, 7))
    fields = _fields(case, 7)
    _env(monkeypatch, "xlines")
    lines, _, _ = _visct_of_one_call(case, fields)
    ok, live = _lines_all_zero_or_all_positive(lines)
    assert np.isfinite(lines).all() and ok and live > 0
    _env(monkeypatch, "planes", 0, True)
    planes, _, _ = _visct_of_one_call(case, fields)
    assert relerr(lines, planes) > 1e-3


def test_x_lines_against_the_end_of_step_golden(monkeypatch):
    """The 64 x 12 x 12 duct of the reference built for x lines: the device's end-of-step eddy viscosity is the golden's (1e-8, the whole-step bound), has
    the golden's set of clipped lines, and is not the plane-averaged golden's."""
    _env(monkeypatch, "xlines")
    g, case = load_golden("average/xlines_duct_dsmag_x64")
    h = G._hot(case)
    h.upload(*(F(g["s0raw_" + k]) for k in "uvwp")); h.startup()
    h.step(float(g["dt"]))
    visct = h.download()[4]
    h.close()
    assert relerr(visct, g["r3_s9_visct"]) < 1e-8
    ok, live = _lines_all_zero_or_all_positive(visct[1:-1, 1:-1, 1:-1])
    ok_g, live_g = _lines_all_zero_or_all_positive(g["r3_s9_visct"][1:-1, 1:-1, 1:-1])
    assert ok and ok_g and live == live_g
    assert relerr(visct, load_golden("duct_dsmag_x64")[0]["r3_s9_visct"]) > 1e-3


@pytest.mark.parametrize("sequence", [False, True], ids=["tiles", "sequence"])
@pytest.mark.parametrize("ave", ["volume", "xlines"])
def test_the_averaging_is_not_a_no_op(ave, sequence, monkeypatch):
    case = _shaped_case("chan_dsmag", (64, 16, 12))
    fields = _fields(case, SEED_CHAN)      # (volume: a live coefficient -- against a clipped one the planes' field would differ whatever the kernels do)
    _env(monkeypatch, ave, 0, sequence)
    on, form_on, _ = _visct_of_one_call(case, fields)
    _env(monkeypatch, "planes", 0, sequence)
    off, form_off, _ = _visct_of_one_call(case, fields)
    assert form_off == ("dsmag_reference_sequence" if sequence else "dsmag_tiles(pair_fields)")
    assert form_on == (form_off if ave == "volume" else "dsmag_reference_sequence")      # (x lines: the sequence whatever is asked for)
    assert np.isfinite(on).all() and np.abs(on).max() > 0. and relerr(on, off) > 1e-3


@pytest.mark.parametrize("ave", ["volume", "xlines"])
def test_slabs_equal_one_rank(ave, monkeypatch):
    """Two emulated slabs against one rank, two steps: under volume every rank folds the same all-reduced plane sums, under x lines nothing travels."""
    from tests.test_gpu_decomp import _case, _slabs_against_single_rank
    _env(monkeypatch, ave)
    case = _case("chan_dsmag", (64, 16, 12))
    assert _plan(case)["sgs_average"] == {"volume": "volume", "xlines": "x_lines"}[ave]
    _slabs_against_single_rank(case, 2, 2)


def test_slabs_equal_one_rank_with_a_live_volume_coefficient(monkeypatch):
    """The un-perturbed initial field of the test above has a negative volume coefficient (the reference built with -D_DIT returns visct = 0 on it:
    gen_golden_average.py --noise-seeds, seed -1), so there k_volume_fold behind the all-reduce of the plane sums is held to 0 = 0. Here the field carries
    the noise of SEED_CHAN, on which the reference's coefficient is positive: the eddy viscosity behind the start-up's cmpt_sgs is non-zero, and after
    two steps under it two slabs give the one rank's u, v, w and eddy viscosity (1e-10, the bound of _slabs_against_single_rank)."""
    from cales_amd.decomp import run_loopback
    from cales_amd.hotpath import HotPath
    _env(monkeypatch, "volume")
    case = _shaped_case("chan_dsmag", (64, 16, 12))
    fields = _fields(case, SEED_CHAN)
    h = HotPath(case)
    assert h.describe_plan()["sgs_average"] == "volume"
    h.upload(*fields); h.startup()
    start = h.get("visct")[1:-1, 1:-1, 1:-1].max()
    h.close()
    h = HotPath(case)
    h.upload(*fields); h.startup()
    dt = 0.5 * h.chkdt()
    for _ in range(2):
        h.step(dt)
    one = h.download()
    h.close()
    print(f"one rank, volume: max visct behind the start-up {start:.3e}, after two steps {one[4][1:-1, 1:-1, 1:-1].max():.3e}")
    assert start > 0.      # (the reference's 3.53e-6 on this field; it acts on u, v, w in the first step whatever sign the later coefficients take)

    def body(h, r):
        h.upload_global(*fields); h.startup()
        for _ in range(2):
            h.step(dt)
        return h.download() + [h.lo, h.n]
    for r, R in enumerate(run_loopback(case, 2, body)):
        sl = slice(R[5][1], R[5][1] + R[6][1])
        for q, nm in ((0, "u"), (1, "v"), (2, "w"), (4, "visct")):
            assert relerr(R[q][:, 1:-1, :], one[q][:, sl, :]) < 1e-10, (r, nm)


def test_fortran_host_reads_the_variable(tmp_path):
    """`cales` with CALES_DSMAG_AVERAGE=volume writes the checkpoint of the Python host with Case.dsmag_average = 'volume' (same library, same sequence:
    the same bits, as tests/test_gpu_fortran_host.py holds the two hosts to), and another one than without the variable."""
    from cales_amd.hotpath import HotPath, initflow
    from cales_amd.nml import parse_text
    from tests import test_gpu_fortran_host as FH
    if not os.path.exists(FH.EXE):
        pytest.skip("Fortran host not built (amdflang absent)")
    text = FH._nml("chan_dsmag", nstep=4, icheck=2, iout0d=2, iout1d=0, iout2d=0, iout3d=0, isave=100000)
    text = re.sub(r"stop_type\(1:3\) = .*", "stop_type(1:3) = T, F, F", text)
    env = {k: v for k, v in os.environ.items() if k not in ("CALES_DSMAG_AVERAGE", "CALES_FILTER_2D", "CALES_DSMAG_REFERENCE_SEQUENCE")}
    out_on = FH._run(str(tmp_path / "on"), text, env=dict(env, CALES_DSMAG_AVERAGE="volume"))
    assert "*** Fim ***" in out_on and "sgs_average=volume" in out_on
    assert "*** Fim ***" in FH._run(str(tmp_path / "off"), text, env=env)
    case = parse_text(text); case.dsmag_average = "volume"; case.filter2d = False
    ng = tuple(int(x) for x in case.ng)
    on, t_on, istep = FH._read_fld(os.path.join(tmp_path, "on", "fld.bin"), ng)
    off, _, _ = FH._read_fld(os.path.join(tmp_path, "off", "fld.bin"), ng)
    assert istep == 4
    h = HotPath(case)
    assert h.describe_plan()["sgs_average"] == "volume"
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

"""The reference's _DIT / _CHANNEL / _DUCT (the directions the dynamic model averages the Germano identity over, src/sgs.f90:359-370) as a run-time
choice, host side: the one switch as the Python host hands it to the library (Case.dsmag_average / CALES_DSMAG_AVERAGE -> a flag of
enum cales_sgs_average OR-ed onto cales_case.sgstype), what cales_check_case refuses, and the reference-made goldens under tests/golden/average
(gen_golden_average.py)."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.util import GOLD, load_golden

AVE = os.path.join(GOLD, "average")
# file stem -> (dsmag_average, plane filter, end-of-step state only)
FILES = {"volume_tgv_dsmag_ppp": ("volume", 0, 0), "volume_chan_dsmag": ("volume", 0, 0), "volume_chan_dsmag_wm": ("volume", 0, 0),
         "volume_duct_dsmag": ("volume", 0, 0), "volume_cavity_dsmag": ("volume", 0, 0), "volume_tgv_dsmag_ppp_x64": ("volume", 0, 1),
         "volume_chan_dsmag_x64": ("volume", 0, 1), "volume_f2d_tgv_dsmag_ppp": ("volume", 1, 0), "volume_f2d_chan_dsmag": ("volume", 1, 0),
         "xlines_duct_dsmag": ("xlines", 0, 0), "xlines_duct_dsmag_wm": ("xlines", 0, 0), "xlines_tgv_dsmag_ppp": ("xlines", 0, 0),
         "xlines_duct_dsmag_x64": ("xlines", 0, 1), "xlines_f2d_duct_dsmag": ("xlines", 1, 0)}


def test_the_switch_reaches_the_library_as_flags_on_sgstype(monkeypatch):
    from cales_amd import capi
    monkeypatch.delenv("CALES_DSMAG_AVERAGE", raising=False)
    monkeypatch.delenv("CALES_FILTER_2D", raising=False)
    _, case = load_golden("chan_dsmag")
    assert case.dsmag_average is None
    assert capi.make_case(case).sgstype == 2
    assert capi.make_case(case.copy(dsmag_average="planes")).sgstype == 2
    assert capi.make_case(case.copy(dsmag_average="volume")).sgstype == 6
    assert capi.make_case(case.copy(dsmag_average="xlines")).sgstype == 10
    assert capi.make_case(case.copy(dsmag_average="volume", filter2d=True)).sgstype == 7
    assert capi.make_case(case.copy(dsmag_average="xlines", filter2d=True)).sgstype == 11
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "volume")
    assert capi.make_case(case).sgstype == 6
    assert capi.make_case(case.copy(dsmag_average="planes")).sgstype == 2      # the field, when set, decides
    assert capi.make_case(case.copy(dsmag_average="xlines")).sgstype == 10
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "xlines")
    assert capi.make_case(case).sgstype == 10
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    assert capi.make_case(case).sgstype == 11
    monkeypatch.delenv("CALES_FILTER_2D")
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "")      # empty = unset = planes
    assert capi.make_case(case).sgstype == 2


def test_the_other_models_ignore_the_switch(monkeypatch):
    """... as the reference ignores the macros outside case('dsmag') -- even an unknown word."""
    from cales_amd import capi
    for word in ("volume", "xlines", "cube"):
        monkeypatch.setenv("CALES_DSMAG_AVERAGE", word)
        for name, code in (("chan_smag", 1), ("tgv_ppp", 0)):
            _, other = load_golden(name)
            assert capi.make_case(other).sgstype == code
            assert capi.make_case(other.copy(dsmag_average="volume")).sgstype == code
            assert capi.make_case(other.copy(dsmag_average="cube")).sgstype == code


def test_an_unknown_word_is_an_error(monkeypatch):
    from cales_amd import capi
    monkeypatch.delenv("CALES_DSMAG_AVERAGE", raising=False)
    _, case = load_golden("chan_dsmag")
    with pytest.raises(ValueError, match="averaging"):
        capi.make_case(case.copy(dsmag_average="cube"))
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "Volume")      # (the words are case-sensitive, like the reference's macros)
    with pytest.raises(ValueError, match="averaging"):
        capi.make_case(case)
    assert capi.make_case(case.copy(dsmag_average="volume")).sgstype == 6


def test_header_names_the_flags():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "cales.h")).read()
    m = re.search(r"enum cales_sgs_average \{([^}]*)\}", text)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert vals == {"CALES_SGS_AVE_VOLUME": 4, "CALES_SGS_AVE_XLINES": 8}
    f90 = open(os.path.join(root, "cales_amd", "fortran", "cales_c.f90")).read()
    assert re.search(r"CALES_SGS_AVE_VOLUME = 4, CALES_SGS_AVE_XLINES = 8", f90)


def test_check_case_accepts_the_four_and_refuses_the_rest():
    from cales_amd import capi
    L = capi.lib()      # (host-side entry: no GPU needed, as in tests/test_host_side.py)
    _, case = load_golden("chan_dsmag")
    buf = C.create_string_buffer(512)
    cs = capi.make_case(case)
    for ok in (2, 3, 6, 7, 10, 11):
        cs.sgstype = ok
        assert L.cales_check_case(C.byref(cs), buf, 512) == 0, (ok, buf.value)
    for bad in (12, 13, 14, 15):      # both flags together
        cs.sgstype = bad
        assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"exclude" in buf.value, (bad, buf.value)
    for bad in (4, 5, 8, 9):      # a flag on 'none' or 'smag'
        cs.sgstype = bad
        assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"dynamic" in buf.value, (bad, buf.value)
    for bad in (-1, 16, 18, 34):      # any other value
        cs.sgstype = bad
        assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"SGS" in buf.value, (bad, buf.value)


def test_manifest_matches_the_files():
    man = json.load(open(os.path.join(AVE, "manifest.json")))
    files = sorted(f for f in os.listdir(AVE) if f.endswith(".npz"))
    assert files == sorted(man["files"]) == sorted(n + ".npz" for n in FILES)
    for f, h in man["files"].items():
        assert hashlib.sha256(open(os.path.join(AVE, f), "rb").read()).hexdigest()[:16] == h, f
        assert os.path.getsize(os.path.join(AVE, f)) <= 1 << 20, f
    listed = {v + "_" + n: (d["dsmag_average"], int(d["filter2d"]), int(n in d["end_only"])) for v, d in man["variants"].items() for n in d["stage_by_stage"] + d["end_only"]}
    assert listed == FILES


@pytest.mark.parametrize("stem", sorted(FILES))
def test_golden_is_of_its_build_and_shows_its_coefficients(stem):
    """Every file says which build made it, is the same case as its plane-averaged counterpart and differs from it where the averaging acts. The clip
    max(.,0) (sgs.f90:377) hides every error of a zeroed coefficient: the volume files have a positive coefficient after every substep they hold, the
    x-line files one in at least two fifths of their lines."""
    ave, f2d, end = FILES[stem]
    name = stem[len(ave) + (5 if f2d else 1):]
    g, case = load_golden("average/" + stem)
    g3, _ = load_golden(("filter2d/" if f2d else "") + name)
    assert str(g["dsmag_average"]) == ave and ("filter2d" in g.files) == bool(f2d) and "dsmag_average" not in g3.files
    assert str(g["input_nml"]) == str(g3["input_nml"]) and case.sgstype == "dsmag"
    assert sorted(set(g.files) - {"dsmag_average"}) == sorted(g3.files)
    assert ("r1_s9_visct" in g.files) == (not end)
    assert np.array_equal(g["s0raw_u"], g3["s0raw_u"])
    v, v3 = g["r3_s9_visct"], g3["r3_s9_visct"]
    assert np.isfinite(v).all() and g["r3_div"][1] < 1e-12
    assert np.abs(v - v3).max() > 1e-3 * np.abs(v3).max()
    if ave == "volume":
        for k in ("r1_s9_visct", "r2_s9_visct", "r3_s9_visct"):
            if k in g.files:
                assert g[k][1:-1, 1:-1, 1:-1].max() > 0., k
    else:
        inner = v[1:-1, 1:-1, 1:-1]
        live = int((np.abs(inner).max(axis=0) > 0.).sum())
        assert 5 * live >= 2 * inner.shape[1] * inner.shape[2], (live, inner.shape)
        lo, hi = inner.min(axis=0), inner.max(axis=0)
        assert ((hi == 0.) | (lo > 0.)).all()      # a line is all zero or all positive: |S| > 0 times one coefficient

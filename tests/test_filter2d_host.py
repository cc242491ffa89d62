"""The reference's -D_FILTER_2D as a run-time choice, host side: the reference-made goldens under tests/golden/filter2d (gen_golden_filter2d.py)
and the one switch as the Python host hands it to the library (Case.filter2d / CALES_FILTER_2D -> cales_case.sgstype = 3)."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.util import GOLD, load_golden

F2D = os.path.join(GOLD, "filter2d")
STAGES = ["chan_dsmag", "chan_dsmag_wm", "tgv_dsmag_ppp", "duct_dsmag", "duct_dsmag_wm", "cavity_dsmag"]
END = ["chan_dsmag_x64", "chan_dsmag_x128", "tgv_dsmag_ppp_x64", "duct_dsmag_x64"]


def test_manifest_matches_the_files():
    man = json.load(open(os.path.join(F2D, "manifest.json")))
    assert man["cases"] == STAGES + END and man["stage_by_stage"] == STAGES and man["end_only"] == END
    files = sorted(f for f in os.listdir(F2D) if f.endswith(".npz"))
    assert files == sorted(man["files"]) == sorted(n + ".npz" for n in STAGES + END)
    for f, h in man["files"].items():
        assert hashlib.sha256(open(os.path.join(F2D, f), "rb").read()).hexdigest()[:16] == h, f
        assert os.path.getsize(os.path.join(F2D, f)) <= 1 << 20, f


@pytest.mark.parametrize("name", STAGES + END)
def test_golden_is_of_the_flag_build_and_shows_its_planes(name):
    """Every file says which build made it, is the same case as its 3-D-filter counterpart, differs from it where the filter acts, and has a non-zero
    coefficient in at least half of its z planes (a plane the clip of sgs.f90:372-380 has zeroed hides every error of its sums)."""
    g, case = load_golden("filter2d/" + name)
    g3, case3 = load_golden(name)
    assert int(g["filter2d"]) == 1 and "filter2d" not in g3.files
    assert str(g["input_nml"]) == str(g3["input_nml"]) and case.sgstype == "dsmag"
    assert sorted(set(g.files) - {"filter2d"}) == sorted(g3.files)
    assert np.array_equal(g["s0raw_u"], g3["s0raw_u"])
    v, v3 = g["r3_s9_visct"], g3["r3_s9_visct"]
    assert np.isfinite(v).all() and g["r3_div"][1] < 1e-12
    assert np.abs(v - v3).max() > 1e-3 * np.abs(v3).max()
    inner = v[1:-1, 1:-1, 1:-1]
    live = int((np.abs(inner).reshape(-1, inner.shape[2]).max(axis=0) > 0.).sum())
    assert 2 * live >= inner.shape[2], (live, inner.shape[2])


def test_the_switch_reaches_the_library_as_sgstype_3(monkeypatch):
    from cales_amd import capi
    monkeypatch.delenv("CALES_FILTER_2D", raising=False)
    _, case = load_golden("chan_dsmag")
    assert case.filter2d is None
    assert capi.make_case(case).sgstype == 2
    assert capi.make_case(case.copy(filter2d=True)).sgstype == 3 == capi.SGS_DSMAG_FILTER2D
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    assert capi.make_case(case).sgstype == 3
    assert capi.make_case(case.copy(filter2d=False)).sgstype == 2      # the field, when set, decides
    monkeypatch.setenv("CALES_FILTER_2D", "0")
    assert capi.make_case(case).sgstype == 2
    # the reference ignores the flag for the other models
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    for name, code in (("chan_smag", 1), ("tgv_ppp", 0)):
        _, other = load_golden(name)
        assert capi.make_case(other).sgstype == code and capi.make_case(other.copy(filter2d=True)).sgstype == code


def test_header_names_the_value():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "cales.h")).read()
    m = re.search(r"enum cales_sgstype \{([^}]*)\}", text)
    vals = dict((k.strip(), int(v)) for k, v in (e.split("=") for e in m.group(1).split(",")))
    assert vals == {"CALES_SGS_NONE": 0, "CALES_SGS_SMAG": 1, "CALES_SGS_DSMAG": 2, "CALES_SGS_DSMAG_FILTER2D": 3}


def test_check_case_accepts_3_and_refuses_4():
    from cales_amd import capi
    L = capi.lib()      # (host-side entry: no GPU needed, as in tests/test_host_side.py)
    _, case = load_golden("chan_dsmag")
    buf = C.create_string_buffer(512)
    cs = capi.make_case(case.copy(filter2d=True))
    assert cs.sgstype == 3 and L.cales_check_case(C.byref(cs), buf, 512) == 0, buf.value
    cs.sgstype = 4
    assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"SGS" in buf.value

"""The reference's _CAVITY (no averaging of the Germano identity: visct = max(|S| MijLij / MijMij, 0) cell by cell, src/sgs.f90:368-377) as a run-time
choice, host side: the word `local` as the Python host hands it to the library (Case.dsmag_average / CALES_DSMAG_AVERAGE -> CALES_SGS_AVE_LOCAL = 64
OR-ed onto cales_case.sgstype: 66, 67), what cales_check_case accepts and refuses, the flag as the header and cales_c.f90 declare it, and the
reference-made goldens under tests/golden/local (gen_golden_local.py)."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.util import GOLD, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOC = os.path.join(GOLD, "local")
# file stem -> (plane filter, end-of-step state only)
FILES = {"local_cavity_dsmag": (0, 0), "local_cavity_dsmag_wm_mixed": (0, 0), "local_tgv_dsmag_ppp": (0, 0), "local_chan_dsmag": (0, 0),
         "local_chan_dsmag_wm": (0, 0), "local_duct_dsmag": (0, 0), "local_f2d_chan_dsmag": (1, 0), "local_tgv_dsmag_ppp_x64": (0, 1),
         "local_chan_dsmag_x64": (0, 1)}


def test_the_word_reaches_the_library_as_66_and_67(monkeypatch):
    from cales_amd import capi
    monkeypatch.delenv("CALES_DSMAG_AVERAGE", raising=False)
    monkeypatch.delenv("CALES_FILTER_2D", raising=False)
    _, case = load_golden("chan_dsmag")
    assert capi.SGS_AVE["local"] == 64
    assert capi.make_case(case).sgstype == 2
    assert capi.make_case(case.copy(dsmag_average="local")).sgstype == 66
    assert capi.make_case(case.copy(dsmag_average="local", filter2d=True)).sgstype == 67
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "local")
    assert capi.make_case(case).sgstype == 66
    assert capi.make_case(case.copy(dsmag_average="planes")).sgstype == 2      # the field, when set, decides
    assert capi.make_case(case.copy(dsmag_average="volume")).sgstype == 6
    monkeypatch.setenv("CALES_FILTER_2D", "1")
    assert capi.make_case(case).sgstype == 67
    monkeypatch.delenv("CALES_FILTER_2D")
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "volume")
    assert capi.make_case(case.copy(dsmag_average="local")).sgstype == 66


def test_the_other_models_ignore_the_word(monkeypatch):
    from cales_amd import capi
    monkeypatch.setenv("CALES_DSMAG_AVERAGE", "local")
    for name, code in (("chan_smag", 1), ("tgv_ppp", 0)):
        _, other = load_golden(name)
        assert capi.make_case(other).sgstype == code
        assert capi.make_case(other.copy(dsmag_average="local")).sgstype == code


def test_unknown_words_stay_errors(monkeypatch):
    from cales_amd import capi
    monkeypatch.delenv("CALES_DSMAG_AVERAGE", raising=False)
    _, case = load_golden("chan_dsmag")
    for word in ("cube", "Volume", "Local", "cavity"):      # (the words are case-sensitive, like the reference's macros)
        with pytest.raises(ValueError, match="averaging"):
            capi.make_case(case.copy(dsmag_average=word))
        monkeypatch.setenv("CALES_DSMAG_AVERAGE", word)
        with pytest.raises(ValueError, match="averaging"):
            capi.make_case(case)
        monkeypatch.delenv("CALES_DSMAG_AVERAGE")


def test_header_and_fortran_module_declare_the_flag():
    text = open(os.path.join(ROOT, "include", "cales.h")).read()
    m = re.search(r"enum cales_sgs_average \{([^}]*)\}", text)      # the closed list of the two other flags stays as it is ...
    assert "CALES_SGS_AVE_LOCAL" not in m.group(1)
    decl = re.findall(r"^enum\s*\{\s*CALES_SGS_AVE_LOCAL\s*=\s*(\d+)\s*\};", text, re.M)      # ... the new flag has a declaration of its own
    assert decl == ["64"], decl
    f90 = open(os.path.join(ROOT, "cales_amd", "fortran", "cales_c.f90")).read()
    assert re.search(r"integer\(c_int32_t\), parameter :: CALES_SGS_AVE_LOCAL = 64", f90)
    assert re.search(r"CALES_SGS_AVE_VOLUME = 4, CALES_SGS_AVE_XLINES = 8", f90)
    main = open(os.path.join(ROOT, "cales_amd", "fortran", "cales_main.f90")).read()
    assert re.search(r"case\('local'\);\s*cs%sgstype = ior\(cs%sgstype,CALES_SGS_AVE_LOCAL\)", main)


def test_check_case_accepts_66_and_67_and_refuses_the_rest():
    from cales_amd import capi
    L = capi.lib()      # (host-side entry: no GPU needed, as in tests/test_host_side.py)
    _, case = load_golden("chan_dsmag")
    buf = C.create_string_buffer(512)
    cs = capi.make_case(case)
    for ok in (2, 3, 6, 7, 10, 11, 66, 67):
        cs.sgstype = ok
        assert L.cales_check_case(C.byref(cs), buf, 512) == 0, (ok, buf.value)
    for bad in (70, 71, 74, 75, 78, 79, 12, 15):      # local with volume, with x lines, with both; the two others together
        cs.sgstype = bad
        assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"exclude" in buf.value, (bad, buf.value)
    for bad in (64, 65, 4, 9):      # a flag on 'none' or 'smag'
        cs.sgstype = bad
        assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"dynamic" in buf.value, (bad, buf.value)
    for bad in (-1, 16, 18, 34, 32, 50, 82, 98, 128, 130, 194):      # any other value: the bits 16, 32 and 128 mean nothing
        cs.sgstype = bad
        assert L.cales_check_case(C.byref(cs), buf, 512) != 0 and b"SGS" in buf.value, (bad, buf.value)


def test_linebench_takes_the_word():
    import importlib.util
    spec = importlib.util.spec_from_file_location("linebench", os.path.join(ROOT, "tools", "linebench.py"))
    lb = importlib.util.module_from_spec(spec); spec.loader.exec_module(lb)
    assert lb.load("turbulent_channel.nml:64x16x12:sgs=dsmag,average=local").dsmag_average == "local"
    with pytest.raises(SystemExit):
        lb.load("turbulent_channel.nml:64x16x12:sgs=dsmag,average=cube")


def test_manifest_matches_the_files():
    man = json.load(open(os.path.join(LOC, "manifest.json")))
    files = sorted(f for f in os.listdir(LOC) if f.endswith(".npz"))
    assert files == sorted(man["files"]) == sorted(n + ".npz" for n in FILES)
    for f, h in man["files"].items():
        assert hashlib.sha256(open(os.path.join(LOC, f), "rb").read()).hexdigest()[:16] == h, f
        assert os.path.getsize(os.path.join(LOC, f)) <= 1 << 20, f
    listed = {v + "_" + n: (int(d["filter2d"]), int(n in d["end_only"])) for v, d in man["variants"].items() for n in d["stage_by_stage"] + d["end_only"]}
    assert listed == FILES and all(d["dsmag_average"] == "local" for d in man["variants"].values())


@pytest.mark.parametrize("stem", sorted(FILES))
def test_golden_is_of_its_build_and_shows_its_cells(stem):
    """Every file says which build made it, is the same case as its plane-averaged counterpart and differs from it. The clip max(.,0) (sgs.f90:377)
    hides every error of a cell it has zeroed: every eddy viscosity the file holds is finite (no cell with 0/0) and more than two fifths of the
    interior cells of the last one are non-zero."""
    f2d, end = FILES[stem]
    name = stem[len("local_f2d_" if f2d else "local_"):]
    g, case = load_golden("local/" + stem)
    g3, _ = load_golden(("filter2d/" if f2d else "") + name)
    assert str(g["dsmag_average"]) == "local" and ("filter2d" in g.files) == bool(f2d) and "dsmag_average" not in g3.files
    assert str(g["input_nml"]) == str(g3["input_nml"]) and case.sgstype == "dsmag"
    assert sorted(set(g.files) - {"dsmag_average"}) == sorted(g3.files)
    assert ("r1_s9_visct" in g.files) == (not end)
    assert np.array_equal(g["s0raw_u"], g3["s0raw_u"])
    for k in g.files:
        if k.endswith("_visct"):
            assert np.isfinite(g[k]).all(), k
    v, v3 = g["r3_s9_visct"], g3["r3_s9_visct"]
    assert g["r3_div"][1] < 1e-12
    assert np.abs(v - v3).max() > 0.1 * np.abs(v).max()
    inner = v[1:-1, 1:-1, 1:-1]
    assert 5 * int((inner != 0.).sum()) > 2 * inner.size and inner.min() >= 0.

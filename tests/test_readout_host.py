"""The host part of what the field read-outs share (cales_amd/csrc/readout.hpp) and the launch geometry of the spectra (spectral_line.hpp), checked on the CPU.

tests/readout_host.cpp is a stand-alone program (its own main, nothing loaded into Python) that includes the headers api.hip, k_pdf.hip and k_spectra.hip
use: the rows-per-block rule against the two functions it replaced, restated to the letter, over n1, n2 = 1..2048 and 1..64 planes; the geometry of
k_spec_x, k_spec_y and k_spec_y2 for one and two fields and reals of 4 and 8 bytes against the rules the power spectra and the cross-spectra had when
each had kernels of its own, restated to the letter, over the same ranges; the carver of a
call's temporary (16-byte alignment of every part, no overlap, the end inside the total, for reals of 4 and 8 bytes); the plane list (three refusals,
repeats in any order accepted). Built with the host compiler under -fsanitize=address,undefined and run once."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cales_amd", "csrc")


def test_row_rule_carver_and_plane_list(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "readout_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "readout_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"(\d+) row rules, (\d+) spectra geometries, (\d+) carved temporaries, (\d+) plane lists checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 10 ** 6 and int(m.group(2)) > 4 * 10 ** 6 and int(m.group(3)) > 10 ** 4 and int(m.group(4)) >= 10, r.stdout


def test_the_field_id_is_checked_in_one_place():
    """`>= CALES_NFIELDS` appears in the library once: in field_ptr (api.hip), which every entry that takes a field id goes through"""
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cpp", ".hpp")):
            hits += [name for line in open(os.path.join(CSRC, name)) if ">= CALES_NFIELDS" in line]
    assert hits == ["api.hip"], hits

"""The lane map of the packed remainder tile of the dynamic model's last pass (cales_amd/csrc/lmf_pack.hpp), checked on the CPU.

tests/lmf_packing_host.cpp is a stand-alone program (its own main, nothing loaded into Python) that includes the header the kernel uses and walks every
row length 1..1100 and row count 1..40: full tiles plus packed blocks put out every cell exactly once, x neighbours sit in the adjacent lanes of the
same segment with the wrapped column at the row's ends, dead segments and lanes stay inside the field, and packing is chosen exactly when full >= 1,
rem >= 1 and S >= 2. Built with the host compiler under -fsanitize=address,undefined and run once."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lane_map_of_the_packed_remainder_tile(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lmf_packing_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "cales_amd", "csrc"), os.path.join(ROOT, "tests", "lmf_packing_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "0 failures" in r.stdout and not r.stdout.startswith("0 packed shapes"), r.stdout


def test_the_switch_is_listed_in_the_design_document():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "CALES_LMF_UNPACKED_REMAINDER" in text[text.index("Run-time switches"):]

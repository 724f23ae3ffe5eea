"""The grid of k_pairs_gram (csrc/ba_internal.h, ba_plan_tail_grid) on the host: tests/trial_tail_plan_check.cpp, a stand-alone program built
with the host compiler and -fsanitize=address,undefined from the check, ba_structure.cpp and ba_problem.cpp, run as a program.  The pair
workgroups of ba_plan_schur come first with their count unchanged (a multiple of the band count: a block index keeps its band), the
Gram part has one workgroup per eight chunks of the camera-sorted view, and none when there is no such chunk."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_grid_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "bundleadjustment_benchmarks_amd", "csrc")
    exe = str(tmp_path / "trial_tail_plan_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "trial_tail_plan_check.cpp"), os.path.join(csrc, "ba_structure.cpp"),
                        os.path.join(csrc, "ba_problem.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "data")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "19 cases, 0 failures" in r.stdout

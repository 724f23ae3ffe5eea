"""The trailing-update schedule of the dense LDL^T (csrc/ba_ldlt_schedule.h) on the host: tests/ldlt_schedule_check.cpp, a
stand-alone program, built with the host compiler and -fsanitize=address,undefined and run as a program.  It replays the schedule of
every block-column count 2 ... 47 (row blocks = columns, and one more), budgets {0, 1, 50, 300, unbounded} and caps {1, 2, 3, 4}
launch by launch against the invariants the header lists: every (tile, panel) unit once, panels ascending, a panel only after its
launch, no tile twice per launch, every block column complete up to the last panel but one before its own launch, depth <= cap,
units per launch <= effective budget + forced work, and the unbounded budget = one depth-1 job per trailing tile and launch."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_invariants_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ldlt_schedule_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "bundleadjustment_benchmarks_amd", "csrc"), os.path.join(ROOT, "tests", "ldlt_schedule_check.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "1840 cases, 0 failures" in r.stdout

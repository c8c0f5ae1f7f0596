"""The host side of the Welch segment engine (csrc/welch_plan.hpp): tests/welch_plan_check.cpp, built with the host
compiler and no HIP.  The launch planner must tile every call exactly and in order, within rmax runs and without a run
across a record boundary, with the run and record counts a brute-force walk of welch_sub finds; welch_size must give the
(spr, sub, sb, rmax) recorded in tests/golden/welch_sizing.txt from the formulas the monitors and the analyser had of
their own; welch_tables must give, bit for bit, the windows, twiddles and sums of the three expressions it replaced."""
import os
import subprocess

from conftest import ROOT


def test_planner_sizing_and_tables(tmp_path):
    exe = str(tmp_path / "welch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-I" + os.path.join(ROOT, "airspy-fmradion_amd", "csrc"),
                    os.path.join(ROOT, "tests", "welch_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "welch_sizing.txt")], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["planner", "sizing", "tables"] and all(ln.endswith(" ok") for ln in lines)
    assert int(lines[1].split()[1]) == 57 * 4 + 57 * 8 and int(lines[2].split()[1]) == 7 * 3

"""The PLL down-sweep as a descent through the up-sweep's tree (csrc/pll_compose.hpp) on the host:
tests/pll_descend_host.cpp, built with the host compiler under the address and undefined-behaviour sanitizers, against the
sequential sweep and a long-double sweep for groups of 1, 2, 3, 5, 16, 17, 31 and 32 chunks."""
import os
import subprocess

from conftest import ROOT


def test_tree_descent_equals_sweep(tmp_path):
    exe = str(tmp_path / "pll_descend_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "airspy-fmradion_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pll_descend_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("n ")]
    assert [int(ln.split()[1]) for ln in lines] == [1, 2, 3, 5, 16, 17, 31, 32] and all(ln.endswith("ok") for ln in lines)

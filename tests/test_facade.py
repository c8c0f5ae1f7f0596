"""The C++ facade (reference class names and signatures) builds against the C-ABI."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")


def _build(tmp_path, name="facade_smoke"):
    fmr.build_library()
    exe = os.path.join(tmp_path, name)
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", name + ".cpp"),
                    "-L", libdir, "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = _build(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode == 10 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_facade_runs_on_gpu(tmp_path):
    exe = _build(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gpu path" in r.stdout


@pytest.mark.gpu
def test_enabled_stages_survive_a_chain_made_anew(tmp_path):
    """tests/facade_stages_smoke.cpp: FmDecoder and AmDecoder with every optional stage they offer, through
    attach_front_end() and enable_rds(): every stage is still on, with its configuration."""
    exe = _build(str(tmp_path), "facade_stages_smoke")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fm stages kept" in r.stdout and "am stages kept" in r.stdout, r.stdout


def test_remembered_stages_on_the_host(tmp_path):
    """tests/facade_stages_host.cpp: fmr_detail::Stages against stubs of the C functions, under the address and
    undefined-behaviour sanitizers: the order of apply(), the configurations, what a refusal leaves."""
    exe = str(tmp_path / "facade_stages_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "facade_stages_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "stages ok" in r.stdout, r.stdout + r.stderr

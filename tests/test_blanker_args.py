"""CPU-side checks of the impulse blanker's entry points (include/fmradion_amd.h, fmr_enable_blanker / fmr_blanker_read /
fmr_blanker_derive): the struct layouts of header and binding, every refusal that can be reached without a chain, by field
name and before the chain is looked at, the exports, and the host-only derive call on hand-made records."""
import ctypes as C
import importlib
import math
import subprocess

import numpy as np
import pytest

import blanker_fixture as bf
from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.BlankerConfig(struct_size=C.sizeof(fmr.BlankerConfig))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_blanker(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_blanker_config", "BlankerConfig", 40), ("fmr_blanker_info", "BlankerInfo", 72),
    ("fmr_blanker_levels", "BlankerLevels", 80)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_blanker_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.BLANKER_RECORD, bf.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 72


def test_constants_agree_with_the_fixture():
    assert (fmr.NB_MEASURE, fmr.NB_ACT) == (0, 1) and fmr.NB_Q == bf.Q == 4096


@pytest.mark.parametrize("field,value", [
    ("mode", 2), ("mode", -1), ("threshold_db", 5.9), ("threshold_db", 40.1), ("threshold_db", -12.0),
    ("threshold_db", math.nan), ("gate_samples", -1), ("gate_samples", 257), ("max_run_samples", -1),
    ("max_run_samples", 1025), ("average_intervals", -1), ("average_intervals", 65), ("record_intervals", -1),
    ("record_intervals", 4097), ("max_records", -1), ("max_records", 65537)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_blanker" in msg and field in msg, msg


def test_max_run_below_the_gate(L):
    rc, msg = _enable(L, _cfg(gate_samples=16, max_run_samples=15))
    assert rc == fmr.ERR_BAD_ARG and "max_run_samples" in msg and "16" in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.BlankerConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_blanker_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.BlankerConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_blanker(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_blanker_read(None, 0, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_blanker_derive(None, 1, 1e6, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_debug_read(None, 0, 6, None, 0) == fmr.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [
    {}, {"struct_size": 0}, {"mode": 1, "threshold_db": 6.0, "gate_samples": 1, "max_run_samples": 1, "average_intervals": 1,
                             "record_intervals": 1, "max_records": 1},
    {"threshold_db": 40.0, "gate_samples": 256, "max_run_samples": 1024, "average_intervals": 64, "record_intervals": 4096,
     "max_records": 65536}, {"gate_samples": 256}, {"max_run_samples": 3}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_blanker", "fmr_blanker_read", "fmr_blanker_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- fmr_blanker_derive ------------------------------------------------------------------------------------------
def _hand_made():
    r = np.zeros(3, dtype=fmr.BLANKER_RECORD)
    r["index"], r["first_interval"], r["n_intervals"] = [4, 5, 6], [1024, 1280, 1536], [256, 256, 128]
    r["n_triggers"], r["n_blanked"], r["n_nonfinite"], r["n_runs"] = [0, 20, 3], [0, 80, 10], [0, 1, 0], [0, 10, 2]
    r["power_q"] = [256 * (1 << 33), 256 * (1 << 34), 128 * (1 << 33)]       # mean |x|^2 of 1/8, 1/4, 1/8
    r["peak"], r["threshold"] = [0.5, 100.0, 0.75], [2.0, 2.5, 3.0]
    return r


def test_derive_on_hand_made_records():
    got = fmr.blanker_levels(_hand_made(), 2.5e6)
    n = 640 * 4096
    assert (got["n_intervals"], got["n_triggers"], got["n_blanked"], got["n_nonfinite"], got["n_runs"]) == (640, 23, 90, 1, 12)
    assert got["blanked_share"] == 90 / n and got["runs_per_second"] == 12 * 2.5e6 / n
    mean = (256 / 8 + 256 / 4 + 128 / 8) / 640
    assert abs(got["level_dbfs"] - 10 * math.log10(mean)) < 1e-12 and abs(got["peak_dbfs"] - 20.0) < 1e-12


def test_derive_of_silence_and_refusals(L):
    r = _hand_made()[:1]
    r["power_q"], r["peak"] = 0, 0.0
    got = fmr.blanker_levels(r, 10e6)
    assert got["level_dbfs"] == -math.inf and got["peak_dbfs"] == -math.inf and got["blanked_share"] == 0.0
    out = fmr.BlankerLevels()
    bad = _hand_made()
    bad["n_intervals"][1] = 0
    assert L.fmr_blanker_derive(bad.ctypes.data, 3, 1e6, C.byref(out), 0) == fmr.ERR_BAD_ARG
    assert "n_intervals" in L.fmr_last_error().decode()
    good = _hand_made()
    assert L.fmr_blanker_derive(good.ctypes.data, 0, 1e6, C.byref(out), 0) == fmr.ERR_BAD_ARG
    for rate in (0.0, -1.0, math.nan, math.inf):
        assert L.fmr_blanker_derive(good.ctypes.data, 3, rate, C.byref(out), 0) == fmr.ERR_BAD_ARG
        assert "input_rate" in L.fmr_last_error().decode()
    # a caller that knows a shorter struct gets that many bytes
    out.runs_per_second = 123.0
    assert L.fmr_blanker_derive(good.ctypes.data, 3, 1e6, C.byref(out), 16) == fmr.OK
    assert out.runs_per_second == 123.0 and out.struct_size == C.sizeof(fmr.BlankerLevels) and out.blanked_share == 90 / (640 * 4096)

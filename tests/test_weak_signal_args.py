"""CPU-side checks of the weak-signal stage's entry points (include/fmradion_amd.h, fmr_enable_weak_signal /
fmr_weak_signal_read / fmr_weak_signal_derive): the struct layouts of header and binding, every refusal that can be reached
without a chain, by name and before the chain is looked at, and the host-only derive call on hand-made records."""
import ctypes as C
import importlib
import math
import subprocess

import numpy as np
import pytest

import weak_signal_fixture as wf
from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.WeakSignalConfig(struct_size=C.sizeof(fmr.WeakSignalConfig))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_weak_signal(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_weak_signal_config", "WeakSignalConfig", 104), ("fmr_weak_signal_info", "WeakSignalInfo", 64),
    ("fmr_weak_signal_levels", "WeakSignalLevels", 104)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_weak_signal_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.WEAK_SIGNAL_RECORD, wf.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 96


def test_constants_agree_with_the_fixture():
    assert (fmr.WS_MEASURE, fmr.WS_ACT) == (0, 1)
    assert (fmr.WS_BLEND, fmr.WS_HIGHCUT, fmr.WS_MUTE) == (wf.BLEND, wf.HIGHCUT, wf.MUTE) == (1, 2, 4)


@pytest.mark.parametrize("field,value", [
    ("mode", 2), ("mode", -1), ("actions", 8), ("actions", 0x17),
    ("record_intervals", -1), ("record_intervals", 1001), ("max_records", -1), ("max_records", 65537),
    ("attack_ms", -1.0), ("attack_ms", math.nan), ("attack_ms", 60001.0), ("release_ms", -0.5), ("release_ms", math.inf),
    ("highcut_hz", 499.0), ("highcut_hz", 15001.0), ("highcut_hz", math.nan),
    ("mute_floor_db", 1.0), ("mute_floor_db", -math.inf), ("mute_floor_db", math.nan)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_weak_signal" in msg and field in msg, msg


@pytest.mark.parametrize("action", ["blend", "highcut", "mute"])
@pytest.mark.parametrize("lo,hi", [(-20.0, -30.0), (-20.0, -20.0), (math.nan, -20.0), (-30.0, math.inf), (0.0, -5.0)])
def test_threshold_pairs_need_lo_below_hi(L, action, lo, hi):
    rc, msg = _enable(L, _cfg(**{action + "_lo_db": lo, action + "_hi_db": hi}))
    assert rc == fmr.ERR_BAD_ARG and action + "_lo_db" in msg and action + "_hi_db" in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.WeakSignalConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_weak_signal_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.WeakSignalConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_weak_signal(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_weak_signal_read(None, 0, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_weak_signal_derive(None, 1, None, 0) == fmr.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [
    {}, {"struct_size": 0}, {"mode": 1, "actions": 5, "record_intervals": 1, "max_records": 1},
    {"record_intervals": 1000, "max_records": 65536, "attack_ms": 60000.0, "release_ms": 0.01},
    {"blend_lo_db": -50.0, "blend_hi_db": -49.5, "highcut_hz": 500.0, "mute_floor_db": -120.0},
    {"highcut_hz": 15000.0, "mute_lo_db": -3.0, "mute_hi_db": 3.0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_weak_signal", "fmr_weak_signal_read", "fmr_weak_signal_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- fmr_weak_signal_derive ------------------------------------------------------------------------------------------
def _hand_made():
    r = np.zeros(3, dtype=fmr.WEAK_SIGNAL_RECORD)
    r["index"], r["first_interval"], r["n_intervals"] = [4, 5, 6], [200, 250, 300], [50, 50, 25]
    r["n_nonfinite"] = [0, 3, 1]
    r["usn_sum"], r["usn_peak"] = [50 * 1e-6, 50 * 1e-3, 25 * 1e-4], [2e-6, 4e-3, 2e-4]
    r["smoothed"] = [1e-6, 1e-3, 5e-4]
    r["t_blend"], r["t_highcut"], r["t_mute"] = [0, 1, 0.75], [0, 0.5, 0.25], [0, 0, 0]
    r["max_blend"], r["max_highcut"], r["max_mute"] = [0, 1, 1], [0, 0.5, 0.5], [0, 0, 0]
    return r


def test_derive_on_hand_made_records():
    r = _hand_made()
    got, want = fmr.weak_signal_levels(r), wf.derive(r)
    assert got["n_intervals"] == 125 and got["n_nonfinite"] == 4
    mean = (50e-6 + 50e-3 + 25e-4) / 125
    assert abs(got["usn_mean_db"] - 10 * math.log10(mean)) < 1e-9 and abs(got["usn_peak_db"] - 10 * math.log10(4e-3)) < 1e-9
    assert abs(got["usn_mean_hz"] - 75000.0 * math.sqrt(mean)) < 1e-6 and abs(got["usn_peak_hz"] - 75000.0 * math.sqrt(4e-3)) < 1e-6
    assert got["blend_share"] == 75 / 125 and got["highcut_share"] == 75 / 125 and got["mute_share"] == 0.0
    assert (got["t_blend"], got["t_highcut"], got["t_mute"]) == (0.75, 0.25, 0.0)
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-9 * max(1.0, abs(v)), (k, got[k], v)


def test_derive_of_silence_and_refusals(L):
    r = _hand_made()[:1]
    r["usn_sum"], r["usn_peak"] = 0.0, 0.0
    got = fmr.weak_signal_levels(r)
    assert got["usn_mean_db"] == -math.inf and got["usn_peak_db"] == -math.inf and got["usn_mean_hz"] == 0.0
    out = fmr.WeakSignalLevels()
    bad = _hand_made()
    bad["n_intervals"][1] = 0
    assert L.fmr_weak_signal_derive(bad.ctypes.data, 3, C.byref(out), 0) == fmr.ERR_BAD_ARG
    assert "n_intervals" in L.fmr_last_error().decode()
    assert L.fmr_weak_signal_derive(bad.ctypes.data, 0, C.byref(out), 0) == fmr.ERR_BAD_ARG
    # a caller that knows a shorter struct gets that many bytes
    out.usn_peak_db = 123.0
    good = _hand_made()
    assert L.fmr_weak_signal_derive(good.ctypes.data, 3, C.byref(out), 16) == fmr.OK
    assert out.usn_peak_db == 123.0 and out.struct_size == C.sizeof(fmr.WeakSignalLevels)

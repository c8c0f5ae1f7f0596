"""CPU-side checks of the modulation monitor's entry points (include/fmradion_amd.h, fmr_enable_monitor /
fmr_monitor_read / fmr_monitor_derive): the struct layouts of header and binding, every configuration refusal by name
before the chain is looked at, and the host-only derive call against tests/monitor_fixture.py."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

import monitor_fixture as mf
from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.MonitorConfig(C.sizeof(fmr.MonitorConfig), 0, 0, 0.0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_monitor(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_monitor_config", "MonitorConfig", 32), ("fmr_monitor_info", "MonitorInfo", 72),
    ("fmr_monitor_levels", "MonitorLevels", 80)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_monitor_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.MONITOR_RECORD, mf.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 56


@pytest.mark.parametrize("field,value", [
    ("interval_samples", 511), ("interval_samples", 513), ("interval_samples", 256), ("interval_samples", (1 << 30) + 512),
    ("interval_samples", 384001), ("hist_bins", 1), ("hist_bins", -4), ("hist_bins", 1025), ("hist_range", -1.0),
    ("hist_range", float("nan")), ("hist_range", float("inf")), ("max_records", -1), ("max_records", 4097)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_monitor" in msg and field in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.MonitorConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_monitor_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.MonitorConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_monitor(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_monitor_read(None, 0, None, None, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_monitor_derive(None, None, 1, None, 0) == fmr.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [{}, {"interval_samples": 512, "hist_bins": 2, "hist_range": 1e-3, "max_records": 1},
                                {"interval_samples": 1 << 30, "hist_bins": 1024, "hist_range": 100.0, "max_records": 4096},
                                {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_monitor", "fmr_monitor_read", "fmr_monitor_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- fmr_monitor_derive against the fixture's derive ----------------------------------------------------------------
def _station(n):
    t = np.arange(n, dtype=np.float64) / mf.F
    rng = np.random.default_rng(5)
    return (0.02 + 0.5 * np.sin(2 * np.pi * 1000.0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) +
            0.09 * np.sin(2 * np.pi * 19000.0 * t) + (2.0 / 75.0) * np.cos(2 * np.pi * 57000.0 * t) +
            1e-3 * rng.standard_normal(n)).astype(np.float32)


def _same(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, int) or not np.isfinite(w):
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= 1e-9 * max(abs(w), 1e-300), (k, g, w)


@pytest.fixture(scope="module")
def three_records():
    x = _station(3 * 38400 + mf.H)
    x[50000] = np.nan                        # record 1 loses a sample and two segments: the pooling weights differ
    return mf.records(x, M=38400, B=64, R=1.0)


def test_derive_one_record(L, three_records):
    recs, _, psd = three_records
    for i in range(3):
        _same(fmr.monitor_levels(recs[i:i + 1], psd[i:i + 1]), mf.derive(recs[i:i + 1], psd[i:i + 1]))


def test_derive_pools_three_records(L, three_records):
    recs, _, psd = three_records
    assert len({int(s) for s in recs["segments"]}) == 2
    got, want = fmr.monitor_levels(recs, psd), mf.derive(recs, psd)
    _same(got, want)
    assert got["n_finite"] == 3 * 38400 - 1 and abs(got["pilot_deviation_hz"] - 6750.0) < 0.01 * 6750.0
    # (the 997 / 1003 Hz products of the modulated tone do not complete a cycle in 0.3 s: up to 0.125 x 2 / (2 pi 997 x 0.3)
    # of mean, 10 Hz)
    assert abs(got["rds_deviation_hz"] - 2000.0) < 0.01 * 2000.0 and abs(got["tuning_offset_hz"] - 1500.0) < 12.0


def test_derive_without_variance(L):
    """A constant MPX (var <= 0 after rounding, or exactly 0) and an empty record: -inf dBr, rms 0."""
    x = np.full(2 * 4096 + mf.H, 0.25, dtype=np.float32)
    recs, _, psd = mf.records(x, M=4096, B=64, R=1.0)
    got, want = fmr.monitor_levels(recs, psd), mf.derive(recs, psd)
    _same(got, want)
    assert got["mpx_power_dbr"] == -np.inf and got["rms"] == 0.0 and got["peak_deviation_hz"] == 0.0
    assert abs(got["tuning_offset_hz"] - 18750.0) < 1e-6
    x[:] = np.nan
    recs, _, psd = mf.records(x, M=4096, B=64, R=1.0)
    got = fmr.monitor_levels(recs, psd)
    _same(got, mf.derive(recs, psd))
    assert got["n_finite"] == 0 and got["segments"] == 0 and got["mpx_power_dbr"] == -np.inf

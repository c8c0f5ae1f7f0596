"""CPU-side checks of the RF monitor's entry points (include/fmradion_amd.h, fmr_enable_rf_monitor /
fmr_rf_monitor_read / fmr_rf_monitor_derive): the struct layouts of header and binding, every configuration refusal by
name before the chain is looked at, and the host-only derive call against tests/rfmon_fixture.py."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import rfmon_fixture as rx
from cheader import header_struct as _header_struct
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.RfMonitorConfig(C.sizeof(fmr.RfMonitorConfig), 0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_rf_monitor(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_rf_monitor_config", "RfMonitorConfig", 12), ("fmr_rf_monitor_info", "RfMonitorInfo", 64),
    ("fmr_rf_monitor_levels", "RfMonitorLevels", 112)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_rf_monitor_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.RF_MONITOR_RECORD, rx.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 56
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    assert f"#define FMR_RF_HIST_BINS {fmr.RF_HIST_BINS}\n" in hdr and f"#define FMR_RF_PSD_BINS {fmr.RF_PSD_BINS}\n" in hdr
    assert (fmr.RF_HIST_BINS, fmr.RF_PSD_BINS) == (rx.HIST_BINS, rx.PSD_BINS)


@pytest.mark.parametrize("field,value", [
    ("interval_samples", 511), ("interval_samples", 513), ("interval_samples", 256), ("interval_samples", (1 << 30) + 512),
    ("interval_samples", 38401), ("max_records", -1), ("max_records", 4097)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_rf_monitor" in msg and field in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.RfMonitorConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_rf_monitor_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.RfMonitorConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_rf_monitor(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_rf_monitor_read(None, 0, None, None, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_rf_monitor_derive(None, None, None, 1, None, 0) == fmr.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [{}, {"interval_samples": 512, "max_records": 1},
                                {"interval_samples": 1 << 30, "max_records": 4096}, {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_rf_monitor", "fmr_rf_monitor_read", "fmr_rf_monitor_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- fmr_rf_monitor_derive against the fixture's derive -------------------------------------------------------------
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
    """A fading carrier with 5 % AM at 19 kHz in noise; record 1 loses a sample and two segments."""
    n = 3 * 38400 + rx.H
    x = rx.fm_iq(n, amplitude=0.3, am=0.05, f_am=19000.0, noise=0.09e-3, seed=4).astype(np.complex128)
    x *= 1.0 - 0.8 * np.exp(-0.5 * ((np.arange(n) - 60000.0) / 4000.0) ** 2)
    p = rx.power(x)
    p[50000] = np.nan
    return rx.records(p)


def test_derive_one_record(L, three_records):
    recs, hist, psd = three_records
    for i in range(3):
        _same(fmr.rf_levels(recs[i:i + 1], hist[i:i + 1], psd[i:i + 1]), rx.derive(recs[i:i + 1], hist[i:i + 1], psd[i:i + 1]))


def test_derive_pools_three_records(L, three_records):
    recs, hist, psd = three_records
    assert len({int(s) for s in recs["segments"]}) == 2
    got, want = fmr.rf_levels(recs, hist, psd), rx.derive(recs, hist, psd)
    _same(got, want)
    print(got)
    assert got["n_finite"] == 3 * 38400 - 1 and got["segments"] == 3 * 75 - 2
    assert got["p10_dbfs"] < got["p50_dbfs"] <= got["p90_dbfs"] and got["p10_dbfs"] < got["p50_dbfs"] - 2.0     # (the fade)
    # 5 % AM at 19 kHz: (2 m)^2 / 2 / 4 = m^2 / 2 relative to the carrier, -29 dB, a little less with the fade's weight
    assert abs(got["am_pilot_db"] - 10.0 * np.log10(0.05 ** 2 / 2.0)) < 1.5 and got["am_audio_db"] < got["am_pilot_db"]


def test_derive_infinities(L):
    """A pure carrier (S > 0 and Nn <= 0, or d rounding either way): the +-INFINITY cases as the fixture has them; all
    samples zero; all samples non-finite; no histogram and no PSD."""
    Mr = 4096
    p = np.full(2 * Mr + rx.H, 0.25, dtype=np.float32)
    recs, hist, psd = rx.records(p, M=Mr)
    got = fmr.rf_levels(recs, hist, psd)
    _same(got, rx.derive(recs, hist, psd))
    assert got["cn_db"] == np.inf and got["noise_dbfs"] == -np.inf and got["am_rms"] == 0.0
    assert abs(got["level_dbfs"] - 10.0 * np.log10(0.25)) < 1e-12 and abs(got["carrier_dbfs"] - got["level_dbfs"]) < 1e-12
    assert got["p10_dbfs"] == got["p90_dbfs"] == 10.0 * np.log10(0.25)
    p[:] = 0.0
    recs, hist, psd = rx.records(p, M=Mr)
    got = fmr.rf_levels(recs, hist, psd)
    _same(got, rx.derive(recs, hist, psd))
    assert got["level_dbfs"] == -np.inf and got["cn_db"] == -np.inf and got["am_audio_db"] == -np.inf
    assert got["p50_dbfs"] == 10.0 * np.log10(2.0 ** -40)
    p[:] = np.nan
    recs, hist, psd = rx.records(p, M=Mr)
    got = fmr.rf_levels(recs, hist, psd)
    _same(got, rx.derive(recs, hist, psd))
    assert got["n_finite"] == 0 and got["segments"] == 0 and got["p50_dbfs"] == -np.inf
    # either array may be NULL
    recs, hist, psd = rx.records(np.full(Mr + rx.H, 0.09, dtype=np.float32), M=Mr)
    out = fmr.RfMonitorLevels()
    assert L.fmr_rf_monitor_derive(recs.ctypes.data, None, None, 1, C.byref(out), C.sizeof(out)) == fmr.OK
    assert out.p50_dbfs == -np.inf and out.am_audio_db == -np.inf and abs(out.level_dbfs - 10 * np.log10(np.float32(0.09))) < 1e-9

"""CPU-side checks of the audio monitor's entry points (include/fmradion_amd.h, fmr_enable_loudness / fmr_loudness_read /
fmr_loudness_derive): the struct layouts of header and binding, every configuration refusal by name before the chain is
looked at, and the host-only derive call against tests/loudness_fixture.py."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

import loudness_fixture as lf
from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.LoudnessConfig(C.sizeof(fmr.LoudnessConfig), 0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_loudness(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_loudness_config", "LoudnessConfig", 12), ("fmr_loudness_info", "LoudnessInfo", 48),
    ("fmr_loudness_levels", "LoudnessLevels", 120)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_loudness_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.LOUDNESS_RECORD, lf.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 104


@pytest.mark.parametrize("field,value", [
    ("step_samples", 32), ("step_samples", 47), ("step_samples", 50), ("step_samples", 4801), ("step_samples", (1 << 20) + 16),
    ("max_records", -1), ("max_records", 65537)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_loudness" in msg and field in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.LoudnessConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_loudness_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.LoudnessConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_loudness(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_loudness_read(None, 0, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_loudness_derive(None, 1, -60.0, None, 0) == fmr.ERR_BAD_ARG
    recs = np.zeros(2, dtype=fmr.LOUDNESS_RECORD)
    out = fmr.LoudnessLevels()
    assert L.fmr_loudness_derive(recs.ctypes.data, 0, -60.0, C.byref(out), 0) == fmr.ERR_BAD_ARG
    assert L.fmr_loudness_derive(recs.ctypes.data, 2, -60.0, C.byref(out), 0) == fmr.ERR_BAD_ARG      # step_samples 0
    assert "step_samples" in L.fmr_last_error().decode()
    recs["step_samples"], recs["channels"] = 480, 2
    assert L.fmr_loudness_derive(recs.ctypes.data, 2, float("nan"), C.byref(out), 0) == fmr.ERR_BAD_ARG
    assert L.fmr_loudness_derive(recs.ctypes.data, 2, -60.0, C.byref(out), 0) == fmr.OK


@pytest.mark.parametrize("kw", [{}, {"step_samples": 48, "max_records": 1}, {"step_samples": 1 << 20, "max_records": 65536},
                                {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_loudness", "fmr_loudness_read", "fmr_loudness_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- fmr_loudness_derive against the fixture's derive ----------------------------------------------------------------
def _same(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, int) or not np.isfinite(w):
            assert g == w, (k, g, w)
        elif k.endswith(("_lufs", "_db", "_dbfs", "_dbtp")):
            assert abs(g - w) <= 1e-9, (k, g, w)
        else:
            assert abs(g - w) <= 1e-9 * max(abs(w), 1e-300), (k, g, w)


@pytest.fixture(scope="module")
def programme():
    """Forty sub-blocks of 480: two tones of unlike level with noise, a fade, four silent sub-blocks, a quiet tail."""
    Q, n = 480, 40 * 480
    t = np.arange(n) / 48000.0
    rng = np.random.default_rng(11)
    left = 0.4 * np.sin(2 * np.pi * 1000.0 * t) + 1e-3 * rng.standard_normal(n)
    right = 0.25 * np.sin(2 * np.pi * 400.0 * t + 0.4) + 1e-3 * rng.standard_normal(n)
    env = np.ones(n)
    env[10 * Q:14 * Q] = np.linspace(1.0, 1e-3, 4 * Q)
    env[14 * Q:18 * Q] = 0.0
    env[34 * Q:] = 1e-4
    a = np.stack([left * env, right * env], axis=1).reshape(-1)
    a[2 * 777] = np.nan
    return lf.records(a, 2, Q)


def test_derive_against_the_fixture(L, programme):
    got, want = fmr.loudness_levels(programme), lf.derive(programme)
    print(got)
    _same(got, want)
    assert got["momentary_windows"] == 37 and got["longest_silence_blocks"] == 6 and got["trailing_silence_blocks"] == 6
    assert got["n_nonfinite"] == 1 and np.isfinite(got["integrated_lufs"]) and np.isfinite(got["short_term_lufs"])
    assert 0 < got["gated_windows"] < 37


def test_derive_over_a_gap_a_short_run_and_one_record(L, programme):
    cut = np.concatenate([programme[:16], programme[17:]])
    _same(fmr.loudness_levels(cut), lf.derive(cut))
    assert fmr.loudness_levels(cut)["momentary_windows"] == 13 + 20
    assert fmr.loudness_levels(programme[:34])["longest_silence_blocks"] == 4
    assert fmr.loudness_levels(cut[:33])["longest_silence_blocks"] == 2 and fmr.loudness_levels(cut[:33])["trailing_silence_blocks"] == 0
    for recs in (programme[:3], programme[5:6], programme[14:18]):
        got = fmr.loudness_levels(recs, silence_dbfs=-50.0)
        _same(got, lf.derive(recs, silence_dbfs=-50.0))
        assert got["integrated_lufs"] == -np.inf
    assert fmr.loudness_levels(programme[14:18])["sample_peak_dbfs"] == -np.inf


def test_derive_of_mono_and_antiphase_records(L):
    n = 8 * 480
    x = 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / 48000.0)
    mono = lf.records(x, 1, 480)
    _same(fmr.loudness_levels(mono), lf.derive(mono))
    assert fmr.loudness_levels(mono)["correlation"] == 0.0
    anti = lf.records(np.stack([x, -x], axis=1).reshape(-1), 2, 480)
    got = fmr.loudness_levels(anti)
    _same(got, lf.derive(anti))
    assert got["side_to_mid_db"] == np.inf and got["correlation"] == pytest.approx(-1.0, abs=1e-12)

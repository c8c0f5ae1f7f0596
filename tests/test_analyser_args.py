"""CPU-side checks of the audio analyser's entry points (include/fmradion_amd.h, fmr_enable_analyser / fmr_analyser_read /
fmr_analyser_derive): the struct layouts of header and binding, every refusal that can be reached without a chain, by
name and before the chain is looked at, and the host-only derive call against tests/analyser_fixture.py to 1e-9."""
import ctypes as C
import importlib
import math
import subprocess

import numpy as np
import pytest

import analyser_fixture as af
from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.AnalyserConfig(C.sizeof(fmr.AnalyserConfig), 0, 0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_analyser(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_analyser_config", "AnalyserConfig", 16), ("fmr_analyser_info", "AnalyserInfo", 64),
    ("fmr_analyser_rule", "AnalyserRule", 56), ("fmr_analyser_levels", "AnalyserLevels", 176)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_analyser_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.ANALYSER_RECORD, af.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 72


@pytest.mark.parametrize("field,value", [
    ("fft_size", 512), ("fft_size", 1000), ("fft_size", 16384), ("fft_size", -4096),
    ("interval_samples", 1024), ("interval_samples", 2048 + 1024), ("interval_samples", (1 << 24) + 2048),
    ("max_records", -1), ("max_records", 4097)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_analyser" in msg and field in msg, msg


def test_interval_is_checked_against_the_fft_size_given(L):
    rc, msg = _enable(L, _cfg(fft_size=1024, interval_samples=512))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, msg
    rc, msg = _enable(L, _cfg(fft_size=8192, interval_samples=2048))
    assert rc == fmr.ERR_BAD_ARG and "interval_samples" in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.AnalyserConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_analyser_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.AnalyserConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_analyser(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_analyser_read(None, 0, None, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_analyser_derive(None, None, 1, None, 0, None, 0) == fmr.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [{}, {"fft_size": 1024, "interval_samples": 512, "max_records": 1},
                                {"fft_size": 8192, "interval_samples": 1 << 24, "max_records": 4096}, {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_analyser", "fmr_analyser_read", "fmr_analyser_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out
    assert b"0.4" in L.fmr_version()


# ---- fmr_analyser_derive: refusals ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tone():
    """8 N frames at N = 1024 in records of N: a 1 kHz sine with harmonics at -40 and -50 dBc and a little noise"""
    N = 1024
    t = np.arange(8 * N) / 48000.0
    rng = np.random.default_rng(3)
    x = 0.0866 * (np.sin(2 * np.pi * 1000.0 * t + 0.3) + 1e-2 * np.sin(2 * np.pi * 2000.0 * t + 0.2)
                  + 10.0 ** -2.5 * np.sin(2 * np.pi * 3000.0 * t + 0.3)) + 1e-5 * rng.standard_normal(8 * N)
    return x


def _derive(L, recs, sp, n=None, rule=None, rule_size=None):
    out = fmr.AnalyserLevels()
    rc = L.fmr_analyser_derive(recs.ctypes.data, sp.ctypes.data, len(recs) if n is None else n,
                               None if rule is None else C.byref(rule),
                               (C.sizeof(fmr.AnalyserRule) if rule_size is None else rule_size) if rule is not None else 0,
                               C.byref(out), 0)
    return rc, L.fmr_last_error().decode(), out


def _rule(**kw):
    r = fmr.AnalyserRule(struct_size=C.sizeof(fmr.AnalyserRule))
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_derive_refusals(L, tone):
    recs, sp = af.records(tone, 1, 1024, 1024)
    rc, msg, _ = _derive(L, recs, sp, n=0)
    assert rc == fmr.ERR_BAD_ARG and "n < 1" in msg
    rc, msg, out = _derive(L, recs, sp)                       # rule NULL: all defaults
    assert rc == fmr.OK and out.tone_found == 1
    for view in (1, 2, 3, 4, -1):
        rc, msg, _ = _derive(L, recs, sp, rule=_rule(view=view))
        assert rc == fmr.ERR_BAD_ARG and "view" in msg, (view, msg)
    for kw, word in (({"band_lo_hz": 16000.0}, "band_lo_hz"), ({"band_hi_hz": 24001.0}, "band_hi_hz"),
                     ({"band_lo_hz": -1.0}, "band_lo_hz"), ({"band_lo_hz": 1000.0, "band_hi_hz": 1300.0}, "bins"),
                     ({"band_lo_hz": math.nan}, "band_lo_hz"),
                     ({"tone_hz": -5.0}, "tone_hz"), ({"tone_hz": 30000.0}, "tone_hz"), ({"tone_hz": math.nan}, "tone_hz"),
                     ({"tone_search_hz": -1.0}, "tone_search_hz"), ({"tone_search_hz": math.inf}, "tone_search_hz"),
                     ({"max_harmonic": 1}, "max_harmonic"), ({"max_harmonic": 65}, "max_harmonic"),
                     ({"reserved": 1}, "reserved"), ({"min_tone_dbfs": math.nan}, "min_tone_dbfs")):
        rc, msg, _ = _derive(L, recs, sp, rule=_rule(**kw))
        assert rc == fmr.ERR_BAD_ARG and "fmr_analyser_derive" in msg and word in msg, (kw, rc, msg)
    rc, msg, _ = _derive(L, recs, sp, rule=_rule(), rule_size=C.sizeof(fmr.AnalyserRule) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_analyser_rule" in msg
    # unlike records
    r2, s2 = af.records(tone, 1, 2048, 2048)
    mixed = np.concatenate([recs[:1], r2[:1]])
    rc, msg, _ = _derive(L, mixed, np.zeros((2, 3, 1025)))
    assert rc == fmr.ERR_BAD_ARG and "fft_size" in msg
    two = recs[:2].copy()
    two["channels"][1] = 2
    rc, msg, _ = _derive(L, two, sp[:2].copy())
    assert rc == fmr.ERR_BAD_ARG and "channels" in msg
    bad = recs[:1].copy()
    bad["fft_size"] = 1000
    rc, msg, _ = _derive(L, bad, sp[:1].copy())
    assert rc == fmr.ERR_BAD_ARG and "fft_size" in msg


# ---- fmr_analyser_derive against the fixture's derive ---------------------------------------------------------------
def _same(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        g = got[k]
        if k == "harmonic_dbc":
            for a, b in zip(g, w):
                assert (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= 1e-9, (k, g, w)
        elif isinstance(w, int):
            assert g == w, (k, g, w)
        elif math.isnan(w):
            assert math.isnan(g), (k, g, w)
        elif not math.isfinite(w):
            assert g == w, (k, g, w)
        elif k.endswith(("_db", "_dbfs", "_hz")):
            assert abs(g - w) <= 1e-9, (k, g, w)
        else:
            assert abs(g - w) <= 1e-9 * max(abs(w), 1e-300), (k, g, w)


def _sine(N, f, amp=0.0866, harmonics=()):
    t = np.arange(8 * N) / 48000.0
    x = amp * np.sin(2 * np.pi * f * t + 0.3)
    for h, dbc in harmonics:
        x = x + amp * 10.0 ** (dbc / 20.0) * np.sin(2 * np.pi * h * f * t + 0.1 * h)
    return x


@pytest.mark.parametrize("N", [1024, 4096, 8192])
@pytest.mark.parametrize("f", [880.0, 997.0, 1000.0, "off"])
def test_derive_against_the_fixture_on_sines(L, N, f):
    f = (round(1500.0 * N / 48000.0) + 0.37) * 48000.0 / N if f == "off" else f
    rng = np.random.default_rng(7)
    for x in (_sine(N, f), _sine(N, f, harmonics=((2, -40.0), (3, -50.0))), _sine(N, f) + 1e-4 * rng.standard_normal(8 * N)):
        recs, sp = af.records(x, 1, N)
        got, want = fmr.analyser_levels(recs, sp), af.derive(recs, sp)
        _same(got, want)
        assert got["tone_found"] == 1 and abs(got["tone_hz"] - f) < 0.05


def test_derive_views_no_tone_skips_gaps_and_hints(L, tone):
    N = 1024
    x = _sine(N, 1000.0)
    y = _sine(N, 3000.0, amp=0.02)
    for pair in ((x, -x), (x, x), (x, y)):
        recs, sp = af.records(np.stack(pair, axis=1).reshape(-1), 2, N, 2048)
        for view in ("L", "R", "M", "S"):
            _same(fmr.analyser_levels(recs, sp, view=view), af.derive(recs, sp, view=view))
    recs, sp = af.records(np.stack((x, -x), axis=1).reshape(-1), 2, N)
    assert fmr.analyser_levels(recs, sp, view="M")["tone_found"] == 0
    assert abs(fmr.analyser_levels(recs, sp, view="S")["tone_dbfs"] - 20.0 * math.log10(0.0866)) < 1e-4
    # no tone, silence, a tone too low in frequency
    rng = np.random.default_rng(8)
    for sig in (1e-5 * rng.standard_normal(8 * N), np.zeros(8 * N), _sine(N, 200.0)):
        recs, sp = af.records(sig, 1, N)
        got = fmr.analyser_levels(recs, sp)
        _same(got, af.derive(recs, sp))
        assert got["tone_found"] == 0 and math.isnan(got["thd"])
    # skipped segments, non-finite samples, records with gaps
    z = tone.copy()
    z[700] = np.nan
    z[5 * 1024 + 100] = np.inf
    recs, sp = af.records(z, 1, N, 1024)
    pick = np.array([0, 1, 2, 5, 6])
    got = fmr.analyser_levels(recs[pick], sp[pick])
    _same(got, af.derive(recs[pick], sp[pick]))
    assert got["skipped"] == 3 and got["n_nonfinite"] == 2 and got["segments"] == 7      # (records 0 and 5 hold the two)
    _same(fmr.analyser_levels(recs[:1], sp[:1]), af.derive(recs[:1], sp[:1]))
    # a hint beside a stronger spur, another band, fewer harmonics, a floor above the tone
    recs, sp = af.records(_sine(4096, 880.0) + _sine(4096, 5000.0, amp=0.3), 1, 4096)
    for kw in ({"tone_hz": 880.0}, {"tone_hz": 900.0, "tone_search_hz": 30.0}, {"band_lo_hz": 300.0, "band_hi_hz": 4000.0},
               {"max_harmonic": 3}, {"min_tone_dbfs": -5.0}, {"tone_hz": 880.0, "min_tone_dbfs": -21.0}):
        _same(fmr.analyser_levels(recs, sp, **kw), af.derive(recs, sp, **kw))
    assert abs(fmr.analyser_levels(recs, sp, tone_hz=880.0)["tone_hz"] - 880.0) < 1e-3
    assert fmr.analyser_levels(recs, sp, min_tone_dbfs=-5.0)["tone_found"] == 0

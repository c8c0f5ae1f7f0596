"""CPU-side checks of the band spectrum and the station finder (include/fmradion_amd.h, fmr_spectrum_* /
fmr_find_stations): every refusal of fmr_spectrum_create by name before a device is touched, FMR_ERR_NO_DEVICE for a
valid configuration without one, and the finder against its numpy restatement (tests/spectrum_fixture.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import spectrum_fixture as sf

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.SpectrumConfig()
    c.struct_size, c.device, c.n_rows, c.input_rate, c.input_format = C.sizeof(c), 0, 1, 10e6, fmr.IQ_CF32
    c.fft_size, c.hop, c.window, c.max_call_len = 8192, 0, fmr.WINDOW_HANN, 1 << 16
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _create(L, cfg, size=None):
    h = C.c_void_p()
    rc = L.fmr_spectrum_create(C.byref(cfg), C.sizeof(cfg) if size is None else size, C.byref(h))
    if rc == 0:
        L.fmr_spectrum_destroy(h)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("field,value", [
    ("fft_size", 1000), ("fft_size", 128), ("fft_size", 32768), ("fft_size", 0), ("hop", -1), ("hop", 8193),
    ("window", 3), ("window", -1), ("input_format", 4), ("input_format", -1), ("input_rate", 0.0), ("input_rate", -1e6),
    ("n_rows", 0), ("n_rows", 65536), ("max_call_len", 0), ("max_call_len", (1 << 30) + 1),
])
def test_create_refusals_name_the_field(L, field, value):
    rc, msg = _create(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert field in msg, msg


def test_create_refuses_a_larger_struct(L):
    rc, msg = _create(L, _cfg(), C.sizeof(fmr.SpectrumConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    rc, msg = _create(L, _cfg(struct_size=C.sizeof(fmr.SpectrumConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg


def test_valid_config_without_device(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for kw in ({}, {"fft_size": 256, "hop": 256, "window": fmr.WINDOW_RECT}, {"fft_size": 16384, "hop": 1, "n_rows": 3,
                                                                               "input_format": fmr.IQ_U8}):
        rc, msg = _create(L, _cfg(**kw))
        assert rc == fmr.ERR_NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)


def test_struct_layout():
    assert C.sizeof(fmr.SpectrumConfig) == 48
    assert C.sizeof(fmr.SpectrumInfo) == 48
    assert C.sizeof(fmr.StationRule) == 32
    assert C.sizeof(fmr.Station) == 32


# ---- station finder ---------------------------------------------------------------------------------------------------
F = 10e6


def _check(psd, **rule):
    got = fmr.find_stations(psd, F, **rule)
    ref = sf.find_stations(psd, F, **rule)
    assert [g["offset_hz"] for g in got] == [r[0] for r in ref], ([g["offset_hz"] for g in got], [r[0] for r in ref])
    for g, r in zip(got, ref):
        assert abs(g["level_db"] - r[1]) <= 1e-9 and abs(g["snr_db"] - r[2]) <= 1e-9, (g, r)
        assert abs(g["centroid_hz"] - r[3]) <= 1e-6 * max(1.0, abs(r[3])), (g, r)
    return got


def _bumps(N, centres, levels, width_hz=150e3, seed=0):
    rng = np.random.default_rng(seed)
    fk = (np.arange(N) - N // 2) * F / N
    p = 1e-9 * (1 + 0.2 * rng.random(N))
    for c, l in zip(centres, levels):
        p = p + np.where(np.abs(fk - c) <= width_hz / 2, l * (1 - (2 * (fk - c) / width_hz) ** 2), 0.0)
    return p


def test_finder_matches_restatement_random_scenes():
    for seed in range(6):
        rng = np.random.default_rng(seed)
        cents = rng.choice(np.arange(-45, 46) * 100000, size=7, replace=False)
        lev = 10 ** rng.uniform(-8, -4, size=7)
        psd = _bumps(8192, cents, lev, seed=seed)
        got = _check(psd, raster_hz=100000, threshold_db=10.0)
        assert len(got) >= 3


def test_finder_raster_offset():
    cents = [-2150000, -50000, 1250000, 3950000]
    psd = _bumps(8192, cents, [1e-5, 1e-6, 3e-6, 1e-5])
    got = _check(psd, raster_hz=100000, raster_offset_hz=50000, threshold_db=10.0)
    assert [g["offset_hz"] for g in got] == cents


def test_finder_ties_and_plateau():
    N = 8192
    psd = np.full(N, 1e-9)
    fk = (np.arange(N) - N // 2) * F / N
    psd[np.abs(fk - 1e6) <= 400e3] = 1e-6          # a plateau several candidates wide: equal band powers inside
    got = _check(psd, raster_hz=100000, bandwidth_hz=200000, threshold_db=6.0)
    assert got, "the plateau must yield a station"
    # an exact tie between two neighbours: the lower frequency wins.  Two candidates whose bands hold the same number of
    # bins, one spike between them (inside both bands), floor and spike powers of two: both band sums are exact and equal
    df = F / N
    count = lambda f: int(np.sum(np.abs(fk - f) <= 100000.0))
    f1 = next(f for f in np.arange(-20, 0) * 100000.0 if count(f) == count(f + 100000.0))
    psd = np.full(N, 2.0 ** -30)
    k = int(np.ceil((f1 + 30000.0) / df)) + N // 2
    assert f1 < fk[k] < f1 + 100000.0
    psd[k] = 2.0 ** -16
    got = _check(psd, raster_hz=100000, bandwidth_hz=200000, threshold_db=3.0)
    assert [g["offset_hz"] for g in got] == [int(f1)], got


def test_finder_candidate_on_max_abs_edge():
    psd = _bumps(8192, [-4000000, 4000000, 0], [1e-5, 1e-5, 1e-5])
    got = _check(psd, raster_hz=100000, max_abs_offset_hz=4000000, threshold_db=10.0)
    assert got[0]["offset_hz"] == -4000000 and got[-1]["offset_hz"] == 4000000
    got = _check(psd, raster_hz=100000, max_abs_offset_hz=3999999, threshold_db=10.0)
    assert all(abs(g["offset_hz"]) < 4000000 for g in got)


def test_finder_default_max_abs_and_percentile():
    psd = _bumps(4096, [-4800000, 4800000, -4500000, 2e6], [1e-5] * 4)
    got = _check(psd, raster_hz=100000)                   # max_abs 0 = (F - 384 kHz) / 2 = 4.808 MHz
    assert 2000000 in [g["offset_hz"] for g in got]
    _check(psd, raster_hz=100000, floor_percentile=50.0)
    _check(psd, raster_hz=100000, floor_percentile=99.9)


def test_finder_cap_smaller_than_count():
    cents = [-3e6, -1e6, 0, 1e6, 3e6]
    psd = _bumps(8192, cents, [1e-5] * 5)
    allst = _check(psd, raster_hz=100000)
    assert len(allst) == 5
    L = fmr.lib()
    out = (fmr.Station * 2)()
    rule = fmr.StationRule(100000, 0, 200000, 0, 10.0, 0.0)
    n = L.fmr_find_stations(np.ascontiguousarray(psd).ctypes.data_as(C.POINTER(C.c_double)), len(psd), F, C.byref(rule), out, 2)
    assert n == 5
    assert [s.offset_hz for s in out] == [int(c) for c in cents[:2]]
    assert [g["offset_hz"] for g in fmr.find_stations(psd, F, raster_hz=100000, cap=2)] == [int(c) for c in cents[:2]]


@pytest.mark.parametrize("kw", [dict(raster_hz=0), dict(raster_hz=-5), dict(bandwidth_hz=0), dict(bandwidth_hz=-1),
                                dict(floor_percentile=100.0), dict(floor_percentile=-1.0)])
def test_finder_refusals(kw):
    psd = np.ones(8192)
    rule = dict(raster_hz=100000, bandwidth_hz=200000)
    rule.update(kw)
    with pytest.raises(fmr.FmrError, match=r"fmr_find_stations failed \(-2\)"):
        fmr.find_stations(psd, F, **rule)


def test_finder_refuses_bad_size_and_rate():
    L = fmr.lib()
    rule = fmr.StationRule(100000, 0, 200000, 0, 10.0, 0.0)
    psd = np.ones(8192)
    dp = psd.ctypes.data_as(C.POINTER(C.c_double))
    assert L.fmr_find_stations(dp, 1000, F, C.byref(rule), None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_find_stations(dp, 8192, 0.0, C.byref(rule), None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_find_stations(dp, 8192, -1.0, C.byref(rule), None, 0) == fmr.ERR_BAD_ARG

"""tests/monitor_fixture.py (the float64 restatement the GPU tests hold the modulation monitor to) against analytic
truth: a noise-free second of a 1 kHz tone, a 19 kHz pilot and a biphase-keyed 57 kHz subcarrier."""
import importlib

import numpy as np
import pytest

import monitor_fixture as mf

fmr = importlib.import_module("airspy-fmradion_amd")      # (the fixture's own tests need no device; this pins the import path)

M = 384000
T = np.arange(M + mf.H, dtype=np.float64) / mf.F          # one record and the 512 samples that complete it


def station():
    sq = np.sign(np.sin(2 * np.pi * 1187.5 * T) + 1e-300)
    return (0.5 * np.sin(2 * np.pi * 1000.0 * T) + 0.09 * np.sin(2 * np.pi * 19000.0 * T + 0.3) +
            (2.0 / 75.0) * sq * np.cos(2 * np.pi * 57000.0 * T))


@pytest.fixture(scope="module")
def one_second():
    x = station().astype(np.float32)
    return x, mf.records(x, M=M, B=256, R=2.0)


def test_one_record_of_one_second(one_second):
    x, (recs, hist, psd) = one_second
    assert len(recs) == 1 and mf.n_complete(len(x) - 1, M) == 0
    r = recs[0]
    assert (int(r["index"]), int(r["first_sample"]), int(r["n_finite"]), int(r["n_nonfinite"])) == (0, 0, M, 0)
    assert int(r["segments"]) == M // mf.H and int(r["segments_skipped"]) == 0


def test_pilot_deviation(one_second):
    _, (recs, _, psd) = one_second
    lv = mf.derive(recs, psd)
    print("pilot", lv["pilot_deviation_hz"])
    assert abs(lv["pilot_deviation_hz"] - 6750.0) <= 1e-3 * 6750.0


def test_psd_integrates_to_the_mean_square(one_second):
    x, (recs, _, psd) = one_second
    ms = np.mean(x[:M].astype(np.float64) ** 2)
    total = np.sum(psd[0]) * mf.F / mf.N
    print("rel", abs(total - ms) / ms)
    assert abs(total - ms) <= 1e-5 * ms
    assert abs(float(recs[0]["sumsq"]) / M - ms) <= 1e-12 * ms


def test_mpx_power_of_the_bs412_reference_sine():
    x = ((19.0 / 75.0) * np.sin(2 * np.pi * 400.0 * T)).astype(np.float32)
    recs, _, psd = mf.records(x, M=M)
    lv = mf.derive(recs, psd)
    print("dBr", lv["mpx_power_dbr"])
    assert abs(lv["mpx_power_dbr"]) <= 1e-6
    assert abs(lv["peak_deviation_hz"] - 19000.0) <= 1.0 and abs(lv["tuning_offset_hz"]) <= 1e-3


def test_peak_deviation_is_the_sample_extremes(one_second):
    x, (recs, _, psd) = one_second
    v = x[:M].astype(np.float64)
    lv = mf.derive(recs, psd)
    assert float(recs[0]["min"]) == v.min() and float(recs[0]["max"]) == v.max()
    want = 75000.0 * max(v.max() - v.mean(), v.mean() - v.min())
    assert abs(lv["peak_deviation_hz"] - want) <= 1e-9 * want
    assert abs(lv["tuning_offset_hz"] - 75000.0 * v.mean()) <= 1e-6


def test_every_sample_is_in_exactly_one_bin(one_second):
    x, (recs, hist, _) = one_second
    assert int(hist[0].sum()) == M
    # away from the bin edges the float32 rule is the real-number rule
    v = x[:M].astype(np.float64)
    u = (v + 2.0) * 256 / 4.0
    clear = np.abs(u - np.round(u)) > 1e-3
    b = mf.bins_of(x[:M], 256, 2.0)
    assert np.array_equal(b[clear], np.floor(u[clear]).astype(np.int64))
    assert np.array_equal(hist[0], np.bincount(b, minlength=256))


def test_out_of_range_samples_land_in_the_end_bins():
    x = (1.2 * np.sin(2 * np.pi * 1000.0 * T[:4096 + mf.H])).astype(np.float32)
    x[7], x[9] = 3.0e38, -3.0e38
    recs, hist, _ = mf.records(x, M=4096, B=64, R=1.0)
    v = x[:4096]
    assert int(hist[0].sum()) == 4096
    assert int(hist[0][63]) == int(np.sum(v >= 1.0 - 1.0 / 32)) >= int(np.sum(v >= 1.0)) > 1
    assert int(hist[0][0]) == int(np.sum(v < -1.0 + 1.0 / 32)) >= int(np.sum(v < -1.0)) > 1


def test_a_non_finite_sample_is_counted_and_skips_its_two_segments():
    x = station()[:5 * 4096 + mf.H].astype(np.float32)
    clean = mf.records(x, M=4096, B=64, R=1.0)
    y = x.copy()
    y[5000] = np.nan
    y[3 * 4096] = np.inf                     # a record's first sample: one segment in record 2, one in record 3
    recs, hist, psd = mf.records(y, M=4096, B=64, R=1.0)
    assert [int(v) for v in recs["n_nonfinite"]] == [0, 1, 0, 1, 0]
    assert [int(v) for v in recs["n_finite"]] == [4096, 4095, 4096, 4095, 4096]
    assert [int(v) for v in recs["segments_skipped"]] == [0, 2, 1, 1, 0]
    assert [int(v) for v in recs["segments"]] == [8, 6, 7, 7, 8]
    assert np.isfinite(psd).all() and all(np.isfinite(recs[k]).all() for k in ("min", "max", "sum", "sumsq"))
    assert np.array_equal(hist.sum(axis=1), recs["n_finite"])
    for i in (0, 4):
        assert recs[i] == clean[0][i] and np.array_equal(hist[i], clean[1][i]) and np.array_equal(psd[i], clean[2][i])
    # all samples of a record non-finite: an empty record of zeros
    z = x.copy()
    z[4096:8192 + mf.H] = np.nan
    r1 = mf.records(z, M=4096, B=64, R=1.0)
    assert int(r1[0][1]["n_finite"]) == 0 and int(r1[0][1]["segments"]) == 0
    assert float(r1[0][1]["min"]) == 0.0 == float(r1[0][1]["max"]) and not r1[2][1].any() and not r1[1][1].any()

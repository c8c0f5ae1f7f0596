"""tests/rfmon_fixture.py (the float64 restatement of the RF monitor the GPU tests take as their oracle) against analytic
truth: C/N of a constant-envelope carrier in Gaussian noise, the envelope AM of a known modulation, the histogram's
integer rule and its percentiles, and the non-finite rules.  No device, no library."""
import numpy as np
import pytest

import rfmon_fixture as rx

M = 38400


def _one(p, M=M):
    recs, hist, psd = rx.records(p, M=M)
    return recs, hist, psd, rx.derive(recs, hist, psd)


@pytest.mark.parametrize("cn", [10.0, 20.0, 30.0])
def test_cn_of_fm_in_gaussian_noise(cn):
    """Constant-envelope FM of amplitude 0.3 plus white complex Gaussian noise, one record: cn_db within 0.25 dB (the
    moment estimator's own scatter over 38400 samples is 0.09 dB at worst over 20 seeds per level)."""
    x = rx.fm_iq(M + rx.H, amplitude=0.3, noise=0.09 / 10.0 ** (cn / 10.0), seed=int(cn))
    recs, _, _, lv = _one(rx.power(x))
    assert len(recs) == 1 and recs["n_finite"][0] == M and recs["segments"][0] == M // rx.H
    print(cn, lv["cn_db"], lv["level_dbfs"], lv["carrier_dbfs"], lv["noise_dbfs"])
    assert abs(lv["cn_db"] - cn) <= 0.25
    assert abs(lv["carrier_dbfs"] - 10.0 * np.log10(0.09)) <= 0.1
    assert abs(lv["level_dbfs"] - 10.0 * np.log10(0.09 * (1.0 + 10.0 ** (-cn / 10.0)))) <= 0.1


def test_envelope_am_of_a_known_modulation():
    """x = A (1 + m sin 2 pi 3000 t) e^{j phi}, m = 0.1 (3000 Hz is bin 8): p = A^2 (1 + m^2/2 + 2 m sin - (m^2/2) cos 2w t)."""
    m, A = 0.1, 0.3
    x = rx.fm_iq(M + rx.H, amplitude=A, am=m)
    p = rx.power(x)
    recs, hist, psd, lv = _one(p)
    want = 10.0 * np.log10((2 * m * m + m ** 4 / 8) / (4 * (1 + m * m / 2) ** 2))
    assert abs(want + 23.05) < 0.01
    assert abs(lv["am_audio_db"] - want) <= 0.01, (lv["am_audio_db"], want)
    p64 = p[:M].astype(np.float64)
    assert abs(psd[0].sum() * rx.F / rx.N - np.mean(p64 * p64)) <= 1e-6 * np.mean(p64 * p64)
    # the same modulation read from the moments: rms of (|x| / A - 1) is m / sqrt 2 to first order
    assert abs(lv["am_rms"] - m / np.sqrt(2.0)) <= 0.01 * m
    assert lv["am_pilot_db"] < want - 60.0 and lv["am_floor_dbc_hz"] < -120.0
    assert abs(lv["level_dbfs"] - 10.0 * np.log10(A * A * (1 + m * m / 2))) <= 1e-4


def test_histogram_bins_of_the_stated_values():
    p = np.array([0.0, 1e-13, 2.0 ** -40, 0.09, 1.0, 255.9, 256.0, 1e9], dtype=np.float32)
    assert list(rx.bins_of(p)) == [0, 0, 0, 291, 320, 383, 383, 383]
    # eight bins per octave; an edge belongs to the bin it opens
    assert rx.bin_edge(320) == 1.0 and rx.bin_edge(328) == 2.0 and rx.bin_edge(324) == 1.5 and rx.bin_edge(0) == 2.0 ** -40
    for b in (1, 5, 100, 291, 383):
        e = np.float32(rx.bin_edge(b))
        assert rx.bins_of(np.array([e]))[0] == b and rx.bins_of(np.array([np.nextafter(e, np.float32(0))]))[0] == b - 1


def test_percentiles_of_a_two_level_signal():
    """90 % of the samples at -10 dBFS (p = 0.1 = 1.6 x 2^-4: the bin from 1.5 x 2^-4) and 10 % at -30 dBFS (p = 0.001 =
    1.024 x 2^-10: the bin from 2^-10)."""
    Mr = 5120
    p = np.full(Mr + rx.H, 0.1, dtype=np.float32)
    p[100:100 + Mr // 10] = 0.001
    recs, hist, psd, lv = _one(p, M=Mr)
    assert hist[0].sum() == Mr and sorted(hist[0][hist[0] > 0]) == [Mr // 10, Mr - Mr // 10]
    lo, hi = 10.0 * np.log10(2.0 ** -10), 10.0 * np.log10(1.5 * 2.0 ** -4)
    assert abs(lv["p10_dbfs"] - lo) < 1e-12 and abs(lv["p50_dbfs"] - hi) < 1e-12 and abs(lv["p90_dbfs"] - hi) < 1e-12
    p[100 + Mr // 10 - 1] = 0.1                     # one sample fewer than 10 % in the fade: p10 moves up
    assert abs(_one(p, M=Mr)[3]["p10_dbfs"] - hi) < 1e-12
    assert recs["p_min"][0] == np.float32(0.001) and recs["p_max"][0] == np.float32(0.1)


def test_non_finite_samples_are_counted_and_their_segments_skipped():
    Mr = 4096
    rng = np.random.default_rng(1)
    p = (0.09 * (1.0 + 0.1 * rng.standard_normal(3 * Mr + rx.H)) ** 2).astype(np.float32)
    clean = rx.records(p, M=Mr)
    p[700] = np.nan                  # mid-record: segments 0 and 1
    p[Mr + 512 * 3] = np.inf         # a segment's first sample: segments 10 and 11 of record 1 (8 segments per record)
    p[2 * Mr - 1] = np.nan           # record 1's last sample: its last two segments
    p[2 * Mr + 2000:2 * Mr + 2003] = -np.inf
    recs, hist, psd = rx.records(p, M=Mr)
    assert list(recs["n_nonfinite"]) == [1, 2, 3] and list(recs["n_finite"]) == [Mr - 1, Mr - 2, Mr - 3]
    assert list(recs["segments_skipped"]) == [2, 4, 2] and list(recs["segments"]) == [6, 4, 6]
    assert [int(h.sum()) for h in hist] == [Mr - 1, Mr - 2, Mr - 3]
    for i in range(3):
        v = p[i * Mr:(i + 1) * Mr].astype(np.float64)
        v = v[np.isfinite(v)]
        assert recs["m2"][i] == v.sum() and recs["m4"][i] == (v * v).sum()
        assert recs["p_min"][i] == v.min() and recs["p_max"][i] == v.max()
    # the segments that stay are the clean run's: record 0 keeps 2 .. 7
    P, ok = rx.mf.segment_psd(p, 0, 8)
    assert list(ok) == [False, False] + [True] * 6 and np.allclose(psd[0], P[2:].mean(axis=0), rtol=1e-12)
    assert np.isfinite(psd).all() and not np.array_equal(psd[0], clean[2][0])
    # a record of nothing but non-finite values
    recs, hist, psd = rx.records(np.full(Mr + rx.H, np.nan, dtype=np.float32), M=Mr)
    lv = rx.derive(recs, hist, psd)
    assert recs["n_finite"][0] == 0 and recs["p_min"][0] == 0 and recs["p_max"][0] == 0 and recs["segments"][0] == 0
    assert lv["level_dbfs"] == -np.inf and lv["cn_db"] == -np.inf and lv["p50_dbfs"] == -np.inf and lv["am_rms"] == 0.0


def test_power_is_unfused_float32():
    x = rx.fm_iq(1000, amplitude=0.3, noise=1e-3, seed=2)
    p = rx.power(x)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    assert p.dtype == np.float32 and np.array_equal(p, (re * re).astype(np.float32) + (im * im).astype(np.float32))
    bad = np.array([complex(np.nan, 0), complex(np.inf, 1), complex(3e19, 3e19)], dtype=np.complex64)
    assert not np.isfinite(rx.power(bad)).any()

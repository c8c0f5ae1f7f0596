"""The analyser's float64 restatement (tests/analyser_fixture.py) against analytic truth: a sine's level and frequency
on and off bin centres, known harmonic ratios, a known noise floor, the mid / side views, the skip rule and pooling.
Each signal is 8 N frames.  The window's -92 dB side lobes are the instrument's floor: a pure sine reads a THD of
1.1e-5 .. 4.7e-5 of nothing but leakage, which is what the bounds on thd and thd_n of a pure sine allow for."""
import math

import numpy as np
import pytest

import analyser_fixture as af

A = 0.0866
SIZES = (1024, 4096, 8192)


def _tones(N):
    """880, 997 and 1000 Hz, and one 0.37 bin off a bin centre"""
    return (880.0, 997.0, 1000.0, (round(1500.0 * N / 48000.0) + 0.37) * 48000.0 / N)


def _sine(N, f, amp=A, phase=0.3, harmonics=()):
    t = np.arange(8 * N) / 48000.0
    x = amp * np.sin(2 * np.pi * f * t + phase)
    for h, dbc in harmonics:
        x = x + amp * 10.0 ** (dbc / 20.0) * np.sin(2 * np.pi * h * f * t + 0.1 * h)
    return x


CASES = [(N, f) for N in SIZES for f in _tones(N)]


@pytest.mark.parametrize("N,f", CASES)
def test_pure_sine(N, f):
    recs, sp = af.records(_sine(N, f), 1, N)
    assert len(recs) == 1 and recs["segments"][0] == 12 and recs["skipped"][0] == 0
    d = af.derive(recs, sp)
    print(N, f, d)
    assert d["tone_found"] == 1
    assert abs(d["tone_dbfs"] - 20.0 * math.log10(A)) <= 1e-4
    assert abs(d["tone_hz"] - f) <= 1e-5
    assert d["thd"] < 1e-5 and d["thd_n"] < 1e-4
    k_hi = math.floor(15000.0 * N / 48000.0)      # a harmonic counts while its lobe lies inside the band
    assert d["harmonics_counted"] == sum(1 for h in range(2, 11) if math.floor(h * f * N / 48000.0 + 0.5) + 4 <= k_hi)


@pytest.mark.parametrize("N,f", CASES)
def test_known_harmonics(N, f):
    recs, sp = af.records(_sine(N, f, harmonics=((2, -40.0), (3, -50.0))), 1, N)
    d = af.derive(recs, sp)
    print(N, f, d)
    assert abs(d["thd"] - 0.010488) <= 1e-5
    assert abs(d["harmonic_dbc"][0] + 40.0) <= 0.01 and abs(d["harmonic_dbc"][1] + 50.0) <= 0.01
    assert d["harmonic_dbc"][2] < -90.0
    assert abs(d["sinad_db"] + 20.0 * math.log10(d["thd_n"])) < 1e-3      # (THD+N small: SINAD = -20 log10 THD+N)


@pytest.mark.parametrize("N", SIZES)
def test_noise_floor(N):
    rng = np.random.default_rng(5)
    sigma = 1e-4
    x = _sine(N, 997.0) + sigma * rng.standard_normal(8 * N)
    recs, sp = af.records(x, 1, N)
    d = af.derive(recs, sp)
    print(N, d)
    want = 10.0 * math.log10(2.0 * sigma * sigma * 14980.0 / 24000.0)
    assert abs(d["noise_dbfs"] - want) <= 0.5
    assert abs(d["total_dbfs"] - 10.0 * math.log10(A * A + 2.0 * sigma * sigma)) <= 0.05
    assert abs(d["dc"]) < 1e-3


@pytest.mark.parametrize("N", SIZES)
def test_mid_and_side_views(N):
    x = _sine(N, 1000.0)
    anti = np.stack([x, -x], axis=1).reshape(-1)
    same = np.stack([x, x], axis=1).reshape(-1)
    ra, sa = af.records(anti, 2, N)
    rs, ss = af.records(same, 2, N)
    lvl = 20.0 * math.log10(A)
    assert abs(af.derive(ra, sa, view="S")["tone_dbfs"] - lvl) <= 1e-4
    assert af.derive(ra, sa, view="M")["tone_found"] == 0 and af.derive(ra, sa, view="M")["band_dbfs"] < lvl - 150.0      # (fp64 rounding of P_L + P_R -+ 2 C)
    assert abs(af.derive(rs, ss, view="M")["tone_dbfs"] - lvl) <= 1e-4
    assert af.derive(rs, ss, view="S")["tone_found"] == 0 and af.derive(rs, ss, view="S")["band_dbfs"] < lvl - 150.0      # (fp64 rounding of P_L + P_R -+ 2 C)
    for v in ("L", "R"):
        assert abs(af.derive(ra, sa, view=v)["tone_dbfs"] - lvl) <= 1e-4
    # unlike channels: each view reads its own tone
    y = _sine(N, 3000.0, amp=0.02)
    ru, su = af.records(np.stack([x, y], axis=1).reshape(-1), 2, N)
    assert abs(af.derive(ru, su, view="L")["tone_hz"] - 1000.0) <= 1e-3
    assert abs(af.derive(ru, su, view="R")["tone_hz"] - 3000.0) <= 1e-3
    assert abs(af.derive(ru, su, view="R")["tone_dbfs"] - 20.0 * math.log10(0.02)) <= 1e-3
    assert math.isnan(af.derive(ru, su, view="M")["total_dbfs"])


def test_no_tone():
    rng = np.random.default_rng(6)
    recs, sp = af.records(1e-5 * rng.standard_normal(8 * 1024), 1, 1024)
    d = af.derive(recs, sp)
    assert d["tone_found"] == 0 and math.isnan(d["thd"]) and math.isnan(d["tone_hz"]) and d["noise_dbfs"] == d["band_dbfs"]
    # a tone below the strongest-bin rule's reach (k0 < 2 W + 1) is none either
    recs, sp = af.records(_sine(1024, 200.0), 1, 1024)
    assert af.derive(recs, sp)["tone_found"] == 0
    # silence
    recs, sp = af.records(np.zeros(8 * 1024), 1, 1024)
    d = af.derive(recs, sp)
    assert d["tone_found"] == 0 and d["band_dbfs"] == -math.inf and d["total_dbfs"] == -math.inf


def test_skipped_segments_and_nonfinite_samples():
    N, M = 1024, 2048
    x = _sine(N, 1000.0)
    x[700] = np.nan                      # segments 0 and 1 (H = 512) hold it: record 0 counts 2 of its 4
    x[5 * 1024 + 100] = np.inf           # segments 9 and 10: record 2 (segments 8 .. 11)
    recs, sp = af.records(x, 1, N, M)
    assert len(recs) == 3                # 15 segments, 4 per record
    assert list(recs["segments"]) == [2, 4, 2] and list(recs["skipped"]) == [2, 0, 2]
    assert list(recs["n_nonfinite"]) == [1, 0, 1]
    clean = np.where(np.isfinite(x), x, 0.0)
    for i in range(3):
        assert abs(recs["sum"][i][0] - np.sum(clean[i * M:(i + 1) * M])) < 1e-12
        assert abs(recs["sumsq"][i][0] - np.sum(clean[i * M:(i + 1) * M] ** 2)) < 1e-12
    d = af.derive(recs, sp)
    assert d["segments"] == 8 and d["skipped"] == 4 and d["n_nonfinite"] == 2
    assert abs(d["tone_dbfs"] - 20.0 * math.log10(A)) <= 1e-4
    # a record of skipped segments only has zero rows and no weight
    x[:] = np.nan
    recs, sp = af.records(x, 1, N, M)
    assert np.all(recs["segments"] == 0) and not sp.any()
    assert af.derive(recs, sp)["tone_found"] == 0


def test_pooling_weights_by_segments_over_gaps():
    N, M = 1024, 1024
    x = np.concatenate([_sine(N, 1000.0, amp=0.1)[:4 * N], _sine(N, 1000.0, amp=0.2)[:4 * N]])
    x[100] = np.nan                      # record 0 counts one of its two segments
    recs, sp = af.records(x, 1, N, M)
    assert len(recs) == 7
    pick = np.array([0, 1, 5, 6])        # a gap, as dropped records leave it
    d = af.derive(recs[pick], sp[pick])
    w = recs["segments"][pick].astype(float)
    assert list(w) == [1, 2, 2, 2]
    lobe = lambda i: float(np.sum(sp[i, 0, 17:26]))      # 1000 Hz is bin 21.33
    want = sum(w[j] * lobe(i) for j, i in enumerate(pick)) / w.sum()
    assert abs(d["tone_dbfs"] - 10.0 * math.log10(2.0 * want)) <= 1e-9
    assert d["segments"] == 7 and d["skipped"] == 1


def test_tone_hint_beside_a_stronger_spur():
    N = 4096
    x = _sine(N, 880.0) + _sine(N, 5000.0, amp=0.3)
    recs, sp = af.records(x, 1, N)
    assert abs(af.derive(recs, sp)["tone_hz"] - 5000.0) <= 1e-3
    d = af.derive(recs, sp, tone_hz=880.0)
    assert abs(d["tone_hz"] - 880.0) <= 1e-3 and abs(d["tone_dbfs"] - 20.0 * math.log10(A)) <= 1e-3
    assert d["thd"] < 1e-4 and d["thd_n"] > 1.0          # (the spur is no harmonic of 880 Hz: it is noise)
    d = af.derive(recs, sp, tone_hz=900.0, tone_search_hz=30.0)
    assert abs(d["tone_hz"] - 880.0) <= 1e-3

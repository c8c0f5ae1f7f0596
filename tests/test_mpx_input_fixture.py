"""tests/mpx_input_fixture.py (the numpy restatement of fmr_create_mpx_decoder's front end) held to the header's
specification: the count law, tones against the same tone delayed by delay_samples, the round trip through the MPX output's
fixture and back, the S16 conversion and the non-finite rule.

Bounds.  One filter: the +-0.001 dB pass band, 1.2e-4 of the amplitude (measured in numpy float64 at 192000, 171000, 228000,
256000 and 96000 with 1 kHz, 19 kHz and 0.9 rate / 2 - 100 Hz: at most 3.8e-6).  Two filters in a row: 2.4e-4."""
import importlib

import numpy as np
import pytest

import mpx_input_fixture as mi
import mpx_output_fixture as mo

fmr = importlib.import_module("airspy-fmradion_amd")

RATES = [96000, 171000, 192000, 228000, 256000]
GEOM = {96000: (1, 4), 171000: (57, 128), 192000: (1, 2), 228000: (19, 32), 256000: (2, 3)}
ONE_FILTER, TWO_FILTERS = 1.2e-4, 2.4e-4


@pytest.mark.parametrize("rate", RATES)
def test_geometry(rate):
    h, L, M, T = mi.taps(rate)
    g = mi.geometry(rate)
    assert g[:2] == GEOM[rate] and g[2] == T > 1 and g[3] == -(-T * L // M) == 143
    assert g[4] == (T * L - 1) / (2.0 * L)
    assert fmr.mpx_input_geometry(rate) == g      # the library's host-only entry says the same
    # the per-phase DC gains of the interpolator: sum over k of h[p + k M] (M / L) is 1 to 1e-6
    K = g[3]
    hp = np.concatenate([h, np.zeros(K * M - T * L)]).reshape(K, M)
    dc = hp.sum(axis=0) * (M / L)
    print(f"rate {rate}: L {L} M {M} T {T} K {K}; phase DC gains within {np.abs(dc - 1).max():.2e} of 1")
    assert np.abs(dc - 1).max() <= 1e-6
    assert mi.geometry(384000) == mi.geometry(0) == (1, 1, 1, 1, 0.0)


@pytest.mark.parametrize("rate", [192000, 171000, 256000])
def test_count_law(rate):
    L, M, T, K, _ = mi.geometry(rate)
    x = (np.random.default_rng(2).standard_normal(1013) * 0.3).astype(np.float32)
    whole, _ = mi.run(x, rate, 1.0)
    for F in (0, 1, K - 1, K, 1013):
        out, nf = mi.run(x[:F], rate, 1.0)
        assert len(out) == -(-F * M // L) == mi.n_out(F, L, M) and nf == 0, (F, len(out))
        assert out.tobytes() == whole[:len(out)].tobytes()      # sample j exists as soon as u[i0] does, and never changes
    # blocks: the difference of the count across each, 0 included where M / L allows none (never here: M >= L)
    bl = [1, 0, 3, 64, 0, 945]
    cnt = mi.block_counts(bl, L, M)
    assert cnt.sum() == mi.n_out(sum(bl), L, M) and cnt[1] == cnt[4] == 0 and cnt[0] == mi.n_out(1, L, M)
    assert mi.block_counts(bl[2:], L, M, frames_before=1).tolist() == cnt[2:].tolist()


def _tone_error(rate, f, A=0.25, gain=2.0, n=600):
    L, M, T, K, delay = mi.geometry(rate)
    s0 = int(np.ceil(2 * delay)) + 2                      # MPX samples until the filter is full
    F = -(-(s0 + n) * L // M) + 1
    u = (A * np.sin(2 * np.pi * f * np.arange(F) / rate)).astype(np.float32)
    x, nf = mi.run(u, rate, gain)
    j = np.arange(len(x))
    want = A * gain * np.sin(2 * np.pi * f * (j - delay) / 384000.0)
    assert len(x) - s0 >= n and nf == 0
    return np.abs(x[s0:] - want[s0:]).max() / (A * gain)


@pytest.mark.parametrize("rate", RATES)
def test_tones_come_out_delayed_by_delay_samples(rate):
    for f in (19000.0, 0.9 * rate / 2 - 100.0):
        err = _tone_error(rate, f)
        print(f"rate {rate}, {f:.0f} Hz: worst deviation from the delayed tone / amplitude: {err:.2e} (bound {ONE_FILTER})")
        assert err <= ONE_FILTER


def test_round_trip_through_the_mpx_output():
    """19 kHz and 57 kHz at 384 kHz through the MPX output's fixture at 192000 F32 gain 1 and back: the sum of both tones,
    delayed by both filters, (T L - 1) / L MPX samples."""
    rate = 192000
    L, M, T, K, delay = mi.geometry(rate)
    A = 0.1
    n = int(4 * delay) + 2000
    t = np.arange(n) / 384000.0
    x = (A * np.sin(2 * np.pi * 19000.0 * t) + A * np.sin(2 * np.pi * 57000.0 * t + 0.3)).astype(np.float32)
    pcm, cl, nf = mo.run(x, rate, 1.0, mo.PCM_F32)
    assert pcm.dtype == np.float32 and (cl, nf) == (0, 0)
    assert mo.info(rate, 1.0, n)["delay_frames"] * M / L == delay      # the same filter, the same delay in MPX samples
    y, nf2 = mi.run(pcm, rate, 1.0)
    assert nf2 == 0 and len(y) == mi.n_out(len(pcm), L, M)
    d = 2 * delay
    j = np.arange(len(y))
    want = A * np.sin(2 * np.pi * 19000.0 * (j - d) / 384000.0) + A * np.sin(2 * np.pi * 57000.0 * (j - d) / 384000.0 + 0.3)
    s0 = int(np.ceil(2 * d)) + 2
    err = np.abs(y[s0:] - want[s0:]).max() / A
    print(f"round trip at {rate}: worst deviation / amplitude {err:.2e} (bound {TWO_FILTERS})")
    assert len(y) - s0 >= 1000 and err <= TWO_FILTERS


def test_384000_has_no_filter():
    x = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    y, nf = mi.run(x, 384000, 1.0)
    assert y.tobytes() == x.tobytes() and nf == 0
    y2, _ = mi.run(x, 0, 0.5)
    assert y2.tobytes() == (x.astype(np.float64) * 0.5).astype(np.float32).tobytes()


def test_s16_conversion():
    v = np.array([-32768, 32767, 0, 1, -1], dtype=np.int16)
    u, nf = mi.convert(v)
    assert nf == 0 and u.dtype == np.float64
    assert u.tolist() == [-32768 / 32767.0, 1.0, 0.0, 1 / 32767.0, -1 / 32767.0] and not np.signbit(u[2])
    y, _ = mi.run(v, 384000, 1.0)
    assert y.tolist() == [np.float32(-32768 / 32767.0), 1.0, 0.0, np.float32(1 / 32767.0), np.float32(-1 / 32767.0)]


def test_nonfinite_f32_becomes_zero_and_is_counted():
    x = np.array([0.5, np.nan, -0.25, np.inf, -np.inf, 0.125], dtype=np.float32)
    u, nf = mi.convert(x)
    assert nf == 3 and u.tolist() == [0.5, 0.0, -0.25, 0.0, 0.0, 0.125] and not np.signbit(u[[1, 3, 4]]).any()
    clean = x.copy()
    clean[[1, 3, 4]] = 0.0
    for rate in (384000, 192000):
        y, n1 = mi.run(x, rate, 1.0)
        y0, n0 = mi.run(clean, rate, 1.0)
        assert (n1, n0) == (3, 0) and y.tobytes() == y0.tobytes() and np.isfinite(y).all()


def test_info():
    want = {"format": mi.PCM_S16, "rate": 171000, "L": 57, "M": 128, "taps_per_phase": mi.taps(171000)[3],
            "taps_per_sample": 143, "delay_samples": mi.geometry(171000)[4], "full_scale_hz": 150000.0, "frames_in": 1013,
            "samples_out": 2275, "nonfinite_in": 0}
    assert mi.info(171000, 2.0, 1013) == want

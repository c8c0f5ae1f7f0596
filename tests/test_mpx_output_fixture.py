"""tests/mpx_output_fixture.py (the numpy restatement of fmr_enable_mpx_output's definition) and the library's prototype
filters (fmr_mpx_output_taps is host only) held to the header's specification: symmetry, sum, pass band, stop band, the
count law, and tones through the 192000 converter."""
import importlib

import numpy as np
import pytest

import mpx_output_fixture as mf

fmr = importlib.import_module("airspy-fmradion_amd")

RATES = [96000, 171000, 192000, 228000, 256000]
GEOM = {96000: (1, 4), 171000: (57, 128), 192000: (1, 2), 228000: (19, 32), 256000: (2, 3)}
PASS_DB, STOP_DB = 0.001, -100.0
PASS_REL = 10.0 ** (PASS_DB / 20.0) - 1.0        # 1.2e-4 of the amplitude
STOP_REL = 10.0 ** (STOP_DB / 20.0)              # 1e-5


def settle(L, M, T):
    return -(-T * L // M) + 2


@pytest.mark.parametrize("rate", RATES)
def test_taps_are_symmetric_and_sum_to_L(rate):
    h, L, M, T = mf.taps(rate)
    assert (L, M) == GEOM[rate] == mf.geometry(rate) and len(h) == T * L and T > 1
    assert h.tobytes() == h[::-1].tobytes()
    assert abs(float(np.sum(h)) - L) <= 1e-12 * L, float(np.sum(h)) - L


@pytest.mark.parametrize("rate", RATES)
def test_response_meets_the_specification(rate):
    """Pass band 0 .. 0.9 rate / 2 within +-0.001 dB and stop band from rate / 2 on >= 100 dB down, read off a zero-padded
    FFT of the taps in float64 (grid: 16 points per main-lobe width at least)."""
    h, L, M, T = mf.taps(rate)
    nfft = 1 << int(np.ceil(np.log2(16 * len(h))))
    H = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(len(H)) * (384000.0 * L / nfft)
    pb = 20 * np.log10(H[f <= 0.9 * rate / 2])
    sb = 20 * np.log10(np.maximum(H[f >= rate / 2], 1e-300))
    print(f"rate {rate}: L {L} M {M} T {T}; pass band {pb.min():+.2e} .. {pb.max():+.2e} dB; stop band {sb.max():.2f} dB")
    assert np.abs(pb).max() <= PASS_DB and sb.max() <= STOP_DB


def test_384000_has_no_filter_and_refused_rates():
    for rate in (384000, 0):
        h, L, M, T = fmr.mpx_output_taps(rate)
        assert (h.tolist(), L, M, T) == ([1.0], 1, 1, 1)
    x = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    pcm, c, n = mf.run(x, 384000, 1.0, mf.PCM_F32)
    assert pcm.tobytes() == x.tobytes() and n == 0 and c == int((np.abs(x) > 1).sum())
    for rate in (95999, 384001, 100001):
        with pytest.raises(fmr.FmrError, match="rate"):
            fmr.mpx_output_taps(rate)


@pytest.mark.parametrize("rate", RATES)
def test_count_law(rate):
    h, L, M, T = mf.taps(rate)
    x = np.random.default_rng(2).standard_normal(1013).astype(np.float32) * 0.3
    whole = mf.run(x, rate, 1.0, mf.PCM_F32)[0]
    for F in (0, 1, T - 1, T, 1013):
        pcm, _, _ = mf.run(x[:F], rate, 1.0, mf.PCM_F32)
        assert len(pcm) == -(-F * L // M) == mf.n_out(F, L, M), (F, len(pcm))
        assert pcm.tobytes() == whole[:len(pcm)].tobytes()      # frame m exists as soon as x[q] does, and never changes


def test_pilot_tone_comes_out_at_19_khz():
    """19 kHz through the 192000 converter against the same tone delayed by delay_frames: within the pass-band bound of the
    amplitude once the filter is full."""
    rate = 192000
    h, L, M, T = mf.taps(rate)
    s0 = settle(L, M, T)
    F = (s0 + 400) * M // L + 1
    A, f, g = 0.1, 19000.0, 0.5
    x = (A * np.sin(2 * np.pi * f * np.arange(F) / 384000.0)).astype(np.float32)
    pcm, c, n = mf.run(x, rate, g, mf.PCM_F32)
    delay = mf.info(rate, g, F)["delay_frames"]
    m = np.arange(len(pcm))
    want = A * g * np.sin(2 * np.pi * f * (m - delay) / rate)
    err = np.abs(pcm[s0:] - want[s0:]).max() / (A * g)
    print("19 kHz at 192000: worst deviation from the delayed tone / amplitude:", err)
    assert len(pcm) - s0 >= 400 and err <= PASS_REL + 2 * 2.0 ** -24 and (c, n) == (0, 0)      # (+ the float32 input and output)
    spec = np.abs(np.fft.rfft(pcm[s0:s0 + 384] * np.hanning(384)))
    assert np.argmax(spec) * (rate / 384.0) == 19000.0


def test_stop_band_tone_is_100_db_down():
    rate = 192000
    h, L, M, T = mf.taps(rate)
    s0 = settle(L, M, T)
    F = (s0 + 400) * M // L + 1
    x = np.sin(2 * np.pi * 150000.0 * np.arange(F) / 384000.0).astype(np.float32)
    pcm, _, _ = mf.run(x, rate, 1.0, mf.PCM_F32)
    peak = np.abs(pcm[s0:]).max()
    print("150 kHz at 192000:", 20 * np.log10(peak), "dB")
    assert len(pcm) - s0 >= 400 and peak <= STOP_REL


def test_s16_rounds_half_even_and_saturates():
    x = np.array([0.5 / 32767, 1.5 / 32767, 1.0, -1.0, 1.001, -1.1, np.nan, np.inf], dtype=np.float32)
    pcm, c, n = mf.run(x, 384000, 1.0, mf.PCM_S16)
    z = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        want = np.clip(np.rint(np.where(np.isnan(z), 0.0, z) * 32767.0), -32768, 32767).astype(np.int16)
    assert pcm.tolist() == want.tolist() and pcm[2:8].tolist() == [32767, -32767, 32767, -32768, 0, 32767]
    assert (c, n) == (3, 2)

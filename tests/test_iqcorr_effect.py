"""What the IQ corrector is for, on the CPU oracle alone (oracle_py IfResampler + FmDecoder) with the fixture's corrector.

The capture (iqcorr_fixture.effect_capture): 2.5 MS/s, 2^21 samples, station 3 at -250 kHz with amplitude 0.3 and station
4 at +250 kHz with amplitude 0.03, through impair(g = 1.05, phi = 3 degrees, dc = 0.01 - 0.006j): the strong station's
image, 28.7 dB down, lands on the weak one.

Audio, W = 64, RMS error against the decode of the unimpaired capture over the last quarter of the audio (stereo locked,
window full).  Measured here: weak station 4.23e-2 uncorrected, 1.30e-3 corrected, ratio 32.5; strong station 4.16e-4 and
1.30e-5, ratio 32.0 (of a 0.618 RMS signal).

Spectrum, W = 4, on the strong station alone (so that the image band holds nothing else), Hann periodogram behind the
first W + 1 intervals, in dB re full-scale power: the 200 kHz band around +250 kHz has -4.79 dB clean (the noise floor),
23.99 dB impaired, -4.58 dB corrected: ratio 720; the 2 kHz band around 0 Hz -24.47, 24.51 and -20.72 dB: ratio 33369.

Each assert is a ratio at one quarter of the measured one; the slack is for other seeds and cuts.  The corrected image
band is also held within 1 dB of the clean capture's."""
import math

import numpy as np

import chanbank_fixture as cb
import iqcorr_fixture as qf

F = qf.F


def decode(u, pilotcut, blk=16384):
    lens = [blk] * (len(u) // blk) + ([len(u) % blk] if len(u) % blk else [])
    return np.concatenate(cb.oracle_fm(u, F, lens, pilotcut)[1])


def rms(a):
    return float(np.sqrt(np.mean(np.abs(a) ** 2)))


def band_power(v, f0, bw):
    """Power of v inside f0 +- bw / 2 from one Hann periodogram, re full scale"""
    w = np.hanning(len(v))
    X = np.fft.fft(v.astype(np.complex128) * w)
    fr = np.fft.fftfreq(len(v), 1.0 / F)
    return float(np.sum(np.abs(X[np.abs(fr - f0) <= bw / 2]) ** 2) / np.sum(w * w))


def test_audio_of_both_stations_with_a_window_of_64(pilotcut):
    x, y = qf.effect_capture()
    r = qf.run(y, W=64)
    assert not r["refused"].any() and not r["skipped"].any()
    for f, floor in zip(qf.OFFS, (32.0 / 4, 32.5 / 4)):
        a0, a1, a2 = (decode(cb.mix_down(v, f, F), pilotcut) for v in (x, y, r["out"]))
        q = len(a0) * 3 // 4
        without, with_ = rms(a1[q:] - a0[q:]), rms(a2[q:] - a0[q:])
        print(f"{f} Hz: signal {rms(a0[q:]):.3f}, error {without:.3g} -> {with_:.3g}, ratio {without / with_:.1f}")
        assert without / with_ >= floor


def test_image_band_and_dc_band_with_a_window_of_4():
    W = 4
    x = cb.composite(qf.N_EFFECT, F, qf.OFFS[:1], qf.IDS[:1], qf.AMPS[:1])
    y = qf.impair(x, qf.G1, qf.PHI1, qf.DC1)
    z = qf.run(y, W=W)["out"]
    s = slice((W + 1) * qf.Q, None)
    got = {}
    for name, f0, bw, floor in (("image", 250e3, 200e3, 720.0 / 4), ("0 Hz", 0.0, 2e3, 33369.0 / 4)):
        clean, impaired, corrected = (band_power(v[s], f0, bw) for v in (x, y, z))
        print(f"{name} band: clean {10 * math.log10(clean):.2f} dB, impaired {10 * math.log10(impaired):.2f} dB, "
              f"corrected {10 * math.log10(corrected):.2f} dB, ratio {impaired / corrected:.0f}")
        assert impaired / corrected >= floor
        got[name] = (clean, corrected)
    clean, corrected = got["image"]
    assert abs(10 * math.log10(corrected / clean)) <= 1.0

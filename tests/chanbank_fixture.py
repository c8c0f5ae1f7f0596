"""Composite captures for the channel-bank tests (fmr_config.channel_offset_hz).

A capture holds several FM-stereo stations, each shifted up by its offset with the exact phasor in float64; channel s
of a bank decodes u_s[n] = x[n] exp(-2 pi i ((f_s n) mod F) / F), which these helpers build the same way for the
oracle chain.  n counts samples from the first sample of the capture.
"""
import numpy as np

import oracle_py as ora
import siggen


def phasor(n, f, F, sign, n0=0):
    """exp(sign 2 pi i ((f k) mod F) / F) for k = n0 .. n0 + n - 1, the phase reduced exactly in integers."""
    k = np.arange(n0, n0 + n, dtype=np.int64)
    ph = (np.int64(int(f) % int(F)) * (k % int(F))) % int(F)
    return np.exp(sign * 2j * np.pi * ph.astype(np.float64) / float(F))


def composite(n, F, offsets, ids, amps):
    """Stations fm_stereo_iq(stream_id=ids[s], amplitude=amps[s]) at +offsets[s] Hz, summed, rounded to complex64."""
    acc = np.zeros(n, dtype=np.complex128)
    for f, i, a in zip(offsets, ids, amps):
        acc += siggen.fm_stereo_iq(n, F, stream_id=i, amplitude=a).astype(np.complex128) * phasor(n, f, F, +1)
    return acc.astype(np.complex64)


def mix_down(x, f, F):
    """u_s: the capture shifted down by f, in float64, rounded to complex64."""
    return (x.astype(np.complex128) * phasor(len(x), f, F, -1)).astype(np.complex64)


def left_tone(id_):
    return 1000.0 + 10.0 * id_


def peak_hz(sig, rate):
    """Frequency of the largest FFT bin of sig (mean removed, Hann window)."""
    s = np.asarray(sig, dtype=np.float64)
    s = (s - s.mean()) * np.hanning(len(s))
    sp = np.abs(np.fft.rfft(s))
    return float(np.argmax(sp)) * rate / len(s)


def oracle_fm(u, F, lens, pilotcut, r8b=False, delay=None):
    """Oracle chain of channel u: IfResampler (FAST or the 180 dB class) -> FmDecoder (stereo), block by block."""
    r = ora.IfResampler(F, 384e3, 180.0, 0.98, True) if r8b else ora.IfResampler(F, 384e3)
    fm = ora.FmDecoder(False, delay, True, 50.0, False, 0, pilotcut)
    out, o = [], 0
    for bl in lens:
        out.append(fm.process(r.process(u[o:o + bl])))
        o += bl
    return fm, out

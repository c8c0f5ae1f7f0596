"""What the blanker is for, on the CPU oracle alone (oracle_py IfResampler + FmDecoder) with the fixture's blanker: the
audio error against the decode of the clean capture, with and without the blanker.

10 MS/s: the benchmark's station (siggen.fm_stereo_iq, amplitude 0.3, sigma 1e-3), 0.2 s, 60 bursts of two samples of
amplitude 3.0 (ten times the carrier) added at positions and phases from default_rng(21), the defaults (12 dB, G = 8,
M = 64, W = 16).  Measured here: error 1.87e-4 without, 3.38e-6 with (of a 0.437 RMS signal), ratio 55; 0.027 % of the
samples zeroed.
2.5 MS/s: two stations (chanbank_fixture.composite, ids 3 and 4, amplitudes 0.3 and 0.2 at -700 and +250 kHz), 0.2 s,
100 bursts of two samples of amplitude 5.0 (16 to 25 times the carriers), default_rng(22), G = 2, M = 16.  Measured:
1.20e-2 -> 2.47e-5 (ratio 486) and 1.07e-2 -> 4.99e-5 (ratio 215).  With G = 8 (3.2 us, more than one IF sample) the
errors only fall to 1.08e-2 and 1.01e-2: the default gate is a time.
Each assert is a ratio at one tenth of the measured one; the slack is for other seeds and block cuts."""
import numpy as np

import blanker_fixture as bf
import chanbank_fixture as cb
import siggen


def decode(u, F, pilotcut, blk):
    lens = [blk] * (len(u) // blk) + ([len(u) % blk] if len(u) % blk else [])
    return np.concatenate(cb.oracle_fm(u, F, lens, pilotcut)[1])


def rms(a):
    return float(np.sqrt(np.mean(np.abs(a) ** 2)))


def with_bursts(x, count, amplitude, seed):
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(np.arange(bf.Q, len(x) - 2), count, replace=False))
    y = x.copy()
    for p in pos:
        y[p:p + 2] += np.complex64(amplitude * np.exp(2j * np.pi * rng.random()))
    return y


def test_10_ms_station_with_the_defaults(pilotcut):
    F = 10e6
    x = siggen.fm_stereo_iq(int(0.2 * F), F).astype(np.complex64)
    y = with_bursts(x, 60, 3.0, 21)
    G, M = bf.defaults(F)
    r = bf.run(y, G, M)
    assert not bf.run(x, G, M)["trig"].any()
    a0, a1, a2 = (decode(v, F, pilotcut, 65536) for v in (x, y, r["out"]))
    without, with_ = rms(a1 - a0), rms(a2 - a0)
    print(f"10 MS/s: signal {rms(a0):.3f}, error {without:.3g} -> {with_:.3g}, ratio {without / with_:.0f}, "
          f"zeroed {r['blank'].mean():.5%}")
    assert without / with_ >= 5.5 and r["blank"].mean() < 0.001


def test_2_5_ms_two_stations_with_a_gate_of_two(pilotcut):
    F, offs = bf.F25, bf.OFFS25
    x = cb.composite(500000, F, offs, [3, 4], [0.3, 0.2])
    y = with_bursts(x, 100, 5.0, 22)
    r = bf.run(y, G=2, M=16)
    r8 = bf.run(y, G=8, M=64)
    for f, floor in zip(offs, (48.0, 21.0)):
        a0, a1, a2, a8 = (decode(cb.mix_down(v, f, F), F, pilotcut, 16384) for v in (x, y, r["out"], r8["out"]))
        without, with_ = rms(a1 - a0), rms(a2 - a0)
        print(f"2.5 MS/s, {f} Hz: error {without:.3g} -> {with_:.3g} (G = 2), ratio {without / with_:.0f}; "
              f"{rms(a8 - a0):.3g} with G = 8")
        assert without / with_ >= floor

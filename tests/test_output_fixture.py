"""tests/output_fixture.py (the output stage of include/fmradion_amd.h restated in numpy) against hand-computed cases:
rounding, saturation, non-finite samples, the gate's boundary, both level filters, skipped blocks, ring arithmetic."""
import numpy as np

import output_fixture as of


def test_half_even_rounding_at_half_an_lsb():
    """y 32767 is exactly k + 0.5 for these y (checked here): ties go to the even integer, both signs."""
    ks = np.array([0.5, 2.5, 4.5, 1.5, 3.5, -0.5, -2.5, -1.5, 16383.5, -16383.5])
    y = ks / 32767.0
    assert np.array_equal(y * 32767.0, ks)
    out, clipped, nonfinite = of.to_s16(y)
    assert out.tolist() == [0, 2, 4, 2, 4, 0, -2, -2, 16384, -16384] and clipped == 0 and nonfinite == 0
    out, _, _ = of.to_s16([0.49999 / 32767.0, 0.50001 / 32767.0, -0.50001 / 32767.0])
    assert out.tolist() == [0, 1, -1]


def test_saturation_with_counts():
    """+1.00002 -> 32767.655 -> 32768: saturated; -1.00002 -> -32768 fits; -1.00005 -> -32769: saturated."""
    out, clipped, nonfinite = of.to_s16([1.0, -1.0, 1.00002, -1.00002, -1.00005, 3.0, -3.0, 1e300])
    assert out.tolist() == [32767, -32767, 32767, -32768, -32768, 32767, -32768, 32767]
    assert clipped == 5 and nonfinite == 0
    out, clipped, nonfinite = of.to_f32([1.0, -1.0, 1.00002, -1.00002, 0.5])
    assert clipped == 2 and nonfinite == 0 and out.dtype == np.float32
    assert np.array_equal(out, np.array([1.0, -1.0, 1.00002, -1.00002, 0.5], dtype=np.float32))


def test_nan_and_inf_in_both_formats():
    y = [np.nan, np.inf, -np.inf, 0.25]
    out, clipped, nonfinite = of.to_s16(y)
    assert out.tolist() == [0, 32767, -32768, 8192] and clipped == 2 and nonfinite == 3      # 0.25 * 32767 = 8191.75
    out, clipped, nonfinite = of.to_f32(y)
    assert np.isnan(out[0]) and out[1] == np.inf and out[2] == -np.inf and out[3] == np.float32(0.25)
    assert clipped == 2 and nonfinite == 3
    # a closed gate multiplies by 0.0: Inf becomes NaN, which becomes 0 in S16 and stays NaN in F32
    recs, pcm = of.run([(0.01, np.array([np.inf, 0.5, -0.5, np.nan]))], 1, squelch_level=0.03)
    assert pcm[:, 0].tolist() == [0, 0, 0, 0] and recs["n_nonfinite"][0] == 2 and recs["n_clipped"][0] == 0
    recs, pcm = of.run([(0.01, np.array([np.inf, 0.5, -0.5]))], 1, squelch_level=0.03, fmt=of.PCM_F32)
    assert np.isnan(pcm[0, 0]) and pcm[1, 0] == 0.0 and pcm[2, 0] == 0.0 and np.signbit(pcm[2, 0])


def test_gate_is_open_at_the_level_exactly():
    lvl = float(np.float32(0.03))
    below = float(np.nextafter(np.float32(0.03), np.float32(0)))
    a = np.array([0.5, -0.25])
    recs, pcm = of.run([(lvl, a), (below, a), (0.0, a)], 1, squelch_level=lvl, gain=1.0)
    assert recs["gate_open"].tolist() == [1, 0, 0]
    assert pcm[:, 0].tolist() == [16384, -8192, 0, 0, 0, 0]
    recs, pcm = of.run([(0.0, a)], 1, squelch_level=0.0)       # the default level is never closed: 0 >= 0
    assert recs["gate_open"].tolist() == [1] and pcm[:, 0].tolist() == [8192, -4096]      # 0.25 * 32767 = 8191.75, -4095.875
    assert of.squelch_level_from_db(20.0) == 0.1 and of.squelch_level_from_db(0.0) == 1.0


def test_both_levels_over_a_block_with_if_but_no_audio_and_a_skipped_block():
    a = np.full(4, 0.5)                       # mean 0.5, rms 0.5
    blocks = [(0.4, a), (0.8, np.zeros(0)), (None, np.zeros(0)), (0.4, a)]
    recs, pcm = of.run(blocks, 2)
    assert recs["block"].tolist() == [0, 1, 3] and recs["first_frame"].tolist() == [0, 2, 2]
    assert recs["n_frames"].tolist() == [2, 0, 2] and recs["channels"].tolist() == [2, 2, 2]
    f = np.float32
    l0 = f(0.25 * float(f(0.4)))
    l1 = f(0.75 * float(l0) + 0.25 * float(f(0.8)))
    l2 = f(0.75 * float(l1) + 0.25 * float(f(0.4)))
    assert recs["if_level"].tolist() == [l0, l1, l2]
    assert abs(float(l1) - 0.275) < 1e-7 and abs(float(l2) - 0.30625) < 1e-7
    a0 = f(0.05 * 0.5)
    a2 = f(0.95 * float(a0) + 0.05 * 0.5)
    assert recs["audio_level"].tolist() == [a0, a0, a2]                   # the block without audio repeats the level
    assert recs["audio_rms"].tolist() == [0.5, 0.0, 0.5] and recs["audio_mean"].tolist() == [0.5, 0.0, 0.5]
    assert recs["gate_open"].tolist() == [1, 1, 1] and pcm.shape == (4, 2) and np.all(pcm == 8192)   # rint(0.25 * 32767 = 8191.75)
    assert len(of.run([(None, np.zeros(0))], 1)[0]) == 0


def test_meters_narrow_to_float32_before_the_gain():
    x = np.array([0.1, -0.3, 1e-50, 0.2])     # 1e-50 narrows to 0
    recs, _ = of.run([(1.0, x)], 1, gain=1.0)
    xf = x.astype(np.float32).astype(np.float64)
    assert recs["audio_mean"][0] == np.float32(xf.sum() / 4) and recs["audio_rms"][0] == np.float32(np.sqrt((xf * xf).sum() / 4))
    # more than one partial row and all four waves: within an ulp of the plain float64 sum, and reproducible
    rng = np.random.default_rng(1)
    x = rng.standard_normal(2 * 777)
    s1, s2 = of.narrowed_sums(x, 2)
    xf = x.astype(np.float32).astype(np.float64)
    assert abs(s1 - xf.sum()) <= 1e-12 * np.abs(xf).sum() and abs(s2 - (xf * xf).sum()) <= 1e-12 * (xf * xf).sum()
    assert (s1, s2) == of.narrowed_sums(x, 2)


def test_ring_overrun_arithmetic():
    assert of.ring_window(7 * 315, 1024) == (7 * 315 - 1024, 7 * 315 - 1024)
    assert of.ring_window(1000, 1024) == (0, 0)
    assert of.ring_window(3000, 1024, read=2500) == (2500, 0)
    assert of.ring_window(7, 4) == (3, 3)

"""tests/loudness_fixture.py against the standards' own figures (ITU-R BS.1770-4, EBU R 128), numpy only: the fixture is
the oracle of the GPU tests, so it is held to truths that do not come from this project."""
import numpy as np
import pytest

import loudness_fixture as lf

FS = 48000.0


def tone(n, f, dbfs, phase=0.0):
    return 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * f * np.arange(n) / FS + phase)


def stereo(left, right):
    return np.stack([left, right], axis=1).reshape(-1)


def test_997_hz_full_scale_in_one_channel_reads_minus_3_01():
    n = 8 * 4800
    lv = lf.derive(lf.records(stereo(tone(n, 997.0, 0.0), np.zeros(n)), 2, 4800))
    print(lv["momentary_lufs"], lv["integrated_lufs"])
    assert abs(lv["momentary_lufs"] + 3.01) <= 0.01 and abs(lv["integrated_lufs"] + 3.01) <= 0.01
    assert lv["momentary_windows"] == 5 and lv["short_term_lufs"] == -np.inf


def test_1_khz_at_minus_23_in_both_channels_reads_minus_23():
    n = 32 * 4800
    x = tone(n, 1000.0, -23.0)
    lv = lf.derive(lf.records(stereo(x, x), 2, 4800))
    print(lv["momentary_lufs"], lv["short_term_lufs"], lv["integrated_lufs"])
    for k in ("momentary_lufs", "momentary_max_lufs", "short_term_lufs", "short_term_max_lufs", "integrated_lufs"):
        assert abs(lv[k] + 23.0) <= 0.1, (k, lv[k])
    assert abs(lv["sample_peak_dbfs"] + 23.0) < 0.01 and lv["correlation"] == pytest.approx(1.0, abs=1e-12)


def _sections(levels_and_blocks, Q=480):
    parts, pos = [], 0
    for dbfs, blocks in levels_and_blocks:
        n = blocks * Q
        parts.append(10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * 1000.0 * (pos + np.arange(n)) / FS) if dbfs is not None
                     else np.zeros(n))
        pos += n
    x = np.concatenate(parts)
    return stereo(x, x)


def test_relative_gate_removes_the_quiet_sections():
    """20 sub-blocks at -36 dBFS, 240 at -23, 20 at -36: the quiet ones are 13 LU down and fall to the relative gate."""
    recs = lf.records(_sections([(-36.0, 20), (-23.0, 240), (-36.0, 20)]), 2, 480)
    lv = lf.derive(recs)
    print(lv["integrated_lufs"], lv["momentary_windows"], lv["gated_windows"])
    assert abs(lv["integrated_lufs"] + 23.0) <= 0.1
    assert lv["momentary_windows"] == 277 and 237 <= lv["gated_windows"] <= 243
    ungated = -0.691 + 10 * np.log10(np.mean([(r["kw_sumsq"][0] + r["kw_sumsq"][1]) / 480 for r in recs]))
    assert ungated < lv["integrated_lufs"] - 0.3


def test_absolute_gate_removes_a_section_at_minus_80():
    """A 1 kHz sine at x dBFS in both channels reads x LUFS.  A section at -72 lies 4 LU under one at -68 -- the relative
    gate (-78) would keep it --, and one at -80 lies under any gate: the absolute gate of -70 removes both."""
    loud = lf.derive(lf.records(_sections([(-68.0, 40)]), 2, 480))
    assert abs(loud["integrated_lufs"] + 68.0) <= 0.1 and loud["gated_windows"] == 37
    for quiet in (-72.0, -80.0):
        both = lf.derive(lf.records(_sections([(-68.0, 40), (quiet, 40)]), 2, 480))
        print(quiet, loud["integrated_lufs"], both["integrated_lufs"], both["gated_windows"])
        assert both["momentary_windows"] == 77 and 37 <= both["gated_windows"] <= 40
        assert abs(both["integrated_lufs"] - loud["integrated_lufs"]) <= 0.1
    only = lf.derive(lf.records(_sections([(-85.0, 40)]), 2, 480))
    assert only["integrated_lufs"] == -np.inf and only["gated_windows"] == 0 and only["momentary_windows"] == 37


def test_true_peak_of_a_quarter_rate_sine_sampled_at_45_degrees():
    n = 4 * 480
    x = np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4)
    recs = lf.records(x, 1, 480)
    print(recs["sample_peak"][:, 0], recs["true_peak"][:, 0])
    assert np.all(np.abs(recs["sample_peak"][:, 0] - np.sqrt(0.5)) < 1e-12)
    # (the first sub-block also holds the onset from the zeros in front of sample 0, which overshoots)
    assert np.all(recs["true_peak"][:, 0] >= 0.99) and np.all(np.abs(recs["true_peak"][1:, 0] - 0.9962) < 1e-4)
    assert np.all(recs["true_peak"][:, 1] == 0) and np.all(recs["sumsq"][:, 1] == 0) and np.all(recs["channels"] == 1)
    assert abs(lf.derive(recs[1:])["true_peak_dbtp"] - 20 * np.log10(0.9962)) < 0.01
    # the identity phase: the true peak never falls below the samples of six steps earlier
    y = np.random.default_rng(1).standard_normal(600)
    assert np.array_equal(np.maximum(lf.true_peak_track(y)[6:], np.abs(y[:-6])), lf.true_peak_track(y)[6:])


def test_correlation_and_side_to_mid():
    n = 8 * 480
    x = tone(n, 440.0, -10.0) + 1e-3 * np.random.default_rng(2).standard_normal(n)
    anti = lf.derive(lf.records(stereo(x, -x), 2, 480))
    assert anti["correlation"] == pytest.approx(-1.0, abs=1e-12) and anti["side_to_mid_db"] == np.inf
    same = lf.derive(lf.records(stereo(x, x), 2, 480))
    assert same["correlation"] == pytest.approx(1.0, abs=1e-12) and same["side_to_mid_db"] == -np.inf
    y = tone(n, 1234.0, -10.0)
    mixed = lf.derive(lf.records(stereo(x, y), 2, 480))
    assert abs(mixed["correlation"]) < 0.05 and abs(mixed["side_to_mid_db"]) < 0.5
    mono = lf.derive(lf.records(x, 1, 480))
    assert mono["correlation"] == 0.0 and mono["side_to_mid_db"] == 0.0


def test_silence_runs():
    """k silent sub-blocks are reported as k, as the longest run and -- at the end -- as the trailing one."""
    recs = lf.records(_sections([(-20.0, 5), (None, 7), (-20.0, 3), (-70.0, 4)]), 2, 480)
    lv = lf.derive(recs, silence_dbfs=-60.0)
    assert lv["longest_silence_blocks"] == 7 and lv["trailing_silence_blocks"] == 4
    lv = lf.derive(recs, silence_dbfs=-80.0)
    assert lv["longest_silence_blocks"] == 7 and lv["trailing_silence_blocks"] == 0
    lv = lf.derive(recs[:12])
    assert lv["longest_silence_blocks"] == 7 and lv["trailing_silence_blocks"] == 7


def test_non_finite_samples_are_counted_and_zeroed():
    n = 4 * 480
    x = tone(n, 500.0, -6.0)
    a = stereo(x, x)
    a[2 * 100] = np.nan                  # L of sample 100
    a[2 * 100 + 1] = np.inf              # R of sample 100
    a[2 * 1000] = -np.inf                # L of sample 1000, sub-block 2
    z = stereo(x, x)
    z[[200, 201, 2000]] = 0.0
    got, want = lf.records(a, 2, 480), lf.records(z, 2, 480)
    assert [int(v) for v in got["n_nonfinite"]] == [2, 0, 1, 0] and not want["n_nonfinite"].any()
    for k in ("kw_sumsq", "sumsq", "sum_lr", "sample_peak", "true_peak"):
        assert np.array_equal(got[k], want[k]), k
    assert lf.derive(got)["n_nonfinite"] == 3 and np.isfinite(got["kw_sumsq"]).all()


def test_a_gap_in_the_indices_breaks_windows_and_silence_runs():
    recs = lf.records(_sections([(-20.0, 6), (None, 8), (-20.0, 2)]), 2, 480)
    whole = lf.derive(recs)
    assert whole["momentary_windows"] == 13 and whole["longest_silence_blocks"] == 8
    cut = np.concatenate([recs[:9], recs[10:]])          # record 9, inside the silence, was dropped
    lv = lf.derive(cut)
    assert lv["momentary_windows"] == (9 - 3) + (6 - 3) and lv["longest_silence_blocks"] == 4
    assert lf.derive(cut[:12])["trailing_silence_blocks"] == 3
    # a run shorter than four records on either side of a gap gives no window at all
    assert lf.derive(np.concatenate([recs[:3], recs[4:7]]))["momentary_windows"] == 0
    assert lf.derive(np.concatenate([recs[:3], recs[4:7]]))["integrated_lufs"] == -np.inf


def test_kweight_is_the_recurrence_and_the_record_type_is_the_header_s_size():
    x = np.zeros(8)
    x[0] = 1.0
    h = lf.kweight(x)
    b0, b1, b2, a1, a2 = lf.STAGES[0]
    assert h[0] == b0 and h[1] == pytest.approx(b1 - a1 * b0 - 2.0 * b0 + 1.99004745483398 * b0, rel=1e-12)
    assert lf.RECORD.itemsize == 104

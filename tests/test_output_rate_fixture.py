"""tests/output_rate_fixture.py (the numpy restatement of fmr_set_output_rate's definition) held to properties that follow
from the definition and the filter's specification, with the library's own taps (fmr_output_rate_taps is host only)."""
import importlib

import numpy as np
import pytest

import output_fixture as of
import output_rate_fixture as orf

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def taps():
    fmr.build_library()
    got = {}

    def get(rate):
        if rate not in got:
            got[rate] = fmr.output_rate_taps(rate)
        return got[rate]
    return get


def one_block(x):
    return [(1.0, np.asarray(x, dtype=np.float64))]


def settle(L, M, T):
    return -(-T * L // M) + 2


@pytest.mark.parametrize("rate", [16000, 44100])
def test_count_law(taps, rate):
    h, L, M, T = taps(rate)
    assert (L, M) == orf.geometry(rate)
    x = np.random.default_rng(1).standard_normal(5 * M + 8)
    for F in (0, 1, M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1, 5 * M + 7):
        _, pcm, _, _ = orf.run(one_block(x[:F]), 1, fmt=of.PCM_F32, L=L, M=M, T=T, h=h)
        assert len(pcm) == -(-F * L // M) == orf.n_out(F, L, M), (F, len(pcm))


@pytest.mark.parametrize("rate,channels,mono", [(8000, 2, False), (44100, 1, False), (32000, 2, True)])
def test_one_block_or_many(taps, rate, channels, mono):
    h, L, M, T = taps(rate)
    x = np.random.default_rng(2).standard_normal(1500 * channels) * 0.3
    cuts = np.array([0, 1, 1, 8, 308, 309, 1100, 1500]) * channels       # (a block with IF samples and no audio among them)
    many = [(0.5, x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    many.insert(3, (None, np.zeros(0)))
    for fmt in (of.PCM_S16, of.PCM_F32):
        kw = dict(fmt=fmt, L=L, M=M, T=T, h=h, mono=mono)
        r1, p1, c1, n1 = orf.run(one_block(x), channels, **kw)
        r2, p2, c2, n2 = orf.run(many, channels, **kw)
        assert p1.tobytes() == p2.tobytes() and (c1, n1) == (c2, n2) and len(r1) == 1 and len(r2) == 7
        assert p1.shape == (orf.n_out(1500, L, M), 1 if mono else channels)


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 32000, 44100])
def test_pass_band_tone_is_the_tone_delayed(taps, rate):
    """1 kHz in, against the same tone delayed by delay_frames: within 1.2e-4 of the amplitude (+-0.001 dB) once the filter
    is full."""
    h, L, M, T = taps(rate)
    s0 = settle(L, M, T)
    F = (s0 + 200) * M // L + 1
    A, f = 0.8, 1000.0
    x = A * np.sin(2 * np.pi * f * np.arange(F) / 48000.0)
    _, pcm, c, n = orf.run(one_block(x), 1, gain=1.0, fmt=of.PCM_F32, L=L, M=M, T=T, h=h)
    delay = (T * L - 1) / (2.0 * M)
    m = np.arange(len(pcm))
    want = A * np.sin(2 * np.pi * f * (m - delay) / rate)
    err = np.abs(pcm[s0:, 0] - want[s0:]).max() / A
    print(rate, "worst deviation from the delayed tone / amplitude:", err)
    assert len(pcm) - s0 >= 200 and err <= 1.2e-4 and (c, n) == (0, 0)


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 32000, 44100])
def test_stop_band_tone_is_100_db_down(taps, rate):
    h, L, M, T = taps(rate)
    s0 = settle(L, M, T)
    F = (s0 + 400) * M // L + 1
    f = 1.05 * rate / 2 + 500.0
    assert rate / 2 < f < 24000
    x = np.sin(2 * np.pi * f * np.arange(F) / 48000.0)
    _, pcm, _, _ = orf.run(one_block(x), 1, gain=1.0, fmt=of.PCM_F32, L=L, M=M, T=T, h=h)
    peak = np.abs(pcm[s0:, 0]).max()
    print(rate, "stop-band tone at", f, "Hz:", 20 * np.log10(peak), "dB")
    assert len(pcm) - s0 >= 400 and peak <= 1e-5


@pytest.mark.parametrize("rate,fmt", [(8000, of.PCM_S16), (44100, of.PCM_F32)])
def test_a_closing_gate_rings_out_over_T_frames(taps, rate, fmt):
    h, L, M, T = taps(rate)
    j0 = 700
    F = j0 + T + 120 * M // L + M
    x = 0.5 * np.sin(2 * np.pi * 997.0 * np.arange(F) / 48000.0) + 0.25
    blocks = [(0.3, x[:j0]), (0.003, x[j0:])]
    recs, pcm, _, _ = orf.run(blocks, 1, squelch_level=0.03, gain=1.0, fmt=fmt, L=L, M=M, T=T, h=h)
    assert recs["gate_open"].tolist() == [1, 0]
    q = (np.arange(len(pcm)) * M) // L
    ringing = (q >= j0) & (q - (T - 1) < j0)
    silent = q - (T - 1) >= j0
    assert silent.sum() > 100 and pcm[silent].tobytes() == bytes(pcm[silent].nbytes)      # exactly +0
    assert np.count_nonzero(pcm[ringing]) > 0.25 * ringing.sum() and ringing.sum() <= T


@pytest.mark.parametrize("rate", [16000, 44100])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_frame_reaches_at_most_T_ring_frames(taps, rate, bad):
    h, L, M, T = taps(rate)
    j0 = 1234
    F = j0 + T + 200
    x = 0.1 * np.random.default_rng(3).standard_normal(F)
    x[j0] = bad
    q = (np.arange(orf.n_out(F, L, M)) * M) // L
    hit = (q >= j0) & (q - (T - 1) <= j0)
    n_hit = int(hit.sum())
    assert 0 < n_hit <= T
    for fmt in (of.PCM_S16, of.PCM_F32):
        _, pcm, c, n = orf.run(one_block(x), 1, gain=1.0, fmt=fmt, L=L, M=M, T=T, h=h)
        assert n == n_hit and c == (0 if np.isnan(bad) else n_hit), (fmt, c, n, n_hit)
        if fmt == of.PCM_F32:
            assert np.array_equal(~np.isfinite(pcm[:, 0]), hit)
        elif np.isnan(bad):
            assert not pcm[hit].any()
        else:
            assert set(np.unique(pcm[hit]).tolist()) <= {-32768, 32767} and np.all(np.abs(pcm[~hit].astype(np.int32)) < 32767)


@pytest.mark.parametrize("rate", [48000, 16000])
def test_mono_downmix_of_opposite_channels_is_zero(taps, rate):
    h, L, M, T = taps(rate)
    xl = np.random.default_rng(4).standard_normal(3000) * 0.4
    x = np.stack([xl, -xl], axis=1).reshape(-1)
    _, pcm, c, n = orf.run(one_block(x), 2, gain=1.0, fmt=of.PCM_F32, L=L, M=M, T=T, h=h, mono=True)
    assert pcm.shape == (orf.n_out(3000, L, M), 1) and not pcm.any() and (c, n) == (0, 0)
    _, st, _, _ = orf.run(one_block(x), 2, gain=1.0, fmt=of.PCM_F32, L=L, M=M, T=T, h=h, mono=False)
    assert st.shape[1] == 2 and st.any()

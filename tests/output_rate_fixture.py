"""The output stage's rate converter (include/fmradion_amd.h, fmr_set_output_rate) restated in numpy on top of
tests/output_fixture.py: z = x g (downmixed first with mono), then ring frame m = sum over k ascending of
h[k L + p] z[q - k] with q = floor(m M / L), p = (m M) mod L, every product and sum rounded by itself.  It sees the whole
stream at once and has no knowledge of calls; the block records are output_fixture.run's, unchanged."""
import numpy as np

import output_fixture as of


def geometry(rate):
    """(L, M) of rate / 48000 in lowest terms."""
    g = int(np.gcd(int(rate), 48000))
    return int(rate) // g, 48000 // g


def n_out(frames, L, M):
    """Ring frames after `frames` decoder frames: ceil(frames L / M)."""
    return -(-int(frames) * L // M)


def gated(blocks, channels, squelch_level, gain, mono):
    """z [F, ring channels] of the whole stream."""
    och = 1 if (mono and channels == 2) else channels
    z = [np.zeros((0, och))]
    for if_rms, audio in blocks:
        if if_rms is None:
            continue
        g = gain if float(np.float32(if_rms)) >= squelch_level else 0.0
        x = np.asarray(audio, dtype=np.float64).reshape(-1, channels)
        with np.errstate(invalid="ignore", over="ignore"):
            if och != channels:
                x = ((x[:, 0] + x[:, 1]) * 0.5).reshape(-1, 1)
            z.append(x * g)
    return np.concatenate(z)


def convolve(z, L, M, T, h):
    """acc [ceil(F L / M), channels]: the serial sum over k, vectorised over the ring frames only."""
    m = np.arange(n_out(len(z), L, M), dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    if T == 1:
        assert L == 1 and M == 1
        return z[q]
    h = np.asarray(h, dtype=np.float64)
    assert len(h) == T * L
    zp = np.concatenate([np.zeros((T - 1, z.shape[1])), z])       # z[j] = +0.0 for j < 0
    acc = np.zeros((len(m), z.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(T):
            acc = acc + h[k * L + p][:, None] * zp[q - k + T - 1]
    return acc


def run(blocks, channels, squelch_level=0.0, gain=0.5, fmt=of.PCM_S16, L=1, M=1, T=1, h=(1.0,), mono=False):
    """blocks as output_fixture.run takes them.  Returns (records, pcm [ring frames, ring channels], pcm_clipped,
    pcm_nonfinite)."""
    records, _ = of.run(blocks, channels, squelch_level, gain, fmt)
    acc = convolve(gated(blocks, channels, squelch_level, gain, mono), L, M, T, h)
    pcm, clipped, nonfinite = (of.to_s16 if fmt == of.PCM_S16 else of.to_f32)(acc)
    return records, pcm, clipped, nonfinite

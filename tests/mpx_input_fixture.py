"""The MPX input (include/fmradion_amd.h, fmr_create_mpx_decoder) restated in numpy float64, from the header's text: frame i
gives u[i] (S16: v / 32767.0; F32: (double)v, non-finite -> +0.0 and counted), z = u g' with g' = gain (M / L), and MPX
sample j = sum over k ascending, while p + k M < T L, of h[p + k M] z[i0 - k] with i0 = floor(j L / M), p = j L - i0 M,
every product and sum rounded by itself, then rounded to float32.  It sees the whole stream at once and has no knowledge of
calls.  Taps come from fmr.mpx_output_taps (host only).  Not a test module."""
import importlib

import numpy as np

MPX_RATE = 384000
PCM_S16, PCM_F32 = 0, 1

_taps = {}


def taps(rate):
    """(h, L, M, T) of the library's prototype at `rate`, computed once per rate."""
    rate = int(rate) or MPX_RATE
    if rate not in _taps:
        fmr = importlib.import_module("airspy-fmradion_amd")
        fmr.build_library()
        _taps[rate] = fmr.mpx_output_taps(rate)
    return _taps[rate]


def geometry(rate):
    """(L, M, T, K, delay_samples): rate / 384000 = L / M in lowest terms, taps per phase, terms per MPX sample
    ceil(T L / M), group delay (T L - 1) / (2 L) MPX samples; 1, 1, 1, 1, 0.0 at 384000."""
    h, L, M, T = taps(rate)
    if T == 1:
        return 1, 1, 1, 1, 0.0
    return L, M, T, -(-T * L // M), (T * L - 1) / (2.0 * L)


def n_out(frames, L, M):
    """MPX samples after `frames` frames: ceil(frames M / L)."""
    return -(-int(frames) * M // L)


def block_counts(block_len, L, M, frames_before=0):
    """MPX samples of each of consecutive blocks of frames: the difference of the count law across the block."""
    edges = np.concatenate([[0], np.cumsum(np.asarray(block_len, dtype=np.int64))]) + int(frames_before)
    cnt = np.array([n_out(f, L, M) for f in edges], dtype=np.int64)
    return np.diff(cnt)


def convert(pcm):
    """(u float64, non-finite count) of int16 or float32 frames."""
    pcm = np.asarray(pcm)
    if pcm.dtype == np.int16:
        return pcm.astype(np.float64) / 32767.0, 0
    assert pcm.dtype == np.float32, pcm.dtype
    u = pcm.astype(np.float64)
    bad = ~np.isfinite(u)
    u[bad] = 0.0
    return u, int(bad.sum())


def resample(z, L, M, T, h):
    """acc [ceil(F M / L)] float64: the serial sum over k ascending, vectorised over the MPX samples only."""
    j = np.arange(n_out(len(z), L, M), dtype=np.int64)
    i0, p = (j * L) // M, (j * L) % M
    h = np.asarray(h, dtype=np.float64)
    assert len(h) == T * L
    K = -(-T * L // M)
    zp = np.concatenate([np.zeros(K), z])           # z[i] = +0.0 for i < 0
    acc = np.zeros(len(j))
    for k in range(K):
        idx = p + k * M
        live = idx < T * L                          # the sample's loop has ended where this is False
        term = h[np.minimum(idx, T * L - 1)] * zp[i0 - k + K]
        acc = np.where(live, acc + term, acc)
    return acc


def run(pcm, rate=192000, gain=2.0):
    """pcm: one stream's frames (int16 or float32).  Returns (x float32 [MPX samples], nonfinite_in)."""
    pcm = np.asarray(pcm)
    assert pcm.ndim == 1
    h, L, M, T = taps(rate)
    u, nf = convert(pcm)
    if T == 1:
        return (u * float(gain)).astype(np.float32), nf
    g = float(gain) * (float(M) / float(L))
    with np.errstate(over="ignore"):
        return resample(u * g, L, M, T, h).astype(np.float32), nf


def info(rate, gain, frames, fmt=PCM_S16, nonfinite=0):
    """What fmr_mpx_input_info says after `frames` frames."""
    L, M, T, K, delay = geometry(rate)
    return {"format": fmt, "rate": int(rate) or MPX_RATE, "L": L, "M": M, "taps_per_phase": T, "taps_per_sample": K,
            "delay_samples": delay, "full_scale_hz": 75000.0 * gain, "frames_in": frames, "samples_out": n_out(frames, L, M),
            "nonfinite_in": nonfinite}

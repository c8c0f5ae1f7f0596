"""The MPX output (include/fmradion_amd.h, fmr_enable_mpx_output) restated in numpy float64: z = (double)x gain, then ring
frame m = sum over k ascending of h[k L + p] z[q - k] with q = floor(m M / L), p = (m M) mod L, every product and sum
rounded by itself, converted by the output stage's PCM rules (tests/output_fixture.py: to_s16, to_f32).  It sees the whole
stream at once and has no knowledge of calls.  Taps come from fmr.mpx_output_taps (host only).  Not a test module."""
import importlib

import numpy as np

import output_fixture as of

MPX_RATE = 384000
PCM_S16, PCM_F32 = of.PCM_S16, of.PCM_F32

_taps = {}


def taps(rate):
    """(h, L, M, T) of the library, computed once per rate."""
    rate = int(rate) or MPX_RATE
    if rate not in _taps:
        fmr = importlib.import_module("airspy-fmradion_amd")
        fmr.build_library()
        _taps[rate] = fmr.mpx_output_taps(rate)
    return _taps[rate]


def geometry(rate):
    """(L, M) of rate / 384000 in lowest terms."""
    rate = int(rate) or MPX_RATE
    g = int(np.gcd(rate, MPX_RATE))
    return rate // g, MPX_RATE // g


def n_out(samples, L, M):
    """Ring frames after `samples` MPX samples: ceil(samples L / M)."""
    return -(-int(samples) * L // M)


def convolve(z, L, M, T, h):
    """acc [ceil(F L / M)]: the serial sum over k ascending, vectorised over the ring frames only."""
    m = np.arange(n_out(len(z), L, M), dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    if T == 1:
        assert L == 1 and M == 1
        return z[q]
    h = np.asarray(h, dtype=np.float64)
    assert len(h) == T * L
    zp = np.concatenate([np.zeros(T - 1), z])       # z[j] = +0.0 for j < 0
    acc = np.zeros(len(m))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(T):
            acc = acc + h[k * L + p] * zp[q - k + T - 1]
    return acc


def run(x, rate=192000, gain=0.5, fmt=PCM_S16):
    """x: the stream's MPX samples (float32 values).  Returns (pcm [ring frames], pcm_clipped, pcm_nonfinite)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    h, L, M, T = taps(rate)
    with np.errstate(invalid="ignore", over="ignore"):
        z = x.astype(np.float64) * float(gain)
    return (of.to_s16 if fmt == PCM_S16 else of.to_f32)(convolve(z, L, M, T, h))


def info(rate, gain, samples):
    """What fmr_mpx_output_info says of the geometry after `samples` MPX samples."""
    h, L, M, T = taps(rate)
    return {"rate": int(rate) or MPX_RATE, "L": L, "M": M, "taps_per_phase": T,
            "delay_frames": (T * L - 1) / (2.0 * M) if T > 1 else 0.0, "full_scale_hz": 75000.0 / gain, "samples_in": samples}

"""float64 oracle of the band spectrum's waterfall (fmr_spectrum_create_waterfall / fmr_spectrum_read_waterfall).

Built on spectrum_fixture: line l of a row is made of the segments [l R, (l + 1) R) by absolute segment index; a segment
with a non-finite sample is skipped; MEAN = sum over the counted segments / their number, PEAK = their maximum, all
zeros when none is counted; density scaling 1 / (F sum w^2), fftshift order.
"""
import numpy as np

import spectrum_fixture as sf

MEAN, PEAK = 0, 1


def lines(x, N, H, kind, F, R, which, line_lo=0, line_hi=None):
    """(lines float64 [n, N], counted int [n]) of the complete lines line_lo .. line_hi - 1 of row x."""
    nseg = (len(x) - N) // H + 1 if len(x) >= N else 0
    done = nseg // R
    line_hi = done if line_hi is None else min(line_hi, done)
    n = max(0, line_hi - line_lo)
    out = np.zeros((n, N))
    cnt = np.zeros(n, dtype=np.int64)
    scale = 1.0 / (F * np.sum(sf.window(kind, N) ** 2))
    for k in range(n):
        l = line_lo + k
        P, ok = sf.segment_powers(x[l * R * H:((l + 1) * R - 1) * H + N], N, H, kind, 0, R)   # the line's own samples
        Pc = P[ok]
        cnt[k] = len(Pc)
        if len(Pc):
            v = Pc.mean(axis=0) if which == MEAN else Pc.max(axis=0)
            out[k] = np.fft.fftshift(v) * scale
    return out, cnt


def close(got, ref, rel=1e-4, absfrac=1e-12):
    """spectrum_fixture.close, line by line: (all ok, worst ratio)."""
    assert len(got) == len(ref), (len(got), len(ref))
    ok, worst = True, 0.0
    for g, r in zip(got, ref):
        if not np.any(r):
            o, w = bool(not np.any(g)), 0.0
        else:
            o, w = sf.close(g.astype(np.float64), r, rel, absfrac)
        ok, worst = ok and o, max(worst, w)
    return ok, worst

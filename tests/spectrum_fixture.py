"""float64 oracle of the band spectrum (fmr_spectrum_*) and a numpy restatement of the station finder (fmr_find_stations).

Welch over the same segments the library defines: segment j of a row covers the absolute samples [j H, j H + N) of
the concatenated input, periodic windows from their formulas, density scaling |sum w x e^-..|^2 / (F sum w^2), output in
fftshift order (element k = bin (k - N/2) F / N Hz).  No scipy.
"""
import numpy as np

HANN, RECT, BLACKMAN_HARRIS = 0, 1, 2


def window(kind, N):
    """Periodic (DFT-even) window in float64, rounded once to float32 and back (what the library holds)."""
    x = 2.0 * np.pi * np.arange(N) / N
    if kind == HANN:
        w = 0.5 - 0.5 * np.cos(x)
    elif kind == BLACKMAN_HARRIS:
        w = 0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)
    else:
        w = np.ones(N)
    return w.astype(np.float32).astype(np.float64)


def segment_powers(x, N, H, kind, seg_lo=0, seg_hi=None):
    """|FFT|^2 (natural bin order, float64) of segments seg_lo .. seg_hi - 1 of row x, and their finite flags."""
    x = np.asarray(x).astype(np.complex128)
    nseg = (len(x) - N) // H + 1 if len(x) >= N else 0
    seg_hi = nseg if seg_hi is None else min(seg_hi, nseg)
    w = window(kind, N)
    idx = np.arange(seg_lo, seg_hi)[:, None] * H + np.arange(N)[None, :]
    segs = x[idx] if seg_hi > seg_lo else np.zeros((0, N), np.complex128)
    ok = np.all(np.isfinite(segs), axis=1)
    segs = np.where(ok[:, None], segs, 0)
    P = np.abs(np.fft.fft(segs * w, axis=1)) ** 2
    return P, ok


def welch(x, N, H, kind, F, seg_lo=0, seg_hi=None):
    """(mean PSD, peak hold, counted, skipped) of one row over segments [seg_lo, seg_hi), library layout and scaling."""
    P, ok = segment_powers(x, N, H, kind, seg_lo, seg_hi)
    scale = 1.0 / (F * np.sum(window(kind, N) ** 2))
    Pc = P[ok]
    if len(Pc) == 0:
        return np.zeros(N), np.zeros(N), 0, int((~ok).sum())
    mean = np.fft.fftshift(Pc.mean(axis=0)) * scale
    peak = np.fft.fftshift(Pc.max(axis=0)) * scale
    return mean, peak, int(ok.sum()), int((~ok).sum())


def close(got, ref, rel=1e-4, absfrac=1e-12):
    """The per-bin bound of the GPU tests: |got - ref| <= rel ref + absfrac max ref; returns (ok, worst ratio)."""
    bound = rel * ref + absfrac * np.max(ref)
    r = np.abs(got - ref) / np.maximum(bound, 1e-300)
    return bool(np.all(np.abs(got - ref) <= bound)), float(np.max(r))


def find_stations(psd, F, raster_hz, raster_offset_hz=0, bandwidth_hz=200000, max_abs_offset_hz=0, threshold_db=10.0,
                  floor_percentile=0.0):
    """The finder's algorithm (include/fmradion_amd.h, fmr_find_stations) restated: list of (offset, level_db, snr_db,
    centroid_hz) in ascending offset order."""
    psd = np.asarray(psd, dtype=np.float64)
    N = len(psd)
    df = F / N
    p = 20.0 if floor_percentile == 0 else floor_percentile
    mab = float(max_abs_offset_hz) if max_abs_offset_hz != 0 else (F - 384000.0) / 2.0
    fk = (np.arange(N) - N // 2).astype(np.float64) * df
    inb = np.sort(psd[np.abs(fk) <= mab])
    if len(inb) == 0:
        return []
    floor = inb[int(np.floor(p / 100.0 * (len(inb) - 1)))]
    cands = []
    j = int(np.ceil((-mab - raster_offset_hz) / raster_hz))
    while True:
        f = raster_offset_hz + j * float(raster_hz)
        j += 1
        if f > mab:
            break
        if abs(f) > mab:
            continue
        sel = np.abs(fk - f) <= bandwidth_hz / 2.0
        B = float(np.sum(psd[sel] * df))
        cen = float(np.sum(fk[sel] * psd[sel]) / np.sum(psd[sel])) if sel.any() else float("nan")
        cands.append((f, B, floor * int(sel.sum()) * df, cen))
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, (f, B, noise, cen) in enumerate(cands):
            snr = 10 * np.log10(B / noise)
            if not snr >= threshold_db:
                continue
            keep = True
            for q, (f2, B2, _, _) in enumerate(cands):
                d = abs(f2 - f)
                if q == i or not (0 < d < bandwidth_hz):
                    continue
                if B2 > B or (B2 == B and f2 < f):
                    keep = False
                    break
            if keep:
                out.append((int(f), 10 * np.log10(B), float(snr), cen))
    return out

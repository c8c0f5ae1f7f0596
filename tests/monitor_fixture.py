"""float64 restatement of the modulation monitor (fmr_enable_monitor / fmr_monitor_read / fmr_monitor_derive,
include/fmradion_amd.h) in numpy.  The input is the float32 MPX of one stream, whole; the output is what the library
reports for it, whatever the cut into calls was.  No scipy.
"""
import numpy as np

F, N, H, PSD_BINS = 384000.0, 1024, 512, 513

RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("n_finite", np.uint32),
                   ("n_nonfinite", np.uint32), ("segments", np.uint32), ("segments_skipped", np.uint32),
                   ("min", np.float32), ("max", np.float32), ("sum", np.float64), ("sumsq", np.float64)])


def window():
    """Periodic Hann in float64, rounded once to float32 and back (what the library holds)."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    return w.astype(np.float32).astype(np.float64)


def n_complete(n_samples, M):
    """Records complete after n_samples: record i needs the absolute sample (i + 1) M + 511."""
    return max(0, (int(n_samples) - H) // int(M))


def bins_of(x, B, R):
    """The histogram's bin of every (finite) float32 sample: unfused float32 arithmetic."""
    x = np.asarray(x, dtype=np.float32)
    rf = np.float32(R)
    scale = np.float32(B / (2.0 * R))
    with np.errstate(over="ignore"):
        t = np.floor((x + rf) * scale)
    return np.clip(t, 0, B - 1).astype(np.int64)


def segment_psd(x, seg_lo, seg_hi):
    """One-sided density P_j[k] (float64, [n, 513]) of the segments seg_lo .. seg_hi - 1 and their finite flags."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    w = window()
    idx = np.arange(seg_lo, seg_hi)[:, None] * H + np.arange(N)[None, :]
    segs = x[idx]
    ok = np.all(np.isfinite(segs), axis=1)
    X = np.fft.rfft(np.where(ok[:, None], segs, 0.0) * w, axis=1)
    c = np.full(PSD_BINS, 2.0)
    c[0] = c[-1] = 1.0
    return c * np.abs(X) ** 2 / (F * np.sum(w * w)), ok


def records(x, M=384000, B=256, R=2.0):
    """(records RECORD [n], hist uint32 [n, B], psd float64 [n, 513]) of every complete record of the float32 MPX x."""
    x = np.asarray(x, dtype=np.float32)
    n = n_complete(len(x), M)
    recs = np.zeros(n, dtype=RECORD)
    hist = np.zeros((n, B), dtype=np.uint32)
    psd = np.zeros((n, PSD_BINS), dtype=np.float64)
    spr = M // H
    for i in range(n):
        seg = x[i * M:(i + 1) * M]
        fin = np.isfinite(seg)
        v = seg[fin]
        r = recs[i]
        r["index"], r["first_sample"] = i, i * M
        r["n_finite"], r["n_nonfinite"] = len(v), len(seg) - len(v)
        if len(v):
            r["min"], r["max"] = v.min(), v.max()
            v64 = v.astype(np.float64)
            r["sum"], r["sumsq"] = v64.sum(), (v64 * v64).sum()
            hist[i] = np.bincount(bins_of(v, B, R), minlength=B).astype(np.uint32)
        P, ok = segment_psd(x, i * spr, (i + 1) * spr)
        r["segments"], r["segments_skipped"] = int(ok.sum()), int((~ok).sum())
        if ok.any():
            psd[i] = P[ok].mean(axis=0)
    return recs, hist, psd


def band(psd, lo, hi):
    """B(lo, hi): sum of psd[k] F / N over lo <= k F / N <= hi."""
    f = np.arange(PSD_BINS) * (F / N)
    sel = (f >= lo) & (f <= hi)
    return float(np.sum(psd[sel]) * (F / N))


def derive(recs, psd):
    """fmr_monitor_derive restated: the levels of the pooled records, as a dict."""
    recs = np.asarray(recs, dtype=RECORD)
    psd = np.asarray(psd, dtype=np.float64).reshape(len(recs), PSD_BINS)
    nf = int(recs["n_finite"].astype(np.uint64).sum())
    seg = int(recs["segments"].astype(np.uint64).sum())
    p = (recs["segments"].astype(np.float64)[:, None] * psd).sum(axis=0) / seg if seg else np.zeros(PSD_BINS)
    mean = float(recs["sum"].sum()) / nf if nf else 0.0
    var = float(recs["sumsq"].sum()) / nf - mean * mean if nf else 0.0
    has = recs["n_finite"] > 0
    mn = float(recs["min"][has].min()) if has.any() else 0.0
    mx = float(recs["max"][has].max()) if has.any() else 0.0
    f = np.arange(PSD_BINS) * (F / N)
    hf = (f >= 100000.0) & (f <= 150000.0)
    return {
        "tuning_offset_hz": 75000.0 * mean,
        "peak_deviation_hz": 75000.0 * max(mx - mean, mean - mn) if nf else 0.0,
        "rms": float(np.sqrt(var)) if var > 0 else 0.0,
        "mpx_power_dbr": 10.0 * np.log10(2.0 * (75.0 / 19.0) ** 2 * var) if var > 0 else -np.inf,
        "pilot_deviation_hz": 75000.0 * np.sqrt(2.0 * band(p, 17875.0, 20125.0)),
        "rds_deviation_hz": 75000.0 * np.sqrt(2.0 * band(p, 54600.0, 59400.0)),
        "hf_noise_density": float(np.mean(p[hf])),
        "n_finite": nf,
        "segments": seg,
    }

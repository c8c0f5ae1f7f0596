"""float64 restatement of the RF monitor (fmr_enable_rf_monitor / fmr_rf_monitor_read / fmr_rf_monitor_derive,
include/fmradion_amd.h) in numpy.  The input is p, the float32 squared magnitude of one stream's IF samples, whole
(power() makes it from complex64 IF samples with the library's rounding); the output is what the library reports for
it, whatever the cut into calls was.  The spectral part is the modulation monitor's (tests/monitor_fixture.py).  No scipy.
"""
import numpy as np

import monitor_fixture as mf

F, N, H, PSD_BINS, HIST_BINS, BIN_BASE = mf.F, mf.N, mf.H, mf.PSD_BINS, 384, 696

RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("n_finite", np.uint32),
                   ("n_nonfinite", np.uint32), ("segments", np.uint32), ("segments_skipped", np.uint32),
                   ("p_min", np.float32), ("p_max", np.float32), ("m2", np.float64), ("m4", np.float64)])

n_complete = mf.n_complete


def power(iq):
    """p = fl(fl(re re) + fl(im im)) of complex64 IF samples, unfused float32."""
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    with np.errstate(over="ignore", invalid="ignore"):
        return iq.real * iq.real + iq.imag * iq.imag


def bins_of(p):
    """The histogram's bin of every float32 p: u = bits >> 20, bin = clamp(u - 696, 0, 383)."""
    u = (np.ascontiguousarray(p, dtype=np.float32).view(np.uint32) >> np.uint32(20)).astype(np.int64)
    return np.clip(u - BIN_BASE, 0, HIST_BINS - 1)


def bin_edge(b):
    """Lower edge of bin b: 2^((u >> 3) - 127) (1 + (u & 7) / 8) with u = b + 696."""
    u = int(b) + BIN_BASE
    return float(np.ldexp(1.0 + (u & 7) / 8.0, (u >> 3) - 127))


def records(p, M=38400):
    """(records RECORD [n], hist uint32 [n, 384], psd float64 [n, 513]) of every complete record of the float32 p."""
    p = np.asarray(p, dtype=np.float32)
    n = n_complete(len(p), M)
    recs = np.zeros(n, dtype=RECORD)
    hist = np.zeros((n, HIST_BINS), dtype=np.uint32)
    psd = np.zeros((n, PSD_BINS), dtype=np.float64)
    spr = M // H
    for i in range(n):
        seg = p[i * M:(i + 1) * M]
        v = seg[np.isfinite(seg)]
        r = recs[i]
        r["index"], r["first_sample"] = i, i * M
        r["n_finite"], r["n_nonfinite"] = len(v), len(seg) - len(v)
        if len(v):
            r["p_min"], r["p_max"] = v.min(), v.max()
            v64 = v.astype(np.float64)
            r["m2"], r["m4"] = v64.sum(), (v64 * v64).sum()
            hist[i] = np.bincount(bins_of(v), minlength=HIST_BINS).astype(np.uint32)
        P, ok = mf.segment_psd(p, i * spr, (i + 1) * spr)
        r["segments"], r["segments_skipped"] = int(ok.sum()), int((~ok).sum())
        if ok.any():
            psd[i] = P[ok].mean(axis=0)
    return recs, hist, psd


def _db(x):
    return 10.0 * np.log10(x) if x > 0 else -np.inf


def derive(recs, hist, psd):
    """fmr_rf_monitor_derive restated: the levels of the pooled records, as a dict."""
    recs = np.asarray(recs, dtype=RECORD)
    hist = np.asarray(hist, dtype=np.uint32).reshape(len(recs), HIST_BINS)
    psd = np.asarray(psd, dtype=np.float64).reshape(len(recs), PSD_BINS)
    nf = int(recs["n_finite"].astype(np.uint64).sum())
    seg = int(recs["segments"].astype(np.uint64).sum())
    P = (recs["segments"].astype(np.float64)[:, None] * psd).sum(axis=0) / seg if seg else np.zeros(PSD_BINS)
    M2 = float(recs["m2"].sum()) / nf if nf else 0.0
    M4 = float(recs["m4"].sum()) / nf if nf else 0.0
    d = 2.0 * M2 * M2 - M4
    S = float(np.sqrt(d)) if d > 0 else 0.0
    Nn = M2 - S
    f = np.arange(PSD_BINS) * (F / N)
    floor = float(np.mean(P[(f >= 100000.0) & (f <= 150000.0)]))
    ref = 4.0 * M2 * M2
    cum = np.cumsum(hist.astype(np.uint64).sum(axis=0).astype(object))

    def pct(q):
        if nf == 0:
            return -np.inf
        for b in range(HIST_BINS):
            if 100 * int(cum[b]) >= q * nf:
                return 10.0 * np.log10(bin_edge(b))
        return -np.inf

    def rel(x):
        return _db(x / ref) if M2 > 0 else -np.inf

    return {
        "level_dbfs": _db(M2),
        "carrier_dbfs": _db(S),
        "noise_dbfs": _db(Nn),
        "cn_db": (10.0 * np.log10(S / Nn) if Nn > 0 else np.inf) if S > 0 else -np.inf,
        "am_rms": float(np.sqrt(max(M4 / (M2 * M2) - 1.0, 0.0))) / 2.0 if M2 > 0 else 0.0,
        "am_audio_db": rel(mf.band(P, 750.0, 15000.0)),
        "am_pilot_db": rel(mf.band(P, 18250.0, 19750.0)),
        "am_floor_dbc_hz": rel(floor),
        "p10_dbfs": pct(10), "p50_dbfs": pct(50), "p90_dbfs": pct(90),
        "n_finite": nf,
        "segments": seg,
    }


def fm_iq(n, amplitude=0.3, am=0.0, f_am=3000.0, noise=0.0, seed=0, dev=60000.0, f_mod=1000.0):
    """A(1 + am sin 2 pi f_am t) exp(j phi(t)) + complex Gaussian noise of total power `noise`, complex64: FM of a tone of
    f_mod Hz at a peak deviation of dev Hz."""
    t = np.arange(n, dtype=np.float64) / F
    phi = -(dev / f_mod) * np.cos(2 * np.pi * f_mod * t)
    x = amplitude * (1.0 + am * np.sin(2 * np.pi * f_am * t)) * np.exp(1j * phi)
    if noise > 0:
        rng = np.random.default_rng(seed)
        x = x + np.sqrt(noise / 2.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)

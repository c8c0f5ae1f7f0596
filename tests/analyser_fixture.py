"""The audio analyser's definitions (include/fmradion_amd.h, fmr_enable_analyser / fmr_analyser_read /
fmr_analyser_derive) restated in float64 numpy: the Blackman-Harris segments, the three rows of a record scaled to power,
and the tone / THD / THD+N / SINAD / noise figures derived from them.  The GPU tests run it on the audio a chain
returned; the CPU tests hold it to analytic truth."""
import math

import numpy as np

RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("segments", np.uint32), ("skipped", np.uint32),
                   ("n_nonfinite", np.uint32), ("channels", np.uint32), ("fft_size", np.uint32),
                   ("interval_samples", np.uint32), ("sum", np.float64, 2), ("sumsq", np.float64, 2)])
RATE = 48000.0
W = 4                                  # half width of the window's main lobe in bins
VIEWS = {"L": 0, "R": 1, "M": 2, "S": 3}


def window(N):
    """Periodic 4-term Blackman-Harris, built in double and rounded once to fp32 (returned as float64)."""
    t = 2.0 * np.pi * np.arange(N) / N
    w = 0.35875 - 0.48829 * np.cos(t) + 0.14128 * np.cos(2.0 * t) - 0.01168 * np.cos(3.0 * t)
    return w.astype(np.float32).astype(np.float64)


def records(audio, ch, N=4096, M=0):
    """The complete records of one stream's audio from the chain's first frame on (`audio` as the chain returns it,
    interleaved L/R for ch = 2): (records RECORD [n], spectra float64 [n, 3, N / 2 + 1] scaled to power)."""
    M = M or 6 * N
    H, nb = N // 2, N // 2 + 1
    assert M % H == 0
    a = np.asarray(audio, dtype=np.float64).reshape(-1, ch)
    spr = M // H
    n_seg = (len(a) - N) // H + 1 if len(a) >= N else 0
    n = n_seg // spr
    w = window(N)
    sw2 = float(np.sum(w * w))
    ck = np.full(nb, 2.0)
    ck[0] = ck[-1] = 1.0
    recs = np.zeros(n, dtype=RECORD)
    spectra = np.zeros((n, 3, nb))
    with np.errstate(over="ignore", invalid="ignore"):
        a32 = a.astype(np.float32)
    for i in range(n):
        r = recs[i]
        r["index"], r["first_sample"], r["channels"], r["fft_size"], r["interval_samples"] = i, i * M, ch, N, M
        t = a[i * M:(i + 1) * M]
        fin = np.isfinite(t)
        tz = np.where(fin, t, 0.0)
        r["n_nonfinite"] = int((~fin).sum())
        for c in range(ch):
            r["sum"][c] = np.sum(tz[:, c])
            r["sumsq"][c] = np.sum(tz[:, c] * tz[:, c])
        rows = np.zeros((3, nb))
        cnt = skip = 0
        for j in range(i * spr, (i + 1) * spr):
            seg = a32[j * H:j * H + N]
            if not np.all(np.isfinite(seg)):
                skip += 1
                continue
            cnt += 1
            Lk = np.fft.rfft(seg[:, 0].astype(np.float64) * w)
            rows[0] += np.abs(Lk) ** 2
            if ch == 2:
                Rk = np.fft.rfft(seg[:, 1].astype(np.float64) * w)
                rows[1] += np.abs(Rk) ** 2
                rows[2] += (Lk * np.conj(Rk)).real
        r["segments"], r["skipped"] = cnt, skip
        if cnt:
            spectra[i] = rows * ck / (N * sw2 * cnt)
    return recs, spectra


def _db(p):
    return 10.0 * math.log10(2.0 * p) if p > 0.0 else -math.inf


def derive(recs, spectra, view=0, band_lo_hz=0.0, band_hi_hz=0.0, tone_hz=0.0, tone_search_hz=0.0, max_harmonic=0,
           min_tone_dbfs=0.0):
    """fmr_analyser_derive: the records pooled by `segments`, in the given view."""
    view = VIEWS.get(view, view)
    N, ch = int(recs["fft_size"][0]), int(recs["channels"][0])
    assert np.all(recs["fft_size"] == N) and np.all(recs["channels"] == ch) and (ch == 2 or view == 0)
    band_lo_hz = band_lo_hz or 20.0
    band_hi_hz = band_hi_hz or 15000.0
    tone_search_hz = tone_search_hz or 50.0
    max_harmonic = max_harmonic or 10
    min_tone_dbfs = min_tone_dbfs or -60.0
    bin_hz = RATE / N
    nan = math.nan
    segw = recs["segments"].astype(np.float64)
    seg = float(segw.sum())
    sp = np.asarray(spectra, dtype=np.float64).reshape(len(recs), 3, N // 2 + 1)
    pooled = np.tensordot(segw, sp, axes=(0, 0)) / seg if seg > 0 else np.zeros((3, N // 2 + 1))
    pl, pr, pc = pooled
    P = [pl, pr, (pl + pr + 2.0 * pc) / 4.0, np.maximum(0.0, (pl + pr - 2.0 * pc) / 4.0)][view]
    out = dict(segments=int(recs["segments"].astype(np.uint64).sum()), skipped=int(recs["skipped"].astype(np.uint64).sum()),
               n_nonfinite=int(recs["n_nonfinite"].astype(np.uint64).sum()), harmonics_counted=0,
               harmonic_dbc=[nan] * 8)
    frames = float(out["segments"] + out["skipped"]) * (N // 2)
    s0, s1 = float(recs["sum"][:, 0].sum()), float(recs["sum"][:, 1].sum())
    q = [float(recs["sumsq"][:, 0].sum()), float(recs["sumsq"][:, 1].sum())]
    sv = [s0, s1, (s0 + s1) / 2.0, (s0 - s1) / 2.0][view]
    out["dc"] = sv / frames if frames > 0 else 0.0
    out["total_dbfs"] = nan if view >= 2 else _db(q[view] / frames) if frames > 0 else -math.inf
    k_lo, k_hi = int(math.ceil(band_lo_hz / bin_hz)), int(math.floor(band_hi_hz / bin_hz))
    B = k_hi - k_lo + 1
    assert B >= 2 * W + 1
    p_band = float(np.sum(P[k_lo:k_hi + 1]))
    out["band_dbfs"] = _db(p_band)
    s_lo, s_hi = k_lo, k_hi
    if tone_hz > 0.0:
        s_lo = max(k_lo, int(math.ceil((tone_hz - tone_search_hz) / bin_hz)))
        s_hi = min(k_hi, int(math.floor((tone_hz + tone_search_hz) / bin_hz)))
    k0, p_t, cen = -1, 0.0, 0.0
    if s_hi >= s_lo:
        k0 = s_lo + int(np.argmax(P[s_lo:s_hi + 1]))
        k0 = min(max(k0, k_lo + W), k_hi - W)
        ks = np.arange(k0 - W, k0 + W + 1)
        p_t = float(np.sum(P[ks]))
        cen = float(np.sum(ks * P[ks]))
    found = k0 >= 2 * W + 1 and p_t > 0.0 and _db(p_t) >= min_tone_dbfs
    out["tone_found"] = int(found)
    if not found:
        out.update(tone_hz=nan, tone_dbfs=nan, thd=nan, thd_n=nan, sinad_db=nan, noise_dbfs=out["band_dbfs"])
        return out
    out["tone_hz"] = cen / p_t * bin_hz
    out["tone_dbfs"] = _db(p_t)
    taken = np.zeros(len(P), dtype=bool)
    taken[k0 - W:k0 + W + 1] = True
    p_h = 0.0
    for h in range(2, max_harmonic + 1):
        kh = int(math.floor(h * out["tone_hz"] / bin_hz + 0.5))
        if kh + W > k_hi:
            break
        ks = np.arange(kh - W, kh + W + 1)
        ks = ks[~taken[ks]]
        ph = float(np.sum(P[ks]))
        taken[ks] = True
        p_h += ph
        out["harmonics_counted"] += 1
        if h <= 9:
            out["harmonic_dbc"][h - 2] = 10.0 * math.log10(ph / p_t) if ph > 0.0 else -math.inf
    E = int(taken.sum())
    band = np.arange(k_lo, k_hi + 1)
    p_free = float(np.sum(P[band[~taken[band]]]))      # = P_band - P_t - P_h, without the cancellation
    p_n = p_free * B / (B - E) if B > E else 0.0
    out["noise_dbfs"] = _db(p_n)
    out["thd"] = math.sqrt(p_h / p_t)
    out["thd_n"] = math.sqrt((p_h + p_n) / p_t)
    out["sinad_db"] = 10.0 * math.log10((p_t + p_h + p_n) / (p_h + p_n)) if p_h + p_n > 0.0 else math.inf
    return out

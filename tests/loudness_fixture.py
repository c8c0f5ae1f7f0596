"""The audio monitor's definitions (include/fmradion_amd.h, fmr_enable_loudness / fmr_loudness_derive) restated in float64
numpy: K-weighting as the serial recurrence, the 4x true-peak interpolator, the sub-block records and the levels derived
from them.  The GPU tests run it on the audio a chain returned; the CPU tests hold it to the standards' own figures."""
import math

import numpy as np

RECORD = np.dtype([("index", np.uint64), ("first_sample", np.uint64), ("n_nonfinite", np.uint32),
                   ("channels", np.uint32), ("step_samples", np.uint32), ("reserved", np.uint32),
                   ("kw_sumsq", np.float64, 2), ("sumsq", np.float64, 2), ("sum_lr", np.float64),
                   ("sample_peak", np.float64, 2), ("true_peak", np.float64, 2)])

# ITU-R BS.1770-4, 48 kHz: the shelf, then the high-pass (b0, b1, b2, a1, a2)
STAGES = ((1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
          (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621))


def kweight(x):
    """One channel through both biquads, w = x - a1 w1 - a2 w2; y = b0 w + b1 w1 + b2 w2, left to right in Python floats
    (IEEE double, nothing fused), state zero in front of the first sample."""
    y = [float(v) for v in x]
    for b0, b1, b2, a1, a2 in STAGES:
        w1 = w2 = 0.0
        for i, v in enumerate(y):
            w = v - a1 * w1 - a2 * w2
            y[i] = b0 * w + b1 * w1 + b2 * w2
            w2 = w1
            w1 = w
    return np.array(y, dtype=np.float64)


def taps():
    """g_p[k] = sinc(k - p/4) (0.5 + 0.5 cos(pi (k - p/4) / 6)) for p = 1 .. 3, k = -5 .. 6, as [3, 12]."""
    g = np.zeros((3, 12))
    for p in range(1, 4):
        for k in range(-5, 7):
            u = math.pi * (float(k) - float(p) / 4.0)
            g[p - 1, k + 5] = (math.sin(u) / u) * (0.5 + 0.5 * math.cos(u / 6.0))
    return g


def true_peak_track(x):
    """max over p of |y[n, p]| for every n: y[n, p] = sum_{k = -5 .. 6} x[n - 6 + k] g_p[k] with k ascending, samples in
    front of index 0 being 0, and y[n, 0] = x[n - 6] itself."""
    n = len(x)
    xp = np.concatenate([np.zeros(11), np.asarray(x, dtype=np.float64)])      # xp[j + i] = x[i - 11 + j]
    m = np.abs(xp[5:5 + n])
    for gp in taps():
        acc = np.zeros(n)
        for j in range(12):
            acc = acc + xp[j:j + n] * gp[j]
        m = np.maximum(m, np.abs(acc))
    return m


def records(audio, ch, Q):
    """The complete records of one stream's audio from the chain's first sample on: `audio` as the chain returns it
    (interleaved L/R for ch = 2)."""
    a = np.asarray(audio, dtype=np.float64).reshape(-1, ch)
    bad = ~np.isfinite(a)
    x = np.where(bad, 0.0, a)
    n = len(x) // Q
    recs = np.zeros(n, dtype=RECORD)
    kw = [kweight(x[:n * Q, c]) for c in range(ch)]
    tp = [true_peak_track(x[:n * Q, c]) for c in range(ch)]
    for q in range(n):
        sl = slice(q * Q, (q + 1) * Q)
        r = recs[q]
        r["index"], r["first_sample"], r["channels"], r["step_samples"] = q, q * Q, ch, Q
        r["n_nonfinite"] = int(bad[sl].sum())
        for c in range(ch):
            r["kw_sumsq"][c] = np.sum(kw[c][sl] * kw[c][sl])
            r["sumsq"][c] = np.sum(x[sl, c] * x[sl, c])
            r["sample_peak"][c] = np.max(np.abs(x[sl, c]))
            r["true_peak"][c] = np.max(tp[c][sl])
        if ch == 2:
            r["sum_lr"] = np.sum(x[sl, 0] * x[sl, 1])
    return recs


def _lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def _db20(v):
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def derive(recs, silence_dbfs=-60.0):
    """fmr_loudness_derive: windows only over records with consecutive index."""
    out = dict(momentary_lufs=-math.inf, momentary_max_lufs=-math.inf, short_term_lufs=-math.inf,
               short_term_max_lufs=-math.inf, integrated_lufs=-math.inf)
    zm, run, longest, consec = [], 0, 0, 0
    thr = 10.0 ** (silence_dbfs / 10.0)
    kw = [float(r["kw_sumsq"][0]) + float(r["kw_sumsq"][1]) for r in recs]
    for i, r in enumerate(recs):
        follows = i > 0 and int(r["index"]) == int(recs[i - 1]["index"]) + 1
        consec = consec + 1 if follows else 1
        if not follows:
            run = 0
        Q = float(r["step_samples"])
        if consec >= 4:
            z = sum(kw[i - 3:i + 1]) / (4.0 * Q)
            zm.append(z)
            out["momentary_lufs"] = _lufs(z)
            out["momentary_max_lufs"] = max(out["momentary_max_lufs"], out["momentary_lufs"])
        if consec >= 30:
            out["short_term_lufs"] = _lufs(sum(kw[i - 29:i + 1]) / (30.0 * Q))
            out["short_term_max_lufs"] = max(out["short_term_max_lufs"], out["short_term_lufs"])
        silent = (float(r["sumsq"][0]) + float(r["sumsq"][1])) / (float(r["channels"]) * Q) < thr
        run = run + 1 if silent else 0
        longest = max(longest, run)
    passed = [z for z in zm if _lufs(z) > -70.0]
    gated = []
    if passed:
        gate = _lufs(sum(passed) / len(passed)) - 10.0
        gated = [z for z in passed if _lufs(z) > gate]
        if gated:
            out["integrated_lufs"] = _lufs(sum(gated) / len(gated))
    sl = sr = slr = 0.0
    for r in recs:                     # record by record, as the library adds them
        sl, sr, slr = sl + float(r["sumsq"][0]), sr + float(r["sumsq"][1]), slr + float(r["sum_lr"])
    out["sample_peak_dbfs"] = _db20(float(np.max(recs["sample_peak"])))
    out["true_peak_dbtp"] = _db20(float(np.max(recs["true_peak"])))
    out["correlation"] = slr / math.sqrt(sl * sr) if sl * sr > 0.0 else 0.0
    side, mid = sl + sr - 2.0 * slr, sl + sr + 2.0 * slr
    out["side_to_mid_db"] = (0.0 if side <= 0.0 and mid <= 0.0 else -math.inf if side <= 0.0 else
                             math.inf if mid <= 0.0 else 10.0 * math.log10(side / mid))
    out["longest_silence_blocks"] = longest
    out["trailing_silence_blocks"] = run
    out["n_nonfinite"] = int(np.sum(recs["n_nonfinite"].astype(np.uint64)))
    out["momentary_windows"] = len(zm)
    out["gated_windows"] = len(gated)
    return out

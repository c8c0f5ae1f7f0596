"""The IQ corrector's definitions (include/fmradion_amd.h, "DC-offset and IQ-imbalance correction on the capture")
restated in numpy.

One input row at a time, the whole row at once: the definitions do not know about blocks or calls.  Everything is exact
(fp32 products rounded one by one, 64-bit integer moments, a fixed sequence of fp64 operations for the coefficients, the
fp32 apply with every product and sum rounded), so the device's rows and records are compared with these bit for bit.
"""
import math

import numpy as np

Q = 4096
DC, BALANCE = 1, 2
RECORD = np.dtype([("index", np.uint64), ("first_interval", np.uint64), ("n_usable", np.uint64),
                   ("n_nonfinite", np.uint64), ("n_skipped", np.uint64), ("n_refused", np.uint64),
                   ("sum_re", np.int64), ("sum_im", np.int64), ("sum_rr", np.int64), ("sum_ii", np.int64),
                   ("sum_ri", np.int64), ("n_intervals", np.uint32), ("dc_re", np.float32), ("dc_im", np.float32),
                   ("w_re", np.float32), ("w_im", np.float32), ("reserved", np.uint32)])
SUMS = ("sum_re", "sum_im", "sum_rr", "sum_ii", "sum_ri")
TWO36 = 2.0 ** 36
P_FLOOR = 2.0 ** -40


def impair(s, g, phi, dc):
    """The receiver model: I exact, Q' = g (Q cos phi + I sin phi), then the offset dc added; float64, rounded to complex64."""
    s = np.asarray(s).astype(np.complex128)
    q = g * (s.imag * math.cos(phi) + s.real * math.sin(phi))
    return (s.real + 1j * q + complex(dc)).astype(np.complex64)


def classify(x):
    """(re, im float32, non-finite, skipped, usable bool) per sample"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    v = x.view(np.float32).reshape(-1, 2)
    re, im = v[:, 0].copy(), v[:, 1].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        p = (re * re) + (im * im)
        nonfin = ~(np.isfinite(re) & np.isfinite(im))
        skipped = ~nonfin & ~(p <= np.float32(4))
    return re, im, nonfin, skipped, ~nonfin & ~skipped


def fix(v):
    """floor(v 2^36) of float32 values, widened to double first, as int64"""
    return np.floor(v.astype(np.float64) * TWO36).astype(np.int64)


def sample_moments(x):
    """[n, 6] int64: (usable, a_r, a_i, a_rr, a_ii, a_ri) per sample, all zero for a sample that is not usable"""
    re, im, _, _, ok = classify(x)
    with np.errstate(over="ignore", invalid="ignore"):
        re0, im0 = np.where(ok, re, np.float32(0)), np.where(ok, im, np.float32(0))
        a = np.stack([ok.astype(np.int64), fix(re0), fix(im0), fix(re0 * re0), fix(im0 * im0), fix(re0 * im0)], axis=1)
    a[~ok] = 0
    return a


def interval_sums(a):
    """[intervals, 6] int64 from sample_moments: complete intervals and the open one behind them"""
    nj = (len(a) + Q - 1) // Q
    pad = np.zeros((nj * Q, 6), dtype=np.int64)
    pad[:len(a)] = a
    return pad.reshape(nj, Q, 6).sum(axis=1, dtype=np.int64)


def window_sums(S, W):
    """[intervals, 6] int64: the sums over the intervals j - c .. j - 1, c = min(j, W), as differences of running totals
    (int64, wrap-around allowed)"""
    with np.errstate(over="ignore"):
        tot = np.concatenate([np.zeros((1, 6), dtype=np.int64), np.cumsum(S, axis=0, dtype=np.int64)])
        j = np.arange(len(S))
        return tot[j] - tot[j - np.minimum(j, W)]


def solve(win):
    """d and w from one window's sums (N, S_r, S_i, S_rr, S_ii, S_ri), fp64, one operation per line.  Returns (m_r, m_i,
    w_r, w_i, refused)."""
    N, S_r, S_i, S_rr, S_ii, S_ri = (int(v) for v in win)
    if N < Q // 2:
        return 0.0, 0.0, 0.0, 0.0, False
    f = np.float64
    den = f(N) * f(TWO36)
    r = f(1.0) / den
    m_r = f(S_r) * r
    m_i = f(S_i) * r
    E_rr = f(S_rr) * r
    E_ii = f(S_ii) * r
    E_ri = f(S_ri) * r
    mrr = m_r * m_r
    mii = m_i * m_i
    mri = m_r * m_i
    P = (E_rr + E_ii) - (mrr + mii)
    C_r = (E_rr - E_ii) - (mrr - mii)
    C_i = f(2.0) * E_ri - f(2.0) * mri
    crr = C_r * C_r
    cii = C_i * C_i
    D = P * P - (crr + cii)
    w_r = w_i = f(0.0)
    refused = False
    if P > P_FLOOR and D > 0.0:
        t = P + np.sqrt(D)
        w_r = C_r / t
        w_i = C_i / t
        if w_r * w_r + w_i * w_i > 0.0625:
            w_r = w_i = f(0.0)
            refused = True
    return float(m_r), float(m_i), float(w_r), float(w_i), refused


def coefficients(S, W, correct=0):
    """(coef [intervals, 4] float32: dr, di, wr, wi as applied; refused [intervals] bool)"""
    correct = correct or (DC | BALANCE)
    win = window_sums(S, W)
    coef = np.zeros((len(S), 4), dtype=np.float32)
    refused = np.zeros(len(S), dtype=bool)
    for j in range(1, len(S)):
        m_r, m_i, w_r, w_i, refused[j] = solve(win[j])
        if correct & DC:
            coef[j, 0], coef[j, 1] = np.float32(m_r), np.float32(m_i)
        if correct & BALANCE:
            coef[j, 2], coef[j, 3] = np.float32(w_r), np.float32(w_i)
    return coef, refused


def apply(x, coef):
    """The corrected row: fp32, every product and sum rounded; non-finite samples and the samples of intervals whose
    coefficients are all zero pass bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    re, im, nonfin, _, _ = classify(x)
    c = np.repeat(coef, Q, axis=0)[:len(x)]
    dr, di, wr, wi = (np.ascontiguousarray(c[:, k]) for k in range(4))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        zr = re - dr
        zi = im - di
        yr = zr - ((wr * zr) + (wi * zi))
        yi = zi - ((wi * zr) - (wr * zi))
    keep = nonfin | ((dr == 0) & (di == 0) & (wr == 0) & (wi == 0))
    out = np.empty((len(x), 2), dtype=np.float32)
    out[:, 0], out[:, 1] = np.where(keep, re, yr), np.where(keep, im, yi)
    out = out.view(np.complex64).reshape(-1)
    out[keep] = x[keep]                      # (bit for bit: the payload of a NaN as well)
    return out


def run(x, W=64, R=256, correct=0):
    """The corrector over one row.  Returns a dict: out (complex64), S ([intervals, 6] int64, the last possibly open), coef,
    refused, nonfin, skipped (bool per sample) and records (RECORD, the complete ones)."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    _, _, nonfin, skipped, _ = classify(x)
    a = sample_moments(x)
    S = interval_sums(a)
    coef, refused = coefficients(S, W, correct)
    out = apply(x, coef)
    n_int = len(x) // Q
    recs = np.zeros(n_int // R, dtype=RECORD)
    for i in range(len(recs)):
        js, ss = slice(i * R, (i + 1) * R), slice(i * R * Q, (i + 1) * R * Q)
        tot = S[js].sum(axis=0, dtype=np.int64)
        last = coef[(i + 1) * R - 1]
        recs[i] = (i, i * R, tot[0], nonfin[ss].sum(), skipped[ss].sum(), refused[js].sum(), *tot[1:], R, *last, 0)
    return {"out": out, "S": S, "coef": coef, "refused": refused, "nonfin": nonfin, "skipped": skipped, "records": recs}


def derive(recs):
    """fmr_iq_correction_derive in numpy: the pooled sums through solve(), then the levels."""
    win = [int(recs["n_usable"].sum())] + [int(recs[k].sum()) for k in SUMS]
    m_r, m_i, w_r, w_i, refused = solve(win)
    w = complex(w_r, w_i)
    rho = (1 - w) / (1 + w)
    n_int = int(recs["n_intervals"].sum())
    return {"refused": int(refused), "dc_re": m_r, "dc_im": m_i,
            "dc_dbfs": 20 * math.log10(abs(complex(m_r, m_i))) if m_r or m_i else -math.inf,
            "w_re": w_r, "w_im": w_i, "image_rejection_db": -20 * math.log10(abs(w)) if abs(w) else math.inf,
            "gain_imbalance_db": 20 * math.log10(abs(rho)), "phase_error_deg": -math.degrees(math.atan2(rho.imag, rho.real)),
            "usable_share": win[0] / (n_int * Q), "n_intervals": n_int, "n_usable": win[0],
            "n_nonfinite": int(recs["n_nonfinite"].sum()), "n_skipped": int(recs["n_skipped"].sum()),
            "n_refused": int(recs["n_refused"].sum())}


# ---- the capture of the GPU tests (tests/test_gpu_iqcorr.py; tests/test_iqcorr_fixture.py guards it) ----
F, BLK, OFFS, IDS, AMPS = 2.5e6, 16384, [-250_000, 250_000], [3, 4], [0.3, 0.03]
N = 122 * Q
CFG = dict(W=4, R=8)
G1, PHI1, DC1 = 1.05, math.radians(3.0), 0.01 - 0.006j           # the main row
G2, PHI2, DC2 = 0.97, math.radians(-2.0), -0.004 + 0.012j        # the second row of a multi-row chain
# the cut into calls the GPU tests use (the blanker's): a call ends behind sample 99303
CALLS = [[BLK] * 5, [BLK, 1000], [BLK] * 4, [7], [BLK] * 8, [BLK] * 8, [BLK] * 4]
CALLS.append([N - sum(map(sum, CALLS))])
# blocks of 1, 7, 4095, 4097, 16384 and a few hundred samples, several blocks per call
RAGGED = [[1], [7, 300], [4095], [4097, 1], [BLK] * 3, [777], [4096, 4096, 123], [1, 1, 2], [BLK, 4095, 4097, 555]]
while sum(map(sum, RAGGED)) + 8 * BLK < N:
    RAGGED.append([BLK] * 8)
RAGGED.append([])
while sum(map(sum, RAGGED)) < N:
    RAGGED[-1].append(min(BLK, N - sum(map(sum, RAGGED))))
# what is planted, by sample index
NEGZERO = 100                      # (-0.0, 0.0) in interval 0
BIG = [30000, 99303]               # finite with p > 4; the second is the last sample of a call
TINY = 70000                       # (1e-39, -1e-39): fp32 denormals whose squares underflow; floor(-tiny) is -1
NAN, INF = 230000, 260000
ZERO3 = (40, 43)                   # three all-zero intervals, then signal: a window of four never empties
ZERO4 = (50, 54)                   # W all-zero intervals: P = 0 exactly at interval 54, then W intervals of recovery
SKIP15 = (60 * Q, 61 * Q + Q // 2)           # one and a half intervals scaled by 10: all skipped
SKIP45 = (66 * Q, 70 * Q + Q // 2)           # four and a half: the window of interval 70 has N = 0, that of 71 N = Q / 2 exactly
QUIET = (85 * Q + 1000, 400000)    # scaled by 0.1: a -20 dB step, and the +20 dB step at sample 400000


def base_capture(n=N):
    import chanbank_fixture as cb
    return cb.composite(n, F, OFFS, IDS, AMPS)


def capture(clean=False):
    """Station 3 at -250 kHz (0.3) and station 4 at +250 kHz (0.03) at 2.5 MS/s, 122 intervals, through impair(G1, PHI1,
    DC1); clean, or with everything planted."""
    x = impair(base_capture(), G1, PHI1, DC1)
    if clean:
        return x
    x[QUIET[0]:QUIET[1]] *= np.float32(0.1)
    for lo, hi in (SKIP15, SKIP45):
        x[lo:hi] *= np.float32(10.0)
    for lo, hi in (ZERO3, ZERO4):
        x[lo * Q:hi * Q] = 0
    v = x.view(np.float32).reshape(-1, 2)
    v[NEGZERO] = (-0.0, 0.0)
    v[BIG[0]] = (1.5, -1.9)
    v[BIG[1]] = (3.0, 0.0)
    v[TINY] = (1e-39, -1e-39)
    v[NAN] = (np.nan, 0.25)
    v[INF] = (0.1, np.inf)
    return x


def second_row():
    """The same stations through impair(G2, PHI2, DC2), one NaN and one skipped sample planted."""
    x = impair(base_capture(), G2, PHI2, DC2)
    v = x.view(np.float32).reshape(-1, 2)
    v[123456] = (0.5, np.nan)
    v[200001] = (-2.5, 0.5)
    return x


def improper_row():
    """A real-valued two-station capture: the I path alone, with the receiver's noise (sigma 1e-3) on Q.  |C| is all but
    P, so every interval with a usable window is refused.  (With Q exactly zero, D is exactly 0 and the row falls under
    !(D > 0) instead: w = 0 without a refusal; tests/test_iqcorr_fixture.py holds that too.)"""
    x = base_capture()
    rng = np.random.default_rng(5)
    return (x.real.astype(np.float64) + 1j * rng.normal(0.0, 1e-3, len(x))).astype(np.complex64)


# ---- the capture of the effect test and of the 10 MS/s GPU test ----
N_EFFECT = 1 << 21


def effect_capture():
    """(clean, impaired): the two stations over 2^21 samples, and the same through impair(G1, PHI1, DC1)"""
    x = base_capture(N_EFFECT)
    return x, impair(x, G1, PHI1, DC1)


F10, BLK10, N10 = 10e6, 65536, 8 * 65536


def capture10():
    """The benchmark's station at 10 MS/s, 128 intervals, through impair(G1, PHI1, DC1)."""
    import siggen
    return impair(siggen.fm_stereo_iq(N10, F10), G1, PHI1, DC1)

"""Float64 model of the weak-signal stage (fmr_enable_weak_signal; include/fmradion_amd.h states the definitions, DESIGN.md
section 16 the design): the ultrasonic-noise detector on a 384 kHz MPX, the attack / release control, the action on the
audio and the records.  Serial, in the order the header writes the sums; no device, no library.  Not a test module.
"""
import math

import numpy as np

F = 384000.0
Q = 768                  # MPX samples per control interval
A = 96                   # audio frames per audio interval
TAPS = 63
BLEND, HIGHCUT, MUTE = 1, 2, 4
DEFAULT_DB = {"blend": (-33.0, -23.0), "highcut": (-23.0, -15.0), "mute": (-15.0, -9.0)}
RECORD = np.dtype([("index", np.uint64), ("first_interval", np.uint64), ("n_intervals", np.uint32),
                   ("n_nonfinite", np.uint32), ("usn_sum", np.float64), ("usn_peak", np.float64),
                   ("smoothed", np.float64), ("t_blend", np.float64), ("t_highcut", np.float64), ("t_mute", np.float64),
                   ("max_blend", np.float64), ("max_highcut", np.float64), ("max_mute", np.float64)])
INT_FIELDS = ("index", "first_interval", "n_intervals", "n_nonfinite")


def config(actions=BLEND | HIGHCUT | MUTE, attack_ms=10.0, release_ms=500.0, blend=None, highcut=None, mute=None,
           highcut_hz=2500.0, mute_floor_db=-20.0, record_intervals=50):
    """The configuration with the defaults filled in; blend / highcut / mute are (lo_db, hi_db)."""
    pairs = [blend or DEFAULT_DB["blend"], highcut or DEFAULT_DB["highcut"], mute or DEFAULT_DB["mute"]]
    return {"on": [bool(actions & b) for b in (BLEND, HIGHCUT, MUTE)], "lo": [float(p[0]) for p in pairs],
            "hi": [float(p[1]) for p in pairs], "c_att": 1.0 - math.exp(-2.0 / attack_ms),
            "c_rel": 1.0 - math.exp(-2.0 / release_ms), "alpha": 1.0 - math.exp(-2.0 * math.pi * highcut_hz / 48000.0),
            "g_floor": 10.0 ** (mute_floor_db / 20.0), "R": int(record_intervals)}


def taps():
    """h = delta[k - 31] - lp, lp the Blackman-windowed sinc with cut-off 110 kHz scaled to sum 1 (float64 [63])."""
    fc = 110000.0 / F
    lp, total = [], 0.0
    for k in range(TAPS):
        x = 2.0 * fc * float(k - 31)
        sinc = 1.0 if k == 31 else math.sin(math.pi * x) / (math.pi * x)
        w = 0.42 - 0.5 * math.cos(2.0 * math.pi * float(k) / 62.0) + 0.08 * math.cos(4.0 * math.pi * float(k) / 62.0)
        lp.append(2.0 * fc * sinc * w)
        total += lp[-1]
    return np.array([(1.0 if k == 31 else 0.0) - lp[k] / total for k in range(TAPS)], dtype=np.float64)


def response_db(h, f_hz):
    """|H(f)| in dB at the frequencies f_hz."""
    k = np.arange(len(h))
    H = np.array([np.sum(h * np.exp(-2j * np.pi * f / F * k)) for f in np.atleast_1d(f_hz)])
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


def _padded(mpx):
    x = np.asarray(mpx, dtype=np.float32)
    bad = ~np.isfinite(x)
    xd = np.where(bad, np.float32(0.0), x).astype(np.float64)
    return np.concatenate([np.zeros(TAPS - 1), xd]), bad


def usn(mpx):
    """The detector on the fp32 MPX of a stream from its first sample: (u float64 [J], n_nonfinite uint32 [J]) of the
    J = len // Q complete intervals.  y[n] = sum_k h[k] x[n - k], k ascending; samples in front of index 0 are 0; a
    non-finite sample is counted and enters as 0."""
    h = taps()
    xp, bad = _padded(mpx)
    J = (len(xp) - (TAPS - 1)) // Q
    n = J * Q
    y = np.zeros(n)
    for k in range(TAPS):
        y += h[k] * xp[TAPS - 1 - k:TAPS - 1 - k + n]
    u = (y * y).reshape(J, Q).sum(axis=1) / float(Q)
    return u, bad[:n].reshape(J, Q).sum(axis=1).astype(np.uint32)


def usn_scale(mpx):
    """mean_n (sum_k |h_k| |x_{n - k}|)^2 per complete interval: what the rounding of u is measured against."""
    h = np.abs(taps())
    xp, _ = _padded(mpx)
    xp = np.abs(xp)
    J = (len(xp) - (TAPS - 1)) // Q
    n = J * Q
    y = np.zeros(n)
    for k in range(TAPS):
        y += h[k] * xp[TAPS - 1 - k:TAPS - 1 - k + n]
    return (y * y).reshape(J, Q).mean(axis=1)


def control(u, cfg, s0=0.0):
    """The control on the interval values u: (s float64 [J], t float64 [J, 3]) -- blend, high cut, mute."""
    u = np.asarray(u, dtype=np.float64)
    s = np.empty(len(u))
    prev = float(s0)
    for j, uj in enumerate(u):
        c = cfg["c_att"] if uj > prev else cfg["c_rel"]
        prev = prev + c * (float(uj) - prev)
        s[j] = prev
    with np.errstate(divide="ignore"):
        D = 10.0 * np.log10(s)
    t = np.zeros((len(u), 3))
    for a in range(3):
        if cfg["on"][a]:
            t[:, a] = np.clip((D - cfg["lo"][a]) / (cfg["hi"][a] - cfg["lo"][a]), 0.0, 1.0)
    return s, t


def ramps(t, n_frames):
    """v(f) [n_frames, 3] for the frames 0 .. n_frames - 1: interval J = f // A - 1 ramped to from J - 1; below 0: 0."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    f = np.arange(n_frames)
    J = f // A - 1
    assert n_frames == 0 or J.max() < len(t), "the audio runs ahead of the control intervals"
    tp = np.concatenate([np.zeros((2, 3)), t])          # tp[j + 2] = t[j]
    v0, v1 = tp[J + 1], tp[J + 2]
    p = ((f % A) + 1) / float(A)
    return v0 + p[:, None] * (v1 - v0)


def act(audio, ch, t, cfg):
    """The action on the audio of a stream from its first frame (interleaved L/R doubles for ch = 2) with the control
    values t [J, 3]: the handled audio, the same layout."""
    x = np.asarray(audio, dtype=np.float64).reshape(-1, ch)
    n = len(x)
    v = ramps(t, n)
    if ch == 2:
        L, R = x[:, 0], x[:, 1]
        S = 0.5 * (L - R)
        x1 = np.stack([L - v[:, 0] * S, R + v[:, 0] * S], axis=1)
    else:
        x1 = x.copy()
    w = np.empty_like(x1)
    al = cfg["alpha"]
    for c in range(ch):
        prev, col, out = 0.0, x1[:, c].tolist(), [0.0] * n
        for i in range(n):
            prev = prev + al * (col[i] - prev)
            out[i] = prev
        w[:, c] = out
    x2 = x1 + v[:, 1:2] * (w - x1)
    g = 1.0 - v[:, 2:3] * (1.0 - cfg["g_floor"])
    return (g * x2).reshape(-1)


def records(u, nonfinite, cfg):
    """The complete records of the intervals (u, nonfinite as usn returns them): a RECORD array."""
    R = cfg["R"]
    s, t = control(u, cfg)
    n = len(u) // R
    out = np.zeros(n, dtype=RECORD)
    for i in range(n):
        sl = slice(i * R, (i + 1) * R)
        acc = 0.0
        for v in u[sl]:
            acc += float(v)
        out[i] = (i, i * R, R, int(np.sum(nonfinite[sl])), acc, np.max(u[sl]), s[sl][-1], t[sl][-1, 0], t[sl][-1, 1],
                  t[sl][-1, 2], t[sl][:, 0].max(), t[sl][:, 1].max(), t[sl][:, 2].max())
    return out


def derive(recs):
    """fmr_weak_signal_derive in numpy."""
    ni = int(recs["n_intervals"].sum())
    mean, peak = float(np.sum(recs["usn_sum"])) / ni, float(recs["usn_peak"].max())
    db = lambda v: 10.0 * math.log10(v) if v > 0 else -math.inf
    share = lambda k: float(recs["n_intervals"][recs[k] > 0].sum()) / ni
    return {"usn_mean_db": db(mean), "usn_peak_db": db(peak), "usn_mean_hz": 75000.0 * math.sqrt(mean),
            "usn_peak_hz": 75000.0 * math.sqrt(peak), "blend_share": share("max_blend"),
            "highcut_share": share("max_highcut"), "mute_share": share("max_mute"), "t_blend": float(recs["t_blend"][-1]),
            "t_highcut": float(recs["t_highcut"][-1]), "t_mute": float(recs["t_mute"][-1]), "n_intervals": ni,
            "n_nonfinite": int(recs["n_nonfinite"].sum())}


# ---- the test signal of tests/test_gpu_weak_signal.py and tests/test_weak_signal_thresholds.py -------------------------
TEST_N = 12 * 65536                                  # 2.05 s at 384 kHz
TEST_NOISY = (345600, 460800)                        # the noisy segment [0.9 s, 1.2 s) in samples: whole intervals
TEST_SIGMA = (1e-3, 0.15)                            # noise per I / Q component, clean and noisy (carrier amplitude 0.3)
TEST_DB = {"blend": (-40.0, -30.0), "highcut": (-30.0, -22.0), "mute": (-22.0, -16.0)}   # thresholds the GPU tests use
TEST_MS = (10.0, 50.0)                               # attack, release: every t is back at 0 before the signal ends


def stepped_iq(n=TEST_N, noisy=TEST_NOISY, sigma=TEST_SIGMA, stream_id=0, seed=11):
    """FM stereo (siggen.fm_stereo_mpx: L and R tones of unlike frequency, a pilot) at 384 kHz with complex white noise
    stepped clean, noisy, clean, as complex64."""
    import siggen
    t = np.arange(n, dtype=np.float64) / F
    x = 0.3 * np.exp(1j * 2 * np.pi * 75000.0 / F * np.cumsum(siggen.fm_stereo_mpx(t, stream_id)))
    rng = np.random.default_rng(seed + stream_id)
    sg = np.full(n, sigma[0])
    sg[noisy[0]:noisy[1]] = sigma[1]
    return (x + sg * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)

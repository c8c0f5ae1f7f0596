"""Bounds of the RDS stage's estimates, computed from the documented design alone, shared by
tests/test_gpu_rds_reference.py, tests/test_gpu_rds_fec.py and tests/test_gpu_rds_front_end.py.  Not a test module.

For the noise-free carrier phase, carrier offset and level the float64 receiver's own deviation is all but zero (1e-6 rad,
3e-5), which no fp32 stage with an 81-tap matched filter can meet.  There a term is added that is sized as four standard
deviations of what the design's approximations put on an estimate from 64 symbols, not as a worst case: phase_term,
level_term.  window_scatter is the receiver's own scatter, window by window, on a given capture.
"""
import numpy as np

import rds_fixture as rf
import rds_reference as rr

FS = 384000.0
SPS = rr.SPS


def wrap(x, period):
    return (x + period / 2) % period - period / 2


def windows_len(nwin):
    """A capture after which window nwin - 1 (symbol periods [64 (nwin - 1), 64 nwin)) is the last complete one whatever
    the stage's latency below half a window: it ends half a window after the window's last symbol."""
    return int((64 * nwin + 33) * SPS)


FS2 = 24000.0                                        # the stage's rate behind its mixing low-pass
SOFT_GAIN = FS2 * rf.TD * np.pi ** 2 / 32            # |soft symbol| per unit subcarrier: (1 / 2) int d^2 dt at 24 kHz
SIGMAS = 4.0


def design_taps():
    """The stage's two filters as DESIGN section 9 states them: 128-tap Blackman-windowed sinc, cut-off 12 kHz at
    384 kHz, unit DC gain; the shaping pulse sampled at 24 kHz over +- 2 symbols (81 taps)."""
    k = np.arange(128)
    h1 = np.sinc(2 * 12000.0 / FS * (k - 63.5)) * (0.42 - 0.5 * np.cos(2 * np.pi * k / 127) + 0.08 * np.cos(4 * np.pi * k / 127))
    return h1 / h1.sum(), rf.pulse((np.arange(81) - 40) / FS2)


def programme_leak(kind):
    """rms of what the programme alone (no subcarrier) leaves behind the two filters, float64 [MPX units x taps' gain]."""
    h1, h2 = design_taps()
    n = int(FS)
    t = np.arange(n) / FS
    y1 = np.convolve(rf.programme(t, kind) * np.exp(-2j * np.pi * 57000.0 * t), h1)[127:n:16]
    y2 = np.convolve(y1, h2)[80:len(y1)]
    return float(np.sqrt(np.mean(np.abs(y2) ** 2)))


def pulse_tail(f_off=None):
    """Share of the shaping pulse the 81 taps cut off, as a root of energy shares (0.0057): the rms of the intersymbol
    interference the cut leaves on a sample of the matched filter's output.  With f_off: its share in quadrature to the
    symbol, the cut-off part belonging to symbols whose carrier has turned by 2 pi f_off t since."""
    n = np.arange(-240000, 240001)
    t = n / FS2
    p2 = rf.pulse(t) ** 2
    w = 1.0 if f_off is None else (2 * np.pi * f_off * t) ** 2
    return float(np.sqrt((p2 * w)[np.abs(n) > 40].sum() / p2.sum()))


def phase_term(kind, level, peak, f_off):
    """SIGMAS standard deviations of the carrier phase of one window [rad].  A soft symbol is the difference of two
    output samples, of size 2 x one pulse; its quadrature error has
      * the programme's leak and the fp32 roundings (2.5 = root of the matched filter's energy gain, 128 roundings of
        2^-24 / sqrt(3) relative to the MPX peak in the mixing filter), twice in quadrature, against level SOFT_GAIN;
      * with a carrier offset, the cut-off pulse tails of turned neighbours: pulse_tail(f_off) / sqrt(2) of the symbol.
    The window averages 64 symbols with independent data."""
    eps = 2.5 * np.sqrt(128.0) * 2.0 ** -24 * peak / np.sqrt(3.0)
    per_symbol = np.sqrt(2 * (programme_leak(kind) ** 2 + eps ** 2)) / (level * SOFT_GAIN) + pulse_tail(f_off) / np.sqrt(2.0)
    return SIGMAS * per_symbol / 8.0


def offset_term(phase_sigmas):
    """The offset is the slope between two windows' phases (sqrt(2), over 64 symbols), smoothed by one half per window
    (variance x 1 / 3) [Hz]."""
    return phase_sigmas * np.sqrt(2.0 / 3.0) / (2 * np.pi * 64 * rf.TD)


def level_term():
    """Relative error of the level: the Catmull-Rom interpolator's rms error over the sampling phase, weighted with the
    spectrum of the matched filter's output (3.0e-4, a loss), plus SIGMAS standard deviations of the cut-off tails'
    interference, pulse_tail() / sqrt(2) per symbol, over 64 symbols and the level's smoothing by 1 / 4 per window
    (variance x 1 / 7).  1.1e-3."""
    f = np.linspace(-2374.0, 2374.0, 2001)
    wgt = (np.cos(np.pi * f * rf.TD / 4) ** 2 * np.abs(1 - np.exp(-1j * np.pi * f * rf.TD))) ** 2
    u = np.linspace(0, 1, 101)[:, None]
    w = 2 * np.pi * f[None, :] / FS2
    c = [-0.5 * u ** 3 + u ** 2 - 0.5 * u, 1.5 * u ** 3 - 2.5 * u ** 2 + 1, -1.5 * u ** 3 + 2 * u ** 2 + 0.5 * u,
         0.5 * u ** 3 - 0.5 * u ** 2]
    err = np.abs(sum(c[j] * np.exp(1j * w * (j - 1)) for j in range(4)) - np.exp(1j * w * u)) ** 2
    cr = np.sqrt((err.mean(axis=0) * wgt).sum() / wgt.sum())
    return float(cr + SIGMAS * pulse_tail() / np.sqrt(2.0) / 8.0 / np.sqrt(7.0))


def f32_spacing(v):
    return float(np.spacing(np.float32(abs(v))))


def window_scatter(mpx, b):
    """b = rr.blind(mpx).  The receiver's own scatter on this capture, per complete window of rr.WIN symbols at b's
    timing (rr.matched, rr.sample): (sqrt(mean |s|^2) over b["level"], minus 1; the residual of arg(sum s^2) / 2 from b's
    fitted line b["phase"] + 2 pi b["f_off"] t, modulo pi [rad])."""
    y = rr.matched(mpx)
    tau = b["t0"] * rr.FS
    pos = tau + rr._symbol_range(len(y), tau) * rr.SPS
    nw = len(pos) // rr.WIN
    s = rr.sample(y, pos[:nw * rr.WIN]).reshape(nw, rr.WIN)
    tw = ((pos[:nw * rr.WIN] + rr.SPS / 4) / rr.FS).reshape(nw, rr.WIN).mean(axis=1)
    level = np.sqrt(np.mean(np.abs(s) ** 2, axis=1)) / b["level"] - 1.0
    phase = wrap(np.angle((s ** 2).sum(axis=1)) / 2 - (b["phase"] + 2 * np.pi * b["f_off"] * tw), np.pi)
    return level, phase


def tracked_timing(mpx, tau):
    """The float64 receiver's own timing, window by window, put through the stage's documented smoothing (DESIGN
    section 9, "smoothed by one half"; the derivation for an MPX whose delay changes is there) [samples, minus tau].

    phi_w: the timing in [0, SPS) that maximises sum |y|^2 of rr.matched over the symbols of window w alone, [64 w,
    64 w + 64) symbol periods from the first sample (those rr.MARGIN symbols inside the capture), searched over a whole
    symbol period: every whole sample, then steps of 1 / 16 sample around the best with a parabola through the top
    three, as rr._timing and rr._window_timing do.  tau_w = tau_(w-1) + (phi_w - tau_(w-1)) / 2, the nearest representative
    modulo a symbol.  Returns tau_w - tau of every complete window."""
    y = rr.matched(mpx)
    nw = int((len(y) - (rr.MARGIN + 0.5) * SPS - 2 - SPS) // (rr.WIN * SPS))
    out, z = [], None
    for w in range(nw):
        k = np.arange(rr.WIN * w, rr.WIN * (w + 1))
        k = k[k >= rr.MARGIN]

        def energy(c):
            v = rr.sample(y, k[None, :] * SPS + np.asarray(c, dtype=np.float64)[:, None])
            return (v.real ** 2 + v.imag ** 2).sum(axis=1)
        c = float(np.argmax(energy(np.arange(int(np.ceil(SPS))))))
        grid = c + np.arange(-16, 17) / 16.0
        e = energy(grid)
        j = min(max(int(np.argmax(e)), 1), len(grid) - 2)
        den = e[j - 1] - 2 * e[j] + e[j + 1]
        phi = grid[j] + (0.5 * (e[j - 1] - e[j + 1]) / den / 16.0 if den < 0 else 0.0)
        d = wrap(phi - tau, SPS)
        z = d if z is None else z + 0.5 * wrap(d - z, SPS)
        out.append(z)
    return np.array(out)

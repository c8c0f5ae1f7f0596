"""A float64 RDS receiver in numpy: the numerical reference of the library's RDS stage.

Written from the standard's definitions (IEC 62106: 57 kHz DSB-SC, 1187.5 symbols per second, biphase symbols shaped by
cos(pi f TD / 4), differential coding, 26-bit blocks with offset words) and independent of the library: nothing here is
taken from the kernels.  It works on an MPX array at 384 kHz.

    genie(mpx, t0, phase, f_off, groups)   knows the symbol times, the carrier and the transmitted bits: the bound no
                                           receiver can beat
    blind(mpx)                             estimates timing, carrier phase (modulo pi), carrier offset and subcarrier
                                           level from the signal, then decides, decodes and synchronises on the blocks

Both correlate with the UNTRUNCATED doublet d(t) = p(t) - p(t - TD / 2) (rds_fixture.pulse): the correlation is done in
the frequency domain with the doublet's transform D(f) = (pi TD / 8) cos(pi f TD / 4) (1 - exp(-i pi f TD)), |f| < 2 / TD,
so no tap is cut off; the capture is zero-padded, so nothing wraps around.  The correlator output is band-limited to
2375 Hz at 384 kHz, and is read between samples with a four-point Lagrange interpolator (relative error below 1e-6).
"""
import numpy as np

import rds_fixture as rf

FS = 384000.0
FC = 57000.0
TD = rf.TD
SPS = FS * TD                               # 323.368... MPX samples per symbol
# correlator output of one isolated symbol of a unit subcarrier: the mixer halves it, and int d^2 dt = TD pi^2 / 16
GAIN = 0.5 * TD * np.pi ** 2 / 16.0
MARGIN = 3.0                                # symbols kept clear of the capture's ends (p decays with 1 / t^2)
WIN = 64                                    # symbols per carrier-phase window of blind()

_SYN = {k: rf.syndrome(v) for k, v in rf.OFFSETS.items()}
_SLOT_OF_SYN = {_SYN["A"]: 0, _SYN["B"]: 1, _SYN["C"]: 2, _SYN["Cp"]: 2, _SYN["D"]: 3}


def doublet_energy(n=1 << 20, span=400.0):
    """int d(t)^2 dt / TD by quadrature over +- span symbols (the analytic value is pi^2 / 16)."""
    t = np.linspace(-span * TD, span * TD, n)
    d = rf.pulse(t) - rf.pulse(t - TD / 2)
    return float(np.sum(d * d) * (t[1] - t[0]) / TD)


def _fast_len(n):
    best = 1 << int(np.ceil(np.log2(n)))
    p5 = 1
    while p5 < best:
        p35 = p5
        while p35 < best:
            q = p35
            while q < n:
                q *= 2
            best = min(best, q)
            p35 *= 3
        p5 *= 5
    return best


def matched(mpx, f_off=0.0, phase=0.0):
    """y[n] = int z(u) d(u - n / FS) du / GAIN with z = mpx exp(-i (2 pi (FC + f_off) t + phase)): the correlation of
    the mixed-down MPX with the doublet starting at sample n, in units of the subcarrier level."""
    mpx = np.asarray(mpx, dtype=np.float64)
    n = len(mpx)
    t = np.arange(n, dtype=np.float64) / FS
    z = mpx * np.exp(-1j * (2 * np.pi * (FC + f_off) * t + phase))
    nfft = _fast_len(n + int(8 * SPS))
    zf = np.fft.fft(z, nfft)
    f = np.fft.fftfreq(nfft, 1.0 / FS)
    inside = np.abs(f) < 2.0 / TD
    df = np.where(inside, (np.pi * TD / 8.0) * np.cos(np.pi * f * TD / 4.0), 0.0) * (1.0 - np.exp(-1j * np.pi * f * TD))
    return np.fft.ifft(zf * np.conj(df))[:n] / GAIN


def sample(y, pos):
    """y at the fractional sample positions pos (four-point Lagrange)."""
    pos = np.asarray(pos, dtype=np.float64)
    i = np.floor(pos).astype(np.int64)
    u = pos - i
    c0 = -u * (u - 1) * (u - 2) / 6.0
    c1 = (u + 1) * (u - 1) * (u - 2) / 2.0
    c2 = -(u + 1) * u * (u - 2) / 2.0
    c3 = (u + 1) * u * (u - 1) / 6.0
    return c0 * y[i - 1] + c1 * y[i] + c2 * y[i + 1] + c3 * y[i + 2]


def _symbol_range(n, tau):
    """Symbol numbers k whose doublet, starting at tau + k SPS samples, lies MARGIN symbols inside a capture of n."""
    k_lo = int(np.ceil((MARGIN * SPS - tau) / SPS))
    k_hi = int(np.floor((n - (MARGIN + 0.5) * SPS - 2 - tau) / SPS))
    return np.arange(k_lo, k_hi + 1)


def _blocks_vs_sent(bits, k_first, sent):
    """bits[i] is the data bit of symbol k_first + i; sent the transmitted bits by symbol number.  The complete 26-bit
    blocks: (number of the first, bad flag per block, bit errors, bits compared)."""
    b_lo = -(-k_first // 26)
    b_hi = min((k_first + len(bits)) // 26, len(sent) // 26)
    got = bits[26 * b_lo - k_first:26 * b_hi - k_first].reshape(-1, 26)
    want = np.asarray(sent[26 * b_lo:26 * b_hi], dtype=np.uint8).reshape(-1, 26)
    wrong = got != want
    return b_lo, wrong.any(axis=1), int(wrong.sum()), int(wrong.size)


def genie(mpx, t0, phase, f_off, groups):
    """Known timing t0 [s], carrier phase [rad] and offset [Hz]; `groups` are the transmitted groups.  Returns a dict:
    first_block, bad (flag per complete block), bit_errors, n_bits, soft (the soft symbols, level units)."""
    y = matched(mpx, f_off, phase)
    k = _symbol_range(len(y), t0 * FS)
    s = sample(y, t0 * FS + k * SPS)
    e = (s.real < 0).astype(np.uint8)
    d = e[1:] ^ e[:-1]                                   # data bit of symbols k[1:]
    b_lo, bad, nerr, nbits = _blocks_vs_sent(d, int(k[1]), rf.encode(groups))
    return dict(first_block=b_lo, bad=bad, bit_errors=nerr, n_bits=nbits, soft=s)


def _timing(y):
    """The timing tau in [0, SPS) [samples] that maximises sum_k |y(tau + k SPS)|^2: every whole sample, then steps of
    1 / 64 sample around the best, then a parabola through the top three (the energy's highest harmonic has a period
    of 81 samples, so the parabola's own error is below 1e-4 sample)."""
    n = len(y)

    def energy(tau):
        k = _symbol_range(n, SPS)                        # (the same symbols for every candidate: tau < SPS)
        v = sample(y, tau + k * SPS)
        return float(np.sum(v.real ** 2 + v.imag ** 2))
    coarse = np.array([energy(float(c)) for c in range(int(np.ceil(SPS)))])
    c = float(np.argmax(coarse))
    step = 1.0 / 64
    grid = c + step * np.arange(-64, 65)
    fine = np.array([energy(g) for g in grid])
    j = int(np.argmax(fine))
    j = min(max(j, 1), len(grid) - 2)
    em, e0, ep = fine[j - 1], fine[j], fine[j + 1]
    den = em - 2 * e0 + ep
    tau = grid[j] + (0.5 * (em - ep) / den * step if den < 0 else 0.0)
    return tau % SPS


def _window_timing(y, pos):
    """The same maximisation over each window of WIN symbols alone, +- 2 samples around the symbol starts pos in steps
    of 1 / 16 sample with a parabola through the top three: the deviation of every window's timing [samples]."""
    nw = len(pos) // WIN
    offs = np.arange(-32, 33) / 16.0
    v = sample(y, pos[None, :nw * WIN] + offs[:, None])
    e = (v.real ** 2 + v.imag ** 2).reshape(len(offs), nw, WIN).sum(axis=2)
    j = np.clip(np.argmax(e, axis=0), 1, len(offs) - 2)
    w = np.arange(nw)
    em, e0, ep = e[j - 1, w], e[j, w], e[j + 1, w]
    den = em - 2 * e0 + ep
    return offs[j] + np.where(den < 0, 0.5 * (em - ep) / np.where(den < 0, den, -1.0), 0.0) / 16.0


def blind(mpx):
    """Estimates everything from the signal.  Returns a dict:
    t0 [s, in [0, TD)], phase [rad, modulo pi, at t = 0], f_off [Hz], level (subcarrier level, MPX units): one value
    each from the whole capture; window_dev [samples]: the timing each window of WIN symbols gives on its own, minus t0;
    block_start [samples], block_slot (0..3 = A..D), block_bad and block_info (the 16 information bits) per 26-bit block
    after block synchronisation; group_start [samples] of every group (its block A) at its own window's timing."""
    y = matched(mpx)
    tau = _timing(y)
    k = _symbol_range(len(y), tau)
    pos = tau + k * SPS
    s = sample(y, pos)
    wdev = _window_timing(y, pos)
    t_sym = (pos + SPS / 4) / FS                         # the doublet is odd about a quarter symbol after its start
    # carrier: arg(sum s^2) / 2 per window of WIN symbols, unwrapped, then a weighted straight line over the capture
    nw = len(s) // WIN
    a = (s[:nw * WIN] ** 2).reshape(nw, WIN).sum(axis=1)
    tw = t_sym[:nw * WIN].reshape(nw, WIN).mean(axis=1)
    ang = np.unwrap(np.angle(a)) / 2
    if nw >= 2:
        slope, icpt = np.polyfit(tw, ang, 1, w=np.abs(a))
    else:
        slope, icpt = 0.0, float(ang[0])
    level = float(np.sqrt(np.mean(np.abs(s) ** 2)))
    soft = (s * np.exp(-1j * (icpt + slope * t_sym))).real
    e = (soft < 0).astype(np.uint8)
    d = e[1:] ^ e[:-1]                                   # data bit of symbols k[1:]
    # block synchronisation: the syndrome of every 26-bit stretch, then the bit phase and group position most blocks fit
    h = np.array([[(row >> (9 - b)) & 1 for b in range(10)] for row in rf.H_ROWS], dtype=np.int64)   # [26, 10]
    nblk = len(d) - 25
    syn = np.zeros(nblk, dtype=np.int64)
    for b in range(10):
        par = np.convolve(d.astype(np.int64), h[::-1, b])[25:25 + nblk] & 1
        syn |= par << (9 - b)
    slot_at = np.full(nblk, -1)
    for sv, sl in _SLOT_OF_SYN.items():
        slot_at[syn == sv] = sl
    best = (-1, 0, 0)
    for ph in range(26):
        sl = slot_at[ph::26]
        j = np.arange(len(sl))
        for g in range(4):
            cnt = int(np.sum(sl == (j + g) % 4))
            if cnt > best[0]:
                best = (cnt, ph, g)
    _, ph, g = best
    sl = slot_at[ph::26]
    j = np.arange(len(sl))
    want = (j + g) % 4
    first_bit = ph + 26 * j                              # index into d; its symbol is k[1 + index]
    start = pos[1 + first_bit] + wdev[np.minimum((1 + first_bit) // WIN, len(wdev) - 1)]
    words = np.array([int("".join(map(str, d[i:i + 16])), 2) for i in first_bit], dtype=np.int64)
    return dict(t0=tau / FS, phase=float(icpt % np.pi), f_off=float(slope / (2 * np.pi)), level=level, window_dev=wdev,
                block_start=start, block_slot=want, block_bad=sl != want, block_info=words,
                group_start=start[want == 0])

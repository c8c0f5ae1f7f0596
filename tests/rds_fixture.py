"""RDS test encoder (IEC 62106 data link layer), pure numpy, independent of the library's decoder.

groups -> 26-bit blocks (16 information bits, checkword of g(x) = x^10+x^8+x^7+x^5+x^4+x^3+1 computed by polynomial
division, offset word of the block's position added) -> bits, first transmitted bit first.  The syndrome here is computed
from the parity-check matrix the standard prints, written out row by row, so the encoder and the library's decoder
(host/fmradion_rds.hpp, which builds its matrix with a feedback shift) check each other.
"""
import numpy as np

G = 0b10110111001                      # g(x)
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "Cp": 0x350, "D": 0x1B4}
# parity-check matrix H (26 x 10) as printed in the standard: row i belongs to the i-th bit on air
H_ROWS = [
    0b1000000000, 0b0100000000, 0b0010000000, 0b0001000000, 0b0000100000,
    0b0000010000, 0b0000001000, 0b0000000100, 0b0000000010, 0b0000000001,
    0b1011011100, 0b0101101110, 0b0010110111, 0b1010000111, 0b1110011111,
    0b1100010011, 0b1101010101, 0b1101110110, 0b0110111011, 0b1000000001,
    0b1111011100, 0b0111101110, 0b0011110111, 0b1010100111, 0b1110001111,
    0b1100011011,
]


def checkword(info):
    r = (int(info) & 0xFFFF) << 10
    for b in range(25, 9, -1):
        if r >> b & 1:
            r ^= G << (b - 10)
    return r & 0x3FF


def syndrome(block26):
    s = 0
    for i in range(26):
        if block26 >> (25 - i) & 1:
            s ^= H_ROWS[i]
    return s


def block_word(info, offset):
    return ((int(info) & 0xFFFF) << 10) | (checkword(info) ^ OFFSETS[offset])


def group_bits(g):
    """g = (A, B, C, D): the 104 bits of one group; block 3 takes offset C' when B says version B."""
    a, b, c, d = (int(v) & 0xFFFF for v in g)
    third = "Cp" if (b >> 11) & 1 else "C"
    out = []
    for info, off in ((a, "A"), (b, "B"), (c, third), (d, "D")):
        w = block_word(info, off)
        out.extend((w >> (25 - i)) & 1 for i in range(26))
    return out


def encode(groups):
    """Data bits of consecutive groups (uint8)."""
    return np.array([bit for g in groups for bit in group_bits(g)], dtype=np.uint8)


def ps_groups(pi, ps, pty=10, n=None, rt=None):
    """A repeating programme: 0A groups carrying PS (four segments), then, if rt is given, 2A groups carrying RadioText
    (sixteen segments of four characters).  n groups in all (default: one cycle)."""
    ps = (ps + " " * 8)[:8]
    cyc = []
    for seg in range(4):
        b = (0 << 12) | (0 << 11) | (pty << 5) | seg
        cyc.append((pi, b, 0xE0CD, (ord(ps[2 * seg]) << 8) | ord(ps[2 * seg + 1])))
    if rt is not None:
        rt = (rt + " " * 64)[:64]
        for seg in range(16):
            b = (2 << 12) | (0 << 11) | (pty << 5) | seg
            s = rt[4 * seg:4 * seg + 4]
            cyc.append((pi, b, (ord(s[0]) << 8) | ord(s[1]), (ord(s[2]) << 8) | ord(s[3])))
    n = len(cyc) if n is None else n
    return [cyc[i % len(cyc)] for i in range(n)]


def diff_encode(bits, e0=0):
    """Differential coding of the transmitter: e[k] = d[k] xor e[k-1]."""
    e = np.empty(len(bits), dtype=np.uint8)
    prev = e0
    for k, b in enumerate(bits):
        prev = int(b) ^ prev
        e[k] = prev
    return e


def diff_decode(e, e_prev=0):
    """The receiver's inverse: d[k] = e[k] xor e[k-1] (a polarity flip of every e changes no d)."""
    e = np.asarray(e, dtype=np.uint8)
    return np.bitwise_xor(e, np.concatenate([[e_prev], e[:-1]]).astype(np.uint8))


# ---- the RDS signal on the MPX --------------------------------------------------------------------------------------
TD = 1.0 / 1187.5                      # one RDS symbol
_FD = 380_000.0                        # design rate of the waveform: 320 samples per symbol


def pulse(t):
    """The standard's shaping filter cos(pi f TD / 4), |f| < 2 / TD, in time: p(t) = cos(4 pi t / TD) / (1 - (8 t / TD)^2),
    p(0) = 1 (the value pi / 4 where the denominator vanishes)."""
    u = 8.0 * np.asarray(t, dtype=np.float64) / TD
    den = 1.0 - u * u
    near = np.abs(den) < 1e-9
    return np.where(near, np.pi / 4, np.cos(np.pi * u / 2) / np.where(near, 1.0, den))


def rds_baseband(t, groups, t0):
    """Biphase baseband of the groups' bits (differentially coded) at times t [s]: symbol k is the doublet
    p(t - t_k) - p(t - t_k - TD / 2), t_k = t0 + k TD, signed by the coded bit."""
    a = 1.0 - 2.0 * diff_encode(encode(groups)).astype(np.float64)
    k0 = int(round(t0 * _FD))
    n_d = int(np.ceil(t[-1] * _FD)) + 2 + 1400
    imp = np.zeros(n_d + 1400)
    pos = k0 + 320 * np.arange(len(a))
    ok = pos + 160 < len(imp)
    np.add.at(imp, pos[ok], a[ok])
    np.add.at(imp, pos[ok] + 160, -a[ok])
    h = pulse((np.arange(-1280, 1281)) / _FD)
    m = np.convolve(imp, h)[1280:1280 + len(imp)]
    return np.interp(t, (np.arange(len(m)) + (t0 * _FD - k0)) / _FD, m)


def group_times(groups, t0):
    """Start time [s] of each group's first bit."""
    return t0 + 104 * TD * np.arange(len(groups))


def station_mpx(t, groups, level=2.0 / 75.0, phase=-np.pi / 2, stereo_id=0, pilot=0.10, mono=False, t0=0.002):
    """MPX of a station: 0.9 x siggen.fm_stereo_mpx (or a mono programme without pilot) plus the RDS subcarrier
    level m(t) cos(2 pi 57000 t + phase).  phase = -pi/2: in phase with the third harmonic of the pilot sin(2 pi 19 k t);
    phase = 0: in quadrature."""
    prog = programme(t, "mono") if mono else programme(t, "stereo", stereo_id, pilot)
    return prog + level * rds_baseband(t, groups, t0) * np.cos(2 * np.pi * 57000.0 * t + phase)


def fm_iq(mpx, fs, amplitude=0.3, sigma=1e-3, seed=1):
    """75 kHz deviation FM of the MPX at rate fs, complex128 (noise sigma per component)."""
    x = amplitude * np.exp(1j * 2 * np.pi * 75000.0 / fs * np.cumsum(mpx))
    if sigma > 0:
        rng = np.random.default_rng(seed)
        x = x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    return x


# ---- a known MPX in front of the RDS stage (tests/rds_reference.py is the receiver it is compared with) ---------------
def programme(t, kind, stereo_id=0, pilot=0.10):
    """The programme part of an MPX: "mono" (two tones, no pilot), "stereo" (0.9 x siggen.fm_stereo_mpx), "tone15"
    (pilot plus a full-scale 15 kHz L-R tone: its upper sideband lies at 53 kHz, 4 kHz below the RDS subcarrier)."""
    import siggen
    if kind == "mono":
        return 0.45 * (np.sin(2 * np.pi * 1000.0 * t) + np.sin(2 * np.pi * 400.0 * t))
    if kind == "stereo":
        return 0.9 * siggen.fm_stereo_mpx(t, stereo_id, pilot)
    if kind == "tone15":
        th = 2 * np.pi * 19000.0 * t
        return 0.9 * (0.10 * np.sin(th) + 0.9 * np.sin(2 * np.pi * 15000.0 * t) * np.sin(2 * th))
    raise ValueError(kind)


def known_mpx(n, groups, kind="mono", level=2.0 / 75.0, phase=-np.pi / 2, t0=0.002, f_off=0.0, fs=384000.0):
    """n samples of programme + level m(t) cos(2 pi (57000 + f_off) t + phase), float64: what rds_reference receives and,
    through mpx_iq, what the chain's discriminator hands to the RDS stage."""
    t = np.arange(n, dtype=np.float64) / fs
    return programme(t, kind) + level * rds_baseband(t, groups, t0) * np.cos(2 * np.pi * (57000.0 + f_off) * t + phase)


def mpx_iq(mpx, fs=384000.0, amplitude=0.3):
    """Constant-envelope, noise-free FM of the MPX (75 kHz deviation) as complex64.  Noise goes on the MPX before the
    modulation: the phase discriminator then returns the MPX as generated, noise included, sample for sample (peak
    |mpx| must stay below fs / 150000 = 2.56, where the phase step would wrap)."""
    assert np.abs(mpx).max() < fs / 150000.0
    return fm_iq(mpx, fs, amplitude=amplitude, sigma=0).astype(np.complex64)

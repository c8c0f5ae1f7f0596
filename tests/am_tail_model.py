"""A float64 restatement of the multiple shooting behind AmDecoder's audio AGC (AfSimpleAgc), and the inputs and oracle
runs that tests/test_am_tail_model.py (CPU) and tests/test_gpu_am_long_calls.py (GPU) share.

Nothing here is taken from the kernels but the published rule:
  * chunks of 256 samples, every chunk integrated from its node value g with its sensitivity dg = d g_end / d g_start:
        xg = v*g; sq = xg*xg; z = 1 + rate*(1 - sq); dg *= z - 2*rate*sq; g *= z
        g not finite -> g = init, dg = 0;  g > 1.5 -> g = 1.5, dg = 0
  * node pass: v[c+1] = G[c] + M[c] * (v[c] - old[c]), v[0] the carried gain
  * a round is accepted when no node moved by more than 1e-13 relative, or from round 4 on by more than 1e-9; 6 rounds.
`stale=True` restates a node pass that walks the chunks in tiles of 512 and reads old[c] of a tile's first chunk after
the tile before has overwritten it: that chunk's map then has no correction term, v[c+1] = G[c].

The model's input v is the oracle's DC-blocked demodulated signal, built from the stage classes of tests/oracle_py.py in
the order of AmDecoder::process: (mixers and the 2049-tap filters for USB / LSB / CW / WSPR, or) LowPassFilterFirIQ ->
IfSimpleAgc(1, 1e6, rate) -> abs or real part -> HighPassFilterIir(60 / 48000).  The high-pass is the stage class's
coefficients run by scipy.signal.lfilter with the state carried (the class itself steps sample by sample through ctypes:
two seconds per call of half a million samples); the two differ in the order of float64 sums only.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.signal import lfilter

import oracle_py as ora
from conftest import load_filter

CHUNK, TILE, ROUNDS = 256, 512, 6
AF_INIT, AF_MAX = 1.0, 1.5
FS, BLK = 48000.0, 2048
LONG = 257                                  # blocks: 526 336 samples = 2056 chunks
CALLS = (LONG, LONG, 70, LONG)
MODES = {"am": ora.MODE_AM, "dsb": ora.MODE_DSB, "usb": ora.MODE_USB, "lsb": ora.MODE_LSB, "cw": ora.MODE_CW, "wspr": ora.MODE_WSPR}
SSB_LIKE, CW_LIKE = ("usb", "lsb", "cw", "wspr"), ("cw", "wspr")


def af_rate(mode):
    return 0.00125 if mode in CW_LIKE else 0.001


# ----------------------------------------------------------------------------------------------------------- the model
def shoot(v, nodes, rate):
    """One integration pass: every chunk of v from its node.  Returns (G, M, n_nonfinite)."""
    n = len(v)
    nc = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(nc * CHUNK)
    pad[:n] = v
    pad = pad.reshape(nc, CHUNK)
    last = n - (nc - 1) * CHUNK             # samples of the last chunk
    g = np.array(nodes[:nc], dtype=np.float64)
    dg = np.ones(nc)
    resets = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(CHUNK):
            xg = pad[:, i] * g
            sq = xg * xg
            z = 1.0 + rate * (1.0 - sq)
            dn = dg * (z - 2.0 * rate * sq)
            gn = g * z
            bad = ~np.isfinite(gn)
            clamp = ~bad & (gn > AF_MAX)
            resets += int(bad[:-1].sum()) + int(bad[-1] and i < last)
            gn = np.where(bad, AF_INIT, np.where(clamp, AF_MAX, gn))
            dn = np.where(bad | clamp, 0.0, dn)
            if i >= last:                   # the last chunk ends early
                gn[-1], dn[-1] = g[-1], dg[-1]
            g, dg = gn, dn
    return g, dg, resets


def node_pass(nodes, G, M, stale=False):
    """v[c+1] = G[c] + M[c] (v[c] - old[c]).  Returns (new nodes, largest relative movement)."""
    new = np.empty_like(nodes)
    new[0] = nodes[0]
    for c in range(len(G)):
        old = new[c] if (stale and c > 0 and c % TILE == 0) else nodes[c]
        new[c + 1] = G[c] + M[c] * (new[c] - old)
    move = np.abs(new[1:] - nodes[1:]) / np.maximum(np.abs(new[1:]), 1e-300)
    return new, float(move.max())


def accepted(round_no, move):
    return move <= 1e-13 or (round_no >= 4 and move <= 1e-9)


def rounds(v, g0, rate, stale=False, max_rounds=ROUNDS):
    """The Newton rounds of one call.  Returns dict(moves=[movement per round], accepted=round or None, resets=count of
    non-finite resets over all passes, gain=the end gain of the last pass, edge_M=[M at the chunks in front of a tile])."""
    nc = (len(v) + CHUNK - 1) // CHUNK
    nodes = np.full(nc + 1, float(g0))
    moves, acc, resets = [], None, 0
    M = np.ones(nc)
    for r in range(1, max_rounds + 1):
        G, M, nf = shoot(v, nodes, rate)
        resets += nf
        nodes, move = node_pass(nodes, G, M, stale)
        moves.append(move)
        if accepted(r, move):
            acc = r
            break
    return dict(moves=moves, accepted=acc, resets=resets, gain=float(nodes[nc]), edge_M=[float(M[c]) for c in range(TILE - 1, nc - 1, TILE)])


def serial(v, g0, rate, every=0):
    """The recurrence itself, sample by sample.  Returns the end gain (every > 0: and the gain after every `every` samples)."""
    g, marks = float(g0), []
    for i, x in enumerate(v.tolist(), 1):
        xg = x * g
        g *= 1.0 + rate * (1.0 - xg * xg)
        if not np.isfinite(g):
            g = AF_INIT
        elif g > AF_MAX:
            g = AF_MAX
        if every and i % every == 0:
            marks.append(g)
    return (g, marks) if every else g


def fixed_point(v, g0, rate, cap=64):
    """The Newton rounds run on until no node moves: every chunk then starts where the chunk before it ended, which is
    the serial recurrence itself, bit for bit, at a fraction of a Python loop's time.  None: not within `cap` rounds."""
    nc = (len(v) + CHUNK - 1) // CHUNK
    nodes = np.full(nc + 1, float(g0))
    for _ in range(cap):
        G, M, _nf = shoot(v, nodes, rate)
        nodes, move = node_pass(nodes, G, M)
        if move == 0.0:
            return float(nodes[nc])
    return None


def expect_fallback(m):
    """What a model run says of af_agc_fallback: 0 where the exact model accepts with margin (movement <= 1e-12 at the
    accepted round, <= 1e-6 at the round before, no reset), 1 where its movement at round 6 is >= 1e-3 with no reset,
    None in between (the flag is recorded only)."""
    if m["resets"]:
        return None
    a = m["accepted"]
    if a is not None and m["moves"][a - 1] <= 1e-12 and (a == 1 or m["moves"][a - 2] <= 1e-6):
        return 0
    if a is None and len(m["moves"]) == ROUNDS and m["moves"][-1] >= 1e-3:
        return 1
    return None


# ----------------------------------------------------------------------------------- the oracle's stages in front of it
class _FineTuner(C.Structure):
    _fields_ = [("index", C.c_uint), ("size", C.c_uint), ("tab", C.POINTER(C.c_float))]


class FineTuner:
    """FineTuner of the oracle library (table-driven mixer, phase-continuous across calls)."""

    def __init__(self, table_size, freq_shift):
        self.s = _FineTuner()
        ora._raw("ora_finetuner_init", None, [C.POINTER(_FineTuner), C.c_uint, C.c_int])(C.byref(self.s), table_size, freq_shift)

    def __del__(self):
        if self.s.tab:
            ora._raw("ora_finetuner_free", None, [C.POINTER(_FineTuner)])(C.byref(self.s))

    def process(self, iq):
        iq = ora.as_iq32(iq)
        out = np.empty_like(iq)
        ora._raw("ora_finetuner_process", None, [C.POINTER(_FineTuner), ora.c_float_p, C.c_int, ora.c_float_p])(
            C.byref(self.s), ora._fp(iq), len(iq), ora._fp(out))
        return out


def filters():
    return load_filter("jj1bdx_am_48khz_narrow"), load_filter("jj1bdx_cw_48khz_500hz"), load_filter("jj1bdx_ssb_48khz_1500hz")


class Front:
    """AmDecoder::process up to the input of AfSimpleAgc, from the stage classes."""

    def __init__(self, mode):
        am, cw, ssb = filters()
        self.mode = mode
        up, down = FineTuner(480, 15), FineTuner(480, -15)
        if mode == "usb":
            self.steps = [down, ora.LowPassFilterFirIQ(ssb), up]
        elif mode == "lsb":
            self.steps = [up, ora.LowPassFilterFirIQ(ssb), down]
        elif mode == "cw":
            self.steps = [ora.LowPassFilterFirIQ(cw), FineTuner(480, 5)]
        elif mode == "wspr":
            self.steps = [down, ora.LowPassFilterFirIQ(cw), up]
        else:
            self.steps = [ora.LowPassFilterFirIQ(am)]
        self.agc = ora.IfSimpleAgc(1.0, 1000000.0, 0.0006 if mode in CW_LIKE else 0.0003)
        hp = ora.HighPassFilterIir(60 / 48000.0).s
        self.b, self.a, self.zi = [hp.b0, hp.b1, hp.b2], [1.0, hp.a1, hp.a2], np.zeros(2)

    def process(self, iq):
        for st in self.steps:
            iq = st.process(iq)
        y = self.agc.process(iq)
        if self.mode == "am":
            dec = np.sqrt(y.real * y.real + y.imag * y.imag)          # float32, as the oracle's sqrtf
        else:
            dec = y.real
        v, self.zi = lfilter(self.b, self.a, dec.astype(np.float64), zi=self.zi)
        return v


def decoder(mode):
    am, cw, ssb = filters()
    return ora.AmDecoder(am, MODES[mode], cw, ssb) if mode in SSB_LIKE else ora.AmDecoder(am, MODES[mode])


# ------------------------------------------------------------------------------------------------------------ the inputs
def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def _steps(t):
    """1 and 2.5 in turn, 1.7 s each."""
    return np.where(np.floor(t / 1.7).astype(np.int64) % 2 == 0, 1.0, 2.5)


def input_a(n, fs=FS):
    """Carrier at +37 Hz, square-wave modulation of depth 0.9 at 400 Hz, level 0.1 and 0.25 in turn every 1.7 s."""
    t = np.arange(n) / fs
    env = 0.1 * _steps(t) * (1.0 + 0.9 * np.where(np.sin(2 * np.pi * 400.0 * t) >= 0, 1.0, -1.0))
    return (env * np.exp(2j * np.pi * 37.0 * t) + _noise(n, 21)).astype(np.complex64)


def input_b(n, stepped, factor=2.5, shift=0.0):
    """The two-tone input of test_gpu_parity.py::test_am_decoder_ssb_cw_modes, steady or with input A's level steps
    (factor, shift: other steps of the same family, `shift` seconds early)."""
    t = np.arange(n) / FS
    x = 0.05 * np.exp(2j * np.pi * 700 * t) + 0.03 * np.exp(2j * np.pi * 1900 * t) + 0.02 * np.exp(-2j * np.pi * 1100 * t)
    if stepped:
        x = x * (1.0 + (factor - 1.0) * (_steps(t + shift) > 1.0))
    return (x + _noise(n, 11)).astype(np.complex64)


N_ALL = sum(CALLS) * BLK
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def signal(name):
    """'a', 'b' (steady) or 'bs' (stepped): sum(CALLS) blocks of 2048 samples at 48 kHz."""
    make = {"a": lambda: input_a(N_ALL), "b": lambda: input_b(N_ALL, False), "bs": lambda: input_b(N_ALL, True)}[name]
    return cached(("signal", name), make)


def oracle_run(mode, x, calls, resample=None):
    """The oracle decoder over x, block by block: calls = lists of block lengths.  resample: an oracle IfResampler in
    front.  Per call: audio, audio length per block, the AF gain after every block, and the three status values after
    the call.  The decoder is left behind for a caller that goes on."""
    dec = decoder(mode)
    out, o = [], 0
    for lens in calls:
        audio, alen, gains = [], [], []
        for n in lens:
            b = x[o:o + n]
            o += n
            a = dec.process(resample.process(b) if resample else b)
            audio.append(a)
            alen.append(len(a))
            gains.append(dec.get_af_agc_current_gain())
        out.append(dict(audio=np.concatenate(audio), alen=alen, gains=np.array(gains), af_agc=dec.get_af_agc_current_gain(),
                        if_agc=dec.get_if_agc_current_gain(), if_rms=dec.get_if_rms()))
    return out


def model_run(mode, x, calls, resample=None, stale=False):
    """The model over the same calls: the Newton rounds from the gain the serial recurrence carried into each call."""
    front, rate, g, o, out = Front(mode), af_rate(mode), AF_INIT, 0, []
    for lens in calls:
        parts = []
        for n in lens:
            b = x[o:o + n]
            o += n
            parts.append(front.process(resample.process(b) if resample else b))
        v = np.concatenate(parts)
        m = rounds(v, g, rate, stale)
        m["g0"], m["v"] = g, v
        end = fixed_point(v, g, rate)
        g = m["serial"] = serial(v, g, rate) if end is None else end
        out.append(m)
    return out


def long_calls():
    return [[BLK] * n for n in CALLS]


_pool = None


def _submit(fn, *args, **kw):
    """The oracle's filters run in C with the interpreter lock released: a reference costs its wall time only once, and
    several of them little more."""
    global _pool
    if _pool is None:
        ora.lib()
        _pool = ThreadPoolExecutor(max_workers=4)      # (the model's part is Python: more threads only wait for each other)
    return _pool.submit(fn, *args, **kw)


def start(key, mode, make_x, calls, resampler=None):
    """Starts (once per process) the oracle and the exact model of `mode` over `calls` of the input make_x() returns."""
    if key not in _cache:
        x = make_x()
        rs = (lambda: None) if resampler is None else resampler
        _cache[key] = (_submit(oracle_run, mode, x, calls, rs()), _submit(model_run, mode, x, calls, rs()))
    return _cache[key]


def reference(mode, name):
    """(oracle, model) of one mode over the four calls of signal(name)."""
    o, m = start(("ref", mode, name), mode, lambda: signal(name), long_calls())
    return o.result(), m.result()


def edge_signal():
    """Input B's family, two long calls: the level rises sixfold 12 chunks in front of chunk 1024 of the second call, a
    tile edge of the node pass.  The exact model accepts that call at round 6 (9e-7, then 5e-13); with the stale read the
    first chunk behind the edge lags a round (4e-7 at round 6) and the call is not accepted."""
    n = 2 * LONG * BLK
    at = (LONG * BLK + (1024 - 12) * CHUNK) / FS
    return input_b(n, True, factor=6.0, shift=1.7 - at)


def edge_reference():
    o, m = start(("ref", "usb", "edge"), "usb", edge_signal, long_calls()[:2])
    return o.result(), m.result()


LONG_CASES = [("am", "a"), ("dsb", "a")] + [(m, n) for n in ("b", "bs") for m in SSB_LIKE]


def prefetch(cases=LONG_CASES):
    for mode, name in cases:
        start(("ref", mode, name), mode, lambda: signal(name), long_calls())

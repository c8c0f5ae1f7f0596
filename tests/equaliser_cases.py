"""Inputs, block lists and call lists for the equaliser's edge cases (tests/test_gpu_equaliser_edges.py), and the oracle
runs they are compared with.  tests/test_equaliser_cases.py proves, with the oracle alone, that every case is in the
regime it is named for.

A case is one chain: `x` holds one input row per stream, `calls` is a list of calls, each a list of input block lengths.
The first 100 non-empty IF blocks are the decoder's warm-up (FmDecode.cpp:33,107-110); the equaliser runs from the 101st."""
import functools

import numpy as np

import oracle_py as ora
import siggen
from conftest import load_filter

FS_IF = 384e3
WARM = 100                                   # FmDecode.cpp:33
DELAY_3TAPS = np.array([0.0, 1.0, 0.0], dtype=np.float32)
TAIL_LENS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 2046, 2047, 2048, 2049, 2050, 2051, 4095, 4098, 6147]
LENGTH_STAGES = [1, 2, 3, 79, 80, 159, 160]


class Case:
    def __init__(self, name, stages, x, calls, rate=FS_IF, fir=None, note=""):
        self.name, self.stages, self.rate, self.fir, self.note = name, stages, rate, fir, note
        self.x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.complex64)
        self.calls = [list(c) for c in calls]
        self.lens = [n for c in self.calls for n in c]
        assert sum(self.lens) == self.x.shape[1], (name, sum(self.lens), self.x.shape)

    @property
    def n_streams(self):
        return self.x.shape[0]

    @property
    def order(self):
        return 4 * self.stages + 1

    def fir_coeff(self):
        return DELAY_3TAPS if self.fir is None else load_filter(self.fir)


class Ref:
    """One oracle run of one stream of a case, block by block."""

    def __init__(self):
        self.if_len, self.disc, self.audio, self.resets_after, self.error_after = [], [], [], [], []

    @property
    def active_from(self):
        """Index of the block the equaliser first runs on: the 101st non-empty IF block."""
        seen = 0
        for b, n in enumerate(self.if_len):
            if n:
                seen += 1
                if seen == WARM + 1:
                    return b
        return None

    def failed(self, b):
        return self.resets_after[b] > (self.resets_after[b - 1] if b else 0)


def _calls(lens, per_call):
    return [lens[i:i + per_call] for i in range(0, len(lens), per_call)]


def signal(n, delay, stream_id=0, amplitude=0.3, fs=FS_IF):
    """FM stereo through a two-ray channel whose echo is `delay` samples late."""
    return siggen.two_ray(siggen.fm_stereo_iq(n, fs, stream_id=stream_id, amplitude=amplitude), delay)


def bump_ulp(x, seed=20261021):
    """Every float of x moved by one ulp in a random direction (non-finite values stay)."""
    f = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)
    up = np.random.default_rng(seed).random(f.shape) < 0.5
    out = np.where(up, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))).astype(np.float32)
    out = np.where(np.isfinite(f), out, f)
    return out.view(np.complex64)


# ------------------------------------------------------------------------------------------------------------ cases
def _tails(stages, per_call):
    lens = [256] * WARM + TAIL_LENS
    x = signal(sum(lens), 2 if stages < 8 else 20)
    return Case("tails_E%d_by%d" % (stages, per_call), stages, x, _calls([256] * WARM, 20) + _calls(TAIL_LENS, per_call),
                note="every tail length of a chunk, blocks shorter than the taps, one to three samples past a chunk edge")


def _length(stages):
    lens = [256] * WARM + [2518, 2519] * 15
    x = signal(sum(lens), max(1, min(20, 2 * stages)))
    return Case("length_E%d" % stages, stages, x, _calls(lens[:WARM], 20) + _calls(lens[WARM:], 5),
                note="far fewer taps than lanes; both sides of the host's choice of instantiation (320 and 640 taps)")


def _turn_on_384k():
    lens = [256] * 98 + [300, 2517, 2518, 2048, 7, 2049, 2517, 1, 2050, 2519, 2048, 2048]       # block 100 is the call's third
    return Case("turn_on_384k", 4, signal(sum(lens), 3), _calls(lens, 7), note="the equaliser starts inside a call")


def _turn_on_10m():
    """10 MS/s: 6667 input samples give about 256 IF samples, 1 to 20 give one or none (main.cpp:931-934)."""
    tiny = [1, 20, 5, 13, 2, 17, 9, 11, 3, 19, 7, 15]
    lens = []
    for i in range(97):
        lens += [6667, tiny[i % len(tiny)]]
        if i % 5 == 0:
            lens.append(tiny[(i // 5 + 3) % len(tiny)])
    lens += [65536, 4, 65536, 65536, 12, 1, 65536, 30001, 65536, 65536, 65536, 8, 65536, 65536]
    x = signal(sum(lens), 52, fs=10e6)
    return Case("turn_on_10m", 4, x, _calls(lens, 9), rate=10e6, note="empty IF blocks inside the warm-up do not count")


def _walk(name, pos, blk):
    """One NaN at sample `pos` of block 104; 17 blocks follow, in calls of three."""
    lens = [256] * WARM + [blk] * 22
    x = signal(sum(lens), 2).copy()
    x[WARM * 256 + 4 * blk + pos] = np.nan + 0j
    return Case(name, 2, x, _calls(lens[:WARM], 20) + _calls(lens[WARM:], 3), note="NaN at sample %d of block 104" % pos)


OVERFLOW_AT = (104, 76)           # block, sample: 0 mod 4
OVERFLOW_VALUE = np.complex64(6e29 + 8e29j)


def _overflow():
    lens = [256] * WARM + [2048] * 22
    x = signal(sum(lens), 2).copy()
    x[WARM * 256 + (OVERFLOW_AT[0] - WARM) * 2048 + OVERFLOW_AT[1]] = OVERFLOW_VALUE
    return Case("overflow", 2, x, _calls(lens[:WARM], 20) + _calls(lens[WARM:], 3),
                note="a finite sample whose |y|^2 overflows: the error is not finite, the output is")


STEP_LOW, STEP_HIGH = 0.03, 0.9


def _level_step():
    lens = [1024] * WARM + [2048] * 40
    n = sum(lens)
    x = signal(n, 2, amplitude=STEP_LOW).copy()
    up = WARM * 1024 + 5 * 2048 + 1001
    x[up:up + 20 * 2048] *= np.float32(STEP_HIGH / STEP_LOW)
    return Case("level_step", 2, x, _calls(lens[:WARM], 20) + _calls(lens[WARM:], 4), note="x 30 inside block 105, / 30 twenty blocks later")


def _three_streams():
    lens = [256] * WARM + [2048] * 22
    xs = np.stack([signal(sum(lens), d, stream_id=s) for s, d in enumerate((1, 2, 3))])
    xs[1, WARM * 256 + 4 * 2048 + 77] = np.nan + 0j
    return Case("three_streams", 2, xs, _calls(lens[:WARM], 20) + _calls(lens[WARM:], 3), note="stream 1 carries the NaN")


def _if_filter():
    lens = [256] * WARM + [2519] * 30
    return Case("if_filter", 8, signal(sum(lens), 20), _calls(lens[:WARM], 20) + _calls(lens[WARM:], 5), fir="jj1bdx_fm_384kHz_medium")


BUILDERS = {}
for _s in (2, 8):
    for _g in (1, 4):
        BUILDERS["tails_E%d_by%d" % (_s, _g)] = functools.partial(_tails, _s, _g)
for _s in LENGTH_STAGES:
    BUILDERS["length_E%d" % _s] = functools.partial(_length, _s)
BUILDERS["turn_on_384k"] = _turn_on_384k
BUILDERS["turn_on_10m"] = _turn_on_10m
BUILDERS["walk_odd"] = functools.partial(_walk, "walk_odd", 77, 2048)
BUILDERS["walk_mult4"] = functools.partial(_walk, "walk_mult4", 76, 2048)
BUILDERS["walk_chunk2"] = functools.partial(_walk, "walk_chunk2", 2048 + 301, 2517)
BUILDERS["overflow"] = _overflow
BUILDERS["level_step"] = _level_step
BUILDERS["three_streams"] = _three_streams
BUILDERS["if_filter"] = _if_filter
NAMES = list(BUILDERS)
WALKS = ["walk_odd", "walk_mult4", "walk_chunk2"]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# --------------------------------------------------------------------------------------------------------- oracle runs
def run_oracle(c, x_row, stages=None):
    """FmDecoder (behind IfResampler at 10 MS/s) over one input row, block by block."""
    fm = ora.FmDecoder(c.fir is not None, c.fir_coeff(), True, 50.0, False, c.stages if stages is None else stages,
                       load_filter("jj1bdx_48khz_fmaudio"))
    rs = ora.IfResampler(c.rate, FS_IF) if c.rate != FS_IF else None
    r, pos = Ref(), 0
    for n in c.lens:
        b = x_row[pos:pos + n]
        pos += n
        if rs is not None:
            b = rs.process(b)
        if len(b):
            r.audio.append(fm.process(b))
            r.disc.append(fm.debug_vector(0, len(b)))
        else:                                              # main.cpp:931-934: the decoder is not called
            r.audio.append(np.zeros(0)); r.disc.append(np.zeros(0))
        r.if_len.append(len(b))
        r.resets_after.append(fm.get_multipath_resets())
        r.error_after.append(fm.get_multipath_error())
    r.coeff, r.gain, r.stereo = fm.get_multipath_coefficients(), fm.get_if_agc_gain(), int(fm.stereo_detected())
    r.resets, r.error = r.resets_after[-1], r.error_after[-1]
    return r


@functools.lru_cache(maxsize=None)
def reference(name, stream=0):
    c = case(name)
    return run_oracle(c, c.x[stream])


@functools.lru_cache(maxsize=None)
def unequalised(name, stream=0):
    c = case(name)
    return run_oracle(c, c.x[stream], stages=0)


def block_distance(a, b):
    """What the GPU tests bound per block: RMS of the difference over the samples finite in both; the largest
    difference for a block of fewer than 16 samples."""
    ok = np.isfinite(a) & np.isfinite(b)
    d = np.abs(a[ok] - b[ok])
    if not d.size:
        return 0.0
    return float(d.max()) if len(a) < 16 else float(np.sqrt(np.mean(d * d)))


@functools.lru_cache(maxsize=None)
def conditioning(name, stream=0):
    """The oracle's own conditioning: per block, the distance between its discriminator output and that of a second run
    whose every input float is one ulp off; and the RMS distance of the two runs' audio."""
    c = case(name)
    a, b = reference(name, stream), run_oracle(c, bump_ulp(c.x[stream]))
    assert a.if_len == b.if_len
    au, bu = np.concatenate(a.audio), np.concatenate(b.audio)
    return [block_distance(p, q) for p, q in zip(a.disc, b.disc)], block_distance(au, bu) if len(au) == len(bu) else np.inf

"""The FM audio tail stage by stage: reference, unit of the bound, inputs and cases (tests/test_tail_cases.py pins all of it
on the CPU; tests/test_gpu_tail_stereo.py holds the product to it).

The reference takes the PLL out of the comparison.  The chain's own de-emphasised 384 kHz signals (debug taps 3 and 2) go
through the oracle's audio resampler, pilot cut and DC block, one set per channel, and the oracle's output mux
(FmDecode.cpp:242-283).  What is left between chain and oracle is fp64 rounding.

The unit of the bound.  The DC block is a direct-form-II biquad with both poles at 0.99956: its internal state (Biquad.x1)
is 10^3 .. 10^4 times the audio, and the product finds every chunk's start state by a re-associated scan, a few fp64 ulp OF
THAT STATE.  So for a compared stretch
    u_ch     = 2^-52 x rms(DC-block state of channel ch over the stretch)
    u_max_ch = 2^-52 x max|state|
and for stereo output u = u_m + 1.017 u_d (mono: u = u_m; an unlocked block contributes no u_d: its L-R state counts as 0;
pilot shift: the output is d or 0, so u = u_d of the locked blocks).  The margin K_STATE is not chosen freely: it is the
bound the project already asserts on the mono tail (tests/test_gpu_tail_fma.py, cutting "a": err <= 2 x 2.201e-12)
expressed in that unit, ceil(4.402e-12 / u), with u from the ORACLE's mono chain on that test's input (computed on the
CPU by test_tail_cases.py::test_k_state, which asserts the constant below).  The same K_STATE holds rms (x u) and worst
sample (x u_max) of every call of every case.
"""
import ctypes as C
import os

import numpy as np

import oracle_py as ora
import siggen

FS_IF, FS_AU = 384e3, 48e3
BLK = 65536
B = 2517                        # the product's block at 384 kHz (bench.py: 65536 samples at 10 MS/s)
C_DC = 64                       # airspy-fmradion_amd/csrc/fmradion_amd.hip:74  (chunk of the DC block's multiple shooting)
FMR_DC_K = 32                   # airspy-fmradion_amd/csrc/kernels_par.hpp:219  (chunks per lane of the node pass)
FMR_DC_MAXW = 8                 # airspy-fmradion_amd/csrc/kernels_par.hpp:220  (waves per workgroup of the node pass)
PCUT_TILE_SMALL, PCUT_TILE = 320, 1280      # fmradion_amd.hip:2453-2458: k_pilotcut2<320, 320> up to au_max 320, else <320, 1280>
ULP = 2.0 ** -52
STEREO_GAIN = 1.017             # FmDecode.cpp:255-270

# tests/test_gpu_tail_fma.py asserts err <= 2 x PARENT_STAGE_ERR["a"] on its mono cutting "a"
TAIL_FMA_BOUND = 2 * 2.201e-12
# u of the oracle's mono chain on that input, 6355 audio samples from a cold start (CPU, test_tail_cases.py::test_k_state
# prints it): rms(state) = 5715.02 (max 8949.11, the cold start's swing), u = 2^-52 x 5715.02
TAIL_FMA_U = 1.26899e-12
K_STATE = 4                     # ceil(TAIL_FMA_BOUND / TAIL_FMA_U) = ceil(3.469)

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filters")


def load_pilotcut():
    return np.load(os.path.join(_GOLD, "jj1bdx_48khz_fmaudio.npy"))


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def amax(a):
    a = np.asarray(a)
    return float(np.max(np.abs(a))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------------------- the stage oracle
class _Channel:
    """Audio resampler, pilot cut and DC block of one channel, running on."""

    def __init__(self, pilotcut):
        self.rs = ora.Resampler(FS_IF, FS_AU, 180.0)
        self.pc = ora.LowPassFilterFirAudio(pilotcut)
        self.hp = ora.HighPassFilterIir(0.0001)

    def run(self, x384, alens):
        """(audio, DC-block state after every sample) of one call: the resampler over the whole call, the pilot cut per audio
        block (its block-head path; FmDecoder::process returns before it when a block yields no audio), the DC block on."""
        a48 = self.rs.process(x384)
        assert len(a48) == sum(alens), (len(a48), sum(alens))
        y, st = np.empty(len(a48)), np.empty(len(a48))
        step, s = self.hp._step, self.hp.s
        ref = C.byref(s)
        o = 0
        for nb in alens:
            if nb == 0:
                continue
            for v in self.pc.process(a48[o:o + nb]).tolist():
                y[o] = step(ref, v)
                st[o] = s.x1
                o += 1
        return y, st


class StageCall:
    """One call of the stage oracle.  audio: what FmDecoder::process returns for the call's blocks, concatenated (interleaved
    L/R for stereo); m, d: the channels behind the DC block; st_m, st_d: Biquad.x1 after every sample; lock: the block's flag
    per audio sample."""

    def __init__(self, audio, m, d, st_m, st_d, lock, stereo, pilot_shift):
        self.audio, self.m, self.d, self.st_m, self.st_d, self.lock = audio, m, d, st_m, st_d, lock
        self.stereo, self.pilot_shift = stereo, pilot_shift

    def units(self, lo=0, hi=None):
        """{"out" | "mid" | "side": (u, u_max)} of the stretch [lo, hi) of the call's audio samples.  out: the audio as
        returned; mid = (L+R)/2 and side = (L-R)/2 for stereo."""
        sl = slice(lo, hi)
        um = (ULP * rms(self.st_m[sl]), ULP * amax(self.st_m[sl]))
        if not self.stereo:
            return {"out": um}
        sd = self.st_d[sl] * self.lock[sl]
        ud = (ULP * rms(sd), ULP * amax(sd))
        if self.pilot_shift:
            return {"out": ud, "mid": ud, "side": (0.0, 0.0)}
        us = (STEREO_GAIN * ud[0], STEREO_GAIN * ud[1])
        return {"out": (um[0] + us[0], um[1] + us[1]), "mid": um, "side": us}


class stage_oracle:
    """The oracle's audio tail behind the de-emphasis, with a running state per channel."""

    def __init__(self, pilotcut, stereo=True):
        self.stereo = stereo
        self.ch_m = _Channel(pilotcut)
        self.ch_d = _Channel(pilotcut) if stereo else None

    def process_call(self, mono384, diff384, alens, locked=None, pilot_shift=False):
        """mono384 / diff384: the de-emphasised 384 kHz signals of the call (FmDecoder's debug_vector(2) / (1), the chain's
        taps 3 / 2; diff384 None for mono); alens: audio samples per block; locked: stereo_detected() per block."""
        alens = [int(a) for a in alens]
        m, st_m = self.ch_m.run(mono384, alens)
        if not self.stereo:
            return StageCall(m.copy(), m, None, st_m, None, None, False, False)
        d, st_d = self.ch_d.run(diff384, alens)
        lock = np.repeat(np.asarray(locked, dtype=bool), alens)
        if pilot_shift:                          # mono_to_left_right(stereo) / zero_to_left_right
            l = r = np.where(lock, d, 0.0)
        else:
            s = STEREO_GAIN * d
            l, r = np.where(lock, m + s, m), np.where(lock, m - s, m)
        audio = np.empty(2 * len(m))
        audio[0::2], audio[1::2] = l, r
        return StageCall(audio, m, d, st_m, st_d, lock.astype(np.float64), True, pilot_shift)


def mid_side(audio):
    return 0.5 * (audio[0::2] + audio[1::2]), 0.5 * (audio[0::2] - audio[1::2])


# ---------------------------------------------------------------------------------------------------------- the whole oracle
def oracle_blocks(x, calls, pilotcut, in_rate=FS_IF, stereo=True, pilot_shift=False, want_taps=False):
    """ora.FmDecoder (behind ora.IfResampler when in_rate is not 384 kHz) fed the calls' blocks one by one.  Per call:
    (alens, locked) per block -- and with want_taps (audio, debug_vector(2), debug_vector(1)) per block as well."""
    ifr = ora.IfResampler(in_rate, FS_IF) if in_rate != FS_IF else None
    fm = ora.FmDecoder(False, np.array([0.0, 1.0, 0.0], dtype=np.float32), stereo, 50.0, pilot_shift, 0, pilotcut)
    out, pos = [], 0
    for c in calls:
        alens, locked, taps = [], [], []
        for n in c:
            q = x[pos:pos + n]
            pos += n
            if ifr is not None:
                q = ifr.process(q)
            a = fm.process(q)
            alens.append(len(a) // 2 if stereo else len(a))
            locked.append(bool(fm.stereo_detected()) if stereo else False)
            if want_taps:
                k = len(q)
                taps.append((a, np.array(fm.debug_vector(2, k)) if k else np.zeros(0),
                             np.array(fm.debug_vector(1, k)) if k and stereo else np.zeros(0)))
        out.append((alens, locked, taps) if want_taps else (alens, locked))
    return out


# ---------------------------------------------------------------------------------------------------------- regimes
RS_FIRST, RS_PERIOD, RS_PHASES = 450, 24, (0, 6, 15)


def cum_audio(n):
    """Audio samples the oracle's 384 k -> 48 k resampler (decimation by 3, then 3 / 8) has delivered after n input samples,
    from the count alone: the first with input sample 450, then three per 24 inputs, with inputs 0, 6 and 15 of the period
    (test_tail_cases.py holds this against ora.Resampler)."""
    q, r = divmod(n - RS_FIRST, RS_PERIOD)
    return 0 if n < RS_FIRST else 3 * q + sum(r >= p for p in RS_PHASES)


def audio_lens(calls, start=0):
    """Audio samples per block of calls at 384 kHz in, from the block lengths alone."""
    out, n = [], start
    for c in calls:
        al = []
        for b in c:
            al.append(cum_audio(n + b) - cum_audio(n))
            n += b
        out.append(al)
    return out


def fit_block(pos, want):
    """The shortest block behind `pos` input samples that yields `want` audio samples."""
    b = max(0, 8 * (want - 1) - 16)
    while cum_audio(pos + b) - cum_audio(pos) < want:
        b += 1
    return b


def regime(alens):
    """What a call of these audio block lengths reaches: audio samples, DC chunks, waves and passes of k_dc_nodes, the
    pilot cut's tile (320: k_pilotcut2<320, 320>) and its tiles per block (the longest block's)."""
    n = sum(alens)
    nc = -(-n // C_DC)
    au_max = max(alens) if alens else 0
    tile = PCUT_TILE_SMALL if au_max <= PCUT_TILE_SMALL else PCUT_TILE
    return {"n_audio": n, "chunks": nc, "waves": max(1, min(FMR_DC_MAXW, -(-nc // (64 * FMR_DC_K)))),
            "passes": max(1, -(-nc // (64 * FMR_DC_K * FMR_DC_MAXW))), "au_max": au_max, "tile": tile,
            "tiles": -(-au_max // tile), "tiles_per_block": [-(-a // tile) for a in alens]}


def regroup(calls, sizes):
    """The same blocks in the same order, cut into calls of sizes[0], sizes[1], ... blocks (cyclic)."""
    blocks = [b for c in calls for b in c]
    out, i, k = [], 0, 0
    while i < len(blocks):
        out.append(blocks[i:i + sizes[k % len(sizes)]])
        i += sizes[k % len(sizes)]
        k += 1
    return out


# ---------------------------------------------------------------------------------------------------------- inputs
def fm_iq(n, fs=FS_IF, stream_id=0, n0=0):
    x = siggen.fm_stereo_iq(n, fs, stream_id=stream_id, n0=n0)
    x.setflags(write=False)
    return x


def pilot_drop_iq(n, fs=FS_IF, t_off=0.90, t_on=1.10, jump=1.3):
    """siggen.fm_stereo_iq with the pilot and the L-R subcarrier gone between t_off and t_on and back with a phase jump
    (as tests/test_gpu_configs.py::test_pilot_drops_and_returns_mid_call builds it)."""
    t = np.arange(n, dtype=np.float64) / fs
    gate = np.ones(n)
    gate[int(t_off * fs):int(t_on * fs)] = 0.0
    th = 2 * np.pi * 19000.0 * t + np.where(t >= t_on, jump, 0.0)
    left, right = np.sin(2 * np.pi * 1000.0 * t), np.sin(2 * np.pi * 400.0 * t)
    mpx = 0.45 * (left + right) + gate * (0.10 * np.sin(th) + 0.45 * (left - right) * np.sin(2 * th))
    ph = 2 * np.pi * 75000.0 / fs * np.cumsum(mpx)
    rng = np.random.Generator(np.random.PCG64(1))
    x = (0.3 * np.exp(1j * ph) + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 1e-3).astype(np.complex64)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------- cases
LOCK = [BLK] * 6                # 1.02 s at 384 kHz: the pilot lock takes 0.67 s


def product_calls(blk, small):
    """Case 1's calls behind the lock call: 1, 3 and 8 product blocks, a ragged call, three one-block calls, 2 blocks."""
    return [[blk], [blk] * 3, [blk] * 8, small[0], [small[1]], [small[2]], [small[3]], [blk] * 2]


# case 1: both channels, the product's shape of blocks, in two cuttings
CASE1_A = [LOCK] + product_calls(B, ([400, 1, 7, 8, 0, 2517, 1000, 0], 360, 384, 408))
CASE1_B = [LOCK] + regroup(CASE1_A[1:], [2, 5, 1, 3])
# the same shape at 1 MS/s behind the IF resampler (case 6): 65536 in is about 25166 at 384 kHz and 3146 audio samples
LOCK_1M = [BLK] * 16            # 1.05 s
CASE6_1M = [LOCK_1M] + product_calls(BLK, ([10417, 26, 182, 208, 0, 65536, 26042, 0], 938, 1000, 1062))

# case 2: the pilot cut's two forms and its tile seams.  320 | 321 audio samples: the switch between the instantiations;
# 1280 | 1281: one | two tiles of the 1280 form; 2561: three; 8192: seven.  A block of 8 n input samples yields n audio
# samples only where the resampler's period of 24 allows it, so every block is fitted to its place (2560 +- 6, ...)
PCUT_AUDIO = [320, 321, 1280, 1281, 2561, 8192]


def _case2():
    calls, pos = [LOCK], sum(LOCK)

    def put(call):
        nonlocal pos
        out = []
        for b in call:
            b = fit_block(pos, -b) if b < 0 else b          # (-n: a block of n audio samples)
            out.append(b)
            pos += b
        calls.append(out)
    for n in PCUT_AUDIO:
        put([-n])
    put([-n for n in PCUT_AUDIO])
    put([B, B, B, -2561, B])
    return calls


CASE2 = _case2()
CASE2_REGIME = [(320, 320, 1), (321, 1280, 1), (1280, 1280, 1), (1281, 1280, 2), (2561, 1280, 3), (8192, 1280, 7),
                (8192, 1280, 7), (2561, 1280, 3)]         # (au_max, tile, tiles of the longest block) per call behind the lock call


# case 3: the node pass beyond one wave (64 x 32 = 2048 chunks of 64 audio samples), both channels.  36 blocks of 65536:
# 294912 audio samples, 4608 chunks, 3 waves, the third with 512 chunks.  17 blocks and a few samples: 139265 audio
# samples, 2177 chunks -- chunk 2176 is the only one of lane 4 of the second wave and holds one sample (17 blocks alone
# are 2176 chunks or one sample more, by the resampler's phase).  15 blocks and one fitted: exactly 131072, one full wave.
def _case3():
    calls = [LOCK, [BLK] * 36, [B]]
    pos = n_samples(calls)
    got = cum_audio(pos + 17 * BLK) - cum_audio(pos)
    calls.append([BLK] * 17 + [fit_block(pos + 17 * BLK, 139265 - got)])
    calls.append([B] * 2)
    pos = n_samples(calls)
    got = cum_audio(pos + 15 * BLK) - cum_audio(pos)
    calls.append([BLK] * 15 + [fit_block(pos + 15 * BLK, 131072 - got)])
    calls.append([B])
    return calls


def n_samples(calls):
    return sum(sum(c) for c in calls)


CASE3 = _case3()
CASE3_REGIME = {1: (294912, 4608, 3, 1), 3: (139265, 2177, 2, 1), 5: (131072, 2048, 1, 1)}   # call: (audio, chunks, waves, passes)

# case 4: the pass loop (8 waves x 2048 chunks per pass): 1056768 audio samples, 16512 chunks, the second pass with 128
CASE4 = [LOCK, [BLK] * 129, [BLK] * 2]
CASE4_REGIME = {1: (1056768, 16512, 8, 2)}

# case 5: the lock flag changes inside a call.  (a) a cold chain locks inside one call of ragged blocks.  The PLL counts
# the samples of the blocks that end with the pilot present and locks with the block that takes the count to 192000
# (PilotPhaseLock.cpp:43,154-167): the head block places the pattern so that this is a 63-sample block (7 or 8 audio
# samples, not at a multiple of 64 in audio) behind a block of 5 samples and an empty one.  (b) the pilot
# drops out for 0.2 s and returns, one cold call of product blocks: unlocked, locked, unlocked, locked
RAGGED = [2048, 5, 0, 63, 64, 65, 517, 8192]
CASE5A = [[3700] + RAGGED * 36]         # 398044 samples = 1.04 s
CASE5B = [[B] * 306]                    # 770202 samples = 2.0 s


# ---------------------------------------------------------------------------------------------------------- the node pass, modelled
def dc_powers(a1, a2, exact):
    """(A^64, [(A^2048)^(2^k), k = 0 .. 5]) of A = [[-a1, -a2], [1, 0]] as make_dc_coef forms them: exact=False by a chain
    of double products (before the fix), exact=True in long double, each power as (double, what the double leaves)."""
    dt = np.longdouble if exact else np.float64
    a = np.array([[-a1, -a2], [1.0, 0.0]], dtype=dt)
    ac = np.eye(2, dtype=dt)
    for _ in range(C_DC):
        ac = a @ ac
    gk = np.eye(2, dtype=dt)
    for _ in range(FMR_DC_K):
        gk = ac @ gk
    agp = []
    for _ in range(6):
        agp.append(gk.copy())
        gk = gk @ gk

    def split(m):
        hi = m.astype(np.float64)
        return hi, (m - hi.astype(dt)).astype(np.float64)
    return split(ac), [split(m) for m in agp]


def _mv(m, x1, x2, exact):
    """M x as k_dc_nodes applies it: before the fix two rounded products and their rounded sum per row (mv2), now the row's sum
    rounded once plus the remainder's terms (mv2c; the fused multiply-add modelled in long double)."""
    h, l = m
    if not exact:
        return h[0, 0] * x1 + h[0, 1] * x2, h[1, 0] * x1 + h[1, 1] * x2
    L = np.longdouble

    def row(h0, h1, l0, l1):
        p = h1 * x2
        e = (L(h1) * np.asarray(x2, dtype=L) - p).astype(np.float64)
        return ((L(h0) * np.asarray(x1, dtype=L) + p).astype(np.float64) + e) + (l0 * x1 + l1 * x2)
    return row(h[0, 0], h[0, 1], l[0, 0], l[0, 1]), row(h[1, 0], h[1, 1], l[1, 0], l[1, 1])


def dc_scan_model(v, coef, carry=(0.0, 0.0), exact=True):
    """The DC block of one call of at most 2048 chunks as the product computes it, in float64 numpy: k_dc_pass1 (every chunk
    from a zero state), k_dc_nodes (each lane folds its 32 chunks, a log-step scan over the 64 lanes with the powers of
    A^2048, the carry through the product of a lane's powers, the replay) and k_dc_pass2_mux's recurrence.  coef: (b0, b1, b2,
    a1, a2); carry: (x1, x2) the call starts from.  Returns the output."""
    b0, b1, b2, a1, a2 = coef
    ac, agp = dc_powers(a1, a2, exact)
    n = len(v)
    nc = -(-n // C_DC)
    assert nc <= 64 * FMR_DC_K
    ch = np.zeros(nc * C_DC)
    ch[:n] = v
    ch = ch.reshape(nc, C_DC)
    x1, x2 = np.zeros(nc), np.zeros(nc)
    for j in range(C_DC):
        x0 = ch[:, j] - (a1 * x1 + a2 * x2)
        x2, x1 = x1, x0
    g1, g2 = x1, x2
    lane = np.arange(64)
    q1, q2 = np.zeros(64), np.zeros(64)
    for j in range(FMR_DC_K):
        c = lane * FMR_DC_K + j
        ok, cc = c < nc, np.minimum(c, nc - 1)
        n1, n2 = _mv(ac, q1, q2, exact)
        q1, q2 = np.where(ok, n1 + g1[cc], q1), np.where(ok, n2 + g2[cc], q2)
    for lv in range(6):
        o = 1 << lv
        m1, m2 = _mv(agp[lv], np.roll(q1, o), np.roll(q2, o), exact)
        q1, q2 = np.where(lane >= o, q1 + m1, q1), np.where(lane >= o, q2 + m2, q2)
    e1, e2 = np.roll(q1, 1), np.roll(q2, 1)
    e1[0] = e2[0] = 0.0
    t1, t2 = np.full(64, carry[0]), np.full(64, carry[1])
    for lv in range(6):
        m1, m2 = _mv(agp[lv], t1, t2, exact)
        bit = (lane & (1 << lv)) != 0
        t1, t2 = np.where(bit, m1, t1), np.where(bit, m2, t2)
    x1, x2 = t1 + e1, t2 + e2
    s1, s2 = np.zeros(nc), np.zeros(nc)
    for j in range(FMR_DC_K):
        c = lane * FMR_DC_K + j
        ok, cc = c < nc, np.minimum(c, nc - 1)
        s1[cc[ok]], s2[cc[ok]] = x1[ok], x2[ok]
        n1, n2 = _mv(ac, x1, x2, exact)
        x1, x2 = np.where(ok, n1 + g1[cc], x1), np.where(ok, n2 + g2[cc], x2)
    x1, x2, y = s1, s2, np.empty((nc, C_DC))
    for j in range(C_DC):
        x0 = ch[:, j] - (a1 * x1 + a2 * x2)
        y[:, j] = b0 * x0 + b1 * x1 + b2 * x2
        x2, x1 = x1, x0
    return y.reshape(-1)[:n]

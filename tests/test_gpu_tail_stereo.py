"""The stereo audio tail stage by stage: both channels of every tail kernel, the L-R halos, the split launch, the DC block's
node pass beyond one wave and one pass, the pilot cut's two forms and tile seams, and the output mux where the lock flag
changes inside a call.

Every chain is created with FMR_DEBUG_TAPS=1.  After every call the chain's own de-emphasised 384 kHz signals (debug taps
3 and 2) go through the oracle's audio resampler, pilot cut and DC block (tests/tail_cases.py: stage_oracle, running on
across the calls) and its output mux with the oracle's lock flag per block (ora.FmDecoder on the same IQ).  Every call is
held by itself, with equal lengths and no sample left out, to
    rms error <= K_STATE x u        worst sample <= K_STATE x u_max
for the audio as returned and, stereo, for (L+R)/2 and (L-R)/2 separately; u = 2^-52 x rms, u_max = 2^-52 x max of the DC
block's internal state over the call (u_m + 1.017 u_d for stereo output; an unlocked block has no u_d; tail_cases.py).
K_STATE = 4 is the bound tests/test_gpu_tail_fma.py asserts on the mono tail in that unit (test_tail_cases.py::test_k_state).
Per block the audio has L == R exactly where the oracle is unlocked and differs where it is locked (pilot shift: exact
zeros | the L-R channel).  Every case asserts the regime it is named for from the audio lengths the chain returned.

Measured on an MI355X (worst call of each test; every steady call lies at 1.0 .. 1.35 u, and the worst sample of every test but
the pilot-shift ones is one and the same: 7.276e-12 = 3.66 u_max in the mono channel of the cold first call, where the
serial kernels (the oracle's own arithmetic behind fused FIRs) show it too):
    test                                     rms error            worst sample
    case 1, cutting a | b                    1.17 | 1.21 u  (3.4e-14)     3.66 u_max (7.3e-12); a against b: 2.9e-8
    case 2, pilot-cut forms                  1.13 u  (3.0e-14)            3.66 u_max
    case 3, 4608 | 2177 | 2048 chunks        mid 1.06 | 1.06 | 1.07 u, side 1.02 | 1.01 | 1.00 u (2.7e-14 .. 2.8e-14);
                                             3.47 | 2.91 | 2.94 u_max (1.4e-13 .. 2.0e-13); short calls behind them 0.97 .. 1.12 u
    case 4, 16512 chunks, stereo | mono      mid 1.06 u, side 1.02 u (2.7e-14, 2.8e-14) | 1.06 u;  3.47 u_max (1.4e-13)
    case 5, lock-in | pilot drop             1.04 | 1.06 u  (4.7e-13 | 3.5e-13)    3.66 u_max;  FMR_SERIAL=1: 1.01 u, 2.17 | 3.66 u_max
            with pilot shift                 1.00 | 0.99 u  (6.0e-15 | 3.9e-15)    3.41 | 2.04 u_max; unlocked blocks exact zeros
    case 6, 384 k | 1 MS/s pipelined | FMR_PIPELINE=0    1.17 | 1.28 | 1.35 u (3.3e-14 .. 3.4e-14)   3.66 u_max; two streams 1.15 | 1.32 u
    case 7                                   taps on and off: bit for bit
Before the DC block's transition powers were formed in long double and applied with one rounding per row
the same cases measured 100 .. 360 u and 160 .. 266 u_max in every long call (3.9e-12 rms, 1.1e-11 worst sample in steady
state; 6.1e-11 and 4.5e-10 in the cold first call), the serial kernels 1.0 u.
"""
import importlib
import json
import os

import numpy as np
import pytest

import siggen
import tail_cases as tc

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")
K = tc.K_STATE
REPORT = {}


def _report(key, rec):
    REPORT[key] = rec
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_report_tail_stereo.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def pilotcut():
    return tc.load_pilotcut()


class Run:
    """What a chain returned: per call and stream the audio, the audio lengths per block and taps 3 and 2."""

    def __init__(self):
        self.audio, self.alens, self.tap3, self.tap2, self.status, self.trace = [], [], [], [], None, None

    def of_stream(self, s):
        r = Run()
        r.audio, r.alens = [a[s] for a in self.audio], self.alens
        r.tap3, r.tap2 = [t[s] for t in self.tap3], [t[s] for t in self.tap2]
        r.status = self.status[s]
        return r


def run_chain(x, calls, *, in_rate=tc.FS_IF, stereo=True, pilot_shift=False, taps=True, serial=False, pipeline=None,
              trace_last=False):
    """x: (S, N) or (N,).  trace_last: the (name, stream) pairs of the kernels of the last call."""
    x = np.atleast_2d(x)
    S = x.shape[0]
    want = {"FMR_DEBUG_TAPS": "1" if taps else None, "FMR_SERIAL": "1" if serial else None,
            "FMR_PIPELINE": None if pipeline is None else str(int(pipeline))}
    old = {k: os.environ.pop(k, None) for k in want}
    os.environ.update({k: v for k, v in want.items() if v is not None})
    try:
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=in_rate, enable_resampler=in_rate != tc.FS_IF, stereo=stereo,
                       pilot_shift=pilot_shift, max_block_len=max(max(max(c) for c in calls), 1),
                       max_blocks=max(len(c) for c in calls), n_streams=S)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    r, pos = Run(), 0
    try:
        for i, c in enumerate(calls):
            n = sum(c)
            if trace_last and i == len(calls) - 1:
                ch.enable_kernel_timing(3)
            a, alen = ch.process_blocks(x[:, pos:pos + n], c)
            pos += n
            r.audio.append(np.array(a))
            r.alens.append([int(v) // (2 if stereo else 1) for v in alen])
            if taps:
                t3 = [ch.debug_read(3, s, cap=n + 4096) for s in range(S)]
                r.tap3.append(t3)
                r.tap2.append([ch.debug_read(2, s, cap=n + 4096) for s in range(S)] if stereo else [None] * S)
        if trace_last:
            r.trace = [(nm, st) for nm, st, _, _ in ch.kernel_trace()]
        r.status = [ch.status(s) for s in range(S)]
    finally:
        ch.close()
    if S > 1:
        return r
    o = r.of_stream(0)
    o.trace = r.trace
    return o


def _ratio(err, u):
    return err / u if u > 0 else (0.0 if err == 0 else float("inf"))


def hold(key, r, flags, pilotcut, *, stereo=True, pilot_shift=False):
    """Every call of run r against the stage oracle on r's own taps, with the oracle's lock flags.  Prints and reports
    every figure, then asserts.  Returns the worst figures."""
    so = tc.stage_oracle(pilotcut, stereo=stereo)
    fails, rows = [], []
    worst = {"rms_u": 0.0, "max_u": 0.0, "rms": 0.0, "max": 0.0}
    for i, (got, alens, (alens_o, locked)) in enumerate(zip(r.audio, r.alens, flags)):
        assert alens == alens_o, (key, i, alens, alens_o)
        ref = so.process_call(r.tap3[i], r.tap2[i] if stereo else None, alens, locked, pilot_shift)
        assert got.shape == ref.audio.shape, (key, i, got.shape, ref.audio.shape)
        if not got.size:
            continue
        un = ref.units()
        views = [("out", got, ref.audio)]
        if stereo:
            (gm, gs), (rm, rs) = tc.mid_side(got), tc.mid_side(ref.audio)
            views += [("mid", gm, rm), ("side", gs, rs)]
        row = {"call": i, "n_audio": sum(alens)}
        for name, g, q in views:
            e_rms, e_max = tc.rms(g - q), tc.amax(g - q)
            u, umax = un[name]
            row[name] = {"rms": e_rms, "max": e_max, "u": u, "u_max": umax, "rms_u": _ratio(e_rms, u), "max_u": _ratio(e_max, umax)}
            if not (e_rms <= K * u and e_max <= K * umax):
                fails.append((i, name, row[name]))
            if name == "out" or u > 0:
                if _ratio(e_rms, u) > worst["rms_u"]:
                    worst["rms_u"], worst["rms"] = _ratio(e_rms, u), e_rms
                if _ratio(e_max, umax) > worst["max_u"]:
                    worst["max_u"], worst["max"] = _ratio(e_max, umax), e_max
        rows.append(row)
        print(f"{key} call {i:2d} ({sum(alens):7d} audio): " + "  ".join(
            f"{nm} rms {row[nm]['rms']:.2e} = {row[nm]['rms_u']:.2f} u, max {row[nm]['max']:.2e} = {row[nm]['max_u']:.2f} u_max"
            for nm, _, _ in views))
        if stereo:      # the lock flag of every block, bit for bit
            l, rr, o = got[0::2], got[1::2], 0
            for nb, lk in zip(alens, locked):
                sl = slice(o, o + nb)
                o += nb
                if nb == 0:
                    continue
                ok = np.array_equal(l[sl], rr[sl])
                if pilot_shift:
                    ok = ok and (np.any(l[sl] != 0.0) if lk else not np.any(l[sl]) and not np.any(rr[sl]))
                elif lk:
                    ok = np.any(l[sl] != rr[sl])
                if not ok:
                    fails.append((i, "lock flag of the block at audio sample", o - nb, lk))
    _report(key, {"worst": worst, "calls": rows})
    print(f"{key}: worst call rms {worst['rms_u']:.2f} u ({worst['rms']:.3e}), worst sample {worst['max_u']:.2f} u_max ({worst['max']:.3e})")
    assert not fails, (key, fails[:6], len(fails))
    return worst


def reached(r, expect):
    """expect: {call: (audio samples, chunks, waves, passes)} -- from the audio lengths the chain returned."""
    for i, want in expect.items():
        g = tc.regime(r.alens[i])
        assert (g["n_audio"], g["chunks"], g["waves"], g["passes"]) == want, (i, g, want)


# ------------------------------------------------------------------------------------------------ case 1 (and 7)
@pytest.fixture(scope="module")
def sig1():
    return tc.fm_iq(tc.n_samples(tc.CASE1_A))


@pytest.fixture(scope="module")
def flags1(sig1, pilotcut):
    return {"a": tc.oracle_blocks(sig1, tc.CASE1_A, pilotcut), "b": tc.oracle_blocks(sig1, tc.CASE1_B, pilotcut)}


@pytest.fixture(scope="module")
def run1a(sig1):
    return run_chain(sig1, tc.CASE1_A)


def test_both_channels_in_the_products_blocks(sig1, flags1, run1a, pilotcut):
    """Case 1.  Calls of 1, 3 and 8 blocks of 2517 behind the lock call, a ragged call (audio blocks of 50, 0, 1, 1, 0, ..),
    one-block calls of 45 / 48 / 51 audio samples, in two cuttings: the L-R halos of stage A, stage B and the pilot cut carry
    over blocks and calls, and the pilot cut's head path covers whole blocks."""
    assert run1a.status.stereo_detected == 1 and all(all(lk) for _, lk in flags1["a"][1:])
    assert all(tc.regime(a)["tile"] == 320 for a in run1a.alens[1:]) and 0 in run1a.alens[4]
    assert [sum(a) for a in run1a.alens[5:8]] == [45, 48, 51]
    hold("case1_cut_a", run1a, flags1["a"], pilotcut)
    rb = run_chain(sig1, tc.CASE1_B)
    assert rb.status.stereo_detected == 1
    hold("case1_cut_b", rb, flags1["b"], pilotcut)
    a, b = np.concatenate(run1a.audio), np.concatenate(rb.audio)
    assert a.shape == b.shape
    d = tc.amax(a - b)
    print(f"cutting a against cutting b: max {d:.3e}")
    assert d < 1e-7                                  # the solves run per call: no tighter than that


def test_taps_do_not_change_the_tail(sig1, run1a):
    """Case 7.  The tap only lengthens the last tile of k_deemph_decim: the same audio with FMR_DEBUG_TAPS unset."""
    r = run_chain(sig1, tc.CASE1_A, taps=False)
    assert r.alens == run1a.alens
    for i, (a, b) in enumerate(zip(r.audio, run1a.audio)):
        assert np.array_equal(a, b), (i, tc.amax(a - b))


# ------------------------------------------------------------------------------------------------ case 2
def test_pilot_cut_forms_and_seams(pilotcut):
    """Case 2.  Audio blocks of 320 | 321 (the switch between k_pilotcut2<320, 320> and <320, 1280>), 1280 | 1281 (one | two
    tiles), 2561 (three) and 8192 (seven): one call each, one call with all, and 2517-sample blocks beside a 2561 block."""
    x = tc.fm_iq(tc.n_samples(tc.CASE2))
    r = run_chain(x, tc.CASE2)
    assert r.status.stereo_detected == 1
    assert [a[0] for a in r.alens[1:7]] == tc.PCUT_AUDIO and r.alens[7] == tc.PCUT_AUDIO
    for a, want in zip(r.alens[1:], tc.CASE2_REGIME):
        g = tc.regime(a)
        assert (g["au_max"], g["tile"], g["tiles"]) == want
    assert tc.regime(r.alens[8])["tiles_per_block"] == [1, 1, 1, 3, 1]
    hold("case2_pilot_cut", r, tc.oracle_blocks(x, tc.CASE2, pilotcut), pilotcut)


# ------------------------------------------------------------------------------------------------ case 3
def test_dc_node_pass_beyond_one_wave(pilotcut):
    """Case 3.  Calls of 4608 chunks (3 waves, the third partial), 2177 chunks (2 waves, lane 4 of the second holds one chunk
    of one sample) and exactly 2048 chunks (one full wave), each followed by a short call (the carried state)."""
    x = tc.fm_iq(tc.n_samples(tc.CASE3))
    r = run_chain(x, tc.CASE3)
    assert r.status.stereo_detected == 1
    reached(r, tc.CASE3_REGIME)
    hold("case3_node_waves", r, tc.oracle_blocks(x, tc.CASE3, pilotcut), pilotcut)


# ------------------------------------------------------------------------------------------------ case 4
def test_dc_node_pass_loop(pilotcut):
    """Case 4.  One call of 129 blocks of 65536: 1056768 audio samples, 16512 chunks, two passes of k_dc_nodes (the second
    with 128 chunks), behind a lock call and before a 2-block call; stereo and mono.  The only test of that loop: about 20 s,
    most of it the oracle's DC block on the CPU."""
    x = tc.fm_iq(tc.n_samples(tc.CASE4))
    r = run_chain(x, tc.CASE4)
    assert r.status.stereo_detected == 1
    reached(r, tc.CASE4_REGIME)
    hold("case4_pass_loop_stereo", r, tc.oracle_blocks(x, tc.CASE4, pilotcut), pilotcut)
    del r
    r = run_chain(x, tc.CASE4, stereo=False)
    reached(r, tc.CASE4_REGIME)
    hold("case4_pass_loop_mono", r, tc.oracle_blocks(x, tc.CASE4, pilotcut, stereo=False), pilotcut, stereo=False)


# ------------------------------------------------------------------------------------------------ case 5
@pytest.fixture(scope="module")
def sig5():
    return {"lock_in": (tc.fm_iq(tc.n_samples(tc.CASE5A)), tc.CASE5A),
            "pilot_drop": (tc.pilot_drop_iq(tc.n_samples(tc.CASE5B)), tc.CASE5B)}


@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("pilot_shift", [False, True])
@pytest.mark.parametrize("case", ["lock_in", "pilot_drop"])
def test_lock_flag_changes_inside_a_call(sig5, pilotcut, case, pilot_shift, serial):
    """Case 5.  (a) a cold chain locks inside one call of ragged blocks, with the 63-sample block that takes the PLL's count
    to its threshold, behind an empty audio block and not at a multiple of 64 in audio; (b) the pilot drops out for 0.2 s and
    returns inside one call of 2517-sample blocks; both with pilot shift (the L-R channel | exact zeros), and all of it
    through k_fm_out's mux as well (FMR_SERIAL=1)."""
    x, calls = sig5[case]
    flags = tc.oracle_blocks(x, calls, pilotcut, pilot_shift=pilot_shift)
    alens, locked = flags[0]
    ne = [lk for lk, a in zip(locked, alens) if a > 0]
    assert ne.count(False) >= 2 and ne.count(True) >= 2
    edges = [i for i in range(1, len(locked)) if locked[i] != locked[i - 1]]
    assert len(edges) == (1 if case == "lock_in" else 3) and all(sum(alens[:i]) % 64 for i in edges)
    r = run_chain(x, calls, pilot_shift=pilot_shift, serial=serial)
    assert r.status.stereo_detected == int(locked[-1]) == 1
    hold(f"case5_{case}{'_pilot_shift' if pilot_shift else ''}{'_serial' if serial else ''}", r, flags, pilotcut,
         pilot_shift=pilot_shift)


# ------------------------------------------------------------------------------------------------ case 6
def _deemph_launches(r):
    return [st for nm, st in r.trace if nm == "deemph_decim"]


@pytest.mark.parametrize("way", ["in_order_384k", "pipelined_1M", "in_order_1M"])
def test_split_launch_and_pipelined_drain(pilotcut, sig1, flags1, way):
    """Case 6.  Case 1's calls with the mono channel launched by itself: at 384 kHz (in-order chain, mono on the AGC stream
    beside the PLL), at 1 MS/s behind the IF resampler (pipelined chain: the drain path of enqueue_tail; 65536-sample blocks
    are 3146 audio samples, three pilot-cut tiles), and the same with FMR_PIPELINE=0.  The last call is traced: the
    de-emphasis kernel is launched twice, once per channel."""
    if way == "in_order_384k":
        x, calls, rate, pipe, flags = sig1, tc.CASE1_A, tc.FS_IF, None, flags1["a"]
    else:
        calls, rate, pipe = tc.CASE6_1M, 1e6, None if way == "pipelined_1M" else 0
        x = siggen.fm_stereo_iq(tc.n_samples(calls), rate)
        flags = tc.oracle_blocks(x, calls, pilotcut, in_rate=rate)
    old = os.environ.pop("FMR_PIPELINE", None)
    try:
        if pipe is not None:
            os.environ["FMR_PIPELINE"] = str(pipe)
        shape = fmr.chain_shape(mode=fmr.MODE_FM, input_rate=rate, enable_resampler=rate != tc.FS_IF, stereo=True,
                                max_block_len=tc.BLK, max_blocks=16)
    finally:
        os.environ.pop("FMR_PIPELINE", None)
        if old is not None:
            os.environ["FMR_PIPELINE"] = old
    assert shape.pipelined == (way == "pipelined_1M")
    r = run_chain(x, calls, in_rate=rate, pipeline=pipe, trace_last=True)
    assert r.status.stereo_detected == 1
    if rate != tc.FS_IF:
        assert tc.regime(r.alens[2])["tiles_per_block"] == [3, 3, 3]
    print(f"{way}: deemph_decim launches of the last call on streams {_deemph_launches(r)}")
    assert len(_deemph_launches(r)) == 2, r.trace
    hold(f"case6_{way}", r, flags, pilotcut)


def test_two_streams_in_one_chain(pilotcut, sig1):
    """Case 6, the s x stride side of every channel-1 pointer: two unlike streams in one chain, each against its own oracle."""
    n = len(sig1)
    xs = np.stack([sig1, tc.fm_iq(n, stream_id=1, n0=12345)])
    r = run_chain(xs, tc.CASE1_A)
    for s in range(2):
        rs = r.of_stream(s)
        assert rs.status.stereo_detected == 1
        hold(f"case6_two_streams_{s}", rs, tc.oracle_blocks(xs[s], tc.CASE1_A, pilotcut), pilotcut)
    assert not np.array_equal(r.audio[2][0], r.audio[2][1])

"""The multipath equaliser (k_mpf4 beside k_if_agc_wave) against the oracle where its code takes other paths: every tail
length of a chunk, blocks shorter than the taps, equalisers far shorter than a wave and on both sides of the host's
choice of instantiation, a start inside a call, the aftermath of a non-finite sample, several streams, the IF filter.

Every block of every call is compared: the call's discriminator output (debug tap 1) cut at the oracle's block lengths
against the oracle's after each FmDecoder::process, the audio of the whole run, and after the run the taps, the error,
the reset count, the AGC gain and the stereo flag.  The cases and their oracle runs are tests/equaliser_cases.py; that
each case is in the regime it is named for is tests/test_equaliser_cases.py (no GPU).

Bounds, the project's own (tests/test_gpu_parity.py): tap 1 2e-6 RMS per block (the largest difference for a block of fewer
than 16 samples), taps 1e-4 RMS, audio 1e-5 RMS, if_agc_gain rel 1e-5.  Lengths, finiteness masks, reset counts, the block
where equalisation starts and the stereo flag are compared exactly."""
import importlib
import os

import numpy as np
import pytest

import equaliser_cases as ec

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")

TAP_TOL, COEFF_TOL, AUDIO_TOL, GAIN_RTOL = 2e-6, 1e-4, 1e-5, 1e-5


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def run_chain(c):
    """The case through fmr.Chain call by call: per stream the discriminator output and the audio of every block, then
    the chain's final status, taps and the per-call counters."""
    os.environ["FMR_DEBUG_TAPS"] = "1"          # taps 1 (discriminator output) and 4 (AGC gains) stay readable
    try:
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=c.rate, enable_resampler=c.rate != ec.FS_IF, fmfilter_enable=c.fir is not None,
                       filter_coeff=c.fir_coeff(), stereo=True, deemphasis_us=50.0, multipath_stages=c.stages,
                       max_block_len=max(c.lens), max_blocks=max(len(k) for k in c.calls), n_streams=c.n_streams)
    finally:
        del os.environ["FMR_DEBUG_TAPS"]
    S = c.n_streams
    disc, audio = [[] for _ in range(S)], [[] for _ in range(S)]
    pos = b0 = 0
    for call in c.calls:
        m = sum(call)
        a, alen = ch.process_blocks(c.x[:, pos:pos + m], call)
        pos += m
        for s in range(S):
            ref = ec.reference(c.name, s)
            if_len = ref.if_len[b0:b0 + len(call)]
            assert [int(v) for v in alen] == [len(q) for q in ref.audio[b0:b0 + len(call)]], (c.name, b0)
            tap = ch.debug_read(1, stream=s)
            assert len(tap) == sum(if_len), (c.name, b0, len(tap), sum(if_len))
            assert len(ch.debug_read(4, stream=s)) == sum(if_len)
            disc[s] += np.split(tap.astype(np.float64), np.cumsum(if_len)[:-1])
            audio[s] += np.split(a[s], np.cumsum(alen)[:-1])
            st = ch.status(s)
            assert st.agc_fallback == 0 and st.agc_sync_timeouts == 0, (c.name, b0, st.agc_fallback, st.agc_sync_timeouts)
        b0 += len(call)
    out = [(disc[s], audio[s], ch.status(s), ch.multipath_coefficients(s)) for s in range(S)]
    ch.close()
    return out


def check_stream(c, s, disc, audio, st, coeff):
    ref = ec.reference(c.name, s)
    tag = "%s[%d]" % (c.name, s)
    # ---- discrete results first: they say what went wrong more plainly than a distance does
    print(f"{tag}: resets {st.multipath_resets} (oracle {ref.resets}), error {st.multipath_error!r} (oracle {ref.error!r}), "
          f"gain {st.if_agc_gain!r} (oracle {ref.gain!r}), equaliser from block {ref.active_from}")
    worst = (0.0, -1)
    bad_mask, over = [], []
    for b, (g, q) in enumerate(zip(disc, ref.disc)):
        assert len(g) == len(q), (tag, b)
        if not np.array_equal(np.isfinite(g), np.isfinite(q)):
            bad_mask.append(b)
        d = ec.block_distance(g, q)
        if d > worst[0]:
            worst = (d, b)
        if not d < TAP_TOL:
            over.append((b, len(q), d))
    ga, qa = np.concatenate(audio), np.concatenate(ref.audio)
    fin = np.isfinite(qa)
    aerr = rms(ga[fin] - qa[fin]) if len(ga) == len(qa) else np.inf
    cerr = rms(coeff - ref.coeff) if len(coeff) == len(ref.coeff) else np.inf
    print(f"{tag}: tap 1 worst block {worst[1]} at {worst[0]:.3e}, blocks over the bound {over[:8]}{' ...' if len(over) > 8 else ''}, "
          f"audio {aerr:.3e}, taps {cerr:.3e} (rms {rms(ref.coeff):.3f})")
    assert st.multipath_resets == ref.resets, (tag, st.multipath_resets, ref.resets)
    assert not bad_mask, (tag, "finiteness of tap 1 differs in blocks", bad_mask)
    if ref.active_from is not None and c.stages:      # a just-started equaliser is a delay: one block early or late is gross
        for b in (ref.active_from - 1, ref.active_from):
            while b >= 0 and not ref.if_len[b]:
                b -= 1
            assert ec.block_distance(disc[b], ref.disc[b]) < TAP_TOL, (tag, "equalisation starts in another block than the oracle's", b)
    assert not over, (tag, "tap 1 per block (block, length, distance)", over)
    assert len(ga) == len(qa) and np.array_equal(np.isfinite(ga), fin), tag
    assert aerr < AUDIO_TOL, (tag, aerr)
    assert len(coeff) == len(ref.coeff) == c.order, (tag, len(coeff))
    assert cerr < COEFF_TOL, (tag, cerr)
    if np.isfinite(ref.error):
        # error = 1 - |y|^2 of the last update, y = <state, taps>: |d error| <= 2 |y| |state| |d taps|, with |y| ~ 1,
        # |state| ~ sqrt(N) (the AGC holds |g x| at 1) and |d taps| <= sqrt(N) COEFF_TOL
        assert abs(st.multipath_error - ref.error) < 2 * c.order * COEFF_TOL, (tag, st.multipath_error, ref.error)
    else:
        assert np.array_equal(np.float64(st.multipath_error), np.float64(ref.error), equal_nan=True), (tag, st.multipath_error, ref.error)
    assert st.if_agc_gain == pytest.approx(ref.gain, rel=GAIN_RTOL), tag
    assert st.stereo_detected == ref.stereo, tag
    assert st.agc_fallback == 0 and st.agc_sync_timeouts == 0, tag


def check_case(name):
    c = ec.case(name)
    for s, (disc, audio, st, coeff) in enumerate(run_chain(c)):
        check_stream(c, s, disc, audio, st, coeff)


@pytest.mark.parametrize("per_call", [1, 4])
@pytest.mark.parametrize("stages", [2, 8])
def test_chunk_tails_and_block_edges(stages, per_call):
    """(a) Blocks of 1 .. 11 samples (N = 9 at two stages), 2046 .. 2051, 4095, 4098 and 6147: every cn % 4 of a last
    chunk, in the first chunk of a block and behind one, two and three whole ones; one block per call and four."""
    check_case("tails_E%d_by%d" % (stages, per_call))


@pytest.mark.parametrize("stages", ec.LENGTH_STAGES)
def test_equaliser_lengths(stages):
    """(b) 5, 9 and 13 taps (a fraction of the chain wave), and 317 / 321 and 637 / 641 taps: the last of k_mpf4<5> and the first
    of <10>, the last of <10> and the first of <20>.  Blocks of 2518 and 2519 samples: tails of two and three."""
    check_case("length_E%d" % stages)


def test_equaliser_starts_inside_a_call():
    """(c) The 101st block is the third of its call."""
    check_case("turn_on_384k")


def test_equaliser_start_skips_empty_if_blocks():
    """(c) 10 MS/s: input blocks of 1 to 20 samples that give no IF sample are not decoder blocks and do not count towards
    the warm-up (main.cpp:931-934, FmDecode.cpp:107-110)."""
    check_case("turn_on_10m")


@pytest.mark.parametrize("name", ec.WALKS)
def test_walk_of_a_nan_through_the_state(name):
    """(d) The NaN stays in the filter's state: every following block fails at its first sample and moves it down one cell,
    4 stages + 1 resets in all; in the block that starts with it in cell 0 the first push drops it and the block succeeds
    (MultipathFilter.cpp:164-197, FmDecode.cpp:107-123)."""
    check_case(name)


def test_error_overflow_with_a_finite_output():
    """(e) A finite sample so large that |y|^2 overflows: the block ends on its error, not on its output
    (MultipathFilter.cpp:190-192); while the sample is in the window mu is 0, once it has left adaptation goes on."""
    check_case("overflow")


def test_level_step():
    """(f) x 30 inside a block, / 30 twenty blocks later: |g x| <= 100, the AGC in its ordinary regime."""
    check_case("level_step")


def test_three_streams_one_of_them_with_a_nan():
    """(g) Three streams through three two-ray channels in one chain, each against its own oracle; stream 1 walks a NaN
    through its state, streams 0 and 2 never reset."""
    c = ec.case("three_streams")
    res = run_chain(c)
    assert res[0][2].multipath_resets == 0 and res[2][2].multipath_resets == 0
    assert res[1][2].multipath_resets == ec.reference(c.name, 1).resets == c.order
    for s, (disc, audio, st, coeff) in enumerate(res):
        check_stream(c, s, disc, audio, st, coeff)


def test_if_filter_in_front_of_the_equaliser():
    """(h) -f medium with -E 8, blocks of 2519 samples."""
    check_case("if_filter")

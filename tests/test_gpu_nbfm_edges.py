"""NBFM parity at key-up, on silence, in long calls and around non-finite input: the HIP chain against the oracle of
tests/nbfm_cases.py (whose conditions tests/test_nbfm_cases.py proves on the CPU), sample by sample.

Comparison rule, every case and every stream:
  * the audio lengths of every block equal the oracle's, and the audio is finite wherever the oracle's is;
  * for every wrap-ambiguous IF sample i (wrap margin < 2e-5: atan2f may round either way and a flipped wrap is a step of
    2 x bound) audio i ... i + 62 and discriminator sample i are left out -- at most 8 such samples and 0.5 % of a case;
  * on the kept samples the audio RMS error of every segment (floor, carrier, tail; each against its own samples) is under
    1e-6 (1e-5 through the resampler), and the worst sample is within 32 x the distance the oracle itself moves when every
    input float goes up one ulp at random (nbfm_cases.sensitivity; 1e-6 is about 32 x the oracle's own 3-5e-8 RMS);
  * after every call: the discriminator tap (debug_read 1) within 2e-6 RMS on the kept samples of every block (the measure
    and the bound of test_gpu_parity._fm_case's disc_err; the worst sample is recorded: the oracle's own moves by 1e-5 ... 1e-4
    on the noise floor when its input moves by one ulp, a weak sample's phase is that ill-conditioned); the gain sequence
    (debug_read 4) with the oracle's sign at every sample and its size within rel 1e-4; if_agc_gain at rel 1e-4 sign
    included, if_rms at rel 1e-5, baseband_level and baseband_mean x dev as test_nbfm_decoder_48k holds them;
  * agc_iterations, agc_fallback and agc_residual_history are recorded; agc_fallback == 0 is asserted only on steady
    calls: the oracle's gain moves by less than 2 % over the call and the one before it, or every chunk of the call holds
    a sample on the clamp (the stationary cycle entered before the call; see steady()).
Every figure goes to out/parity_report_nbfm.json.

Measured on an MI355X (DESIGN.md 2 has the table per case): audio RMS error 1.8e-8 ... 3.9e-8 per segment (8e-8 ... 9e-8
through the resampler), worst kept sample 0.2 ... 1.4 x the oracle's own one-ulp distance, discriminator tap 1.8e-7 ...
6.7e-7 RMS in its worst block (1.3e-6 through the resampler), gains within 4.8e-5, no sign error, no wrap that fell the other
way; the serial fallback runs in the call that holds the key-up (and in the one that holds the end of a cycle), nowhere
else.  The 22 tests take 7 s together, most of it the oracle on the CPU.
"""
import importlib
import json
import os

import numpy as np
import pytest

import nbfm_cases as nc

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FACTOR = 32
REPORT = {}


def _report(key, rec):
    REPORT[key] = rec
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_report_nbfm.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


def steady(ref, lo_prev, lo, hi):
    """A call [lo, hi) whose IF AGC has nothing to iterate on, by the oracle's gain alone.  Either the gain is smooth: it moves
    by less than 2 % over the call and the one before it.  Or the call lies in the stationary cycle: every chunk of 256
    samples (the chunks of k_agc_round count from the call's first sample) holds a sample on the clamp, where the gain
    forgets what it was (dg = 0), and the cycle is running when the call begins (one of the two samples in front of it is on
    the clamp).  The cycle has period two and a chunk an even length: the state the call starts from is then the right guess
    for every node, the first round reproduces it and the second can only confirm.  (A call that begins with the key-up has
    a clamped sample in every chunk too, but each chunk falls into the cycle with a parity of its own, which a Newton step
    with dg = 0 cannot mend: the serial kernel's case, recorded only.)"""
    g = ref.gain[lo_prev:hi]
    g = g[np.isfinite(g)]
    if len(g) == hi - lo_prev and g.min() > 0 and g.max() / g.min() < 1.02:
        return True
    with np.errstate(invalid="ignore"):
        on_clamp = np.abs(ref.gain[max(lo - 2, 0):hi] / nc.AGC[1] - 1.0) < 1e-6
    before, on_clamp = on_clamp[:lo - max(lo - 2, 0)], on_clamp[lo - max(lo - 2, 0):]
    return bool(before.any()) and all(on_clamp[k:k + 256].any() for k in range(0, hi - lo, 256))


def drive(cases, key=None):
    """The cases (one per stream, all with the same filter, deviation, rate and calls) through one chain, every call and
    every stream held to its oracle.  Returns the report records."""
    c0 = cases[0]
    refs = [c.reference() for c in cases]
    xs = np.stack([c.signal() for c in cases])
    S = len(cases)
    ch = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=float(c0.fs), enable_resampler=c0.fs != nc.FS, filter_coeff=c0.coeff,
                   nbfm_freq_dev=c0.freq_dev, max_block_len=max(max(c0.lens), 1), max_blocks=max(len(c) for c in c0.calls), n_streams=S)
    got = [[] for _ in range(S)]
    calls = [[] for _ in range(S)]
    flipped = [False] * S
    fails = []

    def check(ok, *what):       # every figure of a case is printed and reported before the first miss ends the test
        if not ok:
            fails.append(what)
    xo, blk, ao = 0, 0, [0] * S          # input offset, block index, IF = audio offset per stream
    try:
        for i, lens in enumerate(c0.calls):
            n_in = sum(lens)
            audio, alen = ch.process_blocks(xs[:, xo:xo + n_in], lens)
            xo += n_in
            blk += len(lens)
            for s, (c, r) in enumerate(zip(cases, refs)):
                want_len = r.alen[blk - len(lens):blk]
                assert [int(v) for v in alen] == want_len, (c.name, i, list(alen), want_len)
                n, lo = sum(want_len), ao[s]
                assert audio.shape[1] == n
                got[s].append(audio[s])
                st = ch.status(s)
                rec = dict(n=n, agc_iterations=st.agc_iterations, agc_fallback=st.agc_fallback, if_agc_gain=st.if_agc_gain,
                           ref_if_agc_gain=r.nb_gain_blk[blk - 1],
                           agc_residual_history=[float(v) for v in st.agc_residual_history[:max(0, min(st.agc_iterations, 16))]])
                calls[s].append(rec)
                where = f"{c.name} stream {s} call {i} (IF samples {lo} ... {lo + n})"
                if n:
                    # ---- stage taps of this call
                    disc, gain = ch.debug_read(1, s, cap=n + 16), ch.debug_read(4, s, cap=n + 16)
                    assert len(disc) == n == len(gain), where
                    amb = r.ambiguous[(r.ambiguous >= lo) & (r.ambiguous < lo + n)]
                    kd = np.ones(n, dtype=bool)
                    kd[amb - lo] = False
                    rd = r.disc[lo:lo + n]
                    flipped[s] |= bool(np.any(np.abs(disc[~kd] - rd[~kd]) > r.bound))
                    derr = np.abs(disc.astype(np.float64) - rd)
                    derr[~kd] = 0.0
                    rec["disc_max_err"] = float(derr.max())
                    # (_fm_case's disc_err is the RMS error of a block: here of every block of the call, on its kept samples)
                    edges = np.cumsum([0] + want_len)
                    drms = [nc.rms(derr[a:b][kd[a:b]]) for a, b in zip(edges[:-1], edges[1:])]
                    rec["disc_rms_err"] = float(max(drms))
                    rg = r.gain[lo:lo + n]
                    ok = np.isfinite(rg)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        grel = np.where(ok, np.abs(gain.astype(np.float64) / rg - 1.0), 0.0)
                    sign_bad = np.flatnonzero(ok & (np.signbit(gain) != np.signbit(rg)))
                    rec["gain_max_rel"] = float(np.max(grel))
                    rec["gain_sign_errors"] = int(len(sign_bad))
                    print(f"{where}: rounds {st.agc_iterations}, fallback {st.agc_fallback}, {['%.0e' % v for v in rec['agc_residual_history']]} | "
                          f"disc err rms {rec['disc_rms_err']:.2e} max {rec['disc_max_err']:.2e}, gain rel {rec['gain_max_rel']:.2e}, sign errors {len(sign_bad)} | "
                          f"if_agc_gain {st.if_agc_gain:.6g} / {r.nb_gain_blk[blk - 1]:.6g}")
                    check(len(sign_bad) == 0, where, "gain sign", sign_bad[:8] + lo, gain[sign_bad[:8]], rg[sign_bad[:8]])
                    check(rec["gain_max_rel"] < 1e-4, where, "gain", rec["gain_max_rel"], int(np.argmax(grel)) + lo)
                    check(rec["disc_rms_err"] < 2e-6, where, "disc", rec["disc_rms_err"], "block", int(np.argmax(drms)))
                    if c.poke:      # the footprint of the non-finite input in the discriminator: the same samples zeroed
                        check(np.array_equal(disc == 0.0, rd == 0.0), where, "footprint", np.flatnonzero((disc == 0.0) != (rd == 0.0))[:8] + lo)
                # ---- status after the call
                check(st.if_agc_gain == pytest.approx(r.nb_gain_blk[blk - 1], rel=1e-4), where, "if_agc_gain", st.if_agc_gain, r.nb_gain_blk[blk - 1])
                check(st.if_rms == pytest.approx(r.if_rms_blk[blk - 1], rel=1e-5, nan_ok=True), where, "if_rms", st.if_rms, r.if_rms_blk[blk - 1])
                if not flipped[s]:      # (a wrap that fell the other way is in the block's mean and level as well)
                    check(st.baseband_level == pytest.approx(r.bb_level_blk[blk - 1], rel=1e-4, abs=1e-7), where, "baseband_level", st.baseband_level, r.bb_level_blk[blk - 1])
                    check(st.baseband_mean * c.freq_dev == pytest.approx(r.tuning_blk[blk - 1], rel=1e-3, abs=1e-2), where, "tuning offset", st.baseband_mean * c.freq_dev, r.tuning_blk[blk - 1])
                rec["steady"] = bool(i > 0 and n and steady(r, lo - calls[s][i - 1]["n"], lo, lo + n))
                if rec["steady"]:
                    check(st.agc_fallback == 0, where, "agc_fallback on a steady call")
                ao[s] += n
    finally:
        ch.close()
    recs = []
    for s, (c, r) in enumerate(zip(cases, refs)):
        a = np.concatenate(got[s])
        assert len(a) == len(r.audio)
        check(np.all(np.isfinite(a[np.isfinite(r.audio)])), c.name, "non-finite audio")
        a = np.where(np.isfinite(a), a, np.inf)
        ka, _ = nc.kept(r)
        excluded = float(np.mean(~ka))
        seg_sens, worst_sens = nc.sensitivity(c)
        d = np.abs(a - r.audio)
        d[~ka] = 0.0
        seg = [nc.rms(d[lo:hi][ka[lo:hi]]) for lo, hi in c.segments]
        worst, at = float(d.max()), int(np.argmax(d))
        tol = 1e-5 if c.fs != nc.FS else 1e-6
        rec = dict(case=c.name, stream=s, n=len(a), ambiguous=[int(v) for v in r.ambiguous], excluded_share=excluded, flipped=flipped[s],
                   audio_rms_err=seg, audio_rms=[nc.rms(r.audio[lo:hi]) for lo, hi in c.segments], audio_max_err=worst, audio_max_err_at=at,
                   sensitivity_rms=seg_sens, sensitivity_max=worst_sens, max_err_over_sensitivity=worst / worst_sens if worst_sens else 0.0,
                   negative=r.negative, clamped=r.clamped, resets=r.resets, calls=calls[s])
        _report(f"{key or c.name}" + (f"_s{s}" if S > 1 else ""), rec)
        recs.append(rec)
        print(f"{c.name} stream {s}: audio RMS error per segment {['%.2e' % v for v in seg]} (oracle +1 ulp: {['%.2e' % v for v in seg_sens]}), "
              f"worst kept sample {worst:.2e} at {at} (oracle +1 ulp: {worst_sens:.2e}, x{rec['max_err_over_sensitivity']:.1f}), "
              f"excluded {excluded:.2%}, fallbacks {[k['agc_fallback'] for k in calls[s]]}")
        check(excluded <= 0.005, c.name, "excluded", excluded)
        check(max(seg) < tol, c.name, "audio RMS error per segment", seg)
        check(worst <= FACTOR * worst_sens, c.name, "worst kept sample", worst, at, "against", FACTOR, "x", worst_sens)
    for f in fails:
        print("MISS:", *f)
    assert not fails, (len(fails), fails[:6])
    return recs


# ------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", nc.FILTER_CASES)
def test_four_filters(name):
    """1: default, narrow, medium and wide at 8000, wide at 17000; floor 1e-4, level 0.2 (three fast attacks, two cycles).
    The two calls that lie whole in the cycle are steady: no serial fallback there."""
    rec = drive([nc.CASES[name]])[0]
    if name.startswith("wide"):
        assert sum(k["steady"] for k in rec["calls"]) >= 2, [k["steady"] for k in rec["calls"]]


def test_persistent_negative_gain():
    """2: the gain turns negative at key-up and stays negative through the carrier, the noise behind it and every later call."""
    rec = drive([nc.CASES["negative"]])[0]
    last = rec["calls"][-4:]
    assert all(k["if_agc_gain"] < 0 and k["ref_if_agc_gain"] < 0 for k in last), [(k["if_agc_gain"], k["ref_if_agc_gain"]) for k in last]


def test_exact_silence_cold():
    """3: the first call of a new chain is 60 blocks of zeros; on into the clamp at 1e5, key-up from the clamp, zeros again."""
    rec = drive([nc.CASES["silence"]])[0]
    assert rec["calls"][0]["ref_if_agc_gain"] == 1e5 and rec["calls"][0]["if_agc_gain"] == pytest.approx(1e5, rel=1e-6)


@pytest.mark.parametrize("name", nc.KEYUP_CASES)
def test_where_key_up_falls(name):
    """4: mid-chunk (sample 131 of a chunk of 256), on a chunk edge, on the first and on the last sample of a call."""
    c = nc.CASES[name]
    k = c.n[0]
    assert {"keyup_mid_chunk": k % 256 == 131, "keyup_chunk_edge": k % 256 == 0 and k % nc.CALL != 0,
            "keyup_call_first": k % nc.CALL == 0, "keyup_call_last": (k + 1) % nc.CALL == 0}[name]
    drive([c])


@pytest.mark.parametrize("name", ["wide_8000_single", "wide_8000_ragged"])
def test_call_partitions_of_the_cycle_case(name):
    """5: the cycle case one block per call, and in ragged calls of [1000, 1, 47, 2048, 999, 48, 49, 127, 128, 0] (8 x 2048
    per call is test_four_filters[wide_8000]); each partition against the oracle on the same blocks."""
    drive([nc.CASES[name]])


def test_tiny_calls_in_a_row():
    """6: single-block calls of 1, 1, 47, 48, 49, 5, 62, 63, 126, 127, 128 samples on the carrier between normal blocks: 47 / 48
    crosses the switch from k_fm_block2 to the matrix-core filter with k_fir_finish, 127 / 128 the short-block rule, and
    the halos of both FIRs (orders 126 and 62) carry over three and more calls."""
    rec = drive([nc.CASES["tiny_calls"]])[0]
    assert [k["n"] for k in rec["calls"][3:3 + len(nc.TINY)]] == nc.TINY


@pytest.mark.parametrize("name", ["long_wide", "long_default"])
def test_long_call_over_the_node_pass_tile(name):
    """7: one call of 262 blocks = 2096 chunks (agc_node_pass takes 2048 per tile), key-up 131 samples into chunk 2047: with
    the wide filter the cycle runs across the tile hand-off, with the default filter at level 0.005 the gain falls smoothly
    across it (no chunk with dg = 0); an 8-block call follows."""
    rec = drive([nc.CASES[name]])[0]
    assert -(-rec["calls"][0]["n"] // 256) == 2096 and rec["calls"][1]["n"] == 8 * nc.BLK


@pytest.mark.parametrize("name", ["nan3", "inf1", "nan_in_30"])
def test_nan_and_inf(name):
    """8: three NaN samples (one +Inf sample; one NaN inside a call of 30 samples, which takes k_fm_block2) mid-carrier: the
    AGC resets to 1, the discriminator zeroes the differences -- the same ones as the oracle's --, the audio stays finite
    and on the oracle's over the whole stream."""
    rec = drive([nc.CASES[name]])[0]
    assert rec["resets"] >= 126
    if name == "nan_in_30":
        assert [30] in nc.CASES[name].calls


def test_three_unlike_streams():
    """9: the cycle case, exact silence and a steady tone in one chain, each stream held to its own oracle, status per stream;
    the steady stream beside the cycling one keeps agc_fallback == 0 (asserted on its steady calls: at least the last five)."""
    recs = drive([nc.CASES[n] for n in nc.STREAM_CASES], key="streams")
    assert sum(k["steady"] for k in recs[2]["calls"]) >= 5 and all(k["steady"] for k in recs[2]["calls"][-5:])
    assert recs[0]["clamped"] >= 20000 and recs[1]["audio_max_err"] == 0.0


@pytest.mark.parametrize("name", ["resampled_fast", "resampled_negative"])
def test_through_the_resampler(name):
    """10: 384 kS/s -> 48 k, the fast-attack and the negative-gain case synthesised at 384 k; audio to 1e-5 per segment."""
    drive([nc.CASES[name]])

"""AM-family parity at the call lengths at which the time-parallel audio tail takes more than one workgroup, tile and
wave, with the audio AGC off its clamp, and across the hand-off to the serial tail.

A long call is 257 blocks of 2048 samples at 48 kHz = 526 336 samples = 2056 chunks of 256: 33 workgroups of k_af_round
(its last-arrival ticket has 33 arrivals), five tiles of af_node_pass (512 chunks each), two waves of k_dc_nodes (2048
chunks each) and the second tile of agc_node_pass (2048 chunks at 256 threads: the first use of old_next).  The inputs,
the oracle runs and the float64 model of the Newton rounds are those of tests/am_tail_model.py; their conditions are
checked on the CPU by tests/test_am_tail_model.py.

Every call of every case is held to the oracle: audio lengths, audio RMS error < 1e-6 (a decoder fed identical samples)
and max |error| < 1e-5, af_agc_gain at rel 1e-6, if_agc_gain at rel 1e-5 (AM, DSB) or 1e-4 (SSB modes), if_rms at
1e-5.  af_agc_fallback is asserted where the exact model is sure of it (am_tail_model.expect_fallback) and recorded
otherwise; agc_fallback is asserted 0 on the steady inputs from the second call on (the IF AGC starts a cold chain at
gain 1, a step of its own: measured 1 there, the IF goes through k_if_agc_fallback) and recorded on the stepped ones.
Every figure goes to out/parity_report.json under am_long_<case>_call<i>; every test prints the path it took and
asserts it.

Measured on an MI355X: audio RMS error 0 ... 4.9e-7 (0 ... 7e-14 where both sides ran the serial recurrence), max
|error| <= 4.0e-6, af_agc_gain within 2.9e-7; a long call takes 1.3-2.7 ms of wall time, 100-130 ms where the IF AGC
alone falls back to its serial kernel and 210-240 ms where the audio tail does too (every cold long call but USB's);
the module runs in 30 s, 20 s of which are the oracle and the model on the CPU.
"""
import importlib
import time

import numpy as np
import pytest

import am_tail_model as atm
import oracle_py as ora
import siggen
from test_gpu_parity import _report, rms

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

GM = {"am": fmr.MODE_AM, "dsb": fmr.MODE_DSB, "usb": fmr.MODE_USB, "lsb": fmr.MODE_LSB, "cw": fmr.MODE_CW, "wspr": fmr.MODE_WSPR}
BLK, LONG = atm.BLK, atm.LONG


@pytest.fixture(scope="module", autouse=True)
def _references():
    atm.prefetch()


def path_of(n):
    """What a call of n IF samples runs, from the sizes in the kernels (kernels_par.hpp, fmradion_amd.hip)."""
    nc = -(-n // 256)
    return dict(chunks=nc, tail_samples=n - (nc - 1) * 256, af_workgroups=-(-nc // 64), af_tiles=-(-nc // 512),
                dc_waves=min(8, -(-nc // 2048)), agc_tiles=-(-nc // 2048))


def chain(mode, am_narrow, max_blocks, n_streams=1, **kw):
    kw.setdefault("input_rate", 48e3)
    kw.setdefault("max_block_len", BLK)
    return fmr.Chain(mode=GM[mode], filter_coeff=am_narrow, max_blocks=max_blocks, n_streams=n_streams, **kw)


def check(key, i, mode, st, audio, alen, o, m, steady, wall, rms_tol=1e-6, af_rel=1e-6, if_rel=None, expect=None):
    """One call of one stream against its oracle call o and model call m.  Returns the measured figures."""
    same_len = [int(v) for v in alen] == [int(v) for v in o["alen"]] and len(audio) == len(o["audio"])
    d = audio - o["audio"] if same_len else np.array([np.inf])
    err, mx = rms(d), float(np.max(np.abs(d)))
    exp = atm.expect_fallback(m) if expect is None else expect
    if_rel = if_rel or (1e-5 if mode in ("am", "dsb") else 1e-4)
    rec = dict(n=len(audio), audio_rms_err=err, audio_max_err=mx, audio_rms=rms(o["audio"]), af_agc=st.af_agc_gain, ref_af_agc=o["af_agc"],
               if_agc=st.if_agc_gain, ref_if_agc=o["if_agc"], if_rms=st.if_rms, ref_if_rms=o["if_rms"],
               af_fallback=st.af_agc_fallback, af_fallback_expected=exp, model_accepted=m["accepted"],
               model_moves=[float(v) for v in m["moves"]], model_resets=m["resets"], agc_fallback=st.agc_fallback,
               agc_iters=st.agc_iterations, agc_hist=[float(v) for v in st.agc_residual_history[:min(st.agc_iterations, 16)]],
               oracle_gain_min=float(o["gains"].min()), oracle_clamp_fraction=float(np.mean(o["gains"] >= np.float32(1.5))),
               wall_ms=1e3 * wall, **path_of(len(audio)))
    _report(f"am_long_{key}_call{i}", **rec)
    print(f"{key} call {i}: {rec['chunks']} chunks (last {rec['tail_samples']}), k_af_round x {rec['af_workgroups']} workgroups, af_node_pass x "
          f"{rec['af_tiles']} tiles, k_dc_nodes x {rec['dc_waves']} waves, agc_node_pass x {rec['agc_tiles']} tiles | rms err {err:.2e} max {mx:.2e} | "
          f"af gain {st.af_agc_gain:.7f} / {o['af_agc']:.7f}, oracle min {rec['oracle_gain_min']:.3f}, on the clamp {rec['oracle_clamp_fraction']:.3f} | "
          f"af_agc_fallback {st.af_agc_fallback} (model: {exp}, accepted {m['accepted']}, {['%.0e' % v for v in m['moves']]}) | "
          f"agc_fallback {st.agc_fallback}, rounds {st.agc_iterations}, {['%.0e' % v for v in rec['agc_hist']]} | {rec['wall_ms']:.1f} ms")
    assert same_len, ([int(v) for v in alen][:4], o["alen"][:4], len(audio), len(o["audio"]))
    assert err < rms_tol and mx < 1e-5, (err, mx)
    assert st.af_agc_gain == pytest.approx(o["af_agc"], rel=af_rel)
    assert st.if_agc_gain == pytest.approx(o["if_agc"], rel=if_rel)
    assert st.if_rms == pytest.approx(o["if_rms"], rel=1e-5)
    if exp is not None:
        assert st.af_agc_fallback == exp, (st.af_agc_fallback, exp, m["moves"])
    if steady and i > 0:        # (a cold call is a step from nothing for the IF AGC as well: its gain starts at 1)
        assert st.agc_fallback == 0
    return rec


def run(key, mode, ch, xs, calls, refs, steady, **kw):
    """calls (lists of block lengths) of the rows of xs through ch; refs[s] = (oracle calls, model calls) of stream s."""
    xs = np.atleast_2d(xs)
    recs, o = [], 0
    for i, lens in enumerate(calls):
        n = sum(lens)
        t0 = time.perf_counter()
        audio, alen = ch.process_blocks(xs[:, o:o + n], lens)
        wall = time.perf_counter() - t0
        o += n
        recs.append([check(key if len(xs) == 1 else f"{key}_s{s}", i, mode, ch.status(s), audio[s], alen, refs[s][0][i], refs[s][1][i],
                           steady[s] if isinstance(steady, (list, tuple)) else steady, wall, **kw) for s in range(len(xs))])
    return recs


def assert_long_path(rec):
    assert rec["chunks"] > 2048 and rec["af_workgroups"] == 33 and rec["af_tiles"] == 5 and rec["dc_waves"] == 2 and rec["agc_tiles"] == 2, rec


# ------------------------------------------------------------------------------------------------- A: a moving gain
@pytest.mark.parametrize("mode", ["am", "dsb"])
def test_moving_gain_long_calls(mode, am_narrow):
    """Input A in calls of 257, 257, 70 and 257 blocks: the gain is off the clamp for most of every call, the calls
    after the first are accepted at round 6 in the model; the cold first call goes to the serial tail."""
    ch = chain(mode, am_narrow, LONG)
    recs = run(f"a_{mode}", mode, ch, atm.signal("a"), atm.long_calls(), [atm.reference(mode, "a")], steady=False)
    ch.close()
    for i in (0, 1, 3):
        assert_long_path(recs[i][0])
    assert recs[0][0]["af_fallback"] == 1 and recs[0][0]["af_fallback_expected"] == 1            # the model is sure of the cold call
    assert min(r[0]["oracle_gain_min"] for r in recs[1:]) < 1.3 and max(r[0]["oracle_clamp_fraction"] for r in recs[1:]) < 2 / 3
    if mode == "am":
        assert [r[0]["af_fallback"] for r in recs[1:]] == [0, 0, 0] == [r[0]["af_fallback_expected"] for r in recs[1:]]


# ------------------------------------------------------------------------------ B: under the clamp throughout
@pytest.mark.parametrize("name", ["b", "bs"], ids=["steady", "stepped"])
@pytest.mark.parametrize("mode", atm.SSB_LIKE)
def test_gain_under_the_clamp_long_calls(mode, name, am_narrow):
    """The two-tone input, steady and with input A's level steps: in USB and LSB no chunk in front of a tile edge ends
    on the clamp (M != 0 there), which is where a node pass that loses the old node at the edge costs a round.

    The steady USB calls are where the IF AGC's rounds end soonest (node movements 3e-3, 1e-5, 3e-6) and the gains of the
    accepted pass are furthest from the oracle's: without the integration pass that k_agc_round adds behind an accepted
    AM round, af_agc_gain ended the second call 1.3e-6 from the oracle's (1e-6 asserted); with it 2.9e-7."""
    ch = chain(mode, am_narrow, LONG, enable_resampler=False)
    refs = atm.reference(mode, name)
    recs = run(f"{name}_{mode}", mode, ch, atm.signal(name), atm.long_calls(), [refs], steady=(name == "b"))
    ch.close()
    for i in (0, 1, 3):
        assert_long_path(recs[i][0])
    edge = [int(np.count_nonzero(m["edge_M"])) for m in refs[1]]
    print("chunks in front of a tile edge with M != 0 (model), per call:", edge, "| af_agc_fallback per call:", [r[0]["af_fallback"] for r in recs])
    if mode in ("usb", "lsb"):
        assert max(r[0]["oracle_clamp_fraction"] for r in recs[1:]) < 0.05 and min(edge[1], edge[3]) >= 3
        assert [r[0]["af_fallback"] for r in recs[1:]] == [0, 0, 0] == [r[0]["af_fallback_expected"] for r in recs[1:]]


def test_step_in_front_of_a_tile_edge(am_narrow):
    """USB, the level rises sixfold 12 chunks in front of chunk 1024 of the second call: the exact model accepts that
    call at round 6 with margin (<= 1e-6, then <= 1e-11), a node pass that reads the overwritten node at the tile edge is
    at 4e-7 there and would hand half a million samples to one lane."""
    ch = chain("usb", am_narrow, LONG, enable_resampler=False)
    refs = atm.edge_reference()
    recs = run("edge_usb", "usb", ch, atm.edge_signal(), atm.long_calls()[:2], [refs], steady=False)
    ch.close()
    m = refs[1][1]
    assert_long_path(recs[1][0])
    assert m["accepted"] == 6 and m["moves"][4] <= 1e-6 and m["moves"][5] <= 1e-11 and m["edge_M"][1] != 0.0
    assert recs[1][0]["af_fallback_expected"] == 0 and recs[1][0]["af_fallback"] == 0


# ------------------------------------------------------------------------------------------------------- C: edges
EDGE_CALLS = [[BLK] * 70,                                   # warm-up
              [BLK] * 8,                                    # 64 chunks: one workgroup of k_af_round, full
              [BLK] * 8 + [256],                            # 65: the second workgroup has one lane
              [1, 159] + [BLK] * 63 + [1888],               # 512: one full tile of af_node_pass, behind blocks of 1 and 159 samples
              [BLK] * 64 + [256],                           # 513: the second tile has one chunk
              [BLK] * 256,                                  # 2048: one full tile of agc_node_pass, one full wave of k_dc_nodes
              [159, 1] + [BLK] * 256 + [96],                # 2049: the second tile / wave has one chunk
              [1] + [BLK] * 8 + [77]]                       # 65 chunks, the last of 78 samples
EDGE_CHUNKS = [560, 64, 65, 512, 513, 2048, 2049, 65]


def test_chunk_count_edges(am_narrow):
    """Input A in AM after a warm-up call: calls of exactly 64, 65, 512, 513, 2048 and 2049 chunks and one that ends inside
    a chunk; two of them begin with blocks of 1 and 159 samples (fewer than FMR_AM_DE_WARM = 160: the de-emphasis of the
    first chunks runs from the carried state)."""
    n = sum(map(sum, EDGE_CALLS))
    x = atm.signal("a")[:n]
    o, m = atm.start(("ref", "am", "edges"), "am", lambda: x, EDGE_CALLS)
    ch = chain("am", am_narrow, max(len(c) for c in EDGE_CALLS))
    recs = run("edges_am", "am", ch, x, EDGE_CALLS, [(o.result(), m.result())], steady=False)
    ch.close()
    assert [r[0]["chunks"] for r in recs] == EDGE_CHUNKS and [r[0]["tail_samples"] for r in recs] == [256] * 7 + [78]
    assert [r[0]["af_workgroups"] for r in recs[1:3]] == [1, 2] and [r[0]["af_tiles"] for r in recs[3:5]] == [1, 2]
    assert [(r[0]["agc_tiles"], r[0]["dc_waves"]) for r in recs[5:7]] == [(1, 1), (2, 2)]
    print("af_agc_fallback per call:", [r[0]["af_fallback"] for r in recs], "expected (None: recorded only):", [r[0]["af_fallback_expected"] for r in recs])
    # the model is sure of the time-parallel tail in the calls of 512, 513, 2048 and 2049 chunks (the three calls of 64 and 65
    # chunks lie on the clamp: accepted at round 2 with no movement, 5e-3 at round 1 -- recorded)
    assert [r[0]["af_fallback_expected"] for r in recs[3:7]] == [0, 0, 0, 0] == [r[0]["af_fallback"] for r in recs[3:7]]


# ------------------------------------------------------------------------------------------ D: the serial hand-off
def test_serial_hand_off_and_the_call_after(am_narrow):
    """Input A's first call on a cold chain: the model's movement at round 6 is 0.4, k_am_tail runs (af_agc_fallback
    == 1) and the next call starts from the state it left -- parity of both calls, and af_agc_fallback == 0 on the second."""
    ch = chain("am", am_narrow, LONG)
    refs = atm.reference("am", "a")
    recs = run("handoff_am", "am", ch, atm.signal("a")[:2 * LONG * BLK], atm.long_calls()[:2], [refs], steady=False)
    ch.close()
    assert refs[1][0]["moves"][5] > 0.1 and refs[1][0]["resets"] == 0
    assert [r[0]["af_fallback"] for r in recs] == [1, 0]
    print("path: call 0 serial tail (k_am_tail), call 1 time-parallel tail from the state the serial tail left")


def test_serial_hand_off_per_stream(am_narrow):
    """Three streams in one chain, two long calls: stream 0 is cold input A (serial tail in the first call), stream 1
    siggen.am_iq (its cold call is recorded: the model meets non-finite resets there; on the clamp and accepted in the
    second), stream 2 silence (every chunk ends on the clamp, no node moves at round 3: accepted in both calls).  Flags,
    gains and parity per stream: the first call has a stream in the serial tail beside one that committed."""
    n, calls = 2 * LONG * BLK, atm.long_calls()[:2]
    xs = np.stack([atm.signal("a")[:n], siggen.am_iq(n, atm.FS), np.zeros(n, dtype=np.complex64)])
    started = [atm.start(("ref", "am", "a2"), "am", lambda: xs[0], calls), atm.start(("ref", "am", "am_iq2"), "am", lambda: xs[1], calls),
               atm.start(("ref", "am", "silence2"), "am", lambda: xs[2], calls)]
    refs = [(o.result(), m.result()) for o, m in started]
    silent = refs[2][1]
    assert all(m["accepted"] is not None and m["moves"][-1] == 0.0 and m["resets"] == 0 for m in silent), [m["moves"] for m in silent]
    ch = chain("am", am_narrow, LONG, n_streams=3)
    xs_run = np.ascontiguousarray(xs)
    recs, o = [], 0
    for i, lens in enumerate(calls):
        t0 = time.perf_counter()
        audio, alen = ch.process_blocks(xs_run[:, o:o + sum(lens)], lens)
        wall = time.perf_counter() - t0
        o += sum(lens)
        recs.append([check(f"streams_s{s}", i, "am", ch.status(s), audio[s], alen, refs[s][0][i], refs[s][1][i], s > 0, wall,
                           if_rel=1e-5, expect=0 if s == 2 else None) for s in range(3)])
    ch.close()
    flags = [[r["af_fallback"] for r in call] for call in recs]
    print("af_agc_fallback [call][stream]:", flags)
    assert flags[0][0] == 1 and flags[0][2] == 0 and flags[1] == [0, 0, 0]
    assert recs[1][1]["oracle_clamp_fraction"] == 1.0 and recs[1][1]["af_fallback_expected"] == 0


# ------------------------------------------------------------------------------------------ E: through the resampler
def test_long_call_through_the_resampler(am_narrow):
    """AM, 384 kS/s -> 48 k, input A's modulation: a warm-up call of 70 and a call of 257 blocks of 16 384 input samples
    (2048 IF samples each).  The IF comes from the GPU's front end (fp32 FMA against the oracle's float64 sums, 2e-6
    relative), so the audio tolerance is test_am_config3_full_chain's 1e-5 and the gains are held at 1e-5 as well."""
    blk = 16384
    calls = [[blk] * 70, [blk] * LONG]
    n = sum(map(sum, calls))
    x = atm.cached(("signal", "a384"), lambda: atm.input_a(n, fs=384e3))
    o, m = atm.start(("ref", "am", "a384"), "am", lambda: x, calls, resampler=lambda: ora.IfResampler(384e3, 48e3))
    ch = chain("am", am_narrow, LONG, input_rate=384e3, enable_resampler=True, max_block_len=blk)
    recs = run("resampled_am", "am", ch, x, calls, [(o.result(), m.result())], steady=False, rms_tol=1e-5, af_rel=1e-5)
    forms = ch.front_end_forms()
    ch.close()
    print("front-end forms:", sorted(forms))
    assert_long_path(recs[1][0])
    assert forms and recs[1][0]["n"] == LONG * 2048

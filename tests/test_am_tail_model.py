"""The float64 model of the audio AGC's multiple shooting (tests/am_tail_model.py) against the CPU oracle, and the
conditions on the inputs of tests/test_gpu_am_long_calls.py, which are conditions on the oracle alone.

Figures of the oracle over the calls of 257, 257, 70 and 257 blocks of 2048 samples (per-block AF gain after the first
call: min ... max, fraction of the blocks that end on the clamp 1.5), and of the exact model (round accepted, movement
at the last two rounds; cold = the first call):
  input A, AM    0.918 ... 1.5, 0.11-0.14 on the clamp;  cold: not accepted, 0.4 at round 6;  warm: round 6,
                 8e-8 / 1e-9 / 6e-9 at round 5 and <= 6e-15 at round 6
  input A, DSB   1.05 ... 1.5, 0.60-0.62 on the clamp (1.448 ... 1.5 in the call of 70 blocks);  cold: 0.2 at round 6
  input B, USB   steady 1.399 ... 1.426, never on the clamp, round 4;  stepped 0.86 ... 1.5, 0.8-2.7 %, round 6
  input B, LSB   steady 1.408 ... 1.419, never on the clamp, round 4;  stepped 0.87 ... 1.5, 1.9-2.9 %, round 6
  input B, CW    steady 0.94 ... 1.5, 17-23 %;  stepped 0.42 ... 1.5, 24-30 %;  no call accepted within 6 rounds
  input B, WSPR  steady 0.97 ... 1.5, 17-23 %;  stepped 0.46 ... 1.5, 24-30 %

Two of the conditions cannot be met by the inputs as they are specified, and the tests say so instead of asserting them:
  * DSB takes the real part of a carrier that turns at 37 Hz: half the envelope's power, so the AGC's equilibrium gain
    (1 / rms) lies above the clamp and the gain only leaves it behind the level steps.  "min < 1.3 and clamp fraction
    < 0.5" holds for AM; for DSB the tests assert min < 1.3 in the long calls and that more than a third of every
    call's blocks end off the clamp.
  * The 500 Hz filter of CW and WSPR passes one edge tone of the two-tone input and little else, and the gain of these
    two modes (rate 0.00125) swings between 0.94 and the clamp on the steady input: "on the clamp for < 5 %" holds for
    USB and LSB; for CW and WSPR the tests assert < 35 %.
"""
import numpy as np
import pytest

import am_tail_model as atm

REL = 2.0 ** -23        # the oracle returns its gain as a float


@pytest.fixture(scope="module", autouse=True)
def _references():
    atm.prefetch()


def clamp_fraction(gains):
    return float(np.mean(gains >= np.float32(atm.AF_MAX)))


def show(mode, name, orc, mod):
    for i, (o, m) in enumerate(zip(orc, mod)):
        print(f"{mode} {name} call {i}: gain {o['gains'].min():.4f} ... {o['gains'].max():.4f}, on the clamp {clamp_fraction(o['gains']):.3f} | "
              f"model: accepted {m['accepted']}, movements {['%.0e' % v for v in m['moves']]}, resets {m['resets']}, "
              f"M in front of the tile edges {['%.2g' % v for v in m['edge_M']]}, expects fallback {atm.expect_fallback(m)}")


@pytest.mark.parametrize("mode,name", atm.LONG_CASES, ids=[f"{m}_{n}" for m, n in atm.LONG_CASES])
def test_serial_recurrence_ends_at_the_oracles_gain(mode, name):
    """After every call: the model's recurrence on the stage classes' signal against get_af_agc_current_gain().  The
    carried gain is the fixed point of the model's own rounds; on the first and the shortest call it is also walked
    sample by sample, and the two are the same double."""
    orc, mod = atm.reference(mode, name)
    show(mode, name, orc, mod)
    for i, (o, m) in enumerate(zip(orc, mod)):
        rel = abs(m["serial"] / o["af_agc"] - 1.0)
        print(f"  call {i}: model {m['serial']:.9f} oracle {o['af_agc']:.9f} rel {rel:.1e}")
        assert rel <= REL, (i, m["serial"], o["af_agc"])
    for i in (0, 2):
        assert atm.serial(mod[i]["v"], mod[i]["g0"], atm.af_rate(mode)) == mod[i]["serial"], i


def test_model_on_the_clamp_has_nothing_to_solve():
    """siggen.am_iq keeps the oracle's gain at 1.5 after every block: every chunk ends with dg = 0 and the model accepts
    at round 1 with no movement at all -- what every oracle-checked AM call has been so far."""
    import siggen
    n = 128 * atm.BLK
    o, m = atm.start(("ref", "am", "clamp64"), "am", lambda: siggen.am_iq(n, atm.FS), [[atm.BLK] * 64] * 2)
    o, m = o.result()[1], m.result()[1]
    print("gain", o["gains"].min(), o["gains"].max(), "movements", m["moves"], "M != 0 in", int(np.count_nonzero(m["edge_M"])), "edge chunks")
    assert np.all(o["gains"] == np.float32(1.5)) and m["accepted"] == 1 and m["moves"] == [0.0] and m["resets"] == 0


@pytest.mark.parametrize("mode", ["am", "dsb"])
def test_input_a_moves_the_gain(mode):
    orc, mod = atm.reference(mode, "a")
    show(mode, "a", orc, mod)
    for i, o in enumerate(orc[1:], 1):
        lo, frac = float(o["gains"].min()), clamp_fraction(o["gains"])
        if mode == "am":
            assert lo < 1.3 and frac < 0.5, (i, lo, frac)
        else:           # (the module's docstring: the equilibrium of DSB lies above the clamp)
            assert frac < 2 / 3 and lo < (1.3 if len(o["gains"]) == atm.LONG else 1.46), (i, lo, frac)
    assert all(m["resets"] == 0 for m in mod)


def test_input_a_cold_call_is_not_accepted_and_the_next_is():
    """Case D: the model's movement at round 6 of the cold call is far from accepted, the call behind it is accepted
    with margin."""
    _, mod = atm.reference("am", "a")
    assert atm.expect_fallback(mod[0]) == 1 and mod[0]["moves"][-1] > 0.1, mod[0]["moves"]
    assert [atm.expect_fallback(m) for m in mod[1:]] == [0, 0, 0] and [m["accepted"] for m in mod[1:]] == [6, 6, 6]


@pytest.mark.parametrize("mode", atm.SSB_LIKE)
@pytest.mark.parametrize("name", ["b", "bs"])
def test_input_b_stays_under_the_clamp(mode, name):
    orc, mod = atm.reference(mode, name)
    show(mode, name, orc, mod)
    for i, (o, m) in enumerate(zip(orc[1:], mod[1:]), 1):
        frac = clamp_fraction(o["gains"])
        if mode in ("usb", "lsb"):
            assert frac < 0.05, (i, frac)
            assert np.count_nonzero(m["edge_M"]) >= len(m["edge_M"]) - 1, m["edge_M"]     # M != 0 at the tile edges
        else:
            assert frac < 0.35, (i, frac)
    assert all(m["resets"] == 0 for m in mod)


def test_stale_read_costs_a_round_where_no_chunk_is_cut():
    """The steady two-tone input in USB, warm: M != 0 in front of every tile edge, the exact pass is accepted at round 4
    and a pass that drops the correction of each tile's first chunk at round 5.  On the cold call the exact pass needs
    all six rounds and the other is not accepted."""
    x, calls = atm.signal("b"), atm.long_calls()
    _, exact = atm.reference("usb", "b")
    stale = atm.model_run("usb", x[:2 * atm.LONG * atm.BLK], calls[:2], stale=True)
    print("exact:", [(m["accepted"], ["%.0e" % v for v in m["moves"]]) for m in exact[:2]])
    print("stale:", [(m["accepted"], ["%.0e" % v for v in m["moves"]]) for m in stale])
    assert exact[1]["accepted"] == 4 and stale[1]["accepted"] == 5
    assert exact[0]["accepted"] == 6 and exact[0]["moves"][5] <= 1e-11 and exact[0]["resets"] == 0
    assert stale[0]["accepted"] is None and stale[0]["moves"][5] >= 1e-8


def test_a_step_in_front_of_a_tile_edge_separates_the_two_passes():
    """Section 3's case with margin: a warm call that the exact model accepts at round 6 (<= 1e-6 at round 5, <= 1e-11 at
    round 6) and the stale pass does not (>= 1e-8 at round 6)."""
    _, exact = atm.edge_reference()
    stale = atm.model_run("usb", atm.edge_signal(), atm.long_calls()[:2], stale=True)
    print("exact:", [(m["accepted"], ["%.0e" % v for v in m["moves"]]) for m in exact])
    print("stale:", [(m["accepted"], ["%.0e" % v for v in m["moves"]]) for m in stale])
    e, s = exact[1], stale[1]
    assert e["accepted"] == 6 and e["moves"][4] <= 1e-6 and e["moves"][5] <= 1e-11 and e["resets"] == 0 and atm.expect_fallback(e) == 0
    assert s["accepted"] is None and s["moves"][5] >= 1e-8 and s["resets"] == 0


def test_partial_last_chunk_and_the_rules_of_the_pass():
    """The model's own edges: a call that ends inside a chunk, the clamp and the non-finite reset cut the sensitivity."""
    rng = np.random.default_rng(5)
    v = 0.7 * rng.standard_normal(3 * atm.CHUNK + 77)
    m = atm.rounds(v, 1.2, 0.001, max_rounds=12)
    assert m["accepted"] is not None and m["gain"] == pytest.approx(atm.serial(v, 1.2, 0.001), rel=1e-12)
    assert atm.serial(v, 1.2, 0.001) == atm.fixed_point(v, 1.2, 0.001)
    G, M, nf = atm.shoot(np.full(atm.CHUNK, 1e-3), np.array([1.4999, 1.0]), 0.001)
    assert G[0] == atm.AF_MAX and M[0] == 0.0 and nf == 0
    G, M, nf = atm.shoot(np.full(atm.CHUNK, 1e160), np.array([1.0, 1.0]), 0.001)
    assert G[0] == atm.AF_INIT and M[0] == 0.0 and nf > 0
    new, move = atm.node_pass(np.array([1.0, 1.0, 1.0]), np.array([1.1, 1.2]), np.array([0.5, 0.5]))
    assert new.tolist() == [1.0, 1.1, 1.2 + 0.5 * (1.1 - 1.0)] and move == pytest.approx(0.25 / 1.25)

"""The float64 model of the weak-signal stage (tests/weak_signal_fixture.py) against its own definitions, and the
library's detector taps (fmr_filter_table "ws_usn") against the model's design.  No device."""
import importlib
import math

import numpy as np

import weak_signal_fixture as wf

fmr = importlib.import_module("airspy-fmradion_amd")


def test_tap_table_response():
    h = wf.taps()
    assert len(h) == 63 and np.abs(h - h[::-1]).max() <= 1e-16          # linear phase
    assert abs(h.sum()) <= 1e-15                                          # DC gain (-2e-16)
    assert wf.response_db(h, np.arange(0.0, 90001.0, 500.0)).max() <= -75.0
    top = wf.response_db(h, np.arange(125000.0, 192001.0, 500.0))
    assert np.abs(top).max() <= 0.015


def test_library_taps_equal_the_design_to_one_ulp():
    fmr.build_library()
    got, want = fmr.filter_table("ws_usn"), wf.taps()
    assert got.dtype == np.float64 and len(got) == 63
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))


def test_step_response_of_s_for_attack_and_release():
    cfg = wf.config(attack_ms=10.0, release_ms=500.0)
    n, lvl = 400, 1e-3
    s, _ = wf.control(np.full(n, lvl), cfg)                                # attack from 0: s_j = lvl (1 - (1 - c)^(j + 1))
    j = np.arange(n)
    assert np.allclose(s, lvl * (1.0 - np.exp(-2.0 / 10.0) ** (j + 1)), rtol=1e-12, atol=0)
    s2, _ = wf.control(np.zeros(n), cfg, s0=s[-1])                          # release to 0: s_j = s0 (1 - c)^(j + 1)
    assert np.allclose(s2, s[-1] * np.exp(-2.0 / 500.0) ** (j + 1), rtol=1e-12, atol=0)
    assert abs(s[4] / lvl - (1.0 - math.exp(-1.0))) < 1e-12                # one attack time constant = five intervals


def test_clamps_at_exactly_lo_and_hi():
    cfg = wf.config(blend=(-40.0, -30.0), highcut=(-30.0, -20.0), mute=(-20.0, -10.0), attack_ms=1e-3, release_ms=1e-3)
    u = 10.0 ** (np.array([-40.0, -30.0, -20.0, -10.0, -50.0, -35.0]) / 10.0)   # (c = 1 to fp64: s follows u)
    s, t = wf.control(u, cfg)
    assert np.allclose(10 * np.log10(s), [-40, -30, -20, -10, -50, -35], atol=1e-9)
    assert np.allclose(t[:, 0], [0, 1, 1, 1, 0, 0.5], atol=1e-9) and t[0, 0] <= 1e-12 and t[4, 0] == 0.0
    assert np.allclose(t[:, 1], [0, 0, 1, 1, 0, 0], atol=1e-9) and np.allclose(t[:, 2], [0, 0, 0, 1, 0, 0], atol=1e-9)
    assert t.min() == 0.0 and t.max() == 1.0
    _, t0 = wf.control(np.zeros(3), cfg)                                    # s = 0: D = -inf, every t is 0
    assert not t0.any()
    _, toff = wf.control(u, wf.config(actions=wf.HIGHCUT, blend=(-40.0, -30.0), highcut=(-30.0, -20.0), mute=(-20.0, -10.0)))
    assert not toff[:, 0].any() and not toff[:, 2].any()                    # an action switched off holds 0


def _audio(n, ch, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    x = np.stack([0.4 * np.sin(2 * np.pi * 1000.0 * t), 0.3 * np.sin(2 * np.pi * 5000.0 * t + 0.4)][:ch], axis=1)
    return (x + 1e-3 * rng.standard_normal((n, ch))).reshape(-1)


def test_all_zero_t_returns_the_audio_bit_for_bit():
    for ch in (1, 2):
        x = _audio(1000, ch)
        assert np.array_equal(wf.act(x, ch, np.zeros((12, 3)), wf.config()), x)


def test_ramp_across_an_interval_edge():
    t = np.zeros((4, 3))
    t[1] = (1.0, 0.5, 0.25)                                                 # interval 1 alone is engaged
    v = wf.ramps(t, 5 * wf.A)
    A = wf.A
    assert not v[:2 * A].any()                                              # frames of chunks 0 and 1 use intervals < 1
    assert np.allclose(v[2 * A:3 * A, 0], (np.arange(A) + 1) / A)           # chunk 2 ramps 0 -> t[1]
    assert v[3 * A - 1, 0] == 1.0 and v[3 * A - 1, 1] == 0.5 and v[3 * A - 1, 2] == 0.25
    assert np.allclose(v[3 * A:4 * A, 0], 1.0 - (np.arange(A) + 1) / A)     # chunk 3 ramps back to t[2] = 0
    assert v[4 * A - 1].max() == 0.0 and np.abs(np.diff(v[:, 0])).max() <= 1.0 / A + 1e-15
    # full blend is mono; full mute is the floor; the high cut is the one-pole itself
    x = _audio(5 * A, 2)
    cfg = wf.config(mute_floor_db=-20.0)
    y = wf.act(x, 2, t, cfg).reshape(-1, 2)
    f = 3 * A - 1
    L, R = x.reshape(-1, 2)[f]
    assert np.isfinite(y).all()
    only_blend = wf.act(x, 2, t * [1, 0, 0], cfg).reshape(-1, 2)
    assert abs(only_blend[f, 0] - only_blend[f, 1]) <= 4e-16 and abs(only_blend[f, 0] - 0.5 * (L + R)) <= 4e-16
    only_mute = wf.act(x, 2, t * [0, 0, 4], cfg).reshape(-1, 2)             # t_m = 1 at frame f
    assert np.allclose(only_mute[f], 0.1 * np.array([L, R]), rtol=1e-14, atol=0)


def test_mono_chain():
    x = _audio(4 * wf.A, 1)
    t = np.ones((3, 3))
    cfg = wf.config(highcut_hz=500.0)
    y = wf.act(x, 1, t, cfg)
    w, prev = np.empty(len(x)), 0.0
    for i, v in enumerate(x):
        prev = prev + cfg["alpha"] * (v - prev)
        w[i] = prev
    f = np.arange(3 * wf.A, 4 * wf.A)                                       # chunk 3: every t is 1 throughout
    assert np.allclose(y[f], cfg["g_floor"] * w[f], rtol=0, atol=1e-16)      # (x2 = x1 + (w - x1): an ulp of x1)
    assert np.array_equal(y[:wf.A], x[:wf.A])                                # chunk 0: nothing engaged yet


def test_record_that_spans_a_call_edge():
    rng = np.random.default_rng(5)
    n = 7 * wf.Q + 300
    mpx = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / wf.F) + 1e-2 * rng.standard_normal(n)).astype(np.float32)
    mpx[2 * wf.Q + 5] = np.nan
    u, non = wf.usn(mpx)
    assert len(u) == 7 and non.tolist() == [0, 0, 1, 0, 0, 0, 0]
    cfg = wf.config(record_intervals=3)
    recs = wf.records(u, non, cfg)
    assert len(recs) == 2 and recs["first_interval"].tolist() == [0, 3] and recs["n_nonfinite"].tolist() == [1, 0]
    # the same input cut inside record 1 (and inside interval 4): the intervals do not depend on the cut
    cut = 4 * wf.Q + 123
    u_head, non_head = wf.usn(mpx[:cut])
    assert np.array_equal(u_head, u[:4]) and np.array_equal(non_head, non[:4])
    assert abs(recs["usn_sum"][1] - (u[3] + u[4] + u[5])) <= 1e-18 and recs["usn_peak"][1] == u[3:6].max()
    s, t = wf.control(u, cfg)
    assert recs["smoothed"][1] == s[5] and recs["t_blend"][1] == t[5, 0] and recs["max_blend"][1] == t[3:6, 0].max()
    d = wf.derive(recs)
    assert d["n_intervals"] == 6 and d["n_nonfinite"] == 1

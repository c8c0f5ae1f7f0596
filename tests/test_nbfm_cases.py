"""The input conditions every case of tests/test_gpu_nbfm_edges.py relies on, proved by the oracle alone (no GPU)."""
import numpy as np
import pytest

import nbfm_cases as nc

NAMES = list(nc.CASES)


def regime_of(case, r):
    """The regime the reference run r of case is in, or a string that says why it is in none."""
    if case.regime == "fast":
        return "fast" if r.negative == 0 and r.clamped == 0 and r.gain_blk[-1] > 0 else f"negative {r.negative}, clamped {r.clamped}"
    if case.regime == "negative":
        return "negative" if r.gain_blk[-1] < 0 and r.nb_gain_blk[-1] < 0 else f"end gain {r.gain_blk[-1]}"
    if case.regime in ("cycle", "cycle_short"):
        lo = case.cycle_counts or (20000, 20000)
        return case.regime if r.clamped >= lo[0] and r.negative >= lo[1] else f"clamped {r.clamped}, negative {r.negative}"
    if case.regime == "silence":
        return "silence" if r.zero_disc >= 100000 else f"zero discriminator outputs {r.zero_disc}"
    return None


@pytest.mark.parametrize("name", NAMES)
def test_regime(name):
    case = nc.CASES[name]
    r = case.reference()
    print(f"{name}: negative {r.negative}, clamped {r.clamped}, resets {r.resets}, zero discriminator outputs {r.zero_disc}, end gain {r.gain_blk[-1]:.6g}")
    assert regime_of(case, r) == case.regime
    assert np.all(np.isfinite(r.audio))
    assert sum(r.alen) == len(r.audio) == len(r.disc)
    assert 0 <= sum(case.n) // case.decim - len(r.audio) <= (0 if case.decim == 1 else 64)      # (the resampler's delay)


def test_the_regimes_the_cases_are_named_for():
    """What the cases are for: the cycle alternates sample by sample between the clamp and a negative gain; the negative
    case stays negative across at least three later calls; silence runs into the clamp; the non-finite inputs reset the gain."""
    r = nc.CASES["wide_8000"].reference()
    lo, hi = nc.CASES["wide_8000"].segments[1]
    g = r.gain[lo + 200:hi]
    assert np.all((g[:-1] < 0) != (g[1:] < 0)) and np.nanmin(g) < -1e9 and r.clamped + r.negative >= hi - lo
    c = nc.CASES["negative"]
    ends = np.cumsum([len(x) for x in c.calls])
    assert all(c.reference().nb_gain_blk[e - 1] < 0 for e in ends[-4:])
    s = nc.CASES["silence"].reference()
    assert s.gain_blk[59] == 1e5 and s.clamped > 0                      # the cold call of 60 blocks of zeros ends on the clamp
    lw = nc.CASES["long_wide"].reference()
    assert abs(lw.gain[nc.LONG_KEY - 1] - 8083) < 200 and lw.gain_blk[-1] > 0
    assert np.count_nonzero(lw.gain[2048 * 256:nc.LONG * nc.BLK] < 0) > 3000   # the cycle runs across the node pass's tile edge
    for name, n in (("nan3", 129), ("inf1", 127), ("nan_in_30", 127)):
        assert abs(nc.CASES[name].reference().resets - n) <= 1, name


@pytest.mark.parametrize("name", NAMES)
def test_ambiguity_cap(name):
    r = nc.CASES[name].reference()
    ka, kd = nc.kept(r)
    print(f"{name}: wrap-ambiguous IF samples {list(r.ambiguous)}, margins {[float(r.margin[i]) for i in r.ambiguous]}")
    assert len(r.ambiguous) <= nc.MAX_AMBIGUOUS
    assert np.count_nonzero(~ka) <= 0.005 * len(ka)


@pytest.mark.parametrize("name", NAMES)
def test_sensitivity_changes_no_regime(name):
    case = nc.CASES[name]
    a, b = case.reference(), case.bumped()
    seg, worst = nc.sensitivity(case)
    print(f"{name}: audio distance per segment {['%.2e' % v for v in seg]}, worst sample {worst:.2e}, gain per block rel "
          f"{max(abs(x / y - 1) for x, y in zip(b.gain_blk, a.gain_blk) if y):.1e}")
    assert regime_of(case, b) == case.regime
    assert (b.negative, b.clamped, b.resets) == (a.negative, a.clamped, a.resets)
    assert np.array_equal(np.signbit(a.gain[np.isfinite(a.gain)]), np.signbit(b.gain[np.isfinite(a.gain)]))
    gain_moves = max((abs(x / y - 1) for x, y in zip(b.gain_blk, a.gain_blk) if y), default=0.0)
    assert gain_moves < 2e-5        # (a fifth of the 1e-4 the GPU tests hold if_agc_gain to: where the cycle ends on a negative gain it is 5e-3)
    assert worst < 1e-4 and max(seg) < 1e-6 and (worst > 0 or case.level == 0)         # the reference is well conditioned in every case: parity is a fair demand


@pytest.mark.parametrize("name", NAMES)
def test_discriminator_bound_is_a_fair_demand(name):
    """The GPU tests hold the discriminator tap to 2e-6 RMS per block: the oracle itself, its input moved by one ulp, stays
    within that in every block of every case (measured 1e-7 ... 1.2e-6).  A seed that breaks this is replaced, the bound stays."""
    move = nc.disc_block_sensitivity(nc.CASES[name])
    print(f"{name}: the oracle's own discriminator output moves by {move:.2e} RMS in its worst block")
    assert move < 2e-6


@pytest.mark.parametrize("name", NAMES)
def test_stage_chain_equals_the_decoder(name):
    r = nc.CASES[name].reference()
    assert np.array_equal(r.audio, r.stage_audio)
    assert r.gain_blk == r.nb_gain_blk


def test_signal_builder():
    x = nc.ptt(3, 0.0, 0.2, 100, 50, 70)
    assert x.dtype == np.complex64 and len(x) == 220 and not x[:100].any() and not x[150:].any()
    assert np.allclose(np.abs(x[100:150]), 0.2, rtol=1e-6) and x[100] == np.complex64(0.2)
    assert np.array_equal(x, nc.ptt(3, 0.0, 0.2, 100, 50, 70)) and not np.array_equal(nc.ptt(1, 1e-4, 0.2, 9, 9, 9), nc.ptt(2, 1e-4, 0.2, 9, 9, 9))
    y = nc.bump_ulp(nc.ptt(1, 1e-4, 0.2, 50, 50, 50))
    d = y.view(np.float32) - nc.ptt(1, 1e-4, 0.2, 50, 50, 50).view(np.float32)
    assert np.all(d >= 0) and 0.3 < np.mean(d > 0) < 0.7

"""tests/iqcorr_fixture.py against the definitions in include/fmradion_amd.h ("DC-offset and IQ-imbalance correction on
the capture"): against brute force in Python integers on short rows, and on the captures of tests/test_gpu_iqcorr.py.

Where the planted cases sit (iqcorr_fixture.capture; W = 4, R = 8, calls iqcorr_fixture.CALLS): (-0.0, 0.0) at sample 100
in interval 0; finite samples with p > 4 at 30000 and at 99303, the last sample of the second call; (1e-39, -1e-39) at
70000; a NaN at 230000 and an Inf at 260000; intervals 40 .. 42 all zero (three: the window of four never empties, P > 0
throughout); intervals 50 .. 53 all zero (W of them: P = 0 exactly for interval 54, which passes bit for bit, and four
intervals of recovery behind it); samples [60 Q, 61.5 Q) scaled by 10, all skipped (the windows keep N >= Q / 2);
samples [66 Q, 70.5 Q) scaled by 10: the window of interval 70 has N = 0 and the interval passes bit for bit, that of
interval 71 has N = Q / 2 exactly and is solved; samples [85 Q + 1000, 400000) scaled by 0.1: a -20 dB step inside an
interval and the +20 dB step inside another.

The estimator's own spread, measured over the clean capture's 118 full windows of W = 4: gain 0.091 dB, phase 0.26
degrees (standard deviations of the per-interval estimates; the pooled estimate of all records is 0.018 dB and 0.061
degrees from impair's g = 1.05 and phi = 3 degrees).  derive is held to three times that spread."""
import math

import numpy as np

import iqcorr_fixture as qf

Q = qf.Q
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def main():
    return cached("main", lambda: (qf.capture(), qf.run(qf.capture(), **qf.CFG)))


def short_row(n, seed=3):
    """n samples around 0.3 with an offset, a few of them planted as not usable"""
    rng = np.random.default_rng(seed)
    x = (0.3 * (rng.normal(size=n) + 1j * rng.normal(size=n)) + (0.02 - 0.01j)).astype(np.complex64)
    v = x.view(np.float32).reshape(-1, 2)
    v[5] = (np.nan, 0.0)
    v[Q + 17] = (0.0, -np.inf)
    v[2 * Q - 1] = (2.0, 0.5)           # p = 4.25
    v[2 * Q] = (2.0, 0.0)               # p = 4: usable
    v[77] = (1e-39, -1e-39)
    return x


def brute_sums(x):
    """(N, S_r, S_i, S_rr, S_ii, S_ri) over x in Python integers, sample by sample"""
    f = np.float32
    tot = [0] * 6
    for s in x:
        re, im = f(s.real), f(s.imag)
        if not (math.isfinite(re) and math.isfinite(im)):
            continue
        with np.errstate(under="ignore", over="ignore"):
            rr, ii, ri = f(re * re), f(im * im), f(re * im)
            if not f(rr + ii) <= 4:
                continue
        for k, v in enumerate((None, re, im, rr, ii, ri)):
            tot[k] += 1 if k == 0 else math.floor(float(v) * 2.0 ** 36)
    return tot


def test_sums_against_brute_force_for_any_cut():
    x = short_row(3 * Q + 500)
    a = qf.sample_moments(x)
    S = qf.interval_sums(a)
    assert S.shape == (4, 6)
    for j in range(4):
        assert [int(v) for v in S[j]] == brute_sums(x[j * Q:(j + 1) * Q]), j
    assert S[0][0] == Q - 1 and S[1][0] == Q - 2 and S[2][0] == Q           # the NaN; the Inf and p = 4.25; p = 4 is usable
    rng = np.random.default_rng(4)
    for _ in range(5):                   # any cut: the pieces' sums add up to the interval's
        cuts = np.sort(rng.integers(0, len(x), 9)).tolist()
        parts = [a[lo:hi].sum(axis=0, dtype=np.int64) for lo, hi in zip([0] + cuts, cuts + [len(x)])]
        assert np.array_equal(np.sum(parts, axis=0, dtype=np.int64), S.sum(axis=0, dtype=np.int64))
    # floor, not truncation: the denormal pair gives 0 and -1; its squares and its product underflow to 0 and -0
    m = qf.sample_moments(x[77:78])[0]
    assert m.tolist() == [1, 0, -1, 0, 0, 0]


def test_window_sums_by_differences_equal_direct_sums():
    rng = np.random.default_rng(6)
    S = rng.integers(-2 ** 58, 2 ** 58, (40, 6), dtype=np.int64)            # (running totals wrap; differences do not mind)
    for W in (1, 4, 7, 64):
        win = qf.window_sums(S, W)
        for j in range(len(S)):
            c = min(j, W)
            direct = [sum(int(v) for v in S[j - c:j, k]) for k in range(6)]
            assert [int(v) for v in win[j]] == [((d + 2 ** 63) % 2 ** 64) - 2 ** 63 for d in direct], (W, j)
    x = short_row(6 * Q)
    S = qf.interval_sums(qf.sample_moments(x))
    win = qf.window_sums(S, 4)
    assert [int(v) for v in win[5]] == brute_sums(x[Q:5 * Q]) and not win[0].any()


def test_solve_on_a_row_that_can_be_said_in_advance():
    # I = +-0.5 alternating, Q' = 0.25 I: E_rr = 1/4, E_ii = 1/64, E_ri = 1/16, no mean; all exact in fp32 and fp64
    n = 3 * Q
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    x = (0.5 * sign + 1j * 0.125 * sign).astype(np.complex64)
    r = qf.run(x, W=2, R=1)
    P, C_r, C_i = 1 / 4 + 1 / 64, 1 / 4 - 1 / 64, 2 / 16
    assert P * P - (C_r * C_r + C_i * C_i) == 0.0            # a rectilinear row: D = 0, so w = 0 and no refusal
    assert not r["coef"].any() and not r["refused"].any() and r["out"].tobytes() == x.tobytes()
    # the same with Q' in quadrature on every other pair: proper but unbalanced, g = 1/4
    q = np.where((np.arange(n) // 2) % 2 == 0, 1.0, -1.0)
    y = (0.5 * sign + 1j * 0.125 * q).astype(np.complex64)
    r = qf.run(y, W=2, R=1)
    w = (1 - 0.25) / (1 + 0.25)                              # rho = g = (1 - w) / (1 + w)
    assert r["refused"][1:].all() and w * w > 1 / 16         # 0.6: far more than a receiver's mismatch
    # ... and with g = 3/4 it is solved: w = 1/7 to the last bits
    y = (0.5 * sign + 1j * 0.375 * q).astype(np.complex64)
    r = qf.run(y, W=2, R=1)
    assert not r["refused"].any() and abs(float(r["coef"][2, 2]) - 1 / 7) < 1e-7 and r["coef"][2, 3] == 0
    lv = qf.derive(r["records"])
    assert abs(lv["gain_imbalance_db"] - 20 * math.log10(0.75)) < 1e-9 and abs(lv["phase_error_deg"]) < 1e-9
    assert abs(lv["image_rejection_db"] - 20 * math.log10(7)) < 1e-9 and lv["dc_dbfs"] == -math.inf


def test_intervals_that_pass_bit_for_bit():
    x, r = main()
    coef = r["coef"]
    passing = [j for j in range(len(coef)) if not coef[j].any()]
    assert passing == [0, qf.ZERO4[1], 70]
    for j in passing:
        assert r["out"][j * Q:(j + 1) * Q].tobytes() == x[j * Q:(j + 1) * Q].tobytes()
    assert np.signbit(r["out"][qf.NEGZERO].real) and r["out"][qf.NEGZERO] == 0
    # every other interval moves its samples, and non-finite samples pass wherever they are
    for j in (1, 43, 55, 71, 121):
        assert r["out"][j * Q:(j + 1) * Q].tobytes() != x[j * Q:(j + 1) * Q].tobytes()
    for n in (qf.NAN, qf.INF):
        assert r["out"][n:n + 1].tobytes() == x[n:n + 1].tobytes() and coef[n // Q].all()
    # a finite sample with p > 4 is corrected like any other
    for n in qf.BIG:
        assert r["skipped"][n] and r["out"][n] != x[n]
    # the window of interval 71 holds exactly Q / 2 usable samples
    assert int(qf.window_sums(r["S"], 4)[71][0]) == Q // 2 and int(qf.window_sums(r["S"], 4)[70][0]) == 0
    # the three zero intervals never empty the window; the four do, once
    win = qf.window_sums(r["S"], 4)
    assert all(win[j][3] > 0 for j in range(41, 48)) and not win[54][1:].any() and win[54][0] == 4 * Q


def test_refusal_fires_on_the_improper_row_only():
    _, r = main()
    assert not r["refused"].any()
    assert not qf.run(qf.second_row(), **qf.CFG)["refused"].any()
    imp = qf.improper_row()
    ri = qf.run(imp, **qf.CFG)
    assert ri["refused"][1:].all() and not ri["refused"][0] and not ri["coef"][:, 2:].any()
    assert ri["records"]["n_refused"].tolist() == [7] + [8] * 14
    rb = qf.run(imp, correct=qf.BALANCE, **qf.CFG)
    assert rb["out"].tobytes() == imp.tobytes() and rb["refused"][1:].all()
    # with Q exactly zero D = 0: no w and no refusal
    rp = qf.run((imp.real + 0j).astype(np.complex64), **qf.CFG)
    assert not rp["refused"].any() and not rp["coef"][:, 2:].any()


def test_correct_selects_what_is_applied():
    x, r = main()
    rd = qf.run(x, correct=qf.DC, **qf.CFG)
    rb = qf.run(x, correct=qf.BALANCE, **qf.CFG)
    assert np.array_equal(rd["coef"][:, :2], r["coef"][:, :2]) and not rd["coef"][:, 2:].any()
    assert np.array_equal(rb["coef"][:, 2:], r["coef"][:, 2:]) and not rb["coef"][:, :2].any()
    for k in qf.SUMS + ("n_usable", "n_skipped", "n_nonfinite"):
        assert np.array_equal(rd["records"][k], r["records"][k])
    assert rd["out"].tobytes() != r["out"].tobytes() != rb["out"].tobytes()


def test_derive_recovers_the_impairment_within_the_estimators_spread():
    rc = cached("clean", lambda: qf.run(qf.capture(clean=True), **qf.CFG))
    w = rc["coef"][4:, 2].astype(np.float64) + 1j * rc["coef"][4:, 3].astype(np.float64)
    rho = (1 - w) / (1 + w)
    g_db, phi = 20 * np.log10(np.abs(rho)), -np.degrees(np.angle(rho))
    lv = qf.derive(rc["records"])
    print(f"spread over {len(w)} windows: gain {g_db.std():.4f} dB, phase {phi.std():.4f} deg; pooled estimate off by "
          f"{lv['gain_imbalance_db'] - 20 * math.log10(qf.G1):+.4f} dB and {lv['phase_error_deg'] - math.degrees(qf.PHI1):+.4f} deg")
    assert abs(lv["gain_imbalance_db"] - 20 * math.log10(qf.G1)) <= 3 * g_db.std()
    assert abs(lv["phase_error_deg"] - math.degrees(qf.PHI1)) <= 3 * phi.std()
    assert abs(complex(lv["dc_re"], lv["dc_im"]) - qf.DC1) < 1e-4 and lv["refused"] == 0 and lv["usable_share"] == 1.0
    r2 = qf.run(qf.second_row(), **qf.CFG)
    lv2 = qf.derive(r2["records"])
    assert abs(lv2["gain_imbalance_db"] - 20 * math.log10(qf.G2)) <= 3 * g_db.std()
    assert abs(lv2["phase_error_deg"] - math.degrees(qf.PHI2)) <= 3 * phi.std()
    assert lv2["n_nonfinite"] == 1 and lv2["n_skipped"] == 1


def test_the_planted_cases_sit_where_the_docstring_says():
    x, r = main()
    ends = np.cumsum([sum(c) for c in qf.CALLS])
    assert ends[-1] == qf.N == len(x) and qf.BIG[1] + 1 in ends and qf.BIG[0] + 1 not in ends
    assert sum(map(sum, qf.RAGGED)) == qf.N and max(map(len, qf.RAGGED)) <= 8
    assert qf.NEGZERO < Q and r["nonfin"].sum() == 2 and r["nonfin"][qf.NAN] and r["nonfin"][qf.INF]
    sk = r["skipped"].copy()
    assert sk[qf.BIG].all()
    for lo, hi in (qf.SKIP15, qf.SKIP45):
        assert sk[lo:hi].all() and lo % Q == 0 and hi % Q == Q // 2
        sk[lo:hi] = False
    sk[qf.BIG] = False
    assert not sk.any()
    for lo, hi in (qf.ZERO3, qf.ZERO4):
        assert not x[lo * Q:hi * Q].any() and x[lo * Q - 1] != 0 and x[hi * Q] != 0
    assert (qf.ZERO3[1] - qf.ZERO3[0], qf.ZERO4[1] - qf.ZERO4[0]) == (3, qf.CFG["W"])
    assert qf.QUIET[0] % Q and qf.QUIET[1] % Q              # both steps inside an interval
    lo, hi = (float(np.abs(x[s]).mean()) for s in (slice(qf.QUIET[1] - 2000, qf.QUIET[1]), slice(qf.QUIET[1], qf.QUIET[1] + 2000)))
    assert abs(20 * math.log10(hi / lo) - 20.0) < 0.5
    recs = r["records"]
    assert len(recs) == 15 and recs["n_intervals"].tolist() == [8] * 15 and recs["index"].tolist() == list(range(15))
    assert recs["n_skipped"].sum() == 2 + 6 * Q and recs["n_nonfinite"].sum() == 2
    assert (recs["n_usable"] + recs["n_skipped"] + recs["n_nonfinite"]).tolist() == [8 * Q] * 15

"""tests/blanker_fixture.py against the definitions in include/fmradion_amd.h ("Impulse blanker on the capture"), on
hand-made rows where every value can be said in advance."""
import math

import numpy as np

import blanker_fixture as bf

Q = bf.Q


def row(n, level=0.25):
    """n samples of constant power level^2 (exact in fp32 for 0.25)."""
    return np.full(n, level, dtype=np.complex64)


def test_threshold_at_start_up_in_the_steady_state_and_at_its_floor():
    # intervals of power 1/16, 1/16, 1/4, 1/16 ...: A_j = Q p_j 2^36 exactly
    x = row(8 * Q)
    x[2 * Q:3 * Q] = 0.5
    r = bf.run(x, G=2, M=16, W=3, threshold_db=10.0)
    A = (np.array([1, 1, 4, 1, 1, 1, 1, 1]) * (Q << 32)).astype(np.uint64)
    assert np.array_equal(r["A"], A)
    g = 10.0
    means = [None, 1 / 16, 1 / 16, (1 + 1 + 4) / 48, (1 + 4 + 1) / 48, (4 + 1 + 1) / 48, 1 / 16, 1 / 16]
    assert r["T"][0] == np.inf
    for j in range(1, 8):          # c = min(j, W) intervals; every mean here is exact up to the two roundings of the rule
        c = min(j, 3)
        S = int(A[j - c:j].sum())
        assert r["T"][j] == g * (float(S) * (1.0 / (c * 2.0 ** 48)))
        assert abs(r["T"][j] - g * means[j]) <= 1e-15
    # the floor: an all-zero capture has T = 2^-30 from interval 1 on and triggers nothing
    z = bf.run(np.zeros(3 * Q, dtype=np.complex64), G=2, M=16, W=3)
    assert z["T"].tolist() == [np.inf, 2.0 ** -30, 2.0 ** -30]
    assert not z["trig"].any() and not z["blank"].any() and not z["A"].any()
    assert z["records"].size == 0
    # ... and a sample just over the floor triggers there
    y = np.zeros(2 * Q, dtype=np.complex64)
    y[Q + 5] = 2.0 ** -14                # p = 2^-28 > 2^-30
    y[Q + 9] = 2.0 ** -16                # p = 2^-32
    t = bf.run(y, G=1, M=4, W=3)["trig"]
    assert t[Q + 5] and not t[Q + 9] and t.sum() == 1


def test_an_impulse_in_interval_0_passes():
    x = row(2 * Q)
    x[100] = 50.0
    x[Q + 100] = 50.0
    r = bf.run(x, G=2, M=16, W=4)
    assert not r["trig"][:Q].any() and r["out"][100] == x[100]
    assert r["trig"][Q + 100] and r["out"][Q + 100] == 0
    # its power is in A_0 all the same (clipped at 256)
    assert r["A"][0] == (Q - 1) * (1 << 32) + (256 << 36)


def test_two_triggers_closer_than_g_merge_and_the_gate_is_causal():
    x = row(3 * Q)
    n = Q + 1000
    x[n] = 9.0
    x[n + 3] = 9.0                       # inside the gate of the first (G = 4): one run of 7
    x[n + 20] = 9.0
    x[n + 24] = 9.0                      # one sample behind the gate of the third: contiguous, still one run of 8
    x[n + 40] = 9.0
    x[n + 45] = 9.0                      # an open sample between them: two runs of 4
    r = bf.run(x, G=4, M=64, W=4)
    b = np.flatnonzero(r["blank"])
    want = list(range(n, n + 7)) + list(range(n + 20, n + 28)) + list(range(n + 40, n + 44)) + list(range(n + 45, n + 49))
    assert b.tolist() == want
    assert not r["blank"][n - 1] and r["out"][n - 1] == x[n - 1]          # the sample before the trigger is kept
    assert r["trig"].sum() == 6
    kept = np.ones(len(x), bool)
    kept[b] = False
    assert np.array_equal(r["out"][kept].view(np.uint32), x[kept].view(np.uint32)) and not r["out"][b].any()


def test_give_up_after_exactly_m_samples_and_re_arming_after_one_open_sample():
    G, M = 2, 16
    x = row(4 * Q)
    a = Q + 500
    x[a:a + 100] = 9.0                   # 100 samples over the threshold: M zeroed, the rest passes
    r = bf.run(x, G=G, M=M, W=4)
    assert np.flatnonzero(r["blank"]).tolist() == list(range(a, a + M))
    assert r["gate"][a:a + 101].all() and not r["gate"][a + 101]
    assert np.array_equal(r["out"][a + M:a + 100], x[a + M:a + 100])
    # a second burst that starts right behind the single open sample a + 101 is blanked again, for M samples
    x[a + 102:a + 202] = 9.0
    r = bf.run(x, G=G, M=M, W=4)
    assert np.flatnonzero(r["blank"]).tolist() == list(range(a, a + M)) + list(range(a + 102, a + 102 + M))
    # ... but not when no sample was open in between (the burst starts at a + 101)
    x[a + 101] = 9.0
    r = bf.run(x, G=G, M=M, W=4)
    assert np.flatnonzero(r["blank"]).tolist() == list(range(a, a + M))
    # a +20 dB step zeroes M samples, not everything until the average has caught up
    s = row(4 * Q)
    s[2 * Q + 77:] = 2.5
    r = bf.run(s, G=G, M=M, W=4)
    assert np.flatnonzero(r["blank"]).tolist() == list(range(2 * Q + 77, 2 * Q + 77 + M))
    assert r["trig"][2 * Q + 77:3 * Q].all() and not r["trig"][3 * Q:].any()
    # at the chain's first samples a closed gate counts from sample 0
    f = row(Q)
    f[:40] = np.nan
    assert np.flatnonzero(bf.run(f, G=G, M=M, W=4)["blank"]).tolist() == list(range(M))


def test_nan_and_inf_are_zeroed_counted_and_left_out_of_the_level():
    x = row(2 * Q)
    x[Q + 10] = np.complex64(complex(np.nan, 1.0))
    x[Q + 50] = np.complex64(complex(1.0, -np.inf))
    x[Q + 90] = np.complex64(complex(3e19, 3e19))          # finite parts, p overflows: non-finite
    x[20] = np.complex64(complex(np.inf, np.nan))          # in interval 0: non-finite triggers whatever T is
    r = bf.run(x, G=1, M=8, W=4, R=1)
    assert r["trig"][[20, Q + 10, Q + 50, Q + 90]].all() and r["trig"].sum() == 4
    assert not r["out"][[20, Q + 10, Q + 50, Q + 90]].any() and np.isfinite(r["out"]).all()
    assert r["A"].tolist() == [(Q - 1) << 32, (Q - 3) << 32]
    assert r["records"]["n_nonfinite"].tolist() == [1, 3] and r["records"]["n_blanked"].tolist() == [1, 3]
    assert r["records"]["peak"].tolist() == [0.0625, 0.0625]
    # a run of non-finite samples longer than M passes through as it is
    y = row(2 * Q)
    y[Q:Q + 20] = np.nan
    o = bf.run(y, G=1, M=8, W=4)["out"]
    assert not o[Q:Q + 8].any() and np.isnan(o[Q + 8:Q + 20]).all()


def test_power_over_256_is_clipped_in_the_level_only():
    x = row(3 * Q)
    x[Q + 7] = 100.0                     # p = 10000
    r = bf.run(x, G=1, M=8, W=1, R=1)
    assert r["A"][1] == ((Q - 1) << 32) + (256 << 36)
    assert r["records"]["peak"][1] == np.float32(10000.0) and r["p"][Q + 7] == np.float32(10000.0)
    assert r["T"][2] == math.pow(10.0, 1.2) * (float(int(r["A"][1])) * (1.0 / 2.0 ** 48))


def test_records_across_an_interval_edge_and_a_ragged_end():
    R = 2
    x = row(5 * Q + 123)                 # five complete intervals and a ragged end: two records
    e = 2 * Q                            # a burst across the edge between record 0 and record 1
    x[e - 1] = 9.0
    x[e] = 9.0
    r = bf.run(x, G=3, M=16, W=4, R=R)
    recs = r["records"]
    assert recs["index"].tolist() == [0, 1] and recs["first_interval"].tolist() == [0, 2] and recs["n_intervals"].tolist() == [2, 2]
    assert recs["n_triggers"].tolist() == [1, 1]
    assert recs["n_blanked"].tolist() == [1, 3]          # e - 1 | e, e + 1, e + 2
    assert recs["n_runs"].tolist() == [1, 0]             # one run: it starts in record 0
    assert recs["threshold"].tolist() == [r["T"][1], r["T"][3]]
    assert recs["power_q"].tolist() == [int(r["A"][0] >> 12) + int(r["A"][1] >> 12), int(r["A"][2] >> 12) + int(r["A"][3] >> 12)]
    assert recs["peak"].tolist() == [np.float32(81.0), np.float32(81.0)]
    assert len(r["A"]) == 6 and r["A"][5] == 123 << 32   # the open interval is summed and in no record
    assert bf.defaults(10e6) == (8, 64) and bf.defaults(2.5e6) == (2, 16) and bf.defaults(1e9) == (256, 1024)

"""The thresholds the GPU tests of the weak-signal stage use (weak_signal_fixture.TEST_DB) against the test signal itself,
on the CPU oracle's MPX (tests/oracle_mpx.py), not on the code under test: every interval of the clean segments reads at
least 6 dB under every lo, every interval of the noisy segment at least 6 dB over every hi, so each t goes 0, 1, 0."""
import numpy as np

import oracle_mpx as om
import weak_signal_fixture as wf


def test_clean_and_noisy_segments_clear_every_threshold_by_6_db():
    x = wf.stepped_iq()
    mpx = om.oracle_mpx(x, [65536] * (wf.TEST_N // 65536), wf.F)
    u, non = wf.usn(mpx.astype(np.float32))
    assert not non.any()
    db = 10.0 * np.log10(u)
    delay = wf.TEST_N - len(mpx)                         # the oracle's front end holds a few samples back
    assert 0 <= delay < wf.Q
    a, b = wf.TEST_NOISY[0] // wf.Q, wf.TEST_NOISY[1] // wf.Q
    clean = np.concatenate([db[:a - 1], db[b + 1:]])      # (the intervals that hold an edge belong to neither)
    noisy = db[a + 1:b - 1]
    lo = min(p[0] for p in wf.TEST_DB.values())
    hi = max(p[1] for p in wf.TEST_DB.values())
    print(f"clean max {clean.max():.2f} dB, noisy min {noisy.min():.2f} dB; lo {lo}, hi {hi}")
    assert clean.max() <= lo - 6.0 and noisy.min() >= hi + 6.0
    # ... and with the tests' time constants every t goes 0, 1, 0
    cfg = wf.config(attack_ms=wf.TEST_MS[0], release_ms=wf.TEST_MS[1], **wf.TEST_DB)
    _, t = wf.control(u, cfg)
    assert not t[:a - 1].any() and np.all(t[b - 2] == 1.0) and not t[-50:].any()

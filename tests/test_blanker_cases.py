"""The captures of tests/test_gpu_blanker.py (blanker_fixture.capture25 / capture10) against the fixture alone, not the
code under test: the GPU tests compare bits, and they mean something only while no clean sample is near the threshold and
every burst is far above it.  On the clean captures nothing triggers and the largest p / T is at most 0.5; every injected
burst behind interval 0 has p / T >= 2; less than 1 % of the samples are blanked.  (Measured: 0.124 and 27 at 2.5 MS/s,
0.065 and 5.0 at 10 MS/s; blanked shares 0.53 % and 0.10 %.)"""
import numpy as np
import pytest

import blanker_fixture as bf

Q = bf.Q
CASES = {
    "2.5 MS/s": (bf.capture25, lambda: sum(bf.bursts25().values(), []), dict(bf.CFG25)),
    "10 MS/s": (bf.capture10, lambda: [p + k for p in bf.bursts10() for k in (0, 1)],
                dict(zip(("G", "M"), bf.defaults(bf.F10)), W=16, threshold_db=12.0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_margins_of_the_gpu_captures(case):
    capture, bursts, cfg = CASES[case]
    clean = bf.run(capture(clean=True), **cfg)
    ratio = (clean["p"].astype(np.float64) / np.repeat(clean["T"], Q)[:len(clean["p"])])[Q:]
    print(f"{case}: clean max p / T = {ratio.max():.4f}")
    assert not clean["trig"].any() and ratio.max() <= 0.5
    r = bf.run(capture(), **cfg)
    pos = np.array([p for p in bursts() if p >= Q])
    assert len(pos) >= 50
    over = r["p"][pos].astype(np.float64) / r["T"][pos // Q]
    print(f"{case}: bursts min p / T = {over.min():.3f}, blanked share {r['blank'].mean():.5f}")
    assert over.min() >= 2.0 and r["trig"][pos].all()
    assert 0.0 < r["blank"].mean() < 0.01


def test_what_the_2_5_ms_capture_exercises():
    """Each placement the GPU tests name is really there: the edge, the call boundary, merged and separate gates, give-up
    and re-arm in the train, NaN and Inf, interval 0, the step."""
    r, b, (G, M) = bf.run(bf.capture25(), **bf.CFG25), bf.bursts25(), (bf.CFG25["G"], bf.CFG25["M"])
    blank, trig = r["blank"], r["trig"]
    assert not trig[:Q].any() and not blank[b["interval0"]].any()
    assert blank[10 * Q - 1] and blank[10 * Q] and blank[20 * Q - 1] and blank[20 * Q] and not blank[20 * Q + 1] and not blank[30 * Q - 1]
    edge = sum(map(sum, bf.CALLS25[:2]))
    assert b["call"] == [edge - 1, edge] and blank[edge - 1:edge + G].all() and not blank[edge - 2] and not blank[edge + G]
    assert blank[50000:50003].all() and not blank[50003] and blank[50010:50014].all() and not blank[50014]
    assert blank[50020:50022].all() and not blank[50022] and blank[50023:50025].all()
    t0 = b["train"][0]
    first = b["train"][:3 * M // 2]
    assert blank[t0:t0 + M].all() and not blank[t0 + M:first[-1] + G].any() and r["gate"][t0:first[-1] + G].all()
    t1 = b["train"][3 * M // 2]
    assert not r["gate"][first[-1] + G:t1].any() and t1 - (first[-1] + G) == 3 and blank[t1:t1 + M].all() and not blank[t1 + M]
    assert blank[bf.NAN25] and blank[bf.INF25] and r["records"]["n_nonfinite"].sum() == 2
    assert trig[bf.STEP25:bf.STEP25 + 4 * Q].sum() > 1000 and not trig[bf.STEP25 + 5 * Q:].any()

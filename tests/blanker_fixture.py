"""The impulse blanker's definitions (include/fmradion_amd.h, "Impulse blanker on the capture") restated in numpy.

One input row at a time, the whole row at once: the definitions do not know about blocks or calls.  Everything is exact
(fp32 products and sums rounded one by one, 64-bit integer levels, two fp64 products for the threshold), so the device's
rows and records are compared with these bit for bit.
"""
import math

import numpy as np

Q = 4096
RECORD = np.dtype([("index", np.uint64), ("first_interval", np.uint64), ("n_triggers", np.uint64),
                   ("n_blanked", np.uint64), ("n_nonfinite", np.uint64), ("n_runs", np.uint64),
                   ("power_q", np.uint64), ("threshold", np.float64), ("n_intervals", np.uint32),
                   ("peak", np.float32)])
T_FLOOR = 2.0 ** -30


def defaults(input_rate, gate_samples=0, max_run_samples=0):
    """G and M as fmr_enable_blanker fills them in."""
    G = gate_samples or min(256, max(2, int(np.ceil(0.8e-6 * input_rate))))
    M = max_run_samples or min(1024, 8 * G)
    return G, M


def power(x):
    """p[n] = fl32(fl32(re re) + fl32(im im))"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    v = x.view(np.float32).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        return (v[:, 0] * v[:, 0]) + (v[:, 1] * v[:, 1])


def levels(p):
    """(q [n] uint64, non-finite [n] bool, A [complete and open intervals] uint64)"""
    nonfin = ~np.isfinite(p)
    pc = np.where(nonfin, np.float32(0), np.minimum(p, np.float32(256)))
    q = np.floor(pc.astype(np.float64) * 2.0 ** 36).astype(np.uint64)
    nj = (len(p) + Q - 1) // Q
    qq = np.zeros(nj * Q, dtype=np.uint64)
    qq[:len(p)] = q
    return q, nonfin, qq.reshape(nj, Q).sum(axis=1, dtype=np.uint64)


def thresholds(A, threshold_db, W):
    """T_j for j = 0 .. len(A) - 1 from the A of the intervals before j"""
    g = math.pow(10.0, threshold_db / 10.0)        # (the C library's pow, as the stage calls it)
    T = np.empty(len(A), dtype=np.float64)
    for j in range(len(A)):
        if j == 0:
            T[j] = np.inf
            continue
        c = min(j, W)
        S = int(np.sum(A[j - c:j], dtype=np.uint64))
        r = 1.0 / (float(c) * 2.0 ** 48)
        T[j] = max(g * (float(S) * r), T_FLOOR)
    return T


def run(x, G, M, W=16, threshold_db=12.0, R=256):
    """The blanker over one row.  Returns a dict: out (complex64), p, trig, gate, blank (bool), A (uint64 per interval, the
    last one possibly open), T (per interval) and records (RECORD, the complete ones)."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    N = len(x)
    p = power(x)
    q, nonfin, A = levels(p)
    T = thresholds(A, threshold_db, W)
    Tn = np.repeat(T, Q)[:N]
    trig = nonfin | (p.astype(np.float64) > Tn)
    n = np.arange(N)
    C = np.concatenate(([0], np.cumsum(trig, dtype=np.int64)))
    gate = (C[n + 1] - C[np.maximum(n - G + 1, 0)]) > 0
    Cg = np.concatenate(([0], np.cumsum(gate, dtype=np.int64)))
    blank = gate & ((n < M) | ((Cg[n] - Cg[np.maximum(n - M, 0)]) < M))
    out = x.copy()
    out[blank] = 0
    starts = blank & ~np.concatenate(([False], blank[:-1]))
    n_int = N // Q                     # complete intervals
    n_rec = n_int // R
    recs = np.zeros(n_rec, dtype=RECORD)
    for i in range(n_rec):
        s = slice(i * R * Q, (i + 1) * R * Q)
        fin = ~nonfin[s]
        recs[i] = (i, i * R, trig[s].sum(), blank[s].sum(), nonfin[s].sum(), starts[s].sum(),
                   int(np.sum(A[i * R:(i + 1) * R] >> np.uint64(12), dtype=np.uint64)), T[(i + 1) * R - 1], R,
                   p[s][fin].max() if fin.any() else np.float32(0))
    return {"out": out, "p": p, "trig": trig, "gate": gate, "blank": blank, "A": A, "T": T, "records": recs}


# ---- the captures of the GPU tests (tests/test_gpu_blanker.py; tests/test_blanker_cases.py guards them) ----
F25, BLK25, OFFS25 = 2.5e6, 16384, [-700_000, 250_000]
N25 = 122 * Q
CFG25 = dict(G=2, M=16, W=4, threshold_db=12.0, R=8)
# the cut into calls the GPU tests use: a call ends behind sample 99303
CALLS25 = [[BLK25] * 5, [BLK25, 1000], [BLK25] * 4, [7], [BLK25] * 8, [BLK25] * 8, [BLK25] * 4]
CALLS25.append([N25 - sum(map(sum, CALLS25))])
STEP25 = 400000                    # the +20 dB step
BURST25 = 8.0                      # 16 to 27 times the carriers (0.3 and 0.2)


def bursts25():
    """Burst positions of the 2.5 MS/s capture, by kind (interval 0 passes; the others trigger)."""
    M = CFG25["M"]
    train = [200000 + 2 * k for k in range(3 * M // 2)]          # a trigger every other sample for 3 M samples: give-up
    train += [train[-1] + 5 + 2 * k for k in range(M)]           # ... three open samples, then again: re-arm
    return {"interval0": [100],
            "edge": [10 * Q - 1, 10 * Q, 20 * Q - 1, 30 * Q],    # on both sides of an interval edge
            "call": [99303, 99304],                              # the last sample of a call and the first of the next
            "close": [50000, 50001, 50010, 50012, 50020, 50023],  # within G of each other, and just not
            "train": train}


NAN25, INF25 = 250000, 260000


def capture25(clean=False):
    """Two FM stereo stations at 2.5 MS/s, 122 intervals; clean, or with the bursts, one NaN, one Inf and the step."""
    import chanbank_fixture as cb
    x = cb.composite(N25, F25, OFFS25, [3, 4], [0.3, 0.2])
    if clean:
        return x
    rng = np.random.default_rng(7)
    for pos in sum(bursts25().values(), []):
        x[pos] += np.complex64(BURST25 * np.exp(2j * np.pi * rng.random()))
    x[NAN25] = np.complex64(complex(np.nan, 0.25))
    x[INF25] = np.complex64(complex(0.1, np.inf))
    x[STEP25:] *= np.float32(10.0)
    return x


F10, BLK10, N10 = 10e6, 65536, 8 * 65536
BURST10 = 3.0                      # ten times the carrier (0.3)


def bursts10():
    """60 bursts of two samples at 10 MS/s, two of them across the calls' edges (calls of 2 x 65536)."""
    rng = np.random.default_rng(11)
    pos = sorted(set(int(v) for v in rng.integers(Q, N10 - 2, 58)) | {2 * BLK10 - 1, 4 * BLK10 - 2})
    return pos


def capture10(clean=False):
    """The benchmark's station at 10 MS/s, 128 intervals; clean or with the bursts."""
    import siggen
    x = siggen.fm_stereo_iq(N10, F10).astype(np.complex64)
    if clean:
        return x
    rng = np.random.default_rng(12)
    for pos in bursts10():
        x[pos:pos + 2] += np.complex64(BURST10 * np.exp(2j * np.pi * rng.random()))
    return x

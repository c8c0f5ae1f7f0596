"""The noisy captures of the RDS error-correction tests and the reference's counts on them, computed once per process and
shared by tests/test_rds_fec_reference.py (CPU) and tests/test_gpu_rds_fec.py.

The MPX is built as in tests/test_gpu_rds_reference.py's sensitivity cases: a stereo programme with an RDS subcarrier of
2 / 75 carrying known groups, t0 = 2 ms, 20 s, white noise of sigma on the MPX; three noise seeds."""
import functools

import numpy as np

import rds_fec_reference as fr
import rds_fixture as rf

FS = 384000.0
SECONDS = 20.0
T0 = 0.002
KIND = "stereo"
SEEDS = (5, 6, 7)
SIGMA = (0.10, 0.1122, 0.126)                   # steps of 1 dB
UP = {0.10: 0.1122, 0.1122: 0.126}              # the noise 1 dB up
ACQ_GROUPS, TAIL_GROUPS = 4, 3                  # groups left out at either end, as in test_gpu_rds_reference.py
N = int(SECONDS * FS)
N_SENT = int((N / FS - T0) / (104 * rf.TD))
MODES = {"off": dict(mode=fr.OFF), "burst": dict(mode=fr.BURST, max_burst=2),
         "soft": dict(mode=fr.SOFT, soft_symbols=4, soft_max_cost=1.0)}


@functools.lru_cache(maxsize=None)
def groups():
    return rf.ps_groups(0xBEEF, "NOISYREF", rt="NOISE LEVELS", n=int(N / FS / (104 * rf.TD)) + 2)


@functools.lru_cache(maxsize=None)
def clean():
    m = rf.known_mpx(N, groups(), KIND, t0=T0)
    m.setflags(write=False)
    return m


def noisy(seed, sigma):
    return clean() + sigma * np.random.default_rng(seed).standard_normal(N)


@functools.lru_cache(maxsize=None)
def reference(seed, sigma):
    """{mode: (bad or missing blocks, corrected blocks with wrong bits, corrected blocks)} of the float64 receiver with
    tests/rds_fec_reference.py's correction, over the groups ACQ_GROUPS .. N_SENT - TAIL_GROUPS - 1."""
    sym = fr.blind_symbols(noisy(seed, sigma))
    return {name: fr.counts(sym, groups(), T0, ACQ_GROUPS, N_SENT - TAIL_GROUPS, **kw) for name, kw in MODES.items()}


def pooled(sigma, mode, what=0):
    return sum(reference(seed, sigma)[mode][what] for seed in SEEDS)

"""The float64 RDS receiver of tests/rds_reference.py on its own (no GPU): the conditions tests/test_gpu_rds_reference.py
relies on are checked here, where no GPU is needed.

Theory used below: the correlator's noise on the decision axis is sigma sqrt(32 / (pi^2 SPS)) = 0.1001 sigma in units
of the subcarrier level, a symbol error has the probability Q(level / that), and a block of 26 differentially decoded
bits depends on 27 symbols: 0.06 %, 1.2 % and 10 % of the blocks at sigma 0.065, 0.08 and 0.10 (injection 2 / 75).
"""
import math

import numpy as np
import pytest

import oracle_py as ora
import rds_fixture as rf
import rds_reference as rr

FS = 384000.0


def ngroups(n):
    return int(n / FS / (104 * rf.TD)) + 2


def wrap(x, period):
    return (x + period / 2) % period - period / 2


def block_share_theory(sigma, level=2.0 / 75.0):
    q = 0.5 * math.erfc(level / (sigma * math.sqrt(32.0 / (np.pi ** 2 * rr.SPS))) / math.sqrt(2.0))
    return 1.0 - (1.0 - q) ** 27


def test_doublet_energy_is_pi_squared_over_16():
    """int d^2 dt / TD = pi^2 / 16 = 0.6169: the gain every level estimate is divided by."""
    assert abs(rr.doublet_energy() - np.pi ** 2 / 16) < 1e-6
    assert abs(rr.GAIN - 0.5 * rf.TD * 0.61685) < 1e-9


def test_discriminator_returns_the_mpx():
    """oracle_py.PhaseDiscriminator on the constant-envelope IQ of an MPX (noise on the MPX, before the modulation)
    returns that MPX: delay 0 samples, maximum error 7.3e-7 measured (stereo programme + RDS + sigma 0.1122, peak 1.37).
    The bound: two float32 phases in (-pi, pi] are differenced; each carries half a spacing of 2^-22 from its own
    rounding, one spacing from atan2f and 2^-24 sqrt(2) from the complex64 input: 2 (1.2 + 2.4 + 0.84)e-7 rad, over
    2 pi 75000 / 384000 = 1.227 rad per unit: 7.2e-7, with the division's rounding 1e-6.  The RDS subcarrier is 1.3e-2
    to 1e-1: the MPX in front of the RDS stage is the generated one, and the expected sample_index has no latency."""
    n = 2 * 384000
    groups = rf.ps_groups(0xC0DE, "DISCRIM", n=ngroups(n))
    mpx = rf.known_mpx(n, groups, "stereo") + 0.1122 * np.random.default_rng(5).standard_normal(n)
    assert np.abs(mpx).max() < 1.5
    out = ora.PhaseDiscriminator(75000.0 / FS).process(rf.mpx_iq(mpx)).astype(np.float64)
    err = {lag: float(np.abs(out[2:-2] - mpx[2 - lag:n - 2 - lag]).max()) for lag in (-1, 0, 1)}
    print("discriminator max error by delay:", err)
    assert err[0] < 1e-6 and err[-1] > 0.1 and err[1] > 0.1, err
    assert abs(out[0] - mpx[0]) < 1e-6


PARAMS = [  # t0 [s], phase, f_off [Hz], level
    (0.002, -np.pi / 2, 0.0, 2 / 75),
    (0.00237, 0.3, 3.0, 1 / 75),
    (0.999 * rf.TD, 3.1, -1.14, 7.5 / 75),
]


@pytest.mark.parametrize("kind", ["mono", "stereo", "tone15"])
def test_clean_signal(kind):
    """sigma = 0, every programme (the 15 kHz L-R tone included): genie has no bad block, blind finds the same blocks at
    the same places with the same outcome and the transmitted words, and its estimates are the transmitted values.
    Bounds: the fixture draws the baseband by linear interpolation on a 380 kHz grid (relative error (pi f / fs)^2 / 2 <
    2e-4 at 2.4 kHz: the level; a timing granularity far below 0.01 sample); a window of 64 symbols on its own is
    within 0.2 sample (pattern noise of the timing estimator; measured 0.094)."""
    n = 3 * 384000
    groups = rf.ps_groups(0xC0DE, "REFTEST1", rt="REFERENCE RECEIVER", n=ngroups(n))
    words = [w for g in groups for w in g]
    for t0, phase, f_off, level in PARAMS:
        mpx = rf.known_mpx(n, groups, kind, level, phase, t0, f_off)
        g = rr.genie(mpx, t0, phase, f_off, groups)
        b = rr.blind(mpx)
        assert len(g["bad"]) >= 130 and not g["bad"].any() and g["bit_errors"] == 0
        assert np.abs(np.abs(g["soft"].real) / level - 1).max() < 1e-3          # no intersymbol interference
        blk = (b["block_start"] - t0 * FS) / (26 * rr.SPS)
        num = np.round(blk).astype(int)
        assert np.abs(blk - num).max() * 26 * rr.SPS < 0.2
        assert num[0] <= g["first_block"] + 1 and num[-1] >= g["first_block"] + len(g["bad"]) - 2
        assert np.array_equal(num, num[0] + np.arange(len(num))) and not b["block_bad"].any()
        assert np.array_equal(b["block_slot"], num % 4)
        assert [int(v) for v in b["block_info"]] == words[num[0]:num[0] + len(num)]
        grp = (b["group_start"] - t0 * FS) / (104 * rr.SPS)
        assert np.abs(grp - np.round(grp)).max() * 104 * rr.SPS < 0.2
        est = (wrap((b["t0"] - t0) * FS, rr.SPS), wrap(b["phase"] - phase, np.pi), b["f_off"] - f_off, b["level"] / level - 1)
        print(kind, "timing %.5f samples, phase %.2e rad, offset %.2e Hz, level %.2e, window %.3f samples" %
              (*est, np.abs(b["window_dev"]).max()))
        assert abs(est[0]) < 0.01 and abs(est[1]) < 1e-5 and abs(est[2]) < 1e-5 and abs(est[3]) < 2e-4, est
        assert np.abs(b["window_dev"]).max() < 0.2


def test_noisy_levels():
    """20 s (about 900 blocks) at the levels of the GPU comparison, mono and stereo: genie's share of bad blocks is what
    the theory gives (within four standard deviations of the count, at least +- 3); at 0.08 and 0.10 it lies between 0.3 %
    and 15 %, at 0.065 below 0.3 %; blind has no fewer bad blocks than genie minus those a 10-bit checkword lets pass
    (three) and stays within the same theory window 1 dB up, where the GPU comparison takes its cap."""
    n = 20 * 384000
    groups = rf.ps_groups(0xBEEF, "NOISYREF", rt="NOISE LEVELS", n=ngroups(n))
    noise = np.random.default_rng(5).standard_normal(n)
    for kind in ("mono", "stereo"):
        clean = rf.known_mpx(n, groups, kind)
        for sigma in (0.065, 0.08, 0.10):
            g = rr.genie(clean + sigma * noise, 0.002, -np.pi / 2, 0.0, groups)
            nb, bad = len(g["bad"]), int(g["bad"].sum())
            want = nb * block_share_theory(sigma)
            print(kind, sigma, "genie", bad, "of", nb, "theory %.1f" % want, "BER %.2e" % (g["bit_errors"] / g["n_bits"]))
            assert nb >= 880
            assert abs(bad - want) <= max(3.0, 4.0 * math.sqrt(want)), (kind, sigma, bad, want)
            if sigma >= 0.08:
                assert 0.003 * nb <= bad <= 0.15 * nb, (kind, sigma, bad, nb)
            else:
                assert bad <= 0.003 * nb, (kind, sigma, bad, nb)
            up = sigma * 10 ** (1 / 20)
            b = rr.blind(clean + up * noise)
            gu = rr.genie(clean + up * noise, 0.002, -np.pi / 2, 0.0, groups)
            bb, gb = int(b["block_bad"].sum()), int(gu["bad"].sum())
            print(kind, "%.4f" % up, "blind", bb, "of", len(b["block_bad"]), "genie", gb)
            assert bb >= gb - 3 and bb >= 1, (kind, sigma, bb, gb)
            assert abs(bb - nb * block_share_theory(up)) <= max(3.0, 4.0 * math.sqrt(nb * block_share_theory(up))) + 3
            assert abs(wrap((b["t0"] - 0.002) * FS, rr.SPS)) < 0.5 and abs(b["f_off"]) < 0.01
            assert abs(wrap(b["phase"] + np.pi / 2, np.pi)) < 0.02

"""RDS error correction on the GPU (fmr_set_rds_correction; DESIGN.md section 9, "Error correction"): the symbol
reliabilities the device stage hands over (fmr_debug_read 5) against the float64 receiver of tests/rds_reference.py, and
the corrected chain against that receiver with the numpy correction of tests/rds_fec_reference.py.

As in tests/test_gpu_rds_reference.py every case puts a KNOWN MPX in front of the stage: a 384 kHz FM chain without
resampler is fed the constant-envelope IQ of that MPX, noise added to the MPX before the modulation.  No bound is taken
from the chain's output: the caps are the reference's own counts on the same captures with the noise 1 dB up
(tests/rds_fec_cases.py), the deviation of the reliabilities is held to twice the blind reference's own plus the two
approximations the design documents."""
import functools
import importlib

import numpy as np
import pytest

import chanbank_fixture as cb
import rds_fec_cases as cases
import rds_fixture as rf
import rds_reference as rr
import rds_fec_reference as fr
import test_gpu_rds_reference as tg

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS = cases.FS
BLK = tg.BLK
SPS = rr.SPS
GROUP = 104 * SPS
MODE_ARGS = {"off": (fmr.RDS_FEC_OFF,), "burst": (fmr.RDS_FEC_BURST, 2), "soft": (fmr.RDS_FEC_SOFT, 0, 4, 1.0)}


def run(x, mode=None, **kw):
    ch = tg.make_chain(**kw)
    if mode is not None:
        ch.set_rds_correction(*MODE_ARGS[mode])
    tg.feed(ch, x)
    got, st = ch.rds_groups(0), ch.rds_status(0)
    ch.close()
    return got, st


def group_numbers(got, t0=cases.T0):
    return [int(round((int(g["sample_index"]) - t0 * FS) / GROUP)) for g in got]


def chain_counts(got, groups, lo, hi, t0=cases.T0):
    """Over the groups lo .. hi - 1: (blocks bad or missing, a missing group counting four; corrected blocks whose 16 bits
    are not the ones sent; corrected blocks)."""
    by = dict(zip(group_numbers(got, t0), got))
    bad = wrong = corrected = 0
    for k in range(lo, hi):
        if k not in by:
            bad += 4
            continue
        g = by[k]
        for b in range(4):
            s = int(g["status"][b])
            bad += (s & fmr.RDS_BAD) != 0
            corrected += (s & fmr.RDS_CORRECTED) != 0
            wrong += (s & fmr.RDS_CORRECTED) != 0 and int(g["block"][b]) != groups[k][b]
    return bad, wrong, corrected


@functools.lru_cache(maxsize=None)
def chain_run(seed, sigma, mode):
    got, st = run(rf.mpx_iq(cases.noisy(seed, sigma)), mode)
    num = group_numbers(got)
    assert num == sorted(set(num)), (seed, sigma, mode, num)
    return chain_counts(got, cases.groups(), cases.ACQ_GROUPS, cases.N_SENT - cases.TAIL_GROUPS) + (int(st.blocks_corrected),)


# ---- reliabilities ----------------------------------------------------------------------------------------------------
def interpolation_term():
    """rms error of the stage's Catmull-Rom interpolator over the sampling phase, weighted with the spectrum of the matched
    filter's output, relative to the level (3.0e-4): computed as tests/test_gpu_rds_reference.py's level_term does."""
    f = np.linspace(-2374.0, 2374.0, 2001)
    wgt = (np.cos(np.pi * f * rf.TD / 4) ** 2 * np.abs(1 - np.exp(-1j * np.pi * f * rf.TD))) ** 2
    u = np.linspace(0, 1, 101)[:, None]
    w = 2 * np.pi * f[None, :] / tg.FS2
    c = [-0.5 * u ** 3 + u ** 2 - 0.5 * u, 1.5 * u ** 3 - 2.5 * u ** 2 + 1, -1.5 * u ** 3 + 2 * u ** 2 + 0.5 * u,
         0.5 * u ** 3 - 0.5 * u ** 2]
    err = np.abs(sum(c[j] * np.exp(1j * w * (j - 1)) for j in range(4)) - np.exp(1j * w * u)) ** 2
    return float(np.sqrt((err.mean(axis=0) * wgt).sum() / wgt.sum()))


def feed_and_tap(ch, x):
    """x through process_blocks in calls of up to 16 blocks; tap 5 after every call, joined."""
    rho = []
    for i in range(0, len(x), 16 * BLK):
        m = min(16 * BLK, len(x) - i)
        ch.process_blocks(x[None, i:i + m], [BLK] * (m // BLK) + ([m % BLK] if m % BLK else []))
        rho.append(ch.rds_reliabilities(0))
    return np.concatenate(rho)


def on_air(g):
    """The 104 bits of a group as (block, status) say they were received; None unless every block is good."""
    if any(int(s) & ~fmr.RDS_CPRIME for s in g["status"]):
        return None
    names = ("A", "B", "Cp" if int(g["status"][2]) & fmr.RDS_CPRIME else "C", "D")
    return np.array([(rf.block_word(int(v), o) >> (25 - i)) & 1 for v, o in zip(g["block"], names) for i in range(26)],
                    dtype=np.uint8)


@pytest.mark.parametrize("sigma", [0.0, 0.08])
def test_reliabilities(sigma):
    """fmr_debug_read 5, call after call, is one value per symbol: its signs, differentially decoded, are the bits the
    chain's groups were made of (every block's 16 bits, good or bad, at its place), and the values follow the genie
    receiver's soft symbols (known timing and carrier, level units): rms deviation over the symbols behind the groups the
    chain may lose while it acquires <= 2 x the blind reference's own rms deviation from the genie + the cut-off pulse
    tails (0.0057) + the interpolator's error (3e-4).

    Measured on an MI355X: rms 2.3e-4 noise-free (blind 2.6e-5, bound 0.0061), 0.0847 at sigma 0.08 (blind 0.0801, bound
    0.166; mean |rho| 0.924, the window's energy containing the noise)."""
    nwin = 40
    n = tg.windows_len(nwin)
    level, t0 = 2.0 / 75.0, 0.002
    groups = rf.ps_groups(0x50F7, "SOFTBITS", rt="RELIABILITIES", n=tg.ngroups(n))
    mpx = rf.known_mpx(n, groups, "stereo", level=level, t0=t0)
    if sigma > 0:
        mpx = mpx + sigma * np.random.default_rng(21).standard_normal(n)
    ch = tg.make_chain()
    rho = feed_and_tap(ch, rf.mpx_iq(mpx))
    got = ch.rds_groups(0)
    ch.close()
    assert np.isfinite(rho).all() and len(rho) >= 64 * (nwin - 1) and len(got) >= 9, (len(rho), len(got))
    bits = rf.diff_decode((rho < 0).astype(np.uint8))
    # place: a group with four good blocks, found in the bit stream (bits[i] belongs to rho[i])
    num = group_numbers(got, t0)
    anchor = next(i for i, g in enumerate(got) if on_air(g) is not None)
    pat = on_air(got[anchor])
    hits = [i for i in range(1, len(bits) - 104) if np.array_equal(bits[i:i + 104], pat)]
    hits = [i for i in hits if abs(i - 104 * num[anchor]) < 64]          # (the programme repeats: the one at its time)
    assert len(hits) == 1, hits
    sym0 = hits[0] - 104 * num[anchor]              # index into rho of the transmitter's symbol 0
    for g, k in zip(got, num):
        for b in range(4):
            i = sym0 + 104 * k + 26 * b
            word = int("".join(map(str, bits[i:i + 16])), 2)
            assert word == int(g["block"][b]), (k, b)
    # values: the genie's symbols are numbered from the transmitter's first
    ge = rr.genie(mpx, t0, -np.pi / 2, 0.0, groups)
    kg = rr._symbol_range(n, t0 * FS)
    rho_g = ge["soft"].real / level
    bl = fr.blind_symbols(mpx)
    kb = np.round((bl["symbol_pos"] - t0 * FS) / SPS).astype(int)
    lo = 104 * tg.ACQ_GROUPS
    hi = min(kg[-1], kb[-1], len(rho) - 1 - sym0)
    k = np.arange(lo, hi + 1)
    a, b, c = rho_g[k - kg[0]], bl["rho"][k - kb[0]], rho[k + sym0].astype(np.float64)
    b = b * np.sign(np.dot(a, b))                   # (each receiver knows the carrier modulo pi)
    c = c * np.sign(np.dot(a, c))
    rms_blind = float(np.sqrt(np.mean((b - a) ** 2)))
    rms_chain = float(np.sqrt(np.mean((c - a) ** 2)))
    bound = 2 * rms_blind + tg.pulse_tail() + interpolation_term()
    print(f"\nsigma {sigma}: {len(k)} symbols, rms(rho_chain - rho_genie) {rms_chain:.4g}, rms(rho_blind - rho_genie) "
          f"{rms_blind:.4g}, bound {bound:.4g}; mean |rho| chain {np.abs(c).mean():.4f} genie {np.abs(a).mean():.4f}")
    assert rms_chain <= bound, (rms_chain, bound, rms_blind)


def test_reliabilities_stay_finite():
    """A burst of NaN and a stretch of zeros in the capture: every reliability is finite, and zero where the MPX was."""
    n = tg.windows_len(14)
    groups = rf.ps_groups(0x0BAD, "NANBURST", n=tg.ngroups(n))
    x = rf.mpx_iq(rf.known_mpx(n, groups, "stereo"))
    x[150_000:150_400] = np.nan
    zeros = np.zeros(tg.windows_len(6), dtype=np.complex64)
    ch = tg.make_chain(n_streams=2)
    xs = np.stack([x, np.concatenate([zeros, x[len(zeros):]])])
    ch.process_blocks(xs, [BLK] * (n // BLK) + [n % BLK])
    rho = [ch.rds_reliabilities(s) for s in (0, 1)]
    st = ch.rds_status(0)
    ch.close()
    assert len(rho[0]) >= 64 * 12 and np.isfinite(rho[0]).all() and np.isfinite(rho[1]).all()
    assert np.isfinite([st.injection, st.timing, st.carrier_phase, st.carrier_offset_hz]).all()
    assert np.all(rho[1][:64 * 3] == 0.0) and np.abs(rho[1][-64:]).mean() > 0.5       # (windows 0 .. 2 saw only zeros)
    assert np.abs(rho[0][-64:]).mean() > 0.5


def test_tap_needs_rds():
    ch = tg.make_chain(enable_rds=False)
    ch.process_blocks(np.zeros((1, BLK), dtype=np.complex64), [BLK])
    with pytest.raises(fmr.FmrError, match="fmr_create_rds"):
        ch.rds_reliabilities(0)
    with pytest.raises(fmr.FmrError, match="fmr_create_rds"):
        ch.set_rds_correction(fmr.RDS_FEC_SOFT)
    ch.close()


# ---- sensitivity and safety -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.10, 0.1122])
@pytest.mark.parametrize("mode", ["burst", "soft"])
def test_sensitivity(mode, sigma):
    """Pooled over three seeds of 20 s: the chain's bad or missing blocks with correction on do not exceed the count of the
    float64 receiver with the same correction on the same captures with the noise 1 dB up (the rule of section 9).  That
    cap lies far below what detection alone leaves at sigma (tests/test_rds_fec_reference.py): a chain that only passes
    blocks through cannot meet it.

    Measured on an MI355X (chain / reference at sigma / cap): bursts 16 / 16 / 57 and 60 / 57 / 188, soft 4 / 3 / 28 and
    34 / 28 / 105, at sigma 0.10 and 0.1122."""
    runs = [chain_run(seed, sigma, mode) for seed in cases.SEEDS]
    bad = sum(r[0] for r in runs)
    cap = cases.pooled(cases.UP[sigma], mode)
    print(f"\n{mode} sigma {sigma}: chain {bad} bad blocks {[r[0] for r in runs]} (corrected {[r[2] for r in runs]}), reference "
          f"{cases.pooled(sigma, mode)} at sigma, {cap} at sigma + 1 dB; detection only: reference {cases.pooled(sigma, 'off')}")
    assert all(r[3] >= r[2] for r in runs)              # (blocks_corrected counts them)
    assert bad <= cap, f"{mode} sigma {sigma}: chain {bad} bad blocks, reference 1 dB up {cap}"


@pytest.mark.parametrize("mode", ["burst", "soft"])
def test_safety(mode):
    """Corrected blocks whose 16 bits are not the ones sent, pooled over the sensitivity captures: no more than the
    float64 receiver with bursts of up to 2 -- the standard's own method -- leaves on them with the noise 1 dB up.

    Measured on an MI355X: 6 of 825 (bursts) and 1 of 863 (soft) against a cap of 25."""
    wrong = sum(chain_run(seed, sigma, mode)[1] for sigma in cases.UP for seed in cases.SEEDS)
    corrected = sum(chain_run(seed, sigma, mode)[2] for sigma in cases.UP for seed in cases.SEEDS)
    cap = sum(cases.pooled(up, "burst", 1) for up in cases.UP.values())
    print(f"\n{mode}: chain {wrong} of {corrected} corrected blocks wrong; reference (burst <= 2, 1 dB up) {cap}; reference "
          f"at sigma: {sum(cases.pooled(s, mode, 1) for s in cases.UP)}")
    assert wrong <= cap, (mode, wrong, cap)


@pytest.mark.parametrize("mode", ["burst", "soft"])
def test_noise_only(mode):
    """MPX noise without a subcarrier, correction on: acquisition works on uncorrected syndromes and corrected blocks do
    not hold a lock, so the bounds of test_gpu_rds_reference.py's noise row stand: blocks_ok <= 2, no group of good blocks."""
    n = tg.windows_len(52)
    got, st = run(rf.mpx_iq(0.1 * np.random.default_rng(11).standard_normal(n)), mode)
    print(f"\n{mode}: ok {st.blocks_ok} corrected {st.blocks_corrected} bad {st.blocks_bad}, {len(got)} groups")
    assert st.blocks_ok <= 2, st.blocks_ok
    assert not any(all(int(v) == fmr.RDS_OK for v in g["status"]) for g in got)


# ---- what must not change ---------------------------------------------------------------------------------------------
def short_noisy(nwin, sigma=0.10, seed=5):
    return rf.mpx_iq(cases.noisy(seed, sigma)[:tg.windows_len(nwin)])


def test_off_changes_nothing():
    """set_rds_correction(OFF) and no call at all: identical groups and status."""
    x = short_noisy(80)
    a, sa = run(x)
    b, sb = run(x, "off")
    assert len(a) >= 30 and np.array_equal(a, b) and bytes(sa) == bytes(sb)
    assert sa.blocks_bad > 0 and sa.blocks_corrected == 0


@pytest.mark.parametrize("in_order", [False, True])
def test_cut_independence(in_order):
    """Soft correction on: calls of 1 .. 257 samples through fmr_process over the first 0.3 s, then whole blocks, against
    calls of 16 blocks: identical groups, corrected ones among them."""
    x = short_noisy(40)
    n = len(x)
    ref, st = run(x, "soft", in_order=in_order)
    ch = tg.make_chain(in_order=in_order, max_blocks=1)
    ch.set_rds_correction(*MODE_ARGS["soft"])
    cyc, pos, i = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257), 0, 0
    while pos < n:
        m = min(cyc[i % len(cyc)] if pos < 0.3 * FS else BLK, n - pos)
        ch.process(x[pos:pos + m])
        pos += m
        i += 1
    got = ch.rds_groups(0)
    ch.close()
    assert len(ref) >= 15 and st.blocks_corrected > 0, (len(ref), st.blocks_corrected)
    assert np.array_equal(got, ref), (len(got), len(ref))


def test_switch_in_mid_stream():
    """OFF for the first call, then SOFT: no group is lost; every block in front of one block boundary is what the chain
    with correction off returns (blocks soft correction would have repaired among them), every block behind it what the
    chain with soft correction returns.  The boundary lies between the end of the first call less the stage's latency (at
    most three windows) and the end of the first call."""
    x = short_noisy(120)
    off, _ = run(x, "off")
    soft, _ = run(x, "soft")
    ch = tg.make_chain()
    cut = 16 * BLK
    tg.feed(ch, x[:cut])
    ch.set_rds_correction(*MODE_ARGS["soft"])
    tg.feed(ch, x[cut:])
    got = ch.rds_groups(0)
    ch.close()
    assert len(got) == len(off) == len(soft) >= 60 and np.array_equal(got["sample_index"], off["sample_index"])

    def flat(a):
        return [(int(g["block"][b]), int(g["status"][b])) for g in a for b in range(4)]
    fg, fo, fs = flat(got), flat(off), flat(soft)
    start = [int(g["sample_index"]) + b * 26 * SPS for g in got for b in range(4)]
    split = next((i for i in range(len(fg)) if fg[i] != fo[i]), len(fg))
    assert fg[:split] == fo[:split] and fg[split:] == fs[split:], split
    assert any(s & fmr.RDS_CORRECTED for _, s in fs[:split]) and any(s & fmr.RDS_CORRECTED for _, s in fg[split:])
    for i in range(len(fg)):
        if start[i] >= cut:
            assert fg[i] == fs[i], i
        if start[i] + 26 * SPS <= cut - 3 * 64 * SPS:
            assert fg[i] == fo[i], i


# ---- bank -------------------------------------------------------------------------------------------------------------
BANK_F = 10e6
BANK_OFFS = [-3_900_000, -1_500_000, 600_000, 4_100_000]
BANK_WEAK = 3
BANK_SIGMA = 5e-3                                # IQ noise per component
# The weak station's amplitude A.  The component of the IQ noise in quadrature to the carrier, sigma_iq per sample at F, is
# phase noise of density sigma_iq^2 / (F A^2); the discriminator turns it into MPX noise of (f / 75 kHz)^2 times that.  At
# 57 kHz this equals white MPX noise at 384 kHz of sigma_m = (57 / 75) sqrt(384e3 / F) sigma_iq / A = 0.149 sigma_iq / A.
# sigma_m = 0.12: detection alone leaves about 30 % of the blocks bad (a float64 model of this channel alone -- brick-wall
# channel filter, phase discriminator, rds_reference.blind -- gave 28 of 92, and 1 with soft correction).
BANK_WEAK_AMPLITUDE = (57.0 / 75.0) * np.sqrt(384e3 / BANK_F) * BANK_SIGMA / 0.12
BANK_AMPLITUDE = 0.05                            # the other stations: sigma_m = 0.015, no bad block
BANK_CALLS = 26                                  # calls of 16 blocks: 2.7 s, 23 groups counted on every channel


def bank_capture(weak_amplitude=BANK_WEAK_AMPLITUDE):
    n = BANK_CALLS * BLK * 16
    t = np.arange(n, dtype=np.float64) / BANK_F
    acc = np.zeros(n, dtype=np.complex128)
    sent = []
    for i, f in enumerate(BANK_OFFS):
        g = rf.ps_groups(0x2000 + 0x111 * i, f"FECBANK{i}", n=int(n / BANK_F / (104 * rf.TD)) + 2)
        sent.append(g)
        amp = weak_amplitude if i == BANK_WEAK else BANK_AMPLITUDE
        acc += rf.fm_iq(rf.station_mpx(t, g, t0=cases.T0, stereo_id=3 * i), BANK_F, amplitude=amp, sigma=0, seed=i) * \
            cb.phasor(n, f, BANK_F, +1)
    rng = np.random.default_rng(17)
    x = (acc + BANK_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return x, sent


def bank_run(x, mode):
    n = len(x)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=BANK_F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
                   channel_offsets_hz=BANK_OFFS, enable_rds=True)
    if mode is not None:
        ch.set_rds_correction(*MODE_ARGS[mode])
    lens = [BLK] * (n // BLK)
    for i in range(0, len(lens), 8):
        ch.process_blocks(x[i * BLK:(i + 8) * BLK], lens[i:i + 8])
    out = [(ch.rds_groups(s), ch.rds_status(s)) for s in range(len(BANK_OFFS))]
    ch.close()
    return out


def test_bank_weak_channel():
    """Four stations in one 10 MS/s capture, one of them 18 dB down in the capture's noise: with soft correction that
    channel's bad or missing blocks fall; the other channels' groups are the same but for status bits."""
    x, sent = bank_capture()
    off, soft = bank_run(x, None), bank_run(x, "soft")
    for s in range(len(BANK_OFFS)):
        if s != BANK_WEAK:
            assert len(off[s][0]) >= 9 and off[s][1].blocks_bad == 0
            assert np.array_equal(off[s][0]["sample_index"], soft[s][0]["sample_index"]), s
            assert np.array_equal(off[s][0]["block"], soft[s][0]["block"]), s
    n_sent = int((len(x) / BANK_F - cases.T0) / (104 * rf.TD))
    res = [chain_counts(r[BANK_WEAK][0], sent[BANK_WEAK], cases.ACQ_GROUPS, n_sent - cases.TAIL_GROUPS) for r in (off, soft)]
    print(f"\nweak channel, groups {cases.ACQ_GROUPS} .. {n_sent - cases.TAIL_GROUPS - 1}: (bad or missing, corrected wrong, "
          f"corrected) {res[0]} with detection only, {res[1]} with soft correction")
    assert 8 <= res[0][0] <= 2 * (n_sent - cases.TAIL_GROUPS - cases.ACQ_GROUPS), res     # (bad blocks, but a working channel)
    assert res[1][0] < res[0][0], res

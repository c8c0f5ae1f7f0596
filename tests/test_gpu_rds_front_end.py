"""RDS from wideband IQ, held to the oracle's front end and the float64 receiver.

tests/test_gpu_rds_reference.py and tests/test_gpu_rds_fec.py put a known MPX in front of the stage through a 384 kHz chain
without resampler.  Here the chains are the ones RDS is really used with: the fused front end and its minimax atan2
epilogue, the R8B class (k_ifr_decim16, k_ifr_poly5h's discriminator epilogue), -f medium, bank channels (k_ifr_chan), raw
U8 with the Fs/4 shift, fractional-ratio and ppm-corrected rates, the equaliser.  The reference of every stream or channel:

    m = oracle_mpx(...)     the discriminator output of the oracle's FmDecoder behind its fp64 IfResampler, block by block
                            with the chain's own block lengths (tests/oracle_mpx.py): the MPX the stage is specified to
                            read, in the chain's own sample count, group delay included
    b = rr.blind(m)         the float64 receiver of tests/rds_reference.py on it

No bound is taken from the chain's output, and none removes a constant: sample_index is absolute.  The bounds are those of
tests/test_gpu_rds_reference.py (tests/rds_bounds.py), widened by the reference's own per-window scatter on the capture
(rds_bounds.window_scatter) and by nothing else:

    sample_index        0.5 (rounding) + 2 max |b["window_dev"]| (each group at its own window's timing) + 2 x 8e-4 (blind's
                        documented deviation over a capture), against b's capture-wide symbol grid
    timing              1 / 19 + 2 x 8e-4 sample, against b["t0"]
    carrier_phase       phase_term + 2 x the largest phase residual of window_scatter + the float32 spacing, against b's line
                        at the centre of the last complete window, modulo pi
    carrier_offset_hz   offset_term of that phase bound + the float32 spacing, against b["f_off"]
    injection           level_term + 2 x the largest level deviation of window_scatter, against b["level"]

Case j alone has an MPX whose delay changes while it runs (the equaliser adapts).  blind states one timing for the
capture; the stage follows the signal by its documented rule, one timing per window of 64 symbol periods, smoothed by
one half.  There sample_index and timing are expected at blind's timing plus rds_bounds.tracked_timing, signed: the
float64 receiver's own per-window timing on the oracle's whole MPX, put through that rule.  The bounds stay the ones
above.  DESIGN.md section 9 has the derivation and the figures; every other case keeps the delay of its MPX and is
compared with blind's timing as it is.

The 20 ppm clock-error case stays in tests/test_gpu_rds.py: blind assumes the nominal symbol clock.
"""
import functools
import importlib

import numpy as np
import pytest

import chanbank_fixture as cb
import rds_bounds as rb
import rds_fec_reference as fr
import rds_fixture as rf
import rds_reference as rr
import siggen
from conftest import load_filter
from oracle_mpx import oracle_mpx

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS = 384000.0
SPS = rr.SPS
GROUP = 104 * SPS
ACQ_GROUPS = 4                  # groups the chain may lose while it acquires (the first window + block synchronisation)
TAIL_GROUPS = 3                 # groups whose windows are still open when the capture ends
NWIN = 20                       # windows of 64 symbols in an estimates capture: 1.08 s, 12 groups
BLIND_CAPTURE = 8e-4            # blind's documented deviation of the timing over a whole capture [samples]


# ---- captures ---------------------------------------------------------------------------------------------------------
def n_input(F, n_mpx):
    return int(np.ceil(n_mpx * F / FS))


def station(n, F, pi, ps, t0=0.002, phase=-np.pi / 2, level=2.0 / 75.0, stereo_id=0, amplitude=0.3):
    """(noise-free IQ complex128 of a stereo station with its own groups, the groups)."""
    groups = rf.ps_groups(pi, ps, rt=f"FRONT END {ps}", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    return rf.fm_iq(rf.station_mpx(t, groups, level=level, phase=phase, stereo_id=stereo_id, t0=t0), F,
                    amplitude=amplitude, sigma=0), groups


def ragged_calls(total, blk, max_blocks, seed):
    """Calls (lists of block lengths) that sum to total: a first call of one sample, one of a few samples that yield no IF
    sample, one that mixes both with full blocks; then calls of full blocks only (the tiled kernel forms take no call with
    a tiny block), calls of random lengths, and now and then another tiny one."""
    rng = np.random.default_rng(seed)
    calls, n, i = [], 0, 0
    while n < total:
        if i < 3:
            ll = ([1], [3], [blk, 1, 5, blk])[i][:max_blocks]
        elif i % 7 == 5:
            ll = [int(rng.integers(1, 8))]
        elif i % 2 == 1:
            ll = [blk] * int(rng.integers(min(2, max_blocks), max_blocks + 1))
        else:
            ll = [blk if rng.random() < 0.5 else int(rng.integers(1, blk + 1)) for _ in range(int(rng.integers(1, max_blocks + 1)))]
        ll = [min(b, total - n - sum(ll[:j])) for j, b in enumerate(ll)]
        ll = [b for b in ll if b > 0]
        calls.append(ll)
        n += sum(ll)
        i += 1
    return calls


def uniform_calls(total, blk, max_blocks):
    lens = [blk] * (total // blk) + ([total % blk] if total % blk else [])
    return [lens[i:i + max_blocks] for i in range(0, len(lens), max_blocks)]


def u8_quantise(x):
    """RTL-SDR offset binary: (n, 2) uint8 I, Q."""
    def q(v):
        return np.clip(np.round(v * 127.0 + 127.5), 0, 255)
    return np.stack([q(x.real), q(x.imag)], axis=1).astype(np.uint8)


G_T0 = (0.0, 20.5 / 64 * rf.TD, 0.9995 * rf.TD)
G_PHASE = (0.0, np.pi / 2 - 1e-3, 2.4)
G_LEVEL = (1.0 / 75, 2.0 / 75, 4.0 / 75)
H_OFFS = [-4_100_000, 0, 1_234_567, 1_634_567]           # the last one 400 kHz from its neighbour, and 10 dB below it
H_AMPS = [0.095, 0.2, 0.3, 0.095]
I_OFFS = [-500_000, 0, 1_000_000]
I_AMPS = [0.3, 0.095, 0.2]
BANK_T0 = (0.002, 0.00231, 0.00163, 0.00275)
BANK_PHASE = (-np.pi / 2, 0.4, 1.9, 3.0)
BANK_LEVEL = (2.0 / 75, 4.0 / 75, 2.0 / 75, 3.0 / 75)

# name: (rate told to the chain and used by the generator, block length, blocks per call, forms that must have run)
CASES = {
    "a_10m_fast_fused": (10e6, 65536, 8, {"fused"}),
    "b_10m_r8b": (10e6, 65536, 8, {"decim16", "poly5h_disc"}),
    # (c: front_end_forms has no bit for the IF filter's kernel.  That -f medium ran shows in the reference alone: the oracle
    # runs the same 127-tap filter, whose 63 samples of delay are in its symbol grid: without the filter sample_index misses.)
    "c_10m_fast_f_medium": (10e6, 65536, 8, {"fused"}),
    "d_10m_ppm": (10000015.0, 65536, 8, {"poly_frac"}),
    "e_2m4_u8_fourth_down": (2.4e6, 16384, 8, {"decim2_16", "poly3"}),
    "f_912k": (912e3, 2048, 16, {"poly3"}),
    "g_2m5_three_streams": (2.5e6, 65536, 8, {"decim2_16", "poly"}),
    "h_bank_10m_fast": (10e6, 65536, 8, {"poly4"}),
    "i_bank_2m5_r8b": (2.5e6, 65536, 8, {"poly"}),
    "j_2m5_equaliser": (2.5e6, 4096, 16, {"decim2_16", "poly"}),
}


@functools.lru_cache(maxsize=2)
def capture(name):
    """(what the chain is fed, chain arguments, oracle_mpx arguments, the transmitted groups per stream)."""
    F, blk, per, _ = CASES[name]
    n = n_input(F, rb.windows_len(NWIN))
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per,
              enable_rds=True)
    okw = {}
    case = name[0]
    if case in "abcdf":
        x, g = station(n, F, 0xA000 + ord(case), f"CASE {case.upper()}")
        x, sent = x.astype(np.complex64), [g]
        if case == "b":
            kw["resampler_class"], okw["r8b"] = fmr.RESAMPLER_R8B, True
        if case == "c":
            coeff = load_filter("jj1bdx_fm_384kHz_medium")
            kw.update(fmfilter_enable=True, filter_coeff=coeff)
            okw["filter_coeff"] = coeff
    elif case == "e":
        x, g = station(n, F, 0xA00E, "CASE E")
        x = u8_quantise(x * (1j ** (np.arange(n) % 4)))[None]                    # the station at + F / 4
        sent = [g]
        kw.update(fourth_down=True, input_format=fmr.IQ_U8)
        okw.update(fourth_down=True, u8=True)
    elif case == "g":
        rows = [station(n, F, 0xB000 + s, f"STREAM {s}", t0=G_T0[s], phase=G_PHASE[s], level=G_LEVEL[s], stereo_id=2 * s)
                for s in range(3)]
        x, sent = np.stack([r[0] for r in rows]).astype(np.complex64), [r[1] for r in rows]
        kw["n_streams"] = 3
    elif case in "hi":
        offs, amps = (H_OFFS, H_AMPS) if case == "h" else (I_OFFS, I_AMPS)
        acc, sent = np.zeros(n, dtype=np.complex128), []
        for s, (f, a) in enumerate(zip(offs, amps)):
            xs, g = station(n, F, 0xC000 + 0x10 * ord(case) + s, f"BANK {case.upper()}{s}", t0=BANK_T0[s], phase=BANK_PHASE[s],
                            level=BANK_LEVEL[s], stereo_id=3 * s + 1, amplitude=a)
            acc += xs * cb.phasor(n, f, F, +1)
            sent.append(g)
        x = acc.astype(np.complex64)
        kw["channel_offsets_hz"] = offs
        okw["offsets_hz"] = offs
        if case == "i":
            kw["resampler_class"], okw["r8b"] = fmr.RESAMPLER_R8B, True
    elif case == "j":
        x, g = station(n, F, 0xA00A, "CASE J")
        x, sent = siggen.two_ray(x, 130), [g]              # config 4's echo: 52 us, 0.35 e^{1.1 i}, renormalised
        kw["multipath_stages"] = okw["multipath_stages"] = 64
    else:
        raise KeyError(name)
    return x, kw, okw, sent


# ---- the reference ----------------------------------------------------------------------------------------------------
EQUALISER_SETTLED = 0.1         # |get_multipath_error()| below which tests/test_gpu_configs.py calls the equaliser converged


def settle_point(trace):
    """The first MPX sample, a multiple of 128 (whole periods of 57 kHz at 384 kHz: the carrier phase keeps its
    reference), behind the last block after which the oracle's equaliser error was not yet below EQUALISER_SETTLED."""
    late = [n for n, e in trace if not abs(e) < EQUALISER_SETTLED]
    return 0 if not late else -(-max(late) // 128) * 128


def reference(m, start=0, tracked=False):
    """blind on m[start:] (start a multiple of 128), carried back to m's own sample count, plus its per-window scatter.
    tracked: the MPX changes its delay while it runs; then also rb.tracked_timing of the whole of m against blind's timing."""
    assert start % 128 == 0
    b = rr.blind(m[start:])
    lev, ph = rb.window_scatter(m[start:], b)
    tau = b["t0"] * FS + start
    slot, begin, bad, info = b["block_slot"], b["block_start"] + start, b["block_bad"], b["block_info"]
    groups = [(float(begin[i]), tuple(int(v) for v in info[i:i + 4]), bool(bad[i:i + 4].any()))
              for i in np.flatnonzero(slot == 0) if i + 4 <= len(slot)]
    track = rb.tracked_timing(m, tau) if tracked else None
    return dict(b=b, tau=tau, start=start, groups=groups, track=track, lev=float(np.abs(lev).max()), ph=float(np.abs(ph).max()),
                wdev=float(np.abs(b["window_dev"]).max()), peak=float(np.abs(m[start:]).max()), n=len(m))


def bounds(ref, st):
    b = ref["b"]
    ph = rb.phase_term("stereo", b["level"], ref["peak"], b["f_off"]) + 2 * ref["ph"] + rb.f32_spacing(st.carrier_phase)
    return {
        "index": 0.5 + 2 * ref["wdev"] + 2 * BLIND_CAPTURE,
        "timing": 1 / 19 + 2 * BLIND_CAPTURE,
        "phase": ph,
        "f_off": rb.offset_term(ph) + rb.f32_spacing(st.carrier_offset_hz),
        "level": rb.level_term() + 2 * ref["lev"],
    }


def tracked_shift(track, at):
    """The reference's tracked timing (rb.tracked_timing, signed) at the windows of 64 symbol periods that hold the MPX
    samples `at`; zeros without a track.  A sample within a symbol of a window's edge has no one window: the captures keep
    their compared groups clear of the edges, which is asserted."""
    at = np.atleast_1d(np.asarray(at, dtype=np.float64))
    if track is None:
        return np.zeros(len(at))
    pos = at / (64 * SPS)
    assert np.all(np.abs(pos - np.round(pos)) * 64 > 1.0), (at, pos)
    return track[np.floor(pos).astype(int)]


def deviations(got, st, ref, label):
    """The group checks, then the deviation of every estimate from the reference.  Where the reference carries a tracked
    timing (case j, the top of this file), sample_index and timing are expected at blind's timing plus that, signed."""
    b, tau, R, track = ref["b"], ref["tau"], ref["groups"], ref["track"]
    assert len(R) > ACQ_GROUPS + TAIL_GROUPS and not any(g[2] for g in R), (label, len(R))   # (noise-free: no bad block)
    got = got[got["sample_index"].astype(np.float64) >= R[0][0] - GROUP / 2]       # (case j: groups in front of the settle point)
    idx = got["sample_index"].astype(np.float64)
    starts = np.array([g[0] for g in R])
    num = [int(np.argmin(np.abs(starts - v))) for v in idx]
    assert len(num) >= 1 and num[0] <= ACQ_GROUPS, (label, num)
    assert num == list(range(num[0], num[0] + len(num))), (label, num)
    assert num[-1] >= len(R) - 1 - TAIL_GROUPS, (label, num, len(R))
    assert [tuple(int(v) for v in g["block"]) for g in got] == [R[j][1] for j in num], label
    assert all(int(s) == fmr.RDS_OK for g in got for s in g["status"]) and st.synced == 1, label
    grid = tau + np.round((starts[num] - tau) / SPS) * SPS
    grid = grid + tracked_shift(track, grid)
    tau_last = tau + float(tracked_shift(track, (64 * (NWIN - 1) + 32) * SPS)[0])
    assert 64 * NWIN + 8 < ref["n"] / SPS < 64 * (NWIN + 1), (label, ref["n"])     # window NWIN - 1 is the last complete one
    t_ref = (64 * (NWIN - 1) + 32 + 0.25) * rf.TD
    line = b["phase"] + 2 * np.pi * b["f_off"] * (t_ref - ref["start"] / FS)
    return {
        "index": float(np.abs(idx - grid).max()),
        "timing": abs(rb.wrap(st.timing - tau_last / SPS, 1.0)) * SPS,
        "phase": abs(rb.wrap(st.carrier_phase - line, np.pi)),
        "f_off": abs(st.carrier_offset_hz - b["f_off"]),
        "level": abs(st.injection / b["level"] - 1),
    }


# ---- the chain --------------------------------------------------------------------------------------------------------
def run_chain(x, kw, calls, mode=None):
    """The capture through process_blocks, call by call: (groups, status) per stream, the kernel forms that ran."""
    ch = fmr.Chain(**kw)
    if mode is not None:
        ch.set_rds_correction(*mode)
    axis = 0 if x.ndim == 1 else 1
    pos = 0
    for ll in calls:
        m = sum(ll)
        ch.process_blocks(x[pos:pos + m] if axis == 0 else x[:, pos:pos + m], ll)
        pos += m
    out = [(ch.rds_groups(s), ch.rds_status(s)) for s in range(ch.n_streams)]
    forms = (ch.front_end_forms(), ch.channel_bank_forms())
    ch.close()
    return out, forms


def oracle_rows(x, okw, F, lens, trace=None):
    m = oracle_mpx(x, lens, F, trace=trace, **okw)
    return m if isinstance(m, list) else [m]


@pytest.mark.parametrize("name", list(CASES))
def test_estimates(name):
    """A noise-free stereo station (or a composite of stations) over 20 windows, cut into ragged calls; the same block
    list goes to the oracle and to the chain.  Every stream or channel: its groups are the ones blind synchronised on,
    in order, status OK, after at most ACQ_GROUPS and up to TAIL_GROUPS before the end; sample_index (absolute), timing,
    carrier phase, carrier offset and injection within the bounds at the top of this file.  Case j is compared from the
    first sample behind which the oracle's equaliser error stays below 0.1, sample_index and timing against the
    reference's tracked timing (the top of this file).

    Measured on an MI355X (worst stream, deviation / bound): the table in DESIGN.md section 9; sample_index 0.41 .. 0.53
    of 0.68 .. 0.80 sample, timing below 0.02 of 0.054 sample; case j 0.46 of 1.64 and 0.0035 of 0.054."""
    F, blk, per, want = CASES[name]
    x, kw, okw, sent = capture(name)
    n = x.shape[-2] if x.dtype == np.uint8 else x.shape[-1]
    calls = ragged_calls(n, blk, per, seed=sum(map(ord, name)))
    lens = [b for ll in calls for b in ll]
    trace = [] if name[0] == "j" else None
    ms = oracle_rows(x, okw, F, lens, trace)
    start = settle_point(trace) if trace is not None else 0
    out, (fe, bank) = run_chain(x, kw, calls)
    print(f"\n[{name}] forms {sorted(fe)} bank {sorted(bank)}; compared from MPX sample {start}")
    assert want <= fe, (name, sorted(fe))
    assert bank == ({"modtap"} if "channel_offsets_hz" in kw else set()), bank
    assert len(out) == len(ms) == len(sent)
    fails = []
    for s, ((got, st), m) in enumerate(zip(out, ms)):
        ref = reference(m, start, tracked=trace is not None)
        if ref["track"] is not None:
            assert len(ref["track"]) == NWIN, len(ref["track"])
            print("  the reference's tracked timing, window by window:", np.round(ref["track"], 3))
        dev = deviations(got, st, ref, (name, s))
        assert fmr.rds_pi(got) == sent[s][0][0], (name, s)
        bound = bounds(ref, st)
        print(f"  stream {s}: {len(got)} groups;", " ".join(f"{k} {dev[k]:.3g}/{bound[k]:.3g}" for k in dev),
              f"(reference scatter: window_dev {ref['wdev']:.3g}, phase {ref['ph']:.3g}, level {ref['lev']:.3g})")
        fails += [(name, s, k, dev[k], bound[k]) for k in dev if not dev[k] <= bound[k]]
    assert not fails, fails


def test_cut_independence():
    """Case a once more in uniform blocks of 65536 samples: the group arrays equal the ragged run's."""
    name = "a_10m_fast_fused"
    F, blk, per, _ = CASES[name]
    x, kw, _, _ = capture(name)
    ragged, _ = run_chain(x, kw, ragged_calls(len(x), blk, per, seed=sum(map(ord, name))))
    uniform, (fe, _) = run_chain(x, kw, uniform_calls(len(x), blk, per))
    assert "fused" in fe
    assert len(uniform[0][0]) >= 9 and np.array_equal(uniform[0][0], ragged[0][0]), (len(uniform[0][0]), len(ragged[0][0]))


# ---- sensitivity ------------------------------------------------------------------------------------------------------
SENS_SECONDS = 4.0
SENS_SIGMA_M = 0.10             # the MPX noise at 57 kHz, as white noise at 384 kHz
SENS_T0 = 0.002
SOFT = (fmr.RDS_FEC_SOFT, 0, 4, 1.0)
SOFT_REF = dict(mode=fr.SOFT, soft_symbols=4, soft_max_cost=1.0)
UP_1DB = 10 ** (1 / 20)


def sigma_iq(sigma_m, amplitude, F):
    """The IQ noise per component that gives MPX noise of sigma_m at 57 kHz (tests/test_gpu_rds_fec.py derives it): its
    component in quadrature to the carrier is phase noise of density sigma_iq^2 / (F A^2), which the discriminator turns
    into MPX noise of (f / 75 kHz)^2 times that."""
    return sigma_m * amplitude / ((57.0 / 75.0) * np.sqrt(FS / F))


SENS_BANK_OFFS = [-3_900_000, 600_000, 4_100_000]
SENS_BANK_WEAK = 1
SENS_BANK_SIGMA = 5e-3
SENS_BANK_AMPS = [0.05, SENS_BANK_SIGMA / sigma_iq(SENS_SIGMA_M, 1.0, 10e6), 0.05]      # the weak one: sigma_m = 0.10


def sensitivity_capture(kind):
    """(clean IQ complex64, unit noise complex64, sigma_iq, chain arguments, oracle arguments, the stream to count, its
    groups).  The noise is one seeded array: sigma and sigma + 1 dB scale the same samples."""
    F = 2.5e6 if kind == "single" else 10e6
    n = int(SENS_SECONDS * F)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=65536, max_blocks=8,
              enable_rds=True)
    rng = np.random.default_rng(29)
    if kind == "single":
        clean, g = station(n, F, 0x5E01, "SENSE 1", t0=SENS_T0)
        clean = clean.astype(np.complex64)
        sig, okw, stream = sigma_iq(SENS_SIGMA_M, 0.3, F), {}, 0
    else:
        clean = np.zeros(n, dtype=np.complex64)
        for s, (f, a) in enumerate(zip(SENS_BANK_OFFS, SENS_BANK_AMPS)):
            xs, gs = station(n, F, 0x5E10 + s, f"SENSE B{s}", t0=SENS_T0, stereo_id=3 * s, amplitude=a)
            clean += (xs * cb.phasor(n, f, F, +1)).astype(np.complex64)
            if s == SENS_BANK_WEAK:
                g = gs
        kw["channel_offsets_hz"] = SENS_BANK_OFFS
        sig, okw, stream = SENS_BANK_SIGMA, dict(offsets_hz=[SENS_BANK_OFFS[SENS_BANK_WEAK]]), SENS_BANK_WEAK
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return clean, noise, sig, kw, okw, stream, g


def reference_counts(m, groups, n_sent):
    """blind's bad or missing blocks over the groups ACQ_GROUPS .. n_sent - TAIL_GROUPS - 1 of the delayed transmitter: with
    detection only, and with rds_fec_reference's soft correction."""
    sym = fr.blind_symbols(m)
    delay = float(np.median(rb.wrap(sym["block_start"] - SENS_T0 * FS, 26 * SPS)))   # the chain's group delay, from blind's grid
    assert abs(delay) < 2 * SPS, delay               # (far below the 13 symbols at which the reduction modulo a block would alias)
    t0 = SENS_T0 + delay / FS
    return tuple(fr.counts(sym, groups, t0, ACQ_GROUPS, n_sent - TAIL_GROUPS, **kw)[0] for kw in (dict(mode=fr.OFF), SOFT_REF)), t0


def chain_counts(got, lo, hi, t0):
    """The chain's bad or missing blocks over the groups lo .. hi - 1, a missing group counting four."""
    by = {int(round((int(g["sample_index"]) - t0 * FS) / GROUP)): g for g in got}
    return sum(4 if k not in by else sum((int(s) & fmr.RDS_BAD) != 0 for s in by[k]["status"]) for k in range(lo, hi))


@pytest.mark.parametrize("kind", ["single", "bank"])
def test_sensitivity(kind):
    """4 s in ragged calls, IQ noise that puts white-equivalent sigma_m = 0.10 on the MPX at 57 kHz: a single station at
    2.5 MS/s (FAST, amplitude 0.3), and the weak channel of a 10 MS/s bank beside two strong ones.  The chain's bad or
    missing blocks between ACQ_GROUPS and the last TAIL_GROUPS groups, with correction off and with soft correction, do
    not exceed those of blind (with rds_fec_reference's soft correction for the second run) on oracle_mpx of the same
    capture regenerated with the IQ noise 1 dB up, same seed.

    The condition on the captures, checked on the CPU with this seed over the 152 blocks of groups 4 .. 41: blind at sigma
    leaves at least 10 bad blocks and at most 0.7 of its count 1 dB up.  Single station: 14 at sigma, 34 at sigma + 1 dB
    (the cap); with soft correction 0 and 1 (the cap).  Bank channel: 13 and 31; with soft correction 0 and 0.
    The chain on an MI355X: 16 (cap 34) and 0 (cap 1); bank channel 13 (cap 31) and 0 (cap 0)."""
    clean, noise, sig, kw, okw, stream, groups = sensitivity_capture(kind)
    F, n = kw["input_rate"], len(clean)
    calls = ragged_calls(n, 65536, 8, seed=41)
    lens = [b for ll in calls for b in ll]
    n_sent = int((n / F - SENS_T0) / (104 * rf.TD))
    x = clean + np.float32(sig) * noise
    up = clean + np.float32(sig * UP_1DB) * noise
    (cap_off, cap_soft), t0 = reference_counts(oracle_rows(up, okw, F, lens)[0], groups, n_sent)
    del up
    res = {}
    for label, mode in (("off", None), ("soft", SOFT)):
        out, _ = run_chain(x, kw, calls, mode)
        got, st = out[stream]
        res[label] = chain_counts(got, ACQ_GROUPS, n_sent - TAIL_GROUPS, t0)
        assert st.synced == 1, (kind, label)
    print(f"\n[{kind}] groups {ACQ_GROUPS} .. {n_sent - TAIL_GROUPS - 1}: chain {res['off']} bad or missing blocks (cap {cap_off}), "
          f"with soft correction {res['soft']} (cap {cap_soft}); group delay {(t0 - SENS_T0) * FS:.1f} samples")
    assert res["off"] <= cap_off, (kind, res, cap_off)
    assert res["soft"] <= cap_soft, (kind, res, cap_soft)

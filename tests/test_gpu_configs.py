"""GPU parity tests for BASELINE.json configs[3] and configs[4] as stated, and for the PPS events.

* configs[4] (config 5): 32 independent FM stereo streams in ONE chain (the per-GPU shard of the 256-stream job),
  distinct stream ids, ragged blocks, long enough for every stream to lock; every stream against its own oracle
  instance (one decoder instance per stream, include/FmDecode.h:63-105).
* configs[3] (config 4): the S-MP signal of SURVEY.md 8d at 10 MS/s -- x[n] + 0.35 e^{j1.1} x[n-520], renormalised --
  through IfResampler -> FmDecoder with `-E 64`: 100 warm-up blocks (FmDecode.cpp:107-110) + 3 s.
* PpsEvent generation (PilotPhaseLock.cpp:133-150,163-167) over > 3 s of locked signal.
Tolerance: audio RMS error < 1e-5 (north star), written at each assert.
"""
import importlib
import json
import os

import numpy as np
import pytest

import oracle_py as ora
import siggen

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "out")


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def _report(key, **kw):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "parity_report_configs.json")
    rep = json.load(open(path)) if os.path.exists(path) else {}
    rep[key] = kw
    with open(path, "w") as f:
        json.dump(rep, f, indent=1)


def test_config5_32_streams_per_gpu(pilotcut):
    """32 streams x 0.72 s of 10 MS/s FM stereo (tones offset by 10 Hz * stream_id, noise seed 1 + stream_id,
    SURVEY.md 8d), blocks of ragged length in calls of up to 40 blocks; the pilot locks in every stream."""
    S = 32
    rng = np.random.default_rng(5)
    lens = []
    while sum(lens) < 7_200_000:
        lens.append(65536 if rng.random() < 0.7 else int(rng.integers(1, 65537)))
    n = sum(lens)
    xs = np.stack([siggen.fm_stereo_iq(n, 10e6, stream_id=s) for s in range(S)])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, n_streams=S,
                   max_block_len=65536, max_blocks=40)
    got = [[] for _ in range(S)]
    alens, fallbacks = [], []
    pos = 0
    for i in range(0, len(lens), 40):
        ll = lens[i:i + 40]
        m = sum(ll)
        a, alen = ch.process_blocks(xs[:, pos:pos + m], ll)
        for s in range(S):
            got[s].append(a[s])
        alens += list(alen)
        pos += m
        fallbacks.append(max(ch.status(s).pll_fallback for s in range(S)))
    errs = []
    for s in range(S):
        r = ora.IfResampler(10e6, 384e3)
        fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
        ref, o = [], 0
        for bl in lens:
            ref.append(fm.process(r.process(xs[s, o:o + bl])))
            o += bl
        assert alens == [len(q) for q in ref]
        ref, g = np.concatenate(ref), np.concatenate(got[s])
        assert len(g) == len(ref) > 60000
        errs.append(rms(g - ref))
        st = ch.status(s)
        assert st.stereo_detected == int(fm.stereo_detected()) == 1, s
        assert st.if_rms == pytest.approx(fm.get_if_rms(), rel=1e-5)
        assert st.if_agc_gain == pytest.approx(fm.get_if_agc_gain(), rel=1e-4)
        assert st.pilot_level == pytest.approx(fm.get_pilot_level(), rel=4e-6)      # (the acceptance rule's floor: test_gpu_parity._fm_case)
    _report("config5_32_streams", audio_rms_err_max=max(errs), audio_rms_err_mean=float(np.mean(errs)),
            samples_per_stream=n, blocks=len(lens), pll_fallback_per_call=fallbacks)
    assert max(errs) < 1e-5, errs       # north-star tolerance
    ch.close()


def test_config4_multipath_10msps(pilotcut):
    """configs[3] as stated: 10 MS/s S-MP -> IfResampler -> FmDecoder(-E 64), 100 warm-up blocks + 3 s."""
    blk, nblk, batch = 65536, 100 + 458, 62          # 458 blocks = 3.0 s at 10 MS/s
    n = nblk * blk
    # generated in pieces: phase continuity through n0 / phase0 is not needed (cumsum inside one call), so make the
    # whole stream at once in float64 and cast
    clean = siggen.fm_stereo_iq(n, 10e6)
    x = siggen.two_ray(clean, 520)
    del clean
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, multipath_stages=64,
                   max_block_len=blk, max_blocks=batch)
    r = ora.IfResampler(10e6, 384e3)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 64, pilotcut)
    got, ref = [], []
    for i in range(0, nblk, batch):
        nb = min(batch, nblk - i)
        seg = x[i * blk:(i + nb) * blk]
        a, alen = ch.process_blocks(seg[None, :], [blk] * nb)
        got.append(a[0])
        rr = [fm.process(r.process(b)) for b in siggen.blocks(seg, blk)]
        assert list(alen) == [len(q) for q in rr]
        ref += rr
    got, ref = np.concatenate(got), np.concatenate(ref)
    err = rms(got - ref)
    post = slice(2 * 48000 * 1, len(ref))       # after the first second (stereo interleaved)
    c_got, c_ref = ch.multipath_coefficients(), fm.get_multipath_coefficients()
    cerr = rms(c_got - c_ref)
    st = ch.status()
    _report("config4_multipath_10msps", audio_rms_err=err, audio_rms_err_after_1s=rms(got[post] - ref[post]),
            audio_rms=rms(ref), n_audio=len(ref), coeff_rms_err=cerr, coeff_rms=rms(c_ref),
            mpf_error=st.multipath_error, ref_mpf_error=fm.get_multipath_error(), resets=st.multipath_resets,
            locked=st.stereo_detected)
    assert st.stereo_detected == int(fm.stereo_detected()) == 1
    assert st.multipath_resets == 0
    assert err < 1e-5                          # north-star tolerance
    assert cerr < 1e-4                         # tap RMS error
    assert abs(st.multipath_error) < 0.1       # the equaliser has converged (SURVEY.md 8c known answer)
    ch.close()


@pytest.mark.parametrize("late_ms", [0, 30])
def test_equaliser_waits_for_a_late_agc_kernel(pilotcut, monkeypatch, late_ms):
    """FM + -E: the serial AGC runs BESIDE the equaliser kernel, which waits for the gains of every chunk (a progress word
    per stream, zeroed at the head of every call).  With the AGC kernel held back for 30 ms in every call (test hook) the
    equaliser really has to wait -- and the audio must not change (FmDecode.cpp:99-128: AGC, then equaliser)."""
    fs, blk, nblk, batch = 384e3, 2517, 160, 8
    x = siggen.two_ray(siggen.fm_stereo_iq(nblk * blk, fs), 20)
    monkeypatch.setenv("FMR_TEST_AGC_LATE", str(late_ms))
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs, stereo=True, multipath_stages=8, max_block_len=blk, max_blocks=batch, ab=True)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 8, pilotcut)
    got, ref = [], []
    for i in range(0, nblk, batch):
        seg = x[i * blk:(i + batch) * blk]
        a, _ = ch.process_blocks(seg[None, :], [blk] * batch)
        got.append(a[0])
        ref += [fm.process(b) for b in siggen.blocks(seg, blk)]
    got, ref = np.concatenate(got), np.concatenate(ref)
    st = ch.status()
    assert st.agc_sync_timeouts == 0
    assert len(got) == len(ref) and rms(got - ref) < 1e-6
    ch.close()


def test_equaliser_reports_an_agc_kernel_that_never_runs(pilotcut, monkeypatch):
    """The protocol error the wait is bounded against: the AGC kernel is not launched at all (test hook).  The equaliser
    gives up after its time limit, once per call, the call FAILS (its audio is void) and the status says why; a later,
    healthy call is not confused by what the failed one left behind (the progress words are per call)."""
    fs, blk, batch = 384e3, 2517, 8
    x = siggen.two_ray(siggen.fm_stereo_iq(120 * blk, fs), 20)
    monkeypatch.setenv("FMR_TEST_AGC_LATE", "0")
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs, stereo=True, multipath_stages=8, max_block_len=blk, max_blocks=batch, ab=True)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 8, pilotcut)
    # the equaliser starts after 100 warm-up blocks (FmDecode.cpp:107-110): 13 healthy calls first
    for i in range(0, 13 * batch, batch):
        seg = x[i * blk:(i + batch) * blk]
        a, _ = ch.process_blocks(seg[None, :], [blk] * batch)
        for b in siggen.blocks(seg, blk):
            fm.process(b)
    ch.close()
    monkeypatch.setenv("FMR_TEST_AGC_LATE", "-1")
    bad = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs, stereo=True, multipath_stages=8, max_block_len=blk, max_blocks=batch, ab=True)
    with pytest.raises(fmr.FmrError, match="gave up waiting for the AGC"):
        for i in range(0, 14 * batch, batch):
            bad.process_blocks(x[None, i * blk:(i + batch) * blk], [blk] * batch)
    assert bad.status().agc_sync_timeouts >= 1
    bad.close()


def test_pps_events_locked_signal(pilotcut):
    """PpsEvents over 3.6 s of locked FM stereo at 384 kHz (one event per 19000 pilot periods = 1 s, only while
    locked at block start, PilotPhaseLock.cpp:133-150): the GPU path re-derives them from per-chunk wrap masks, the
    oracle from the serial loop.  Calls of 1 block and of 12 blocks are mixed."""
    blk = 2517
    nblk = 560                                    # 3.67 s
    x = siggen.fm_stereo_iq(nblk * blk, 384e3)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=384e3, enable_resampler=False, stereo=True, max_block_len=blk, max_blocks=12)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
    ev_got, ev_ref = [], []
    i, k = 0, 0
    while i < nblk:
        nb = 1 if (k % 3 == 0) else min(12, nblk - i)
        k += 1
        seg = x[i * blk:(i + nb) * blk]
        ch.process_blocks(seg[None, :], [blk] * nb)
        for (pi, si, bp, b) in ch.pps_events():
            ev_got.append((pi, si, bp, i + b))
        for j, b in enumerate(siggen.blocks(seg, blk)):
            fm.process(b)
            for (pi, si, bp) in fm.get_pps_events():
                ev_ref.append((pi, si, bp, i + j))
        i += nb
    _report("pps_events", n_ref=len(ev_ref), n_got=len(ev_got), ref=ev_ref, got=ev_got)
    assert len(ev_ref) >= 3
    assert len(ev_got) == len(ev_ref)
    for g, r in zip(ev_got, ev_ref):
        assert g[0] == r[0] and g[1] == r[1] and g[3] == r[3], (g, r)
        assert g[2] == pytest.approx(r[2], abs=1e-12)
    ch.close()


def _run_pair(x, blk, batch, pilotcut, stereo=True):
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=stereo, max_block_len=blk, max_blocks=batch)
    r = ora.IfResampler(10e6, 384e3)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, stereo, 50.0, False, 0, pilotcut)
    got, ref, hist = [], [], []
    nblk = len(x) // blk
    for i in range(0, nblk, batch):
        nb = min(batch, nblk - i)
        seg = x[i * blk:(i + nb) * blk]
        a, alen = ch.process_blocks(seg[None, :], [blk] * nb)
        got.append(a[0])
        rr = [fm.process(r.process(b)) for b in siggen.blocks(seg, blk)]
        assert list(alen) == [len(q) for q in rr]
        ref += rr
        st = ch.status()
        hist.append({"pll_rounds": st.pll_iterations, "pll_fallback": st.pll_fallback, "agc_fallback": st.agc_fallback,
                     "locked": st.stereo_detected, "ref_locked": int(fm.stereo_detected())})
    return ch, fm, np.concatenate(got), np.concatenate(ref), hist


@pytest.mark.parametrize("narrow", [False, True])
def test_if_filter_behind_the_fused_front_end(narrow, pilotcut, fm_medium):
    """10 MS/s FM stereo with the IF filter on (main.cpp -f medium / narrow): the fused front end stores the IF samples
    (its IF-only epilogue); round 6: the filter runs on the matrix cores (k_ifr_poly4<48, 48, 127, 2, Poly4FirDiscEpi>: the lags
    1 .. 126 as a banded product, the lag-0 term behind every block's head (H1), the discriminator and the block sums in its
    epilogue; the IF level from the filter's input) -- against IfResampler + FmDecoder(fmfilter_enable) of the oracle, ragged
    blocks included."""
    from conftest import load_filter
    fir = load_filter("jj1bdx_fm_384kHz_narrow") if narrow else fm_medium
    rng = np.random.default_rng(21)
    lens = [65536] * 70 + [int(rng.integers(3000, 65537)) for _ in range(20)] + [65536] * 70
    x = siggen.fm_stereo_iq(sum(lens), 10e6, stream_id=2)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, fmfilter_enable=True,
                   filter_coeff=fir, max_block_len=65536, max_blocks=40)
    r = ora.IfResampler(10e6, 384e3)
    fm = ora.FmDecoder(True, fir, True, 50.0, False, 0, pilotcut)
    got, ref, pos = [], [], 0
    for i in range(0, len(lens), 40):
        ll = lens[i:i + 40]
        seg = x[pos:pos + sum(ll)]; pos += sum(ll)
        a, alen = ch.process_blocks(seg[None, :], ll)
        got.append(a[0])
        o = 0
        for n in ll:
            ref.append(fm.process(r.process(seg[o:o + n]))); o += n
        assert list(alen) == [len(q) for q in ref[-len(ll):]]
    got, ref = np.concatenate(got), np.concatenate(ref)
    err = rms(got - ref)
    st = ch.status()
    _report(f"if_filter_10msps_{'narrow' if narrow else 'medium'}", audio_rms_err=err, n_audio=len(ref), if_rms=st.if_rms,
            ref_if_rms=fm.get_if_rms())
    assert err < 1e-5                                   # north-star tolerance
    assert st.stereo_detected == int(fm.stereo_detected()) == 1
    assert st.if_rms == pytest.approx(fm.get_if_rms(), rel=1e-5)
    ch.close()


def test_stereo_decoder_on_a_mono_station(pilotcut):
    """stereo=True, no pilot at all (a mono station): the PLL never locks; its phase error is the atan2 of filtered
    noise and wraps at +-pi all the time (PilotPhaseLock.cpp:103), so the chunk maps are not smooth, Newton cannot
    converge and every call takes the serial PLL kernel -- measured and reported (bench.py --no-pilot), correctness
    is what is asserted here: duplicated mono output, identical to the oracle, and no lock."""
    blk, nblk, batch = 65536, 120, 30
    x = siggen.fm_stereo_iq(nblk * blk, 10e6, pilot=0.0)
    ch, fm, got, ref, hist = _run_pair(x, blk, batch, pilotcut)
    err = rms(got - ref)
    _report("stereo_on_mono_station", audio_rms_err=err, calls=hist)
    assert not fm.stereo_detected() and ch.status().stereo_detected == 0
    assert err < 1e-5                                   # north-star tolerance
    assert all(h["agc_fallback"] == 0 for h in hist[1:]), hist      # the AGC stays time-parallel after the cold call
    ch.close()


def test_pilot_drops_and_returns_mid_call(pilotcut):
    """The pilot disappears for 0.25 s in the middle of a call and comes back with a phase jump: unlock, re-acquire,
    re-lock (per-block decisions, FmDecode.cpp:162, PilotPhaseLock.cpp:154-167)."""
    fs, blk, nblk, batch = 10e6, 65536, 260, 65        # 1.7 s
    n = nblk * blk
    t = np.arange(n, dtype=np.float64) / fs
    gate = np.ones(n)
    gate[int(0.70 * fs):int(0.95 * fs)] = 0.0
    jump = np.where(t >= 0.95, 1.3, 0.0)                 # pilot phase discontinuity at its return
    fl, fr = 1000.0, 400.0
    left, right = np.sin(2 * np.pi * fl * t), np.sin(2 * np.pi * fr * t)
    th = 2 * np.pi * 19000.0 * t + jump
    mpx = 0.45 * (left + right) + gate * (0.10 * np.sin(th) + 0.45 * (left - right) * np.sin(2 * th))
    ph = 2 * np.pi * 75000.0 / fs * np.cumsum(mpx)
    rng = np.random.Generator(np.random.PCG64(1))
    x = (0.3 * np.exp(1j * ph) + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 1e-3).astype(np.complex64)
    ch, fm, got, ref, hist = _run_pair(x, blk, batch, pilotcut)
    err = rms(got - ref)
    _report("pilot_drop_and_return", audio_rms_err=err, calls=hist)
    assert [h["locked"] for h in hist] == [h["ref_locked"] for h in hist]
    assert hist[-1]["ref_locked"] == 1                   # re-locked by the end
    assert err < 1e-5
    ch.close()


def test_if_phase_discontinuity(pilotcut):
    """A 2.1 rad carrier phase step in the middle of a call (antenna switch, retune): one discriminator spike,
    the AGC / PLL recurrences must converge across it or fall back -- and match the oracle either way."""
    blk, nblk, batch = 65536, 120, 40
    x = siggen.fm_stereo_iq(nblk * blk, 10e6).copy()
    k = 70 * blk + 12345
    x[k:] *= np.exp(2.1j).astype(np.complex64)
    ch, fm, got, ref, hist = _run_pair(x, blk, batch, pilotcut)
    err = rms(got - ref)
    _report("if_phase_step", audio_rms_err=err, calls=hist)
    assert err < 1e-5
    assert ch.status().stereo_detected == int(fm.stereo_detected()) == 1
    ch.close()


def test_carrier_dropout_and_nan_samples(pilotcut):
    """The source delivers 8000 zero samples (carrier off: atan2(0, 0), AGC running up) and, later, three NaN samples
    (a corrupted buffer).  NaN spreads over the resampler's windows, the discriminator zeroes the affected differences
    (Utility.h:336-343), the AGC resets (IfSimpleAgc.cpp:49-50); nothing downstream may see a NaN.
    Through the dropout AND around the NaN samples the chain must follow the oracle: a NaN turns exactly the IF samples
    NaN whose tap support (stage A 103 taps, stage B 210 per phase) holds it -- the banded matrix products of the fused
    front end would spread it over whole tiles (NaN times their structural zeros), so a tile that holds a non-finite value
    is recomputed with the plain tap loops.  (The reference's own FFT resampler would spread a NaN over a whole FFT block;
    the oracle's time-domain resampler is this project's specification, DESIGN.md.)"""
    blk, nblk, batch = 65536, 160, 40
    x = siggen.fm_stereo_iq(nblk * blk, 10e6).copy()
    k0 = 50 * blk + 777
    x[k0:k0 + 8000] = 0
    k1 = 85 * blk + 4321
    x[k1:k1 + 3] = np.complex64(complex(np.nan, np.nan))
    ch, fm, got, ref, hist = _run_pair(x, blk, batch, pilotcut)
    assert len(got) == len(ref)
    assert not np.isnan(got).any() and not np.isnan(ref).any()
    a0 = 2 * int((k1 / 10e6 - 0.002) * 48000)          # interleaved stereo samples before the event
    a1 = 2 * int((k1 / 10e6 + 0.35) * 48000)
    assert a1 + 10000 < len(got)
    err_before, err_during, err_after = rms((got - ref)[:a0]), float(np.max(np.abs((got - ref)[a0:a1]))), rms((got - ref)[a1:])
    _report("carrier_dropout_and_nan", audio_rms_err_before=err_before, audio_max_err_during=err_during,
            audio_rms_err_after=err_after, calls=hist)
    assert err_before < 1e-5                           # cold start, lock and the carrier dropout included
    # the NaN's footprint is the reference's tap support, sample for sample (round 5: tiles of the banded matrix products that
    # hold a non-finite value are recomputed with the plain tap loops; rounds 1-4: 96 instead of 86 IF samples, a click of 0.22)
    assert err_during < 1e-3                           # (measured: 1.2e-7)
    assert err_after < 1e-5
    assert ch.status().stereo_detected == int(fm.stereo_detected()) == 1
    ch.close()


def test_nan_samples_with_the_if_filter_on(pilotcut, fm_medium):
    """Round 6: with -f the IF filter is a banded matrix-core product too (k_ifr_poly4<48, 48, 127>): zero taps times NaN would
    turn whole tiles of its output NaN.  Three NaN input samples: the front end spreads them over its tap support, the filter
    over the 126 lags behind each such IF sample -- outputs whose support holds none must come out as the reference's
    (Poly4FirDiscEpi::lag0 recomputes the tiles that hold a non-finite value with the plain tap loop), the discriminator
    zeroes the differences that touch one (Utility.h:336-343), the AGC resets.  Against the oracle with the filter on."""
    blk, nblk, batch = 65536, 160, 40
    x = siggen.fm_stereo_iq(nblk * blk, 10e6).copy()
    k1 = 85 * blk + 4321
    x[k1:k1 + 3] = np.complex64(complex(np.nan, np.nan))
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, fmfilter_enable=True,
                   filter_coeff=fm_medium, max_block_len=blk, max_blocks=batch)
    r = ora.IfResampler(10e6, 384e3)
    fm = ora.FmDecoder(True, fm_medium, True, 50.0, False, 0, pilotcut)
    got, ref = [], []
    for i in range(0, nblk, batch):
        seg = x[i * blk:(i + batch) * blk]
        a, alen = ch.process_blocks(seg[None, :], [blk] * batch)
        got.append(a[0])
        rr = [fm.process(r.process(b)) for b in siggen.blocks(seg, blk)]
        assert list(alen) == [len(q) for q in rr]
        ref += rr
    got, ref = np.concatenate(got), np.concatenate(ref)
    assert not np.isnan(got).any() and not np.isnan(ref).any()
    a0 = 2 * int((k1 / 10e6 - 0.002) * 48000)
    a1 = 2 * int((k1 / 10e6 + 0.35) * 48000)
    assert a1 + 10000 < len(got)
    err_before, err_during, err_after = rms((got - ref)[:a0]), float(np.max(np.abs((got - ref)[a0:a1]))), rms((got - ref)[a1:])
    _report("nan_with_if_filter", audio_rms_err_before=err_before, audio_max_err_during=err_during, audio_rms_err_after=err_after)
    assert err_before < 1e-5 and err_after < 1e-5
    assert err_during < 1e-3
    assert ch.status().stereo_detected == int(fm.stereo_detected()) == 1
    ch.close()


@pytest.mark.parametrize("seed,shape", [(11, "plain"), (12, "plain"), (13, "plain"), (14, "if_fir"), (15, "equaliser"),
                                        (16, "if_fir+equaliser")])
def test_fused_and_three_kernel_front_ends_agree_on_random_partitions(seed, shape, monkeypatch, fm_medium):
    """Property test without the oracle (cheap, so it can roam): the same two 10 MS/s streams, cut into random blocks
    (1 .. 65536 samples) and random calls (1 .. 40 blocks, so short calls that take the three-kernel path alternate
    with long ones on the fused kernel), through a default chain and through one built with FMR_NO_FUSED=1.  The two
    front ends round differently (fp32), nothing else may differ: audio within 1e-6 RMS, identical block lengths,
    lock decisions and PPS events.
    Shapes: "plain" -- the discriminator is the fused kernel's epilogue; with an IF FIR (main.cpp -f) and / or the
    equaliser (-E) between resampler and discriminator the kernel's epilogue stores the IF samples instead and the chain
    goes on as after the three-kernel front end.  The equaliser adapts on what it is given, so the fp32 difference of the
    two front ends comes out amplified: 1e-5 there."""
    rng = np.random.default_rng(seed)
    extra, tol = {}, 1e-6
    if "if_fir" in shape: extra.update(fmfilter_enable=True, filter_coeff=fm_medium)
    if "equaliser" in shape: extra.update(multipath_stages=16); tol = 1e-5
    lens = []
    while sum(lens) < 6_500_000:
        lens.append(int(rng.integers(1, 65537)) if rng.random() < 0.5 else 65536)
    n = sum(lens)
    xs = np.stack([siggen.fm_stereo_iq(n, 10e6, stream_id=s) for s in range(2)])
    calls, i = [], 0
    while i < len(lens):
        k = int(rng.integers(1, 41))
        calls.append(lens[i:i + k]); i += k

    def run():
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, n_streams=2,
                       max_block_len=65536, max_blocks=40, **extra)
        out, alens, locks, pps, pos = [[], []], [], [], [], 0
        for ll in calls:
            m = sum(ll)
            a, alen = ch.process_blocks(xs[:, pos:pos + m], ll)
            out[0].append(a[0]); out[1].append(a[1])
            alens += list(alen); pos += m
            locks.append((ch.status(0).stereo_detected, ch.status(1).stereo_detected))
            pps.append([(e[0], e[1], e[3]) for e in ch.pps_events(0)])
        ch.close()
        return np.concatenate(out[0]), np.concatenate(out[1]), alens, locks, pps

    a0, a1, al_a, lk_a, pp_a = run()
    monkeypatch.setenv("FMR_NO_FUSED", "1")
    b0, b1, al_b, lk_b, pp_b = run()
    assert al_a == al_b and lk_a == lk_b and pp_a == pp_b
    assert lk_a[-1] == (1, 1)
    _report(f"fused_vs_three_kernel_{shape}_{seed}", audio_rms_diff=[rms(a0 - b0), rms(a1 - b1)], tol=tol)
    assert rms(a0 - b0) < tol and rms(a1 - b1) < tol


@pytest.mark.parametrize("knobs", [
    {"FMR_PLL_V1": "1"},                                   # seven launches per Newton round instead of three
])
def test_launch_structure_switches_do_not_change_the_result(knobs, monkeypatch):
    """The three-launch PLL round (last-arrival tickets, prefix composites, atomicMax slots) and the marker-free stream
    order must decode what the plain forms decode: same stream, ragged blocks, several calls (cold start, acquisition
    with the serial fallback, lock, steady state), once by default and once with the ablation switch.  The node pass
    composes its affine maps in a different order in the two PLL forms, so the start states of the accepted
    trajectory may differ below the acceptance threshold (1e-6 rad): audio within 1e-7 RMS, everything discrete equal."""
    rng = np.random.default_rng(5)
    lens = [int(rng.integers(2000, 65537)) for _ in range(40)] + [65536] * 100
    n = sum(lens)
    x = siggen.fm_stereo_iq(n, 10e6, stream_id=3)[None, :]
    calls = [lens[0:3], lens[3:40], lens[40:41], lens[41:90], lens[90:140]]

    def run(ab=False):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, n_streams=1,
                       max_block_len=65536, max_blocks=50, ab=ab)
        out, alens, st, pos = [], [], [], 0
        for ll in calls:
            m = sum(ll)
            a, alen = ch.process_blocks(x[:, pos:pos + m], ll)
            out.append(a[0]); alens += list(alen); pos += m
            s = ch.status(0)
            st.append((s.stereo_detected, s.pll_iterations, s.pll_fallback, s.agc_fallback,
                       [(e[0], e[1], e[3]) for e in ch.pps_events(0)]))
        ch.close()
        return np.concatenate(out), alens, st

    a, al_a, st_a = run()
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    b, al_b, st_b = run(ab=True)           # (the switch is read by the A/B partner library only)
    assert st_a[-1][0] == 1 and st_a[-1][2] == 0 and st_b[-1][2] == 0        # locked, no serial fallback at the end
    assert al_a == al_b and st_a == st_b
    assert rms(a - b) < 1e-7

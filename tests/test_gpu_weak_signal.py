"""Weak-signal stage on the GPU (fmr_enable_weak_signal): the records and the handled audio of a chain against
tests/weak_signal_fixture.py run on the MPX the chain itself demodulated (tap 1, read per call and joined) and on the audio
of a twin chain that only measures.  Stage and model see the same float32 MPX and the same doubles.

The signal (weak_signal_fixture.stepped_iq): FM stereo at 384 kHz, 2.05 s, complex white noise stepped clean, noisy, clean;
tests/test_weak_signal_thresholds.py shows on the CPU oracle that every t goes 0, 1, 0 with the thresholds used here.

Tolerances (the issue's): |du| <= 1e-12 mean_n (sum_k |h_k| |x_{n-k}|)^2 -- 63 products at 2^-53 bound the error at 1.4e-14
of that; s to 1e-12 relative and t to 1e-9 absolute from the records' own u (log10 may differ by an ulp between device and
numpy); audio to 1e-12 max|audio| (a few ulps per step, amplified by at most 1 / alpha <= 15 in the one-pole)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import loudness_fixture as lf
import output_fixture as of
import siggen
import weak_signal_fixture as wf
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS, BLK = 384000.0, 65536
NB = wf.TEST_N // BLK
ONE = [[BLK] * NB]
# blocks of 1, 767, 769, 65536 and a few hundred samples: intervals (768), audio intervals (96 frames = 768 samples) and
# chunks are cut on both sides of their edges
RAGGED = [[1], [767], [769, 300], [BLK], [1, 2, 3], [20000, 777], [4096, 4096, 4096, 300], [463], [BLK] * 8, [BLK, BLK]]
RAGGED.append([wf.TEST_N - sum(map(sum, RAGGED))])
WS = dict(attack_ms=wf.TEST_MS[0], release_ms=wf.TEST_MS[1], blend_db=wf.TEST_DB["blend"], highcut_db=wf.TEST_DB["highcut"],
          mute_db=wf.TEST_DB["mute"])
_cache = {}


def cfg_of(R=1, **kw):
    return wf.config(attack_ms=wf.TEST_MS[0], release_ms=wf.TEST_MS[1], record_intervals=R, **wf.TEST_DB, **kw)


def chain384(S=1, max_blocks=NB, stereo=True, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=stereo, max_block_len=BLK,
                     max_blocks=max_blocks, n_streams=S, **kw)


def signal():
    if "x" not in _cache:
        _cache["x"] = wf.stepped_iq()
    return _cache["x"]


def feed(ch, x, calls, S=1):
    """x [rows, n] through process_blocks, one call per entry of `calls`: the MPX of every stream as the chain demodulated
    it (tap 1 of every call, joined), the audio [S, m] and the doubles per block."""
    x = np.atleast_2d(x)
    mpx, audio, alen, pos = [[] for _ in range(S)], [], [], 0
    for ll in calls:
        m = int(sum(ll))
        a, al = ch.process_blocks(x[:, pos:pos + m], ll)
        audio.append(a)
        alen += [int(v) for v in al]
        for s in range(S):
            mpx[s].append(ch.debug_read(1, stream=s, cap=1 << 20))
        pos += m
    return [np.concatenate(v) for v in mpx], np.concatenate(audio, axis=1), alen


def run(calls, act, R=1, L=2048, key=None, **kw):
    """The test signal through a 384 kHz chain with the stage: (mpx, audio, records, info)."""
    if key is not None and key in _cache:
        return _cache[key]
    ch = chain384(max_blocks=max(map(len, calls)), **kw)
    ch.enable_weak_signal(act=act, record_intervals=R, max_records=L, **WS)
    (mpx,), audio, _ = feed(ch, signal(), calls)
    recs, info = ch.weak_signal_records(0)
    ch.close()
    out = (mpx, audio[0], recs, info)
    if key is not None:
        _cache[key] = out
    return out


def check_records(recs, mpx, cfg, first=0):
    """The records (R intervals each) against the fixture on the MPX, from record `first` on; returns the fixture's."""
    R = cfg["R"]
    u, non = wf.usn(mpx)
    ref = wf.records(u, non, cfg)
    assert len(recs) == len(ref) - first, (len(recs), len(ref), first)
    ref = ref[first:]
    for k in wf.INT_FIELDS:
        assert np.array_equal(recs[k], ref[k]), (k, recs[k][:8], ref[k][:8])
    scale = wf.usn_scale(mpx)[:len(u) // R * R].reshape(-1, R)[first:]
    du = np.abs(recs["usn_sum"] - ref["usn_sum"]) / scale.sum(axis=1)
    dp = np.abs(recs["usn_peak"] - ref["usn_peak"]) / scale.max(axis=1)
    print("worst |du| / scale: sum %.3g, peak %.3g" % (du.max(), dp.max()))
    assert du.max() <= 1e-12 and dp.max() <= 1e-12
    if R == 1:      # s and t from the records' own u through the fixture
        s, t = wf.control(np.concatenate([u[:first], recs["usn_sum"]]), cfg)
        s, t = s[first:], t[first:]
        ds = np.abs(recs["smoothed"] - s) / s
        dt = max(np.abs(recs[k] - t[:, a]).max() for a, k in enumerate(("t_blend", "t_highcut", "t_mute")))
        print("worst |ds| / s %.3g, |dt| %.3g" % (ds.max(), dt))
        assert ds.max() <= 1e-12 and dt <= 1e-9
        for a, k in enumerate(("max_blend", "max_highcut", "max_mute")):
            assert np.abs(recs[k] - t[:, a]).max() <= 1e-9
        assert np.array_equal(recs["usn_peak"], recs["usn_sum"])
    return ref


def t_of(recs, cfg):
    """The control values of every interval from per-interval records' own u."""
    assert np.array_equal(recs["index"], np.arange(len(recs)))
    return wf.control(recs["usn_sum"], cfg)[1]


def check_audio(got, twin, recs, cfg, ch=2):
    ref = wf.act(twin, ch, t_of(recs, cfg), cfg)
    peak = np.abs(twin).max()
    d = np.abs(got - ref).max() / peak
    print("worst |audio - fixture| / peak: %.3g" % d)
    assert len(got) == len(ref) and d <= 1e-12
    return ref


# ---- 1: measure mode ---------------------------------------------------------------------------------------------------
def test_measure_mode_moves_nothing_and_matches_the_fixture():
    outs = []
    for ws in (False, True):
        ch = chain384(enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_rf_monitor()
        ch.enable_loudness()
        ch.enable_analyser(fft_size=1024)
        if ws:
            ch.enable_weak_signal(record_intervals=1, max_records=2048, **WS)
        ch.enable_kernel_timing(1)
        (mpx,), audio, _ = feed(ch, signal(), ONE)
        names = {k for k, _ in ch.kernel_times()}
        outs.append(dict(mpx=mpx, audio=audio, status=bytes(ch.status(0)), pps=ch.pps_events(0), rds=ch.rds_groups(0),
                         mon=ch.monitor_records(0)[:3], rfm=ch.rf_monitor_records(0)[:3], ld=ch.loudness_records(0)[:1],
                         an=ch.analyser_records(0)[:2], names=names, ws=ch.weak_signal_records(0) if ws else None))
        ch.close()
    a, b = outs
    assert np.array_equal(a["audio"], b["audio"]) and a["status"] == b["status"] and a["pps"] == b["pps"]
    assert np.array_equal(a["rds"], b["rds"]) and np.array_equal(a["mpx"], b["mpx"])
    for k in ("mon", "rfm", "ld", "an"):
        assert len(a[k][0]) >= 1
        for u, v in zip(a[k], b[k]):
            assert u.tobytes() == v.tobytes(), k
    assert not any(k.startswith("ws_") for k in a["names"])
    assert {"ws_usn", "ws_control"} <= b["names"] and not {"ws_nodes", "ws_pass2"} & b["names"]
    recs, info = b["ws"]
    assert len(b["mpx"]) == wf.TEST_N and len(recs) == wf.TEST_N // wf.Q == info["records_complete"]
    assert info["records_dropped"] == 0 and info["intervals_complete"] == len(recs) and info["channels"] == 2
    assert info["mode"] == fmr.WS_MEASURE and info["actions"] == 7 and info["record_intervals"] == 1
    check_records(recs, b["mpx"], cfg_of())
    lo, hi = wf.TEST_NOISY[0] // wf.Q, wf.TEST_NOISY[1] // wf.Q
    for k in ("t_blend", "t_highcut", "t_mute"):      # each t goes 0, 1, 0
        assert not recs[k][:lo].any() and recs[k][hi - 1] == 1.0 and not recs[k][-50:].any(), k
    _cache["twin_one"] = (b["mpx"], b["audio"][0], recs, info)
    lv = fmr.weak_signal_levels(recs)
    assert 0.1 < lv["blend_share"] < 0.5 and lv["t_blend"] == 0.0 and lv["n_intervals"] == len(recs)
    assert -8.0 < lv["usn_peak_db"] < 0.0


# ---- 2: act mode -------------------------------------------------------------------------------------------------------
def test_act_mode_matches_the_fixture_on_the_twins_audio():
    mpx, twin, _, _ = run(ONE, False, key="twin_one")
    mpx2, audio, recs, info = run(ONE, True, key="act_one")
    assert np.array_equal(mpx, mpx2) and info["mode"] == fmr.WS_ACT
    cfg = cfg_of()
    check_records(recs, mpx, cfg)
    check_audio(audio, twin, recs, cfg)
    lead = wf.A * (wf.TEST_NOISY[0] // wf.Q - 1)                 # frames that use clean intervals only
    assert not recs["max_blend"][:wf.TEST_NOISY[0] // wf.Q - 1].any()
    assert np.array_equal(audio[:2 * lead], twin[:2 * lead])     # a clean station's audio is not changed by one bit
    assert not np.array_equal(audio, twin)
    g = wf.TEST_NOISY[1] // wf.Q                                  # chunk g ramps between intervals g - 2 and g - 1: both at t = 1
    assert recs["t_blend"][g - 2] == 1.0 and recs["t_blend"][g - 1] == 1.0
    fr = audio.reshape(-1, 2)[g * wf.A:(g + 1) * wf.A]
    tw = twin.reshape(-1, 2)[g * wf.A:(g + 1) * wf.A]
    assert np.abs(fr[:, 0] - fr[:, 1]).max() <= 1e-12 * np.abs(twin).max() < np.abs(tw[:, 0] - tw[:, 1]).max()   # full blend


def test_mono_chain_and_single_actions():
    """stereo = 0 (one channel, no blend), and a stereo chain with the high cut alone at 500 Hz: 1 / alpha = 15."""
    x = signal()[:6 * BLK]
    for stereo, kw, fk in ((False, {}, {}), (True, dict(actions=fmr.WS_HIGHCUT, highcut_hz=500.0),
                                              dict(actions=wf.HIGHCUT, highcut_hz=500.0))):
        res = []
        for act in (False, True):
            ch = chain384(max_blocks=6, stereo=stereo)
            ch.enable_weak_signal(act=act, record_intervals=1, **WS, **kw)
            (mpx,), audio, _ = feed(ch, x, [[BLK] * 6])
            res.append((audio[0], ch.weak_signal_records(0)))
            ch.close()
        (twin, _), (audio, (recs, info)) = res
        assert info["channels"] == (2 if stereo else 1)
        cfg = cfg_of(**fk)
        check_audio(audio, twin, recs, cfg, ch=2 if stereo else 1)
        assert recs["max_highcut"].max() == 1.0 and not np.array_equal(audio, twin)
        if fk:
            assert not recs["max_blend"].any() and not recs["max_mute"].any()


# ---- 3: cut independence -----------------------------------------------------------------------------------------------
def test_cut_independence():
    assert sum(map(sum, RAGGED)) == wf.TEST_N
    mpx1, _, recs1, _ = run(ONE, True, key="act_one")
    mpx_t, twin, recs_t, _ = run(RAGGED, False)
    mpx2, audio, recs2, _ = run(RAGGED, True)
    mpx3, audio3, recs3, _ = run(RAGGED, True)
    assert np.array_equal(mpx1, mpx2) and np.array_equal(mpx2, mpx_t)      # (the chain's MPX does not depend on the cut)
    cfg = cfg_of()
    check_records(recs2, mpx2, cfg)
    check_audio(audio, twin, recs2, cfg)
    assert recs2.tobytes() == recs3.tobytes() == recs_t.tobytes() and audio.tobytes() == audio3.tobytes()   # the same cut: the same bits
    for k in wf.INT_FIELDS:
        assert np.array_equal(recs1[k], recs2[k]), k
    scale = wf.usn_scale(mpx1)
    assert np.all(np.abs(recs1["usn_sum"] - recs2["usn_sum"]) <= 1e-12 * scale)
    assert np.all(np.abs(recs1["smoothed"] - recs2["smoothed"]) <= 1e-12 * recs1["smoothed"])
    for k in ("t_blend", "t_highcut", "t_mute", "max_blend", "max_highcut", "max_mute"):
        assert np.abs(recs1[k] - recs2[k]).max() <= 1e-9, k


# ---- 4: small rings and records ----------------------------------------------------------------------------------------
def test_records_of_50_intervals_and_a_ring_of_8_overrun():
    mpx, _, recs, info = run(ONE, False, R=50, L=8)
    n = wf.TEST_N // wf.Q // 50
    assert n == 20 and info["records_complete"] == n and info["records_dropped"] == n - 8 and len(recs) == 8
    assert recs["index"].tolist() == list(range(n - 8, n)) and info["first_unread"] == n and info["records_ready"] == 0
    ref = check_records(recs, mpx, cfg_of(R=50), first=n - 8)
    for k in ("smoothed", "t_blend", "t_highcut", "t_mute", "max_blend", "max_highcut", "max_mute"):
        assert np.allclose(recs[k], ref[k], rtol=1e-9, atol=1e-9), k
    assert recs["max_blend"].max() == 1.0
    # cap = 0 returns the count waiting and drains nothing; a ragged cut fills the same records
    ch = chain384()
    ch.enable_weak_signal(record_intervals=50, max_records=8, **WS)
    feed(ch, signal()[:6 * BLK], [[BLK] * 6])
    info = fmr.WeakSignalInfo()
    Lb = fmr.lib()
    for _ in range(2):
        assert Lb.fmr_weak_signal_read(ch.h, 0, None, 0, C.byref(info), C.sizeof(info)) == 8
        assert info.records_ready == 8 and info.records_complete == 10 and info.records_dropped == 2 and info.first_unread == 2
    buf = np.zeros(3, dtype=fmr.WEAK_SIGNAL_RECORD)
    assert Lb.fmr_weak_signal_read(ch.h, 0, buf.ctypes.data, 3, None, 0) == 3 and buf["index"].tolist() == [2, 3, 4]
    rest, info = ch.weak_signal_records(0)
    assert rest["index"].tolist() == [5, 6, 7, 8, 9] and info["records_dropped"] == 2
    ch.close()
    mpx_r, _, recs_r, _ = run(RAGGED, False, R=50, L=32)
    check_records(recs_r, mpx_r, cfg_of(R=50))
    assert np.array_equal(recs_r["n_intervals"], np.full(20, 50))


# ---- 5: three unlike streams -------------------------------------------------------------------------------------------
def test_three_unlike_streams_equal_their_one_stream_chains():
    n = 6 * BLK
    noisy = (150 * wf.Q, 300 * wf.Q)
    x = np.stack([wf.stepped_iq(n, noisy, (1e-3, 1e-3), stream_id=0), wf.stepped_iq(n, noisy, wf.TEST_SIGMA, stream_id=1),
                  wf.stepped_iq(n, noisy, (5e-4, 5e-4), stream_id=2)])
    calls = [[BLK, 1000], [1], [BLK] * 3, [BLK - 1001], [BLK]]
    ch = chain384(S=3, max_blocks=3)
    ch.enable_weak_signal(record_intervals=1, **WS)
    mpx, audio, _ = feed(ch, x, calls, S=3)
    got = [ch.weak_signal_records(s)[0] for s in range(3)]
    ch.close()
    for s in range(3):
        one = chain384(max_blocks=3)
        one.enable_weak_signal(record_intervals=1, **WS)
        (m1,), a1, _ = feed(one, x[s], calls)
        r1, _ = one.weak_signal_records(0)
        one.close()
        assert np.array_equal(m1, mpx[s]) and np.array_equal(a1[0], audio[s]) and r1.tobytes() == got[s].tobytes(), s
        ref = check_records(got[s], mpx[s], cfg_of())
        assert ref["max_mute"].max() == (1.0 if s == 1 else 0.0), s      # (the fixture on the MPX: only stream 1 engages)


# ---- 6: bank -----------------------------------------------------------------------------------------------------------
def test_two_channel_bank(monkeypatch):
    """A two-channel bank at 2.5 MS/s in blocks of 16384: each channel's records against its own tap 1, and the handled
    audio of each channel against the fixture on a measuring twin's."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    F, blk = 2.5e6, 16384
    offs = [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 8, [7]]
    n = sum(map(sum, calls))
    # white noise of 0.1 per component: C/N in 384 kHz of 14 dB for the station of amplitude 0.3 and of 6 dB for the other
    x = (cb.composite(n, F, offs, [3, 4], [0.3, 0.12]) + siggen._noise(n, 0.1, 5)).astype(np.complex64)
    db, cfg = WS, cfg_of()
    res = []
    for act in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       channel_offsets_hz=offs)
        ch.enable_weak_signal(act=act, record_intervals=1, **db)
        mpx, audio, _ = feed(ch, x, calls, S=2)
        res.append((mpx, audio, [ch.weak_signal_records(s)[0] for s in range(2)]))
        ch.close()
    (mpx, twin, _), (mpx_a, audio, recs) = res
    for s in range(2):
        assert np.array_equal(mpx[s], mpx_a[s])
        ref = check_records(recs[s], mpx[s], cfg)
        assert len(ref) >= 20
        check_audio(audio[s], twin[s], recs[s], cfg)
        assert ref["max_blend"].max() > 0.0                        # (the fixture on the MPX: the blend engages)
    print("usn dB per channel:", [fmr.weak_signal_levels(r)["usn_mean_db"] for r in recs])


# ---- 7: pipelining -----------------------------------------------------------------------------------------------------
def test_pipelined_against_in_order():
    """10 MS/s, blocks of 65536, four asynchronous device calls and one fmr_synchronize: records and handled audio are
    those of the in_order chain, bit for bit."""
    import torch
    F, blk, per = 10e6, 65536, 4
    n = 4 * per * blk
    t = np.arange(n, dtype=np.float64) / F
    sg = np.full(n, 1e-3)
    sg[4 * blk:10 * blk] = 0.75                                   # C/N in 384 kHz about 3 dB
    rng = np.random.default_rng(2)
    x = (siggen.fm_stereo_iq(n, F, sigma=0.0) + sg * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    ws = dict(WS, attack_ms=2.0, release_ms=10.0, record_intervals=1)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_weak_signal(act=True, **ws)
    auds = [ref_ch.process_blocks(x[None, i * per * blk:(i + 1) * per * blk], [blk] * per)[0][0] for i in range(4)]
    ref, _ = ref_ch.weak_signal_records(0)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_weak_signal(act=True, **ws)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    cap = 2 * (per * blk // 200 + 4096)
    d_a = torch.zeros(4 * cap, dtype=torch.float64, device="cuda")
    for i in range(4):
        ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * blk, n, [blk] * per, d_a.data_ptr() + 8 * i * cap, cap, sync=False)
    ch.synchronize()
    got, info = ch.weak_signal_records(0)
    ch.close()
    assert len(ref) == info["records_complete"] >= 40 and ref["max_mute"].max() == 1.0
    assert got.tobytes() == ref.tobytes()
    out = d_a.cpu().numpy()
    for i in range(4):
        assert np.array_equal(out[i * cap:i * cap + len(auds[i])], auds[i]), i


def test_serial_recurrence_path(monkeypatch):
    """FMR_SERIAL=1 (the serial recurrence kernels, the output mux in k_fm_out): the stage sits behind the same mux."""
    monkeypatch.setenv("FMR_SERIAL", "1")
    x = signal()[:6 * BLK]
    res = []
    for act in (False, True):
        ch = chain384(max_blocks=3)
        ch.enable_weak_signal(act=act, record_intervals=1, **WS)
        (mpx,), audio, _ = feed(ch, x, [[BLK] * 3, [BLK, 1000], [BLK - 1000, BLK]])
        res.append((mpx, audio[0], ch.weak_signal_records(0)[0]))
        ch.close()
    (mpx, twin, recs_t), (_, audio, recs) = res
    cfg = cfg_of()
    ref = check_records(recs, mpx, cfg)
    assert recs.tobytes() == recs_t.tobytes() and ref["max_mute"].max() == 1.0
    check_audio(audio, twin, recs, cfg)
    assert not np.array_equal(audio, twin)


# ---- 8: downstream stages ----------------------------------------------------------------------------------------------
def test_output_stage_and_loudness_monitor_sit_behind_the_action():
    Qs = 4800
    ch = chain384()
    ch.enable_weak_signal(act=True, record_intervals=1, **WS)
    ch.enable_output(squelch_level=0.0)
    ch.enable_loudness(step_samples=Qs, max_records=64)
    (mpx,), audio, alen = feed(ch, signal(), ONE)
    pcm, orecs, _ = ch.output_read(0)
    ld, _ = ch.loudness_records(0)
    ch.close()
    _, twin, _, _ = run(ONE, False, key="twin_one")
    assert not np.array_equal(audio[0], twin)                      # (the chain returned handled audio)
    blocks, o = [], 0
    for k, m in enumerate(alen):
        blocks.append((orecs["if_rms"][k], audio[0][o:o + m]))
        o += m
    ref, ref_pcm = of.run(blocks, 2, 0.0, 0.5, of.PCM_S16)
    assert pcm.tobytes() == ref_pcm.tobytes() and np.array_equal(orecs["n_frames"], ref["n_frames"])
    _, twin_pcm = of.run([(orecs["if_rms"][k], twin[sum(alen[:k]):sum(alen[:k + 1])]) for k in range(len(alen))], 2, 0.0, 0.5,
                         of.PCM_S16)
    assert pcm.tobytes() != twin_pcm.tobytes()
    lref = lf.records(audio[0], 2, Qs)
    assert len(ld) == len(lref) >= 20
    for k in ("index", "first_sample", "n_nonfinite", "sample_peak"):
        assert np.array_equal(ld[k], lref[k]), k
    assert np.all(np.abs(ld["sumsq"] - lref["sumsq"]) <= 1e-12 * lref["sumsq"])
    assert np.all(np.abs(ld["kw_sumsq"] - lref["kw_sumsq"]) <= 1e-10 * (lref["kw_sumsq"] + lref["kw_sumsq"].max(axis=0)))
    ltw = lf.records(twin, 2, Qs)
    assert not np.allclose(ld["sumsq"], ltw["sumsq"], rtol=1e-6)   # (the twin's audio would read differently)


# ---- 9: refusals with a device -----------------------------------------------------------------------------------------
def test_refusals_with_a_device(nbfm_default):
    am = fmr.Chain(mode=fmr.MODE_AM, input_rate=1.48e6, enable_resampler=True, max_block_len=16384,
                   filter_coeff=fmr.filter_table("jj1bdx_am_48khz_default"))
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_weak_signal"):
        am.enable_weak_signal()
    am.close()
    nb = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                   nbfm_freq_dev=8000.0, max_block_len=2048, max_blocks=8)
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_weak_signal"):
        nb.enable_weak_signal()
    nb.close()
    fe = fmr.Channelizer(2.5e6, [-700_000, 250_000], max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_weak_signal()
    fe.close()
    qmm = chain384(pilot_shift=True)
    with pytest.raises(fmr.FmrError, match=r"error -3.*pilot_shift"):
        qmm.enable_weak_signal()
    qmm.close()
    ch = chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no weak-signal stage"):
        ch.weak_signal_records(0)
    with pytest.raises(fmr.FmrError, match=r"error -2.*highcut_hz"):      # the fields first, also with a chain
        ch.enable_weak_signal(highcut_hz=100.0)
    ch.enable_weak_signal()
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_weak_signal()
    ch.close()
    ch = chain384()
    ch.process_blocks(signal()[None, :4096], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_weak_signal()
    ch.close()


# ---- 10: facade --------------------------------------------------------------------------------------------------------
def test_facade_smoke(tmp_path):
    """tests/weak_signal_smoke.cpp through the facade: FmDecoder and a two-channel ChannelBank."""
    exe = str(tmp_path / "weak_signal_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "weak_signal_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fm records" in r.stdout and "bank0 records" in r.stdout and "bank1 records" in r.stdout, r.stdout

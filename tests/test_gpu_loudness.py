"""Audio monitor on the GPU (fmr_enable_loudness): the records of a chain against tests/loudness_fixture.py run on the
audio the chain itself returned, joined over the calls.  Stage and oracle see the same doubles: the integer fields and the
sample peak must be equal, the true peak equal to 1e-14 (the same twelve products in the same order; the taps come from
two sine routines), sumsq and sum_lr within 1e-12 of the sum of the terms' magnitudes, and kw_sumsq within
1e-10 (S_q + S_max), S_max being the oracle's largest value of that channel in the test: the device restarts the
K-weighting recurrence from chunk states, and what that leaves behind scales with the loudest sub-block nearby (measured
in float64 numpy with 64-sample chunks: 7e-14 relative on a tone with noise; across a 100 dB drop 2.9e-10 of the quiet
sub-block but 6e-14 of S_max)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import loudness_fixture as lf
import rds_fixture as rf
import siggen
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS = 384000.0
BIT_FIELDS = ("index", "first_sample", "n_nonfinite", "channels", "step_samples", "reserved", "sample_peak")


def programme_mpx(n, seed=0, fl=1000.0, fr=400.0, al=0.8, ar=0.5, pilot=0.1):
    """A stereo MPX with unlike tones in L and R plus noise (pilot = 0: a mono station, L + R only)."""
    t = np.arange(n, dtype=np.float64) / FS
    left, right = al * np.sin(2 * np.pi * fl * t), ar * np.sin(2 * np.pi * fr * t + 0.3)
    th = 2 * np.pi * 19000.0 * t
    mpx = 0.45 * (left + right) + 2e-3 * np.random.default_rng(seed).standard_normal(n)
    if pilot > 0:
        mpx = mpx + pilot * np.sin(th) + 0.45 * (left - right) * np.sin(2 * th)
    return mpx


def chain384(S=1, max_blocks=8, stereo=True, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=stereo, max_block_len=65536,
                     max_blocks=max_blocks, n_streams=S, **kw)


def feed(ch, x, calls):
    """x [rows, n] through process_blocks, one call per entry of `calls` (lists of block lengths): the audio [rows, m]."""
    x = np.atleast_2d(x)
    audio, pos = [], 0
    for ll in calls:
        m = int(sum(ll))
        a, _ = ch.process_blocks(x[:, pos:pos + m], ll)
        audio.append(a)
        pos += m
    return np.concatenate(audio, axis=1)


def check_records(recs, audio, nch, Q, first=0):
    """The records against the fixture on the audio, from record `first` on; prints the worst figures before it asserts."""
    ref = lf.records(audio, nch, Q)
    assert len(recs) == len(ref) - first, (len(recs), len(ref), first)
    smax = ref["kw_sumsq"].max(axis=0)
    ref = ref[first:]
    for k in BIT_FIELDS:
        assert np.array_equal(recs[k], ref[k]), (k, recs[k][:4], ref[k][:4])
    a = np.where(np.isfinite(audio), audio, 0.0).reshape(-1, nch)
    worst = dict(true_peak=0.0, sumsq=0.0, sum_lr=0.0, kw_sumsq=0.0)
    for i, r in enumerate(ref):
        seg = a[int(r["first_sample"]):int(r["first_sample"]) + Q]
        for c in range(nch):
            worst["true_peak"] = max(worst["true_peak"], abs(recs[i]["true_peak"][c] - r["true_peak"][c]) /
                                     max(r["true_peak"][c], 1e-300))
            worst["sumsq"] = max(worst["sumsq"], abs(recs[i]["sumsq"][c] - r["sumsq"][c]) / max(r["sumsq"][c], 1e-300))
            worst["kw_sumsq"] = max(worst["kw_sumsq"], abs(recs[i]["kw_sumsq"][c] - r["kw_sumsq"][c]) /
                                    max(r["kw_sumsq"][c] + smax[c], 1e-300))
        if nch == 2:
            worst["sum_lr"] = max(worst["sum_lr"], abs(recs[i]["sum_lr"] - r["sum_lr"]) /
                                  max(np.abs(seg[:, 0] * seg[:, 1]).sum(), 1e-300))
    print("worst deviations:", worst)
    assert worst["true_peak"] <= 1e-14 and worst["sumsq"] <= 1e-12 and worst["sum_lr"] <= 1e-12, worst
    assert worst["kw_sumsq"] <= 1e-10, worst
    if nch == 1:
        for k in ("kw_sumsq", "sumsq", "sample_peak", "true_peak"):
            assert not recs[k][:, 1].any(), k
        assert not recs["sum_lr"].any()
    return ref


# blocks of 1, 511, 513, 4096 and 65536, calls shorter than the true-peak history, and one call of more runs than the
# partial buffers hold at Q = 48 (7 x 65536 / 8 / 48 = 1195 > 1024).  The pilot locks about half a second in: the last
# call is stereo.
RAGGED = [[1], [511], [513, 4096], [65536], [1, 2, 3], [20000, 777], [4096, 4096, 4096, 300], [65536] * 7]


@pytest.mark.parametrize("Q", [480, 48])
def test_records_against_the_oracle(Q):
    """Ragged calls; at Q = 48 a sub-block is shorter than a chunk."""
    n = sum(map(sum, RAGGED))
    x = rf.mpx_iq(programme_mpx(n))
    ch = chain384()
    ch.enable_loudness(step_samples=Q, max_records=2048)
    audio = feed(ch, x, RAGGED)[0]
    assert n // 8 - 100 <= len(audio) // 2 <= n // 8           # (the audio filters' delay is not flushed)
    recs, info = ch.loudness_records(0)
    ref = check_records(recs, audio, 2, Q)
    assert len(ref) == (len(audio) // 2) // Q >= 70000 // Q and info["records_dropped"] == 0 and info["records_complete"] == len(ref)
    assert info["step_samples"] == Q and info["max_records"] == 2048 and info["channels"] == 2
    tail = fmr.loudness_levels(recs[-20:])
    print(tail)
    assert tail["correlation"] < 0.9                      # locked: L and R differ, a swap would show below
    assert np.all(recs["sumsq"][-20:, 0] > 1.5 * recs["sumsq"][-20:, 1])
    ch.close()


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def test_cut_independence():
    """One input as one call, in blocks, in 300-sample calls and in 40-sample calls (5 audio samples: fewer than the
    11 of the true-peak history).

    The oracle knows nothing of calls, so holding every cut to it on that cut's own audio is the statement that nothing
    depends on the cut: index, first_sample, n_nonfinite, channels, step_samples and sample_peak equal, true_peak equal
    (measured: 0.0 deviation in every cut), the sums within the bounds.  The cuts cannot be compared with each other
    bit for bit, because the chain's AUDIO is not the same doubles in every cut (measured here: up to 5.9e-8 apart
    between each of the three cuts and the one-call audio, and no sub-block the same doubles; the decoder's Newton solves
    run per call): where two cuts do return the same doubles their records must be the same bits, and the fields that do
    not depend on the audio are compared across all cuts."""
    n, Q = 48000, 480
    x = rf.mpx_iq(programme_mpx(n, seed=3))
    cuts = {"one": [[n]], "blocks": [[4096]] * (n // 4096) + [[n % 4096]], "short": [[300]] * (n // 300),
            "tiny": [[40]] * (n // 40), "one_again": [[n]]}
    res, auds = {}, {}
    for name, calls in cuts.items():
        ch = chain384(max_blocks=1)
        ch.enable_loudness(step_samples=Q, max_records=16)
        auds[name] = feed(ch, x, calls)[0]
        res[name] = ch.loudness_records(0)[0]
        ref = check_records(res[name], auds[name], 2, Q)
        assert np.array_equal(res[name]["true_peak"], ref["true_peak"]), name
        ch.close()
    assert len(res["one"]) == (len(auds["one"]) // 2) // Q >= 12
    assert np.array_equal(auds["one"], auds["one_again"]) and _same_bits(res["one"], res["one_again"])   # the same cut: the same bits
    b = res["one"]
    for name in ("blocks", "short", "tiny"):
        a = res[name]
        assert len(auds[name]) == len(auds["one"]), name
        print(name, "audio differs from the one-call audio by at most", np.abs(auds[name] - auds["one"]).max())
        for k in ("index", "first_sample", "n_nonfinite", "channels", "step_samples", "reserved"):
            assert np.array_equal(a[k], b[k]), (name, k)
        same = [q for q in range(len(b)) if np.array_equal(auds[name][2 * Q * max(q - 1, 0):2 * Q * (q + 1)],
                                                           auds["one"][2 * Q * max(q - 1, 0):2 * Q * (q + 1)])]
        print(name, "sub-blocks whose audio (with the sub-block in front) is the same doubles:", len(same))
        for k in ("sample_peak", "true_peak"):
            assert np.array_equal(a[k][same], b[k][same]), (name, k)


def test_ring_overrun():
    """L = 4 and eleven records complete before the first read: the newest four, seven dropped; later ones follow on."""
    Q = 480
    n = 14 * Q * 8
    x = rf.mpx_iq(programme_mpx(n, seed=7))
    ch = chain384()
    ch.enable_loudness(step_samples=Q, max_records=4)
    a1 = feed(ch, x, [[Q * 8] * 5, [Q * 8] * 6, [512]])[0]
    recs, info = ch.loudness_records(0, cap=0)
    assert len(recs) == 0 and info["records_ready"] == 4 and info["records_dropped"] == 7 and info["first_unread"] == 7
    assert info["records_complete"] == 11 and info["max_records"] == 4
    one, info = ch.loudness_records(0, cap=1)
    assert [int(v) for v in one["index"]] == [7] and info["records_ready"] == 3 and info["first_unread"] == 8
    a2 = feed(ch, x[11 * Q * 8 + 512:], [[Q * 8]])[0]
    rest, info = ch.loudness_records(0)
    assert [int(v) for v in rest["index"]] == [8, 9, 10, 11]
    assert info["records_dropped"] == 7 and info["records_ready"] == 0 and info["first_unread"] == 12
    check_records(np.concatenate([one, rest]), np.concatenate([a1, a2]), 2, Q, first=7)
    assert len(ch.loudness_records(0)[0]) == 0
    ch.close()


def test_three_streams():
    """Three rows with different programmes: each row's records against its own audio."""
    Q = 480
    calls = [[5000, 3000], [1], [20000], [4096, 777], [30000]]
    n = sum(map(sum, calls))
    x = np.stack([rf.mpx_iq(programme_mpx(n, seed=s, fl=fl, al=al)) for s, (fl, al) in
                  enumerate(((700.0, 0.2), (1000.0, 0.5), (1900.0, 0.9)))])
    ch = chain384(S=3)
    ch.enable_loudness(step_samples=Q, max_records=32)
    audio = feed(ch, x, calls)
    loud = []
    for s in range(3):
        recs, _ = ch.loudness_records(s)
        check_records(recs, audio[s], 2, Q)
        loud.append(fmr.loudness_levels(recs)["momentary_lufs"])
    print(loud)
    assert loud[0] < loud[1] < loud[2]
    ch.close()


def test_mono_chain():
    """stereo = 0: one channel, channel-1 fields 0."""
    Q = 480
    calls = [[7000], [33], [50000, 1000]]
    n = sum(map(sum, calls))
    ch = chain384(stereo=False)
    ch.enable_loudness(step_samples=Q)
    audio = feed(ch, rf.mpx_iq(programme_mpx(n, seed=4)), calls)[0]
    assert n // 8 - 100 <= len(audio) <= n // 8
    recs, info = ch.loudness_records(0)
    check_records(recs, audio, 1, Q)
    assert info["channels"] == 1 and np.all(recs["channels"] == 1) and info["max_records"] == 1024
    lv = fmr.loudness_levels(recs)
    assert lv["correlation"] == 0.0 and lv["side_to_mid_db"] == 0.0 and np.isfinite(lv["momentary_lufs"])
    ch.close()


def test_stereo_chain_on_a_station_without_pilot():
    """No pilot: the mux writes L = R, and the records say so exactly."""
    Q = 480
    n = 60000
    ch = chain384()
    ch.enable_loudness(step_samples=Q)
    audio = feed(ch, rf.mpx_iq(programme_mpx(n, seed=5, pilot=0.0)), [[25000], [35000]])[0]
    recs, _ = ch.loudness_records(0)
    check_records(recs, audio, 2, Q)
    assert np.array_equal(recs["sumsq"][:, 0], recs["sumsq"][:, 1]) and np.array_equal(recs["sumsq"][:, 0], recs["sum_lr"])
    assert np.array_equal(recs["kw_sumsq"][:, 0], recs["kw_sumsq"][:, 1])
    lv = fmr.loudness_levels(recs)
    assert lv["correlation"] == 1.0 and lv["side_to_mid_db"] == -np.inf
    ch.close()


def test_two_channel_bank():
    """A two-channel bank at 2.5 MS/s in blocks of 16384: each channel's records against its own audio."""
    F, blk, Q = 2.5e6, 16384, 480
    offs = [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 8, [7]]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 4], [0.3, 0.12])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                   channel_offsets_hz=offs)
    ch.enable_loudness(step_samples=Q, max_records=32)
    audio = feed(ch, x, calls)
    for s in range(2):
        recs, _ = ch.loudness_records(s)
        ref = check_records(recs, audio[s], 2, Q)
        assert len(ref) >= 8
    ch.close()


def test_pipelined_against_in_order():
    """10 MS/s, blocks of 65536, four asynchronous device calls and one fmr_synchronize: the records are those of the
    in_order chain, bit for bit, and agree with the oracle on the audio in the device buffer."""
    import torch
    F, blk, per, Q = 10e6, 65536, 4, 480
    n = 4 * per * blk
    x = siggen.fm_stereo_iq(n, F)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_loudness(step_samples=Q, max_records=32)
    auds = []
    for i in range(4):
        auds.append(ref_ch.process_blocks(x[None, i * per * blk:(i + 1) * per * blk], [blk] * per)[0])
    ref, _ = ref_ch.loudness_records(0)
    check_records(ref, np.concatenate(auds, axis=1)[0], 2, Q)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_loudness(step_samples=Q, max_records=32)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(2 * (n // 200 + 4096), dtype=torch.float64, device="cuda")
    for i in range(4):
        ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * blk, n, [blk] * per, d_a.data_ptr(), d_a.numel(), sync=False)
    ch.synchronize()
    got, info = ch.loudness_records(0)
    ch.close()
    assert len(ref) == info["records_complete"] >= 8
    assert _same_bits(got, ref)


def test_nothing_else_moves():
    """Audio, fmr_status, PPS events, RDS groups and modulation-monitor records of a chain with all three stages are
    bit-identical with and without the audio monitor; a chain without it runs none of its kernels."""
    F, blk = 10e6, 65536
    n = 10 * blk * 16
    groups = rf.ps_groups(0xA0D1, "LOUDNESS", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    x = rf.fm_iq(rf.station_mpx(t, groups), F).astype(np.complex64)
    outs = []
    for ld in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        if ld:
            ch.enable_loudness()
        ch.enable_kernel_timing(1)
        audio, pps, names = [], [], set()
        for pos in range(0, n, 8 * blk):
            a, _ = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        mon = ch.monitor_records(0)
        outs.append((np.concatenate(audio, axis=1), bytes(ch.status(0)), pps, ch.rds_groups(0), names, mon,
                     ch.loudness_records(0)[0] if ld else None))
        ch.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert len(outs[0][3]) >= 3 and np.array_equal(outs[0][3], outs[1][3])
    assert len(outs[0][5][0]) >= 4
    for k in range(3):
        assert np.array_equal(outs[0][5][k], outs[1][5][k]), k
    assert not any(k.startswith("ld_") for k in outs[0][4])
    assert {"ld_nodes", "ld_pass2", "ld_block", "ld_reduce"} <= outs[1][4]
    recs = outs[1][6]
    assert len(recs) == (outs[1][0].shape[1] // 2) // 4800 >= 10
    check_records(recs, outs[1][0][0], 2, 4800)


def test_refusals_with_a_device(nbfm_default):
    am = fmr.Chain(mode=fmr.MODE_AM, input_rate=1.48e6, enable_resampler=True, max_block_len=16384,
                   filter_coeff=fmr.filter_table("jj1bdx_am_48khz_default"))
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_loudness"):
        am.enable_loudness()
    am.close()
    nb = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                   nbfm_freq_dev=8000.0, max_block_len=2048, max_blocks=8)
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_loudness"):
        nb.enable_loudness()
    nb.close()
    fe = fmr.Channelizer(2.5e6, [-700_000, 250_000], max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_loudness()
    fe.close()
    ch = chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no audio monitor"):
        ch.loudness_records(0)
    ch.enable_loudness()
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_loudness()
    ch.close()
    ch = chain384()
    ch.process_blocks(rf.mpx_iq(programme_mpx(4096))[None, :], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_loudness()
    ch.close()


def test_facade_smoke(tmp_path):
    """tests/loudness_smoke.cpp through the facade: FmDecoder and a two-channel ChannelBank."""
    exe = str(tmp_path / "loudness_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "loudness_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fm records" in r.stdout and "bank0 records" in r.stdout and "bank1 records" in r.stdout, r.stdout

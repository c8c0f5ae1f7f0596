"""Audio analyser on the GPU (fmr_enable_analyser): the records of a chain against tests/analyser_fixture.py run on the
audio the chain itself returned, joined over the calls.  Stage and oracle see the same doubles: the integer fields must
be equal, sum and sumsq within 1e-12 of the sum of the terms' magnitudes, and every row of the spectra within
    1e-4 P + 2 E sqrt(P P_max) + E^2 P_max,   P_max = the largest bin of the record's L and R rows
(the bound form of tests/test_gpu_monitor.py: the fp32 transform's error is relative to the segment's largest line, not
to the bin).  E_MEASURED below is the worst (sqrt(P + d) - sqrt(P)) / sqrt(P_max), d = the deviation beyond 1e-4 P, seen
against the float64 fixture on these tests' signals on an MI355X; E is twice that, rounded up to a power of two times
2^-24, and may not exceed 32 x 2^-24.
Where the 15.2 comes from (found with an fp32 transform of the oracle decoder's audio on the CPU: the same records stand
out): it is the cross row C = Re(L conj R) alone, at bins of a one-segment record where L and R are nearly in
quadrature, so that |C| is 1e-12 of P_max although |L| and |R| are not small.  The error of C is |L| dR + |R| dL, which
the form's 2 E sqrt(|C| P_max) does not see; rows |L|^2 and |R|^2 need 1.2 x 2^-24 there.  So that a loss of accuracy
does not hide under E = 32, every record is also held to E_SHARP (set by the same rule from E_SHARP_MEASURED), rows
|L|^2 and |R|^2 by the form above and row C by the form its error obeys,
    1e-4 |C| + E (sqrt(P_L) + sqrt(P_R)) sqrt(P_max) + E^2 P_max   (the same form when L = R).

Not reachable here: no input makes the output mux write a non-finite audio sample, so the skip
branch of k_an_seg is covered by the fixture's CPU tests (tests/test_analyser_fixture.py) and by reading."""
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import analyser_fixture as af
import chanbank_fixture as cb
import oracle_py as ora
import rds_fixture as rf
import siggen
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS = 384000.0
INT_FIELDS = ("index", "first_sample", "segments", "skipped", "n_nonfinite", "channels", "fft_size", "interval_samples")
E_MEASURED = 15.161 * 2.0 ** -24      # test_records_against_the_oracle[1024-512], row C
E = 32.0 * 2.0 ** -24
E_SHARP_MEASURED = 1.110 * 2.0 ** -24      # test_records_against_the_oracle[1024-512]
E_SHARP = 4.0 * 2.0 ** -24
_worst_e = [0.0, 0.0]


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


def check_records(recs, sp, audio, nch, N, M, first=0):
    """The records against the fixture on the audio, from record `first` on; prints the worst figures before it asserts."""
    r_recs, r_sp = af.records(audio, nch, N, M)
    assert len(recs) == len(r_recs) - first, (len(recs), len(r_recs), first)
    r_recs, r_sp = r_recs[first:], r_sp[first:]
    assert sp.shape == r_sp.shape
    for k in INT_FIELDS:
        assert np.array_equal(recs[k], r_recs[k]), (k, recs[k][:4], r_recs[k][:4])
    a = np.asarray(audio, dtype=np.float64).reshape(-1, nch)
    worst_sum = worst_b = worst_e = worst_sharp = 0.0
    for i, r in enumerate(r_recs):
        seg = a[int(r["first_sample"]):int(r["first_sample"]) + M]
        for c in range(nch):
            worst_sum = max(worst_sum, abs(recs[i]["sum"][c] - r["sum"][c]) / max(np.abs(seg[:, c]).sum(), 1e-300),
                            abs(recs[i]["sumsq"][c] - r["sumsq"][c]) / max((seg[:, c] ** 2).sum(), 1e-300))
        pm = r_sp[i, :2].max()
        assert pm > 0
        P = np.abs(r_sp[i])
        dev = np.abs(sp[i] - r_sp[i])
        bound = 1e-4 * P + 2 * E * np.sqrt(P * pm) + E * E * pm
        worst_b = max(worst_b, float(np.max(dev / bound)))
        d = np.maximum(dev - 1e-4 * P, 0.0)
        worst_e = max(worst_e, float(np.max((np.sqrt(P + d) - np.sqrt(P)) / math.sqrt(pm))))
        # the sharp form: d <= 2 E a sqrt(pm) + E^2 pm with a = sqrt(P) in rows 0 and 1, (sqrt(P_L) + sqrt(P_R)) / 2 in row 2
        amp = np.sqrt(P)
        amp[2] = 0.5 * (amp[0] + amp[1])
        worst_sharp = max(worst_sharp, float(np.max((np.sqrt(amp * amp + d) - amp) / math.sqrt(pm))))
    _worst_e[0], _worst_e[1] = max(_worst_e[0], worst_e), max(_worst_e[1], worst_sharp)
    print(f"records {len(recs)}: sums {worst_sum:.3g}, spectra {worst_b:.3g} of the bound, "
          f"E needed {worst_e * 2 ** 24:.3f} x 2^-24 (so far {_worst_e[0] * 2 ** 24:.3f}), "
          f"E_SHARP needed {worst_sharp * 2 ** 24:.3f} x 2^-24 (so far {_worst_e[1] * 2 ** 24:.3f})")
    assert worst_sum <= 1e-12 and worst_b <= 1.0, (worst_sum, worst_b)
    assert worst_sharp <= E_SHARP, worst_sharp * 2 ** 24
    assert np.isfinite(sp).all()
    if nch == 1:
        assert not sp[:, 1:].any() and not recs["sum"][:, 1].any() and not recs["sumsq"][:, 1].any()
    return r_recs


# blocks of 1, 511, 513, 4096 and 65536, calls shorter than a hop, and one call of 16 blocks: at (1024, 512) its 256
# segments are 256 runs, more than the 128 the partials hold (two launches).  At the defaults, and at N = 8192 with both
# channels, a run of this chain is a sub-block of two segments and the 16-block call is one launch: the defaults' call of
# more runs than a launch holds is test_one_call_of_several_launches_at_the_defaults.  The pilot locks about half a second
# in: the last call is stereo.
RAGGED = [[1], [511], [513, 4096], [65536], [1, 2, 3], [20000, 777], [4096, 4096, 4096, 300], [65536] * 16]


@pytest.mark.parametrize("N,M", [(1024, 512), (0, 0), (8192, 4096)])
def test_records_against_the_oracle(N, M):
    n = sum(map(sum, RAGGED))
    x = rf.mpx_iq(programme_mpx(n))
    ch = chain384(max_blocks=16)
    ch.enable_analyser(fft_size=N, interval_samples=M, max_records=512)
    pos = sum(map(sum, RAGGED[:-1]))
    head = feed(ch, x[:pos], RAGGED[:-1])[0]
    ch.enable_kernel_timing(1)
    ch.kernel_times()
    audio = np.concatenate([head, feed(ch, x[pos:], RAGGED[-1:])[0]])
    launches = sum(1 for k, _ in ch.kernel_times() if k == "an_seg")      # of the 16-block call
    Nn, Mm = N or 4096, M or 6 * 4096
    recs, sp, info = ch.analyser_records(0)
    ref = check_records(recs, sp, audio, 2, Nn, Mm)
    assert len(ref) == ((len(audio) // 2 - Nn) // (Nn // 2) + 1) // (Mm // (Nn // 2)) >= 5
    if (N, M) == (1024, 512):
        assert launches == 2, launches
    assert info["records_dropped"] == 0 and info["records_complete"] == len(ref) and info["channels"] == 2
    assert info["fft_size"] == Nn and info["interval_samples"] == Mm and info["max_records"] == 512
    assert info["bins"] == Nn // 2 + 1 and info["bin_hz"] == 48000.0 / Nn
    tail = slice(-2, None)
    left, right = fmr.analyser_levels(recs[tail], sp[tail], view="L"), fmr.analyser_levels(recs[tail], sp[tail], view="R")
    print(left, right)
    assert abs(left["tone_hz"] - 1000.0) < 1.0 and abs(right["tone_hz"] - 400.0) < 1.0      # locked: a swap would show
    assert left["tone_dbfs"] > right["tone_dbfs"] + 3.0
    ch.close()


def test_one_call_of_several_launches_at_the_defaults(nbfm_default):
    """N = 4096, M = 6 N.  A chain that takes 52 blocks of 65536 samples per call cuts its records into sub-blocks of 16
    segments, more than a record's twelve: a run is a whole record, and a launch holds 128 of them.  One call of 3.4 M
    frames of an NBFM chain at 48 kS/s (ch = 1) completes 138 records: two launches, the first one clipped at 128 whole
    records and without the carry's refresh, the open-record copies flipped between them; a short call in front leaves
    an open record and a carry to begin from."""
    blk, nb = 65536, 52
    n = 4096 + nb * blk
    ch = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                   nbfm_freq_dev=8000.0, max_block_len=blk, max_blocks=nb)
    ch.enable_analyser(max_records=256)
    x = siggen.nbfm_iq(n, 48e3)
    head = feed(ch, x[:4096], [[4096]])[0]
    ch.enable_kernel_timing(1)
    ch.kernel_times()
    audio = np.concatenate([head, feed(ch, x[4096:], [[blk] * nb])[0]])
    names = [k for k, _ in ch.kernel_times()]
    assert names.count("an_seg") == 2 and names.count("an_reduce") == 2, names
    recs, sp, info = ch.analyser_records(0)
    ref = check_records(recs, sp, audio, 1, 4096, 6 * 4096)
    assert len(ref) == ((len(audio) - 4096) // 2048 + 1) // 12 > 128 and info["records_dropped"] == 0
    lv = fmr.analyser_levels(recs[-100:], sp[-100:])
    assert lv["tone_found"] == 1 and abs(lv["tone_hz"] - 1000.0) < 0.1
    ch.close()


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


def test_cut_independence():
    """One input as one call, in 4096-sample blocks, in 300-sample calls and in 40-sample calls (5 audio frames).  The
    oracle knows nothing of calls, so holding every cut to it on that cut's own audio is the statement that nothing
    depends on the cut (the chain's audio is not the same doubles in every cut: the decoder's Newton solves run per call);
    the fields that do not depend on the audio are compared across the cuts, and the same cut gives the same bits."""
    n, N, M = 48000, 1024, 1024
    x = rf.mpx_iq(programme_mpx(n, seed=3))
    cuts = {"one": [[n]], "blocks": [[4096]] * (n // 4096) + [[n % 4096]], "short": [[300]] * (n // 300),
            "tiny": [[40]] * (n // 40), "one_again": [[n]]}
    res, auds = {}, {}
    for name, calls in cuts.items():
        ch = chain384(max_blocks=1)
        ch.enable_analyser(fft_size=N, interval_samples=M, max_records=16)
        auds[name] = feed(ch, x, calls)[0]
        recs, sp, _ = ch.analyser_records(0)
        check_records(recs, sp, auds[name], 2, N, M)
        res[name] = (recs, sp)
        ch.close()
    assert len(res["one"][0]) == ((len(auds["one"]) // 2 - N) // 512 + 1) // 2 >= 4
    assert np.array_equal(auds["one"], auds["one_again"]) and _same_bits(res["one"][0], res["one_again"][0])
    assert np.array_equal(res["one"][1], res["one_again"][1])
    for name in ("blocks", "short", "tiny"):
        assert len(auds[name]) == len(auds["one"]), name
        for k in INT_FIELDS:
            assert np.array_equal(res[name][0][k], res["one"][0][k]), (name, k)


def test_ring_overrun():
    """L = 4 and eleven records complete before the first read: the newest four, seven dropped; later ones follow on."""
    N, M = 1024, 512
    n = 14 * M * 8
    x = rf.mpx_iq(programme_mpx(n, seed=7))
    ch = chain384()
    ch.enable_analyser(fft_size=N, interval_samples=M, max_records=4)
    # record i is complete with frame (i + 1) 512 + 511: 12 x 512 + 128 frames, less the ~55 the audio filters hold
    # back, complete eleven
    a1 = feed(ch, x, [[M * 8] * 5, [M * 8] * 7, [1024]])[0]
    recs, sp, info = ch.analyser_records(0, cap=0)
    assert len(recs) == 0 and info["records_ready"] == 4 and info["records_dropped"] == 7 and info["first_unread"] == 7
    assert info["records_complete"] == 11 and info["max_records"] == 4
    one, sp1, info = ch.analyser_records(0, cap=1)
    assert [int(v) for v in one["index"]] == [7] and info["records_ready"] == 3 and info["first_unread"] == 8
    a2 = feed(ch, x[12 * M * 8 + 1024:], [[M * 8]])[0]
    rest, sp2, info = ch.analyser_records(0)
    assert [int(v) for v in rest["index"]] == [8, 9, 10, 11]
    assert info["records_dropped"] == 7 and info["records_ready"] == 0 and info["first_unread"] == 12
    check_records(np.concatenate([one, rest]), np.concatenate([sp1, sp2]), np.concatenate([a1, a2]), 2, N, M, first=7)
    assert len(ch.analyser_records(0)[0]) == 0
    ch.close()


def test_three_streams():
    """Three rows with different programmes: each row's records against its own audio."""
    N, M = 2048, 2048
    calls = [[5000, 3000], [1], [20000], [4096, 777], [65536, 65536]]
    n = sum(map(sum, calls))
    x = np.stack([rf.mpx_iq(programme_mpx(n, seed=s, fl=fl, al=al)) for s, (fl, al) in
                  enumerate(((700.0, 0.2), (1000.0, 0.5), (1900.0, 0.9)))])
    ch = chain384(S=3)
    ch.enable_analyser(fft_size=N, interval_samples=M, max_records=32)
    audio = feed(ch, x, calls)
    got = []
    for s in range(3):
        recs, sp, _ = ch.analyser_records(s)
        check_records(recs, sp, audio[s], 2, N, M)
        got.append(fmr.analyser_levels(recs[-3:], sp[-3:], view="L", tone_hz=(700.0, 1000.0, 1900.0)[s]))
    print(got)
    for lv, (fl, al) in zip(got, ((700.0, 0.2), (1000.0, 0.5), (1900.0, 0.9))):
        assert abs(lv["tone_hz"] - fl) < 1.0
    assert got[0]["tone_dbfs"] < got[1]["tone_dbfs"] < got[2]["tone_dbfs"]
    ch.close()


def test_mono_chain():
    """stereo = 0: one channel, rows 1 and 2 and the channel-1 sums are 0; N = 8192."""
    N, M = 8192, 4096
    calls = [[7000], [33], [65536, 65536, 1000]]
    n = sum(map(sum, calls))
    ch = chain384(stereo=False)
    ch.enable_analyser(fft_size=N, interval_samples=M)
    audio = feed(ch, rf.mpx_iq(programme_mpx(n, seed=4)), calls)[0]
    recs, sp, info = ch.analyser_records(0)
    check_records(recs, sp, audio, 1, N, M)
    assert info["channels"] == 1 and np.all(recs["channels"] == 1) and info["max_records"] == 64 and len(recs) >= 2
    with pytest.raises(fmr.FmrError, match=r"\(-2\).*view"):
        fmr.analyser_levels(recs, sp, view="S")
    ch.close()


def test_stereo_chain_on_a_station_without_pilot():
    """No pilot: the mux writes L = R; all the power is in M and none in S."""
    N, M = 1024, 2048
    ch = chain384()
    ch.enable_analyser(fft_size=N, interval_samples=M)
    audio = feed(ch, rf.mpx_iq(programme_mpx(60000, seed=5, pilot=0.0)), [[25000], [35000]])[0]
    recs, sp, _ = ch.analyser_records(0)
    check_records(recs, sp, audio, 2, N, M)
    assert np.array_equal(recs["sumsq"][:, 0], recs["sumsq"][:, 1])
    mid, side = fmr.analyser_levels(recs, sp, view="M"), fmr.analyser_levels(recs, sp, view="S")
    left = fmr.analyser_levels(recs, sp, view="L")
    assert abs(mid["band_dbfs"] - left["band_dbfs"]) < 1e-3 and side["band_dbfs"] < mid["band_dbfs"] - 100.0
    ch.close()


@pytest.mark.parametrize("mode", ["am", "nbfm"])
def test_am_and_nbfm_chains_at_48k(mode, am_narrow, nbfm_default):
    """The AM family and NBFM write one channel where their last kernel leaves it: ch = 1."""
    N, M, blk = 1024, 1024, 4096
    calls = [[blk] * 3, [100], [blk, 511], [blk] * 4]
    n = sum(map(sum, calls))
    if mode == "am":
        ch = fmr.Chain(mode=fmr.MODE_AM, input_rate=48e3, filter_coeff=am_narrow, max_block_len=blk, max_blocks=4)
        x = siggen.am_iq(n, 48e3)
    else:
        ch = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                       nbfm_freq_dev=8000.0, max_block_len=blk, max_blocks=4)
        x = siggen.nbfm_iq(n, 48e3)
    ch.enable_analyser(fft_size=N, interval_samples=M)
    audio = feed(ch, x, calls)[0]
    recs, sp, info = ch.analyser_records(0)
    check_records(recs, sp, audio, 1, N, M)
    assert info["channels"] == 1 and len(recs) == ((len(audio) - N) // 512 + 1) // 2 >= 20
    lv = fmr.analyser_levels(recs[-8:], sp[-8:])
    print(lv)
    assert lv["tone_found"] == 1 and abs(lv["tone_hz"] - 1000.0) < 1.0
    ch.close()


def test_two_channel_bank():
    """A two-channel bank at 2.5 MS/s in blocks of 16384: each channel's records against its own audio."""
    F, blk, N, M = 2.5e6, 16384, 1024, 1024
    offs = [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 8, [7]]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 4], [0.3, 0.12])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                   channel_offsets_hz=offs)
    ch.enable_analyser(fft_size=N, interval_samples=M, max_records=32)
    audio = feed(ch, x, calls)
    for s in range(2):
        recs, sp, _ = ch.analyser_records(s)
        ref = check_records(recs, sp, audio[s], 2, N, M)
        assert len(ref) >= 3
    ch.close()


def test_pipelined_against_in_order():
    """10 MS/s, blocks of 65536, four asynchronous device calls and one fmr_synchronize: the records are those of the
    in_order chain, bit for bit, and agree with the oracle on the in_order chain's audio."""
    import torch
    F, blk, per, N, M = 10e6, 65536, 4, 1024, 1024
    n = 4 * per * blk
    x = siggen.fm_stereo_iq(n, F)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_analyser(fft_size=N, interval_samples=M, max_records=32)
    auds = []
    for i in range(4):
        auds.append(ref_ch.process_blocks(x[None, i * per * blk:(i + 1) * per * blk], [blk] * per)[0])
    ref, ref_sp, _ = ref_ch.analyser_records(0)
    check_records(ref, ref_sp, np.concatenate(auds, axis=1)[0], 2, N, M)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_analyser(fft_size=N, interval_samples=M, max_records=32)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(2 * (n // 200 + 4096), dtype=torch.float64, device="cuda")
    for i in range(4):
        ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * blk, n, [blk] * per, d_a.data_ptr(), d_a.numel(), sync=False)
    ch.synchronize()
    got, got_sp, info = ch.analyser_records(0)
    ch.close()
    assert len(ref) == info["records_complete"] >= 4
    assert _same_bits(got, ref) and np.array_equal(got_sp, ref_sp)


def test_nothing_else_moves():
    """Audio, fmr_status, PPS events, RDS groups, the three monitors' records and the output PCM of a chain with every
    other stage are bit-identical with and without the analyser; a chain without it runs none of its kernels."""
    F, blk = 10e6, 65536
    n = 10 * blk * 16
    groups = rf.ps_groups(0xA0D1, "ANALYSER", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    x = rf.fm_iq(rf.station_mpx(t, groups), F).astype(np.complex64)
    outs = []
    for an in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_loudness()
        ch.enable_rf_monitor()
        ch.enable_output()
        if an:
            ch.enable_analyser()
        ch.enable_kernel_timing(1)
        audio, pps, names = [], [], set()
        for pos in range(0, n, 8 * blk):
            a, _ = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        pcm, blocks, _ = ch.output_read(0)
        outs.append(dict(audio=np.concatenate(audio, axis=1), status=bytes(ch.status(0)), pps=pps, rds=ch.rds_groups(0),
                         names=names, mon=ch.monitor_records(0)[:3], ld=ch.loudness_records(0)[0],
                         rfm=ch.rf_monitor_records(0)[:3], pcm=pcm, blocks=blocks,
                         an=ch.analyser_records(0) if an else None))
        ch.close()
    a, b = outs
    assert np.array_equal(a["audio"], b["audio"]) and a["status"] == b["status"] and a["pps"] == b["pps"]
    assert len(a["rds"]) >= 3 and np.array_equal(a["rds"], b["rds"])
    assert len(a["mon"][0]) >= 4 and len(a["ld"]) >= 10 and len(a["rfm"][0]) >= 4 and len(a["pcm"]) > 10000
    for k in range(3):
        assert np.array_equal(a["mon"][k], b["mon"][k]) and np.array_equal(a["rfm"][k], b["rfm"][k]), k
    assert np.array_equal(a["ld"], b["ld"]) and np.array_equal(a["pcm"], b["pcm"]) and np.array_equal(a["blocks"], b["blocks"])
    assert not any(k.startswith("an_") for k in a["names"])
    assert {"an_seg", "an_reduce"} <= b["names"]
    recs, sp, _ = b["an"]
    assert len(recs) >= 1
    check_records(recs, sp, b["audio"][0], 2, 4096, 6 * 4096)


def test_refusals_with_a_device():
    live = fmr.debug_live_resources()
    fe = fmr.Channelizer(2.5e6, [-700_000, 250_000], max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_analyser()
    fe.close()
    ch = chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no analyser"):
        ch.analyser_records(0)
    with pytest.raises(fmr.FmrError, match=r"error -2.*fft_size"):
        ch.enable_analyser(fft_size=3000)
    ch.enable_analyser()                      # (the failed enable left the chain as it was)
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_analyser()
    with pytest.raises(fmr.FmrError, match=r"error -2"):
        ch.analyser_records(1)
    ch.close()
    ch = chain384()
    ch.process_blocks(rf.mpx_iq(programme_mpx(4096))[None, :], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_analyser()
    ch.close()
    assert fmr.debug_live_resources() == live


# ---- one end-to-end reading ------------------------------------------------------------------------------------------
ORACLE_THD = 0.0104846343      # the oracle decoder's own reading of the station below (record 2, view L)


def distorted_station(n):
    """FM stereo, L = an 880 Hz tone of amplitude 0.8 with 2nd and 3rd harmonics at -40 and -50 dBc, R silent."""
    t = np.arange(n, dtype=np.float64) / FS
    left = 0.8 * (np.sin(2 * np.pi * 880.0 * t) + 1e-2 * np.sin(2 * np.pi * 1760.0 * t + 0.2)
                  + 10.0 ** -2.5 * np.sin(2 * np.pi * 2640.0 * t + 0.3))
    th = 2 * np.pi * 19000.0 * t
    return 0.45 * left + 0.1 * np.sin(th) + 0.45 * left * np.sin(2 * th)


def test_end_to_end_reading(pilotcut):
    """THD of a station with known distortion, in the reference's units, three ways: fmr.analyser_levels on the GPU's
    records, the fixture's derive on fixture records of the same audio (thd and thd_n equal to a relative 1e-3, tone_hz
    to 1e-3 Hz), and the fixture on the oracle decoder's audio of the same input, computed on the CPU.

    Against the oracle the GPU reading may differ by twice the project's audio budget expressed relative to the tone.
    The budget is an RMS distance of 1e-5 between the chain's audio and the oracle's (tests/test_gpu_parity.py).  An error
    signal e of that RMS adds at most e_rms^2 to the power of the harmonic lobes if all of it falls there, and moves
    sqrt(P_h) by at most e_rms (triangle inequality in the lobes' bins), so thd = sqrt(P_h / P_t) moves by at most
    e_rms / sqrt(P_t) (P_t itself moves by a relative 1e-5 / 0.28, which is second order); twice that is allowed:
    |thd_gpu - thd_oracle| <= 2 x 1e-5 / sqrt(P_t).  ORACLE_THD records the oracle's own reading, 0.0104 plus what the
    decoder's filters do to the harmonics' ratio (de-emphasis is off: deemphasis_us = 0)."""
    n = 614400                       # 1.6 s: three records of 24576 frames; the last one lies behind the pilot lock
    x = rf.mpx_iq(distorted_station(n))
    ch = chain384(max_blocks=10, deemphasis_us=0.0)
    ch.enable_analyser()
    audio = feed(ch, x, [[65536] * 9 + [n - 9 * 65536]])[0]
    recs, sp, _ = ch.analyser_records(0)
    ch.close()
    check_records(recs, sp, audio, 2, 4096, 6 * 4096)
    assert len(recs) == 3
    r_recs, r_sp = af.records(audio, 2, 4096)
    got = fmr.analyser_levels(recs[2:], sp[2:], view="L")
    want = af.derive(r_recs[2:], r_sp[2:], view="L")
    print("gpu", got)
    print("fixture", want)
    assert got["tone_found"] == 1 and abs(got["tone_hz"] - want["tone_hz"]) <= 1e-3 and abs(got["tone_hz"] - 880.0) < 0.01
    assert abs(got["thd"] - want["thd"]) <= 1e-3 * want["thd"] and abs(got["thd_n"] - want["thd_n"]) <= 1e-3 * want["thd_n"]
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 0.0, False, 0, pilotcut)
    ref_audio = np.concatenate([fm.process(seg) for seg in siggen.blocks(x, 65536)])
    assert len(ref_audio) == len(audio)
    o_recs, o_sp = af.records(ref_audio, 2, 4096)
    oracle = af.derive(o_recs[2:], o_sp[2:], view="L")
    print("oracle", oracle)
    assert abs(oracle["thd"] - ORACLE_THD) <= 1e-6
    p_t = 10.0 ** (oracle["tone_dbfs"] / 10.0) / 2.0
    assert abs(got["thd"] - oracle["thd"]) <= 2.0 * 1e-5 / math.sqrt(p_t), (got["thd"], oracle["thd"], p_t)
    assert abs(got["tone_dbfs"] - oracle["tone_dbfs"]) < 1e-3


def test_facade_smoke(tmp_path):
    """tests/analyser_smoke.cpp through the facade: FmDecoder, AmDecoder and a two-channel ChannelBank."""
    exe = str(tmp_path / "analyser_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "analyser_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fm records" in r.stdout and "am records" in r.stdout and "bank0 records" in r.stdout and "bank1 records" in r.stdout, r.stdout

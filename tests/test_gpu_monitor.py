"""Modulation monitor on the GPU (fmr_enable_monitor): the records of a chain against tests/monitor_fixture.py run on the
MPX the chain itself demodulated (tap 1, read per call and joined).  Stage and oracle see the same float32 samples:
counts, histogram, min and max must be equal, the fp64 sums equal at their rounding, the PSD within the band spectrum
tests' fp32 model."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import monitor_fixture as mf
import rds_fixture as rf
import siggen
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS = 384000.0
INT_FIELDS = ("index", "first_sample", "n_finite", "n_nonfinite", "segments", "segments_skipped", "min", "max")
E = 10.0 * 2.0 ** -24


def loud_mpx(n, level=1.08, seed=0):
    """A 1 kHz tone, pilot and 57 kHz subcarrier: peak level + 0.117 (1.2 for the default: beyond a +-1.0 histogram)."""
    t = np.arange(n, dtype=np.float64) / FS
    rng = np.random.default_rng(seed)
    return (level * np.sin(2 * np.pi * 1000.0 * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t + 0.3) +
            (2.0 / 75.0) * np.cos(2 * np.pi * 57000.0 * t) + 1e-4 * rng.standard_normal(n))


def chain384(S=1, max_blocks=8, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=True, max_block_len=65536,
                     max_blocks=max_blocks, n_streams=S, **kw)


def feed(ch, x, calls, S=1):
    """x [rows, n] through process_blocks, one call per entry of `calls` (lists of block lengths); the MPX of every
    stream as the chain demodulated it (tap 1 of every call, joined) and the audio."""
    x = np.atleast_2d(x)
    mpx, audio, pos = [[] for _ in range(S)], [], 0
    for ll in calls:
        m = int(sum(ll))
        a, _ = ch.process_blocks(x[:, pos:pos + m], ll)
        audio.append(a)
        for s in range(S):
            mpx[s].append(ch.debug_read(1, stream=s, cap=1 << 18))
        pos += m
    return [np.concatenate(v) for v in mpx], np.concatenate(audio, axis=1)


def check_records(got, mpx, M, B, R, first=0):
    """The records `got` = (recs, hist, psd) against the fixture on the MPX, from record `first` on."""
    recs, hist, psd = got
    r_recs, r_hist, r_psd = mf.records(mpx, M=M, B=B, R=R)
    assert len(recs) == len(r_recs) - first, (len(recs), len(r_recs), first)
    r_recs, r_hist, r_psd = r_recs[first:], r_hist[first:], r_psd[first:]
    for k in INT_FIELDS:
        assert np.array_equal(recs[k], r_recs[k]), (k, recs[k][:8], r_recs[k][:8])
    assert np.array_equal(hist, r_hist)
    for i in range(len(recs)):
        seg = mpx[int(r_recs[i]["first_sample"]):int(r_recs[i]["first_sample"]) + M].astype(np.float64)
        seg = seg[np.isfinite(seg)]
        assert abs(recs[i]["sum"] - r_recs[i]["sum"]) <= 1e-12 * np.abs(seg).sum(), i
        assert abs(recs[i]["sumsq"] - r_recs[i]["sumsq"]) <= 1e-12 * (seg * seg).sum(), i
        P, pm = r_psd[i], r_psd[i].max()
        bound = 1e-4 * P + 2 * E * np.sqrt(P * pm) + E * E * pm
        worst = np.max(np.abs(psd[i] - P) / np.maximum(bound, 1e-300)) if pm > 0 else float(np.abs(psd[i]).max())
        assert worst <= 1.0, (i, worst)
    assert np.isfinite(psd).all() and all(np.isfinite(recs[k]).all() for k in ("min", "max", "sum", "sumsq"))
    return r_recs


RAGGED = [[1], [511], [513, 4096], [65536], [1, 2, 3], [20000, 777], [4096, 4096, 4096, 300], [511]]


@pytest.mark.parametrize("M", [4096, 512])
def test_records_against_the_oracle(M):
    """Ragged calls with blocks of 1, 511, 513, 4096 and 65536 samples; M = 512 is one segment per record."""
    n = sum(map(sum, RAGGED))
    x = rf.mpx_iq(loud_mpx(n))
    ch = chain384()
    ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=256)
    (mpx,), _ = feed(ch, x, RAGGED)
    assert len(mpx) == n and np.abs(mpx).max() > 1.1
    got = ch.monitor_records(0)
    ref = check_records(got[:3], mpx, M, 64, 1.0)
    assert len(ref) == (n - 512) // M and got[3]["records_dropped"] == 0 and got[3]["records_complete"] == len(ref)
    assert got[1][:, 0].sum() > 0 and got[1][:, 63].sum() > 0          # the 1.2-peak signal fills both end bins
    assert got[3]["hist_bins"] == 64 and got[3]["psd_bins"] == 513 and got[3]["interval_samples"] == M
    ch.close()


def _same_bits(a, b):
    return all(np.array_equal(a[0][k], b[0][k]) for k in a[0].dtype.names) and np.array_equal(a[1], b[1]) and \
        np.array_equal(a[2], b[2])


def test_cut_independence():
    """One input as one call, as single-block calls and as calls shorter than 512 samples."""
    n, M = 45000, 4096
    x = rf.mpx_iq(loud_mpx(n, seed=3))
    cuts = {"one": [[n]], "blocks": [[4096]] * (n // 4096) + [[n % 4096]], "short": [[300]] * (n // 300),
            "one_again": [[n]]}
    res, taps = {}, {}
    for name, calls in cuts.items():
        ch = chain384(max_blocks=1)
        ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=16)
        (mpx,), _ = feed(ch, x, calls)
        res[name], taps[name] = ch.monitor_records(0)[:3], mpx
        check_records(res[name], mpx, M, 64, 1.0)
        ch.close()
    assert len(res["one"][0]) == (n - 512) // M
    assert _same_bits(res["one"], res["one_again"])                    # the same cut: the same bits
    for name in ("blocks", "short"):
        assert np.array_equal(taps[name], taps["one"]), name             # (the chain's MPX does not depend on the cut)
        a, b = res[name], res["one"]
        for k in INT_FIELDS:
            assert np.array_equal(a[0][k], b[0][k]), (name, k)
        assert np.array_equal(a[1], b[1]), name
        for k in ("sum", "sumsq"):
            scale = np.abs(taps["one"][:4096 * len(b[0])].astype(np.float64)).reshape(len(b[0]), -1)
            scale = (scale if k == "sum" else scale * scale).sum(axis=1)
            assert np.all(np.abs(a[0][k] - b[0][k]) <= 1e-12 * scale), (name, k)
        assert np.all(np.abs(a[2] - b[2]) <= 1e-12 * np.abs(b[2])), name


def test_non_finite_input():
    """NaN and Inf IQ samples mid-run, at a record boundary and in a call's last sample.  Their places in the MPX are
    taken from tap 1: the discriminator of this chain answers a non-finite phase step with 0 (the reference's rule), so
    the tap may hold none at all; whatever it holds, the records agree with the oracle on the same samples."""
    M = 4096
    calls = [[10000], [6384, 4096], [9000], [12000, 3000]]
    n = sum(map(sum, calls))
    x = rf.mpx_iq(loud_mpx(n, level=0.5, seed=5))
    x[5000] = np.complex64(complex(np.nan, 0.0))            # mid-run
    x[3 * M] = np.complex64(complex(np.inf, 1.0))           # a record's first sample
    x[10000 + 6384 + 4096 - 1] = np.complex64(complex(np.nan, np.nan))      # the last sample of the second call
    x[30000:30003] = np.complex64(complex(0.0, -np.inf))
    ch = chain384()
    ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=16)
    (mpx,), _ = feed(ch, x, calls)
    bad = np.flatnonzero(~np.isfinite(mpx))
    print("non-finite MPX samples at", bad)
    got = ch.monitor_records(0)
    ref = check_records(got[:3], mpx, M, 64, 1.0)
    recs = got[0]
    assert len(recs) == (n - 512) // M
    assert int(recs["n_nonfinite"].sum()) == int(np.sum(bad < len(recs) * M))
    assert np.array_equal(recs["segments_skipped"], ref["segments_skipped"])
    assert np.array_equal(recs["n_finite"] + recs["n_nonfinite"], np.full(len(recs), M))
    ch.close()


def test_ring_overrun():
    """L = 4 and seven records complete before the first read: the newest four, three dropped; later records follow on."""
    M = 4096
    n = 9 * M
    x = rf.mpx_iq(loud_mpx(n, level=0.6, seed=7))
    ch = chain384()
    ch.enable_monitor(interval_samples=M, hist_bins=32, hist_range=1.0, max_records=4)
    first = [[M] * 7, [512]]
    (mpx1,), _ = feed(ch, x, first)
    recs, hist, psd, info = ch.monitor_records(0, cap=0)
    assert len(recs) == 0 and info["records_ready"] == 4 and info["records_dropped"] == 3 and info["first_unread"] == 3
    assert info["records_complete"] == 7 and info["max_records"] == 4
    one = ch.monitor_records(0, cap=1)
    assert [int(v) for v in one[0]["index"]] == [3] and one[3]["records_ready"] == 3 and one[3]["first_unread"] == 4
    (mpx2,), _ = feed(ch, x[7 * M + 512:], [[M]])
    mpx = np.concatenate([mpx1, mpx2])
    rest = ch.monitor_records(0)
    assert [int(v) for v in rest[0]["index"]] == [4, 5, 6, 7]
    assert rest[3]["records_dropped"] == 3 and rest[3]["records_ready"] == 0 and rest[3]["first_unread"] == 8
    both = (np.concatenate([one[0], rest[0]]), np.concatenate([one[1], rest[1]]), np.concatenate([one[2], rest[2]]))
    check_records(both, mpx, M, 32, 1.0, first=3)
    assert len(ch.monitor_records(0)[0]) == 0
    ch.close()


def test_three_streams():
    """Three independent 384 kHz rows at different levels: each row's records against its own tap 1."""
    M = 4096
    calls = [[5000, 3000], [1], [20000], [4096, 777]]
    n = sum(map(sum, calls))
    x = np.stack([rf.mpx_iq(loud_mpx(n, level=lv, seed=s)) for s, lv in enumerate((0.2, 0.6, 1.08))])
    ch = chain384(S=3)
    ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=16)
    mpx, _ = feed(ch, x, calls, S=3)
    peaks = []
    for s in range(3):
        got = ch.monitor_records(s)
        check_records(got[:3], mpx[s], M, 64, 1.0)
        peaks.append(fmr.monitor_levels(got[0], got[2])["peak_deviation_hz"])
    assert peaks[0] < peaks[1] < peaks[2]
    ch.close()


def test_two_channel_bank(monkeypatch):
    """A two-channel bank at 2.5 MS/s in blocks of 16384: each channel's records against its own tap 1."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    F, blk, M = 2.5e6, 16384, 4096
    offs = [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 8, [7]]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 4], [0.3, 0.12])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                   channel_offsets_hz=offs)
    ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=16)
    mpx, _ = feed(ch, x, calls, S=2)
    assert ch.channel_bank_forms() == {"modtap"}
    for s in range(2):
        got = ch.monitor_records(s)
        ref = check_records(got[:3], mpx[s], M, 64, 1.0)
        assert len(ref) >= 6
    ch.close()


def test_pipelined_against_in_order():
    """10 MS/s, blocks of 65536, four asynchronous device calls and one fmr_synchronize: the records are those of the
    in_order chain, bit for bit."""
    import torch
    F, blk, per, M = 10e6, 65536, 4, 4096
    n = 4 * per * blk
    x = siggen.fm_stereo_iq(n, F)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=16)
    for i in range(4):
        ref_ch.process_blocks(x[None, i * per * blk:(i + 1) * per * blk], [blk] * per)
    ref = ref_ch.monitor_records(0)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_monitor(interval_samples=M, hist_bins=64, hist_range=1.0, max_records=16)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(2 * (n // 200 + 4096), dtype=torch.float64, device="cuda")
    for i in range(4):
        ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * blk, n, [blk] * per, d_a.data_ptr(), d_a.numel(), sync=False)
    ch.synchronize()
    got = ch.monitor_records(0)
    ch.close()
    assert len(ref[0]) == got[3]["records_complete"] >= 8 and np.all(ref[0]["n_finite"] == M)
    assert _same_bits(got[:3], ref[:3])


def test_nothing_else_moves():
    """Audio, fmr_status, PPS events and RDS groups of an RDS chain are bit-identical with and without the monitor; a
    chain without the monitor runs none of its kernels."""
    F, blk = 10e6, 65536
    n = 10 * blk * 16
    groups = rf.ps_groups(0xA0D1, "MONITOR", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    x = rf.fm_iq(rf.station_mpx(t, groups), F).astype(np.complex64)
    outs = []
    for mon in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       enable_rds=True)
        if mon:
            ch.enable_monitor(interval_samples=38400)
        ch.enable_kernel_timing(1)
        audio, pps, names = [], [], set()
        for pos in range(0, n, 8 * blk):
            a, _ = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        outs.append((np.concatenate(audio, axis=1), bytes(ch.status(0)), pps, ch.rds_groups(0), names,
                     len(ch.monitor_records(0)[0]) if mon else 0))
        ch.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert len(outs[0][3]) >= 3 and np.array_equal(outs[0][3], outs[1][3])
    assert not any(k.startswith("mon") for k in outs[0][4])
    assert {"mon_seg", "mon_reduce"} <= outs[1][4]
    assert outs[1][5] >= 4


def test_refusals_with_a_device():
    am = fmr.Chain(mode=fmr.MODE_AM, input_rate=1.48e6, enable_resampler=True, max_block_len=16384,
                   filter_coeff=fmr.filter_table("jj1bdx_am_48khz_default"))
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_monitor"):
        am.enable_monitor()
    am.close()
    fe = fmr.Channelizer(2.5e6, [-700_000, 250_000], max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_monitor()
    fe.close()
    ch = chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no monitor"):
        ch.monitor_records(0)
    ch.enable_monitor()
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_monitor()
    ch.close()
    ch = chain384()
    ch.process_blocks(rf.mpx_iq(loud_mpx(4096))[None, :], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_monitor()
    ch.close()


def test_levels_end_to_end():
    """A station with a 0.09 pilot and RDS at 2/75, one record of 38400 samples: the chain's pilot and RDS deviation against
    the fixture's on tap 1, and the pilot against what was transmitted."""
    M = 38400
    n = M + 512
    t = np.arange(n, dtype=np.float64) / FS
    groups = rf.ps_groups(0x1234, "LEVELS", n=4)
    x = rf.mpx_iq(rf.station_mpx(t, groups))
    ch = chain384()
    ch.enable_monitor(interval_samples=M)
    (mpx,), _ = feed(ch, x, [[30000, 8912]])
    recs, hist, psd, info = ch.monitor_records(0)
    assert len(recs) == 1 and hist.shape == (1, 256) and info["hist_range"] == 2.0 and info["max_records"] == 64
    got = fmr.monitor_levels(recs, psd)
    r = mf.records(mpx, M=M)
    want = mf.derive(r[0], r[2])
    print(got, want)
    for k in ("pilot_deviation_hz", "rds_deviation_hz"):
        assert abs(got[k] - want[k]) <= 1e-4 * want[k], (k, got[k], want[k])
    assert abs(got["pilot_deviation_hz"] - 6750.0) <= 0.01 * 6750.0
    ch.close()


def test_facade_smoke(tmp_path):
    """tests/monitor_smoke.cpp through the facade: FmDecoder and a two-channel ChannelBank."""
    exe = str(tmp_path / "monitor_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "monitor_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fm records 4" in r.stdout and "bank0 records" in r.stdout and "bank1 records" in r.stdout, r.stdout

"""RF monitor on the GPU (fmr_enable_rf_monitor): the records of a chain against tests/rfmon_fixture.py run on the IF
samples the chain itself saw -- the input of a 384 kHz chain without resampler, tap 0 (read per call and joined)
behind one.  Stage and oracle see the same float32 p: counts, histogram, p_min and p_max must be equal, the fp64 sums
equal at their rounding, the PSD within the band spectrum tests' fp32 model (tests/test_gpu_monitor.py::check_records,
E = 10 x 2^-24)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import rds_fixture as rf
import rfmon_fixture as rx
import siggen
import test_gpu_monitor as tgm
from conftest import ROOT, load_filter

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS = 384000.0
INT_FIELDS = ("index", "first_sample", "n_finite", "n_nonfinite", "segments", "segments_skipped", "p_min", "p_max")
E = 10.0 * 2.0 ** -24


def signal(n, amplitude=0.3, seed=0, am=0.1, noise=1e-4):
    """FM at `amplitude` with 10 % AM at 3 kHz on the envelope and noise (30 dB under a 0.3 carrier)."""
    return rx.fm_iq(n, amplitude=amplitude, am=am, noise=noise, seed=seed)


def chain384(S=1, max_blocks=8, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=True, max_block_len=65536,
                     max_blocks=max_blocks, n_streams=S, **kw)


def feed(ch, x, calls, S=1, taps=False):
    """x [rows, n] through process_blocks, one call per entry of `calls` (lists of block lengths).  taps: the IF samples
    of every stream as the chain saw them (tap 0 of every call, joined); the audio."""
    x = np.atleast_2d(x)
    ifs, audio, pos = [[] for _ in range(S)], [], 0
    for ll in calls:
        m = int(sum(ll))
        a, _ = ch.process_blocks(x[:, pos:pos + m], ll)
        audio.append(a)
        if taps:
            for s in range(S):
                ifs[s].append(ch.debug_read(0, stream=s, cap=1 << 18))
        pos += m
    return [np.concatenate(v) for v in ifs] if taps else None, np.concatenate(audio, axis=1)


def psd_bound(P):
    pm = P.max()
    return 1e-4 * P + 2 * E * np.sqrt(P * pm) + E * E * pm


def check_records(got, p, M, first=0):
    """The records `got` = (recs, hist, psd) against the fixture on the float32 p, from record `first` on."""
    recs, hist, psd = got
    r_recs, r_hist, r_psd = rx.records(p, M=M)
    assert len(recs) == len(r_recs) - first, (len(recs), len(r_recs), first)
    r_recs, r_hist, r_psd = r_recs[first:], r_hist[first:], r_psd[first:]
    for k in INT_FIELDS:
        assert np.array_equal(recs[k], r_recs[k]), (k, recs[k][:8], r_recs[k][:8])
    assert np.array_equal(hist, r_hist)
    worst_all = 0.0
    for i in range(len(recs)):
        assert abs(recs[i]["m2"] - r_recs[i]["m2"]) <= 1e-12 * r_recs[i]["m2"], i
        assert abs(recs[i]["m4"] - r_recs[i]["m4"]) <= 1e-12 * r_recs[i]["m4"], i
        P = r_psd[i]
        worst = np.max(np.abs(psd[i] - P) / np.maximum(psd_bound(P), 1e-300)) if P.max() > 0 else float(np.abs(psd[i]).max())
        worst_all = max(worst_all, worst)
        assert worst <= 1.0, (i, worst)
    print("records", len(recs), "worst psd ratio", worst_all)
    assert np.isfinite(psd).all() and all(np.isfinite(recs[k]).all() for k in ("p_min", "p_max", "m2", "m4"))
    return r_recs


RAGGED = [[1], [511], [513, 4096], [65536], [1, 2, 3], [20000, 777], [4096, 4096, 4096, 300], [511]]


@pytest.mark.parametrize("M", [4096, 512])
def test_records_against_the_oracle(M):
    """Ragged calls with blocks of 1, 511, 513, 4096 and 65536 samples; M = 512 is one segment per record."""
    n = sum(map(sum, RAGGED))
    x = signal(n)
    ch = chain384()
    ch.enable_rf_monitor(interval_samples=M, max_records=256)
    feed(ch, x, RAGGED)
    got = ch.rf_monitor_records(0)
    ref = check_records(got[:3], rx.power(x), M)
    assert len(ref) == (n - 512) // M and got[3]["records_dropped"] == 0 and got[3]["records_complete"] == len(ref)
    assert got[3]["hist_bins"] == 384 and got[3]["psd_bins"] == 513 and got[3]["interval_samples"] == M
    assert got[3]["bin_hz"] == 375.0 and got[3]["max_records"] == 256
    lv = fmr.rf_levels(*got[:3])
    print(lv)
    assert abs(lv["am_audio_db"] + 23.05) < 0.1 and abs(lv["level_dbfs"] - 10 * np.log10(0.09 * 1.005 + 1e-4)) < 0.05
    ch.close()


def _same_bits(a, b):
    return all(np.array_equal(a[0][k], b[0][k]) for k in a[0].dtype.names) and np.array_equal(a[1], b[1]) and \
        np.array_equal(a[2], b[2])


def test_cut_independence():
    """One input as one call, as single-block calls and as calls shorter than 512 samples."""
    n, M = 45000, 4096
    x = signal(n, seed=3)
    p = rx.power(x)
    cuts = {"one": [[n]], "blocks": [[4096]] * (n // 4096) + [[n % 4096]], "short": [[300]] * (n // 300),
            "one_again": [[n]]}
    res = {}
    for name, calls in cuts.items():
        ch = chain384(max_blocks=1)
        ch.enable_rf_monitor(interval_samples=M, max_records=16)
        feed(ch, x, calls)
        res[name] = ch.rf_monitor_records(0)[:3]
        check_records(res[name], p, M)
        ch.close()
    assert len(res["one"][0]) == (n - 512) // M
    assert _same_bits(res["one"], res["one_again"])                    # the same cut: the same bits
    for name in ("blocks", "short"):
        a, b = res[name], res["one"]
        for k in INT_FIELDS:
            assert np.array_equal(a[0][k], b[0][k]), (name, k)
        assert np.array_equal(a[1], b[1]), name
        for k in ("m2", "m4"):
            assert np.all(np.abs(a[0][k] - b[0][k]) <= 1e-12 * b[0][k]), (name, k)
        assert np.all(np.abs(a[2] - b[2]) <= 1e-12 * np.abs(b[2])), name


def test_non_finite_input():
    """NaN and Inf IQ samples mid-run, at a record boundary and in a call's last sample: a 384 kHz chain hands them to the
    decoder as they are, so p is non-finite there: counted, kept out of everything else, their segments skipped."""
    M = 4096
    calls = [[10000], [6384, 4096], [9000], [12000, 3000]]
    n = sum(map(sum, calls))
    x = signal(n, seed=5)
    x[5000] = np.complex64(complex(np.nan, 0.0))            # mid-run
    x[3 * M] = np.complex64(complex(np.inf, 1.0))           # a record's first sample
    x[10000 + 6384 + 4096 - 1] = np.complex64(complex(np.nan, np.nan))      # the last sample of the second call
    x[30000:30003] = np.complex64(complex(0.0, -np.inf))
    ch = chain384()
    ch.enable_rf_monitor(interval_samples=M, max_records=16)
    feed(ch, x, calls)
    got = ch.rf_monitor_records(0)
    p = rx.power(x)
    ref = check_records(got[:3], p, M)
    recs = got[0]
    assert len(recs) == (n - 512) // M
    assert int(recs["n_nonfinite"].sum()) == int(np.sum(~np.isfinite(p[:len(recs) * M]))) == 6
    assert int(recs["segments_skipped"].sum()) == 8 and np.array_equal(recs["segments_skipped"], ref["segments_skipped"])
    assert np.array_equal(recs["n_finite"] + recs["n_nonfinite"], np.full(len(recs), M))
    ch.close()


def test_ring_overrun():
    """L = 4 and seven records complete before the first read: the newest four, three dropped; later records follow on."""
    M = 4096
    n = 9 * M
    x = signal(n, seed=7)
    ch = chain384()
    ch.enable_rf_monitor(interval_samples=M, max_records=4)
    feed(ch, x, [[M] * 7, [512]])
    recs, hist, psd, info = ch.rf_monitor_records(0, cap=0)
    assert len(recs) == 0 and info["records_ready"] == 4 and info["records_dropped"] == 3 and info["first_unread"] == 3
    assert info["records_complete"] == 7 and info["max_records"] == 4
    one = ch.rf_monitor_records(0, cap=1)
    assert [int(v) for v in one[0]["index"]] == [3] and one[3]["records_ready"] == 3 and one[3]["first_unread"] == 4
    feed(ch, x[7 * M + 512:], [[M]])
    rest = ch.rf_monitor_records(0)
    assert [int(v) for v in rest[0]["index"]] == [4, 5, 6, 7]
    assert rest[3]["records_dropped"] == 3 and rest[3]["records_ready"] == 0 and rest[3]["first_unread"] == 8
    both = (np.concatenate([one[0], rest[0]]), np.concatenate([one[1], rest[1]]), np.concatenate([one[2], rest[2]]))
    check_records(both, rx.power(x[:8 * M + 512]), M, first=3)
    assert len(ch.rf_monitor_records(0)[0]) == 0
    ch.close()


def test_three_streams():
    """Three independent 384 kHz rows, noiseless constant-envelope carriers at 0.03, 0.1 and 0.3: each row's records against
    its own oracle, and the level where the amplitude puts it."""
    M = 4096
    calls = [[5000, 3000], [1], [20000], [4096, 777]]
    n = sum(map(sum, calls))
    amps = (0.03, 0.1, 0.3)
    x = np.stack([signal(n, amplitude=a, seed=s, am=0.0, noise=0.0) for s, a in enumerate(amps)])
    ch = chain384(S=3)
    ch.enable_rf_monitor(interval_samples=M, max_records=16)
    feed(ch, x, calls, S=3)
    levels = []
    for s in range(3):
        got = ch.rf_monitor_records(s)
        check_records(got[:3], rx.power(x[s]), M)
        levels.append(fmr.rf_levels(*got[:3])["level_dbfs"])
        assert abs(levels[-1] - 20.0 * np.log10(amps[s])) <= 0.05, (s, levels)
    assert levels[0] < levels[1] < levels[2]
    ch.close()


def test_beside_the_modulation_monitor_with_unlike_parameters():
    """Both segment monitors on one two-stream chain, each with its own record length, histogram and ring depth (1024
    samples, 64 bins, 256 records against 512 samples, 384 bins, 4 records), over the ragged calls: every stream's
    modulation records against the monitor fixture on its tap 1 with nothing dropped, the RF monitor's ring overrun to
    its newest four records, which stand against this file's fixture; neither monitor's partition, carry, ring or read
    position is the other's."""
    S, n = 2, sum(map(sum, RAGGED))
    x = np.stack([signal(n, amplitude=a, seed=11 + s) for s, a in enumerate((0.3, 0.1))])
    ch = chain384(S=S)
    ch.enable_monitor(interval_samples=1024, hist_bins=64, max_records=256)
    ch.enable_rf_monitor(interval_samples=512, max_records=4)
    mpx, _ = tgm.feed(ch, x, RAGGED, S=S)
    n_mod, n_rf = (n - 512) // 1024, (n - 512) // 512
    assert n_mod < 256 and n_rf > 4
    for s in range(S):
        mod = ch.monitor_records(s)
        assert len(tgm.check_records(mod[:3], mpx[s], 1024, 64, 2.0)) == n_mod
        assert mod[3]["records_dropped"] == 0 and mod[3]["records_complete"] == n_mod and mod[3]["hist_bins"] == 64
        got = ch.rf_monitor_records(s)
        assert len(check_records(got[:3], rx.power(x[s]), 512, first=n_rf - 4)) == 4
        assert got[3]["records_dropped"] == n_rf - 4 and got[3]["records_complete"] == n_rf
        assert ch.monitor_records(s)[3]["records_dropped"] == 0
    ch.close()


def test_two_channel_bank(monkeypatch):
    """A two-channel bank at 2.5 MS/s in blocks of 16384: each channel's records against its own tap 0."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    F, blk, M = 2.5e6, 16384, 4096
    offs = [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 8, [7]]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 4], [0.3, 0.12])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                   channel_offsets_hz=offs)
    ch.enable_rf_monitor(interval_samples=M, max_records=16)
    ifs, _ = feed(ch, x, calls, S=2, taps=True)
    for s in range(2):
        got = ch.rf_monitor_records(s)
        ref = check_records(got[:3], rx.power(ifs[s]), M)
        assert len(ref) >= 6
    ch.close()


def test_production_path(monkeypatch):
    """10 MS/s, blocks of 65536: the front end's discriminator epilogue leaves |x|^2 in the slot.  (a) four asynchronous
    device calls and one fmr_synchronize against the in_order chain: bit for bit.  (b) the same input through a twin
    created with FMR_DEBUG_TAPS=1, whose slot holds the IF samples: the twin against the oracle on its tap 0, and the two
    forms of p against each other (they differ by a few fp32 roundings, <= 3 x 2^-24 each)."""
    import torch
    F, blk, per, M = 10e6, 65536, 4, 4096
    n = 4 * per * blk
    x = siggen.fm_stereo_iq(n, F)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per)
    calls = [[blk] * per] * 4
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_rf_monitor(interval_samples=M, max_records=16)
    feed(ref_ch, x, calls)
    ref = ref_ch.rf_monitor_records(0)
    assert "fused" in ref_ch.front_end_forms()
    with pytest.raises(fmr.FmrError):
        ref_ch.debug_read(0)                 # no IF samples behind the epilogue: the slot holds |x|^2
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_rf_monitor(interval_samples=M, max_records=16)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(2 * (n // 200 + 4096), dtype=torch.float64, device="cuda")
    for i in range(4):
        ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * blk, n, [blk] * per, d_a.data_ptr(), d_a.numel(), sync=False)
    ch.synchronize()
    got = ch.rf_monitor_records(0)
    ch.close()
    assert len(ref[0]) == got[3]["records_complete"] >= 8 and np.all(ref[0]["n_finite"] == M)
    assert _same_bits(got[:3], ref[:3])
    # (b)
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    twin = fmr.Chain(**kw)
    twin.enable_rf_monitor(interval_samples=M, max_records=16)
    (ifs,), _ = feed(twin, x, calls, taps=True)
    b = twin.rf_monitor_records(0)
    twin.close()
    check_records(b[:3], rx.power(ifs), M)
    a = got
    assert np.array_equal(a[0]["n_finite"], b[0]["n_finite"]) and np.array_equal(a[0]["segments"], b[0]["segments"])
    for k in ("m2", "m4"):
        rel = np.abs(a[0][k] - b[0][k]) / b[0][k]
        print(k, "worst relative difference", rel.max())
        assert np.all(rel <= 1e-6), (k, rel.max())
    moved = np.abs(a[1].astype(np.int64) - b[1].astype(np.int64)).sum(axis=1)
    print("histogram counts moved", moved, "p_max ratio", a[0]["p_max"] / b[0]["p_max"])
    assert np.all(moved <= 2 + 1e-4 * b[0]["n_finite"])
    for i in range(len(b[0])):
        d = np.abs(a[2][i] - b[2][i])
        worst = max(np.max(d / psd_bound(b[2][i])), np.max(d / psd_bound(a[2][i])))
        assert worst <= 1.0, (i, worst)


@pytest.mark.parametrize("shape", ["if_filter", "equaliser"])
def test_if_filter_and_equaliser_measure_the_unfiltered_input(shape):
    """-f medium and multipath_stages = 16 at 384 kHz: neither writes the IF slot in place; the records are those of the
    unfiltered, unequalised input."""
    M = 4096
    calls = [[8192, 4096], [300], [20000]]
    n = sum(map(sum, calls))
    x = signal(n, seed=11)
    kw = dict(fmfilter_enable=True, filter_coeff=load_filter("jj1bdx_fm_384kHz_medium")) if shape == "if_filter" else \
        dict(multipath_stages=16)
    ch = chain384(**kw)
    ch.enable_rf_monitor(interval_samples=M, max_records=16)
    feed(ch, x, calls)
    got = ch.rf_monitor_records(0)
    ref = check_records(got[:3], rx.power(x), M)
    assert len(ref) == (n - 512) // M
    ch.close()


def test_nothing_else_moves():
    """Audio, fmr_status, PPS events, RDS groups, modulation records and loudness records of an RDS chain with both other
    monitors on are bit-identical with and without the RF monitor; a chain without it runs none of its kernels."""
    F, blk = 10e6, 65536
    n = 10 * blk * 16
    groups = rf.ps_groups(0xA0D1, "RFMON", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    x = rf.fm_iq(rf.station_mpx(t, groups), F).astype(np.complex64)
    outs = []
    for on in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_loudness()
        if on:
            ch.enable_rf_monitor()
        ch.enable_kernel_timing(1)
        audio, pps, names = [], [], set()
        for pos in range(0, n, 8 * blk):
            a, _ = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        mon, ld = ch.monitor_records(0), ch.loudness_records(0)
        outs.append((np.concatenate(audio, axis=1), bytes(ch.status(0)), pps, ch.rds_groups(0), names,
                     (mon[0].tobytes(), mon[1].tobytes(), mon[2].tobytes()), ld[0].tobytes(),
                     ch.rf_monitor_records(0) if on else None))
        ch.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert len(outs[0][3]) >= 3 and np.array_equal(outs[0][3], outs[1][3])
    assert len(outs[0][5][0]) >= 4 * 56 and outs[0][5] == outs[1][5]
    assert len(outs[0][6]) > 0 and outs[0][6] == outs[1][6]
    assert not any(k.startswith("rfm") for k in outs[0][4])
    assert {"rfm_seg", "rfm_reduce"} <= outs[1][4]
    recs = outs[1][7][0]
    assert len(recs) >= 4 and np.all(recs["n_finite"] == 38400) and np.all(recs["segments"] == 75)


def test_refusals_with_a_device():
    am = fmr.Chain(mode=fmr.MODE_AM, input_rate=1.48e6, enable_resampler=True, max_block_len=16384,
                   filter_coeff=fmr.filter_table("jj1bdx_am_48khz_default"))
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_rf_monitor"):
        am.enable_rf_monitor()
    am.close()
    nbfm = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=1.48e6, enable_resampler=True, max_block_len=16384,
                     filter_coeff=fmr.filter_table("jj1bdx_nbfm_48khz_default"))
    with pytest.raises(fmr.FmrError, match=r"error -3.*fmr_enable_rf_monitor"):
        nbfm.enable_rf_monitor()
    nbfm.close()
    fe = fmr.Channelizer(2.5e6, [-700_000, 250_000], max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_rf_monitor()
    fe.close()
    ch = chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no RF monitor"):
        ch.rf_monitor_records(0)
    ch.enable_rf_monitor()
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_rf_monitor()
    ch.close()
    ch = chain384()
    ch.process_blocks(signal(4096)[None, :], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_rf_monitor()
    ch.close()


def test_facade_smoke(tmp_path):
    """tests/rfmon_smoke.cpp through the facade: FmDecoder and a two-channel ChannelBank."""
    exe = str(tmp_path / "rfmon_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "rfmon_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fm records 4" in r.stdout and "bank0 records" in r.stdout and "bank1 records" in r.stdout, r.stdout

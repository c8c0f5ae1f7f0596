"""RDS on the GPU (fmr_create_rds): known groups encoded onto the 57 kHz subcarrier of a station's MPX
(tests/rds_fixture.py), FM-modulated, decoded by the chain; the transmitted payload is the oracle."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import rds_fixture as rf
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

F = 10e6
BLK = 65536
T0 = 0.002
ACQ_GROUPS = 4                        # groups the chain may lose while it acquires (the first window + block sync)
GROUP_SAMPLES = 104 * rf.TD * 384000.0


def ngroups(n, fs):
    """Groups that cover a capture of n samples at fs (the RDS runs from T0 to past its end)."""
    return int(n / fs / (104 * rf.TD)) + 2


def capture(n, fs_gen, groups, **kw):
    t = np.arange(n, dtype=np.float64) / fs_gen
    return rf.fm_iq(rf.station_mpx(t, groups, t0=T0, **kw), fs_gen).astype(np.complex64)


def run_calls(ch, x, calls):
    pos = 0
    for ll in calls:
        m = sum(ll)
        ch.process_blocks(x[pos:pos + m], ll)
        pos += m


def even_calls(n, per=8):
    lens = [BLK] * (n // BLK)
    return [lens[i:i + per] for i in range(0, len(lens), per)]


def check_groups(got, sent, rate_ratio=1.0, acq=ACQ_GROUPS):
    """After at most `acq` groups of acquisition every transmitted group comes back, in order, with no bad block, each
    at the sample index of its first bit: the offsets to the transmitter's times are one constant (the chain's latency,
    a few hundred samples) to within 8 samples.

    These checks are wide on purpose: they hold with noise on the IQ and with a transmitter 20 ppm off the chain's clock.
    The exact ones -- sample_index absolute to 0.7 sample, timing, carrier phase, offset and injection against the float64
    receiver on the oracle's MPX of the same chain -- are in tests/test_gpu_rds_front_end.py; the clock-error case stays
    here alone, since that receiver assumes the nominal symbol clock."""
    blocks = [tuple(int(v) for v in g["block"]) for g in got]
    assert len(blocks) >= 3, len(blocks)
    first = [tuple(g) for g in sent].index(blocks[0])
    assert first <= acq, first
    want = [tuple(g) for g in sent[first:first + len(blocks)]]
    assert blocks == want
    assert all(int(s) == fmr.RDS_OK for g in got for s in g["status"])
    expect = rf.group_times(sent, T0)[first:first + len(blocks)] * 384000.0 * rate_ratio
    off = np.array([int(g["sample_index"]) for g in got], dtype=np.float64) - expect
    assert off.max() - off.min() <= 8.0, off
    assert abs(float(np.median(off))) < 2000, off
    return first


@pytest.mark.parametrize("shape", ["fast", "r8b", "fm_medium"])
def test_exact_groups(shape, fm_medium):
    """A stereo station with RDS at 10 MS/s, FAST and R8B classes, and one with -f medium: every group after acquisition,
    exactly; PS and PI recovered; the injection estimate near the transmitted level."""
    groups = rf.ps_groups(0xC0DE, "GPU RDS1", rt="RADIOTEXT FROM THE GPU TEST", n=ngroups(13 * BLK * 16, F))
    n = 13 * BLK * 16
    x = capture(n, F, groups)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
              enable_rds=True)
    if shape == "r8b":
        kw["resampler_class"] = fmr.RESAMPLER_R8B
    if shape == "fm_medium":
        kw.update(fmfilter_enable=True, filter_coeff=fm_medium)
    ch = fmr.Chain(**kw)
    run_calls(ch, x, even_calls(n))
    got = ch.rds_groups(0)
    st = ch.rds_status(0)
    check_groups(got, groups)
    assert fmr.rds_pi(got) == 0xC0DE and fmr.rds_ps(got) == "GPU RDS1"
    assert st.synced == 1 and st.blocks_bad == 0 and st.groups_dropped == 0
    assert 0.5 * (2 / 75) < st.injection < 2.0 * (2 / 75), st.injection
    assert np.isfinite([st.timing, st.carrier_phase, st.carrier_offset_hz]).all()
    ch.close()


@pytest.mark.parametrize("corrected", [False, True])
def test_no_pilot_quadrature_clock_error(corrected):
    """A mono station without pilot, the subcarrier in quadrature with where 3 x pilot would be, generated 20 ppm off the
    rate the chain is told (subcarrier ~1.1 Hz off 57 kHz, symbol clock 20 ppm off); again as a ppm-corrected chain told
    the true rate.  Both return the transmitted groups."""
    fs_gen = F * (1 + 20e-6)
    groups = rf.ps_groups(0x5EED, "MONO NP", n=ngroups(13 * BLK * 16, F))
    n = 13 * BLK * 16
    x = capture(n, fs_gen, groups, mono=True, pilot=0.0, phase=0.0)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs_gen if corrected else F, enable_resampler=True, stereo=False,
                   max_block_len=BLK, max_blocks=8, enable_rds=True)
    run_calls(ch, x, even_calls(n))
    got = ch.rds_groups(0)
    check_groups(got, groups, rate_ratio=1.0 if corrected else fs_gen / F)
    assert fmr.rds_ps(got) == "MONO NP "
    if not corrected:
        assert abs(abs(ch.rds_status(0).carrier_offset_hz) - 57000 * 20e-6) < 0.5, ch.rds_status(0).carrier_offset_hz
    ch.close()


def _ragged(total, seed):
    rng = np.random.default_rng(seed)
    calls, n = [], 0
    while n < total:
        ll = [int(rng.integers(1, BLK + 1)) if rng.random() < 0.4 else BLK for _ in range(int(rng.integers(1, 9)))]
        ll = [min(b, total - n - sum(ll[:i])) for i, b in enumerate(ll)]
        ll = [b for b in ll if b > 0]
        calls.append(ll)
        n += sum(ll)
    return calls


def test_call_cuts():
    """One capture through four paths and ragged cuts: pipelined, in_order, fmr_process one block at a time, and
    process_blocks_device (asynchronous).  The group lists (blocks and sample indices) are identical."""
    import torch
    groups = rf.ps_groups(0xCAFE, "CUTTEST", rt="CALL CUTS", n=ngroups(11 * BLK * 16, F))
    n = 11 * BLK * 16
    x = capture(n, F, groups)
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
              enable_rds=True)
    res = {}
    ch = fmr.Chain(**kw)
    run_calls(ch, x, _ragged(n, 1))
    res["pipelined"] = ch.rds_groups(0)
    ch.close()
    ch = fmr.Chain(in_order=True, **kw)
    run_calls(ch, x, _ragged(n, 2))
    res["in_order"] = ch.rds_groups(0)
    ch.close()
    ch = fmr.Chain(**dict(kw, max_blocks=1))
    for i in range(0, n, 50_000):
        ch.process(x[i:i + 50_000])
    res["process"] = ch.rds_groups(0)
    ch.close()
    ch = fmr.Chain(**kw)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(2 * (n // 200 + 4096), dtype=torch.float64, device="cuda")
    off = 0
    for ll in _ragged(n, 3):
        ch.process_blocks_device(d_x.data_ptr() + 8 * off, n, ll, d_a.data_ptr(), d_a.numel(), sync=False)
        off += sum(ll)
    ch.synchronize()
    res["device"] = ch.rds_groups(0)
    ch.close()
    ref = res["pipelined"]
    check_groups(ref, groups)
    for k, v in res.items():
        assert np.array_equal(v, ref), k


def test_rds_does_not_touch_the_audio():
    """Audio and fmr_status are bit-identical with and without RDS, pipelined and in_order; without RDS no RDS kernel
    runs."""
    groups = rf.ps_groups(0xA0D1, "AUDIO", n=ngroups(5 * BLK * 16, F))
    n = 5 * BLK * 16
    x = capture(n, F, groups)
    calls = even_calls(n)
    for in_order in (False, True):
        outs = []
        for rds in (False, True):
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=8, in_order=in_order, enable_rds=rds)
            ch.enable_kernel_timing(1)
            audio, pos, names = [], 0, set()
            for ll in calls:
                a, _ = ch.process_blocks(x[pos:pos + sum(ll)], ll)
                audio.append(a)
                names |= {k for k, _ in ch.kernel_times()}
                pos += sum(ll)
            st = ch.status(0)
            outs.append((np.concatenate(audio, axis=1), bytes(st), names))
            ch.close()
        assert np.array_equal(outs[0][0], outs[1][0]), in_order
        assert outs[0][1] == outs[1][1], in_order
        assert not any(k.startswith("rds") for k in outs[0][2])
        assert any(k.startswith("rds") for k in outs[1][2])


BANK_OFFS = [-4_100_000, -2_300_000, -700_000, 400_000, 1_234_567, 4_450_000]


def test_bank_six_stations():
    """Six stations in one 10 MS/s capture, each with its own PI and PS: each channel reports its own groups only."""
    n = 13 * BLK * 16
    t = np.arange(n, dtype=np.float64) / F
    acc = np.zeros(n, dtype=np.complex128)
    sent = []
    for i, f in enumerate(BANK_OFFS):
        g = rf.ps_groups(0x1000 + 0x111 * i, f"STATION{i}", n=ngroups(n, F))
        sent.append(g)
        acc += rf.fm_iq(rf.station_mpx(t, g, t0=T0, stereo_id=3 * i), F, amplitude=0.2, sigma=0, seed=i) * \
            cb.phasor(n, f, F, +1)
    x = (acc + 1e-3 * (np.random.default_rng(9).standard_normal(n) + 1j * np.random.default_rng(8).standard_normal(n))
         ).astype(np.complex64)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
                   channel_offsets_hz=BANK_OFFS, enable_rds=True)
    run_calls(ch, x, even_calls(n))
    for s in range(len(BANK_OFFS)):
        got = ch.rds_groups(s)
        check_groups(got, sent[s])
        assert fmr.rds_pi(got) == 0x1000 + 0x111 * s and fmr.rds_ps(got) == f"STATION{s}"
    ch.close()


def test_nan_and_dropout():
    """NaN samples and a 100 ms dropout in the capture: the status stays finite, the decoder loses the synchronisation and
    is back within 6 groups after the dropout, with the transmitted groups."""
    groups = rf.ps_groups(0xD0D0, "DROPOUT", n=ngroups(25 * BLK * 16, F))
    n = 25 * BLK * 16
    x = capture(n, F, groups)
    x[3_000_000:3_000_010] = np.nan
    x[int(1.0 * F):int(1.1 * F)] = 0
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
                   enable_rds=True)
    run_calls(ch, x, even_calls(n))
    got = ch.rds_groups(0)
    st = ch.rds_status(0)
    assert np.isfinite([st.injection, st.timing, st.carrier_phase, st.carrier_offset_hz]).all()
    good = [g for g in got if all(int(s) == fmr.RDS_OK for s in g["status"])]
    tg = rf.group_times(groups, T0)
    dec = {int(round((int(g["sample_index"]) / 384000.0 - T0) / (104 * rf.TD))): tuple(int(v) for v in g["block"])
           for g in good}
    assert all(dec[i] == tuple(groups[i]) for i in dec)              # nothing decoded wrongly, before or after
    t_end = 1.1 + 6 * 104 * rf.TD                                    # back within 6 groups after the dropout ...
    back = [i for i in range(len(groups)) if t_end < tg[i] < n / F - 3 * 104 * rf.TD]
    assert len(back) >= 4 and all(i in dec for i in back), (back, sorted(dec))   # ... (the last windows are still open)
    assert st.synced == 1
    ch.close()


def test_queue_overflow_counts_dropped_groups():
    """Nobody drains the queue for 25 s of RDS: it holds 256 groups and counts the rest as dropped."""
    groups = rf.ps_groups(0x0F0F, "OVERFLOW", n=320)
    fs = 384000.0
    n = int(26.5 * fs)
    x = capture(n, fs, groups)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs, enable_resampler=False, stereo=True, max_block_len=BLK,
                   max_blocks=16, enable_rds=True)
    run_calls(ch, x, [[BLK] * 16 for _ in range(n // (16 * BLK))])
    st = ch.rds_status(0)
    got = ch.rds_groups(0)
    assert len(got) == 256 and st.groups_dropped == st.groups_decoded - 256 > 0, (len(got), st.groups_dropped)
    ch.close()


def test_facade_smoke(tmp_path):
    """tests/rds_bank_smoke.cpp through the facade: the PS of two bank channels."""
    exe = str(tmp_path / "rds_bank_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "rds_bank_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ps0 [FACADE A]" in r.stdout and "ps1 [FACADE B]" in r.stdout, r.stdout

"""MPX output on the GPU (fmr_enable_mpx_output): the PCM ring, the totals and the info of a chain against
tests/mpx_output_fixture.py run on the MPX a twin chain on the same input delivers through the stage itself at 384000 F32,
gain 1.0 (where the ring is the MPX, bit for bit).  Stage and fixture see the same float32 samples and the same taps and add
in the same order: every ring sample and every counter must be equal bit for bit.

The base chain: FM stereo fed at 384 kHz without the resampler, two unlike streams, 57344 samples (0.149 s, 3.5 blocks of
16384).

The tap against the oracle.  oracle_mpx.oracle_mpx always puts the oracle's IfResampler in front of its FmDecoder, also at
384 kHz in, where it is a filter of its own with 41 samples of latency that a chain with enable_resampler=False does not
have.  For the base chain the reference is therefore what oracle_mpx joins -- FmDecoder.debug_vector(0, n) block by block --
with the same decoder settings and no resampler (oracle_tap below); the bank test holds a bank's tap to oracle_mpx itself.
Bounds: 4 x the largest difference measured once on the MI355X over the samples after the AGC transient (the margin covers
the choice of front-end form, not error growth); the oracle's own float32 resolution, 2.4e-7 (tests/oracle_mpx.py), is the
floor below which a bound means nothing.
  base chain: measured 9.5367e-07 (2^-20, both streams; it is also the largest over all samples), bound 3.815e-06
  bank (2.5 MS/s, three channels): measured 1.4305e-06 (channel 1; 1.0729e-06 on the two others; RMS 2.2e-07), bound 5.722e-06"""
import importlib

import numpy as np
import pytest

import chanbank_fixture as cb
import mpx_output_fixture as mf
import oracle_mpx as om
import oracle_py as ora
import rds_fixture as rf
import siggen
from conftest import load_filter

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS, BLK, N = 384000.0, 16384, 57344
ONE = [[BLK, BLK, BLK, N - 3 * BLK]]
TAP_MEASURED, BANK_MEASURED = 9.5367e-07, 1.4305e-06
TAP_BOUND, BANK_BOUND = 4 * TAP_MEASURED, 4 * BANK_MEASURED
SETTLED = 8192                       # samples the IF AGC and the filters take to settle
INFO_KEYS = ("rate", "L", "M", "taps_per_phase", "delay_frames", "full_scale_hz", "samples_in")
_cache = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rows():
    if "rows" not in _cache:
        _cache["rows"] = np.stack([siggen.fm_stereo_iq(N, FS, stream_id=0),
                                   siggen.fm_stereo_iq(N, FS, stream_id=3, amplitude=0.2, phase0=0.7)])
    return _cache["rows"]


def chain384(S=2, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=True, max_block_len=BLK, max_blocks=8,
                     n_streams=S, **kw)


def feed(ch, x, calls, taps=False):
    """x [rows, n] through process_blocks, one call per entry of `calls`.  Returns the audio [S, m] and, with taps, the MPX
    of every stream as the chain demodulated it (fmr_debug_read 1 after every call, joined)."""
    x = np.atleast_2d(x)
    S = ch.n_streams
    mpx, audio, pos = [[np.zeros(0, np.float32)] for _ in range(S)], [], 0
    for ll in calls:
        m = int(sum(ll))
        a, _ = ch.process_blocks(x[:, pos:pos + m], ll)
        audio.append(a)
        if taps:
            for s in range(S):
                mpx[s].append(ch.debug_read(1, stream=s, cap=1 << 18))
        pos += m
    return np.concatenate(audio, axis=1), [np.concatenate(v) for v in mpx]


def run(x, calls, fmt="s16", rate=192000, gain=0.5, max_frames=0, taps=False, **kw):
    """A base chain with the stage over x in `calls`: per stream (pcm, info), and the joined debug taps if asked."""
    ch = chain384(S=len(x), **kw)
    ch.enable_mpx_output(format=fmt, rate=rate, gain=gain, max_frames=max_frames)
    _, mpx = feed(ch, x, calls, taps)
    out = [ch.mpx_output_read(s) for s in range(len(x))]
    ch.close()
    return out, mpx


def tap():
    """The MPX of both base streams: the stage at 384000 F32, gain 1.0 (held to the chain's debug tap and to the oracle by
    test_the_tap)."""
    if "tap" not in _cache:
        out, mpx = run(rows(), ONE, "f32", 384000, 1.0, taps=True)
        _cache["tap"] = ([p for p, _ in out], [i for _, i in out], mpx)
    return _cache["tap"]


def check(pcm, info, x, rate, gain, fmt, first=0, dropped=0):
    """One stream's drained ring and info against the fixture on the MPX x."""
    ref, cl, nf = mf.run(x, rate, gain, mf.PCM_S16 if fmt == "s16" else mf.PCM_F32)
    assert same_bits(pcm, ref[first:]), (pcm.shape, ref.shape, first)
    want = mf.info(rate, gain, len(x))
    assert {k: info[k] for k in INFO_KEYS} == want, (info, want)
    assert (info["pcm_clipped"], info["pcm_nonfinite"]) == (cl, nf), (info, cl, nf)
    assert (info["first_frame"], info["frames_dropped"], info["frames_waiting"]) == (first, dropped, 0), info
    assert info["format"] == (fmr.PCM_S16 if fmt == "s16" else fmr.PCM_F32)
    return ref


def oracle_tap(x, lens):
    """What oracle_mpx joins, for a chain without the resampler: the oracle FmDecoder's discriminator output per block."""
    fm = ora.FmDecoder(False, om.DELAY_3TAPS, True, 50.0, False, 0, load_filter("jj1bdx_48khz_fmaudio"))
    out, pos = [], 0
    for bl in lens:
        fm.process(x[pos:pos + bl])
        out.append(fm.debug_vector(0, bl).copy())
        pos += bl
    return np.concatenate(out)


# ---- 1: the tap --------------------------------------------------------------------------------------------------------
def test_the_tap():
    """Rate 384000, F32, gain 1.0: the ring is the MPX -- the very bits of the chain's debug tap -- and that MPX is the
    oracle decoder's to TAP_BOUND."""
    pcm, info, mpx = tap()
    for s in range(2):
        assert pcm[s].dtype == np.float32 and len(pcm[s]) == N and same_bits(pcm[s], mpx[s])
        assert {k: info[s][k] for k in INFO_KEYS} == mf.info(384000, 1.0, N)
        assert (info[s]["L"], info[s]["M"], info[s]["taps_per_phase"], info[s]["delay_frames"]) == (1, 1, 1, 0.0)
        assert info[s]["full_scale_hz"] == 75000.0 and info[s]["pcm_nonfinite"] == 0
        assert info[s]["pcm_clipped"] == int((np.abs(pcm[s].astype(np.float64)) > 1.0).sum())
        ref = oracle_tap(rows()[s], ONE[0])
        d = np.abs(pcm[s][SETTLED:].astype(np.float64) - ref[SETTLED:]).max()
        print(f"stream {s}: largest |tap - oracle| after {SETTLED} samples: {d:.3e} (measured {TAP_MEASURED}, bound {TAP_BOUND})")
        assert d <= TAP_BOUND
    assert not same_bits(pcm[0], pcm[1]) and np.abs(pcm[0]).max() > 0.5


# ---- 2: bit parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fmt", [(192000, "s16"), (171000, "s16"), (256000, "f32"), (96000, "f32")])
def test_bit_parity(rate, fmt):
    x = tap()[0]
    out, _ = run(rows(), ONE, fmt, rate, 0.5)
    for s in range(2):
        pcm, info = out[s]
        ref = check(pcm, info, x[s], rate, 0.5, fmt)
        assert len(pcm) == mf.n_out(N, info["L"], info["M"]) and ref.any()
    _cache[("one", rate, fmt)] = [p for p, _ in out]


# ---- 3: cuts -----------------------------------------------------------------------------------------------------------
# 171000: T = 320, M = 128.  A 1-sample call, a call with empty blocks, 128 calls of 129 samples -- each shorter than T - 1 =
# 319 samples, their boundaries 6 + 129 k on every residue of 128 -- a 318-sample call, blocks of 1 inside a call, long calls.
RAGGED = [[1], [0, 5, 0]] + [[129]] * 128 + [[318], [BLK, 1, 1, 1000], [BLK, 3616]]
RAGGED.append([N - sum(map(sum, RAGGED))])


def test_cuts():
    rate, fmt = 171000, "s16"
    h, L, M, T = mf.taps(rate)
    ends = np.cumsum([sum(c) for c in RAGGED])
    assert ends[-1] == N and set((ends % M).tolist()) == set(range(M)) and T - 1 == 319 and RAGGED[-1][0] > 0
    x = tap()[0]
    out, mpx = run(rows(), RAGGED, fmt, rate, 0.5, taps=True)
    one = _cache.get(("one", rate, fmt)) or [p for p, _ in run(rows(), ONE, fmt, rate, 0.5)[0]]
    for s in range(2):
        assert same_bits(mpx[s], x[s])                    # the MPX itself does not depend on the cuts
        check(*out[s], x[s], rate, 0.5, fmt)
        assert same_bits(out[s][0], one[s])


# ---- 4: ring -----------------------------------------------------------------------------------------------------------
def test_ring_overrun_and_a_read_in_the_middle():
    rate, fmt = 192000, "s16"
    x = tap()[0]
    total = N // 2
    out, _ = run(rows(), ONE, fmt, rate, 0.5, max_frames=1000)
    for s in range(2):
        pcm, info = out[s]
        assert len(pcm) == 1000
        check(pcm, info, x[s], rate, 0.5, fmt, first=total - 1000, dropped=total - 1000)
    # a ring of 20000 < 28672 frames: a read after two blocks (16384 frames), then the rest, which wraps
    ch = chain384()
    ch.enable_mpx_output(format=fmt, rate=rate, max_frames=20000)
    feed(ch, rows()[:, :2 * BLK], [[BLK, BLK]])
    first = [ch.mpx_output_read(s) for s in range(2)]
    part = [ch.mpx_output_read(s, cap_frames=0) for s in range(2)]
    feed(ch, rows()[:, 2 * BLK:], [[BLK, N - 3 * BLK]])
    head = [ch.mpx_output_read(s, cap_frames=100) for s in range(2)]
    rest = [ch.mpx_output_read(s) for s in range(2)]
    ch.close()
    for s in range(2):
        ref = mf.run(x[s], rate, 0.5, mf.PCM_S16)[0]
        assert len(first[s][0]) == BLK and first[s][1]["first_frame"] == 0 and first[s][1]["frames_waiting"] == 0
        assert len(part[s][0]) == 0 and part[s][1]["first_frame"] == BLK and part[s][1]["samples_in"] == 2 * BLK
        assert len(head[s][0]) == 100 and head[s][1]["first_frame"] == BLK and head[s][1]["frames_waiting"] == total - BLK - 100
        assert rest[s][1]["first_frame"] == BLK + 100 and rest[s][1]["frames_dropped"] == 0
        assert same_bits(np.concatenate([first[s][0], head[s][0], rest[s][0]]), ref)


# ---- 5: saturation and non-finite samples ------------------------------------------------------------------------------
def test_saturation_at_gain_four():
    x = tap()[0]
    out, _ = run(rows(), ONE, "s16", 192000, 4.0)
    for s in range(2):
        pcm, info = out[s]
        check(pcm, info, x[s], 192000, 4.0, "s16")
        print("stream", s, "pcm_clipped", info["pcm_clipped"])
        assert info["pcm_clipped"] > 0 and pcm.max() == 32767 and pcm.min() == -32768 and info["full_scale_hz"] == 18750.0


def test_a_nan_sample_stays_in_its_stream():
    """One NaN IQ sample mid-input on stream 0.  Its places in the MPX are taken from the tap.  This chain's discriminator
    answers a non-finite phase step with 0 (the reference's rule), and on the MI355X the tap showed no non-finite sample
    at all: stream 0's MPX differs from the clean run's and is finite.  The count is printed, and the ring and
    pcm_nonfinite follow the fixture on the tap either way (the conversion of NaN and Inf themselves is held on the CPU,
    tests/test_mpx_output_fixture.py).  Stream 1 is the bits of its run without the NaN."""
    x = rows().copy()
    x[0, 30000] = np.complex64(complex(np.nan, 0.0))
    clean = tap()[0]
    t_out, _ = run(x, ONE, "f32", 384000, 1.0)
    r_out, _ = run(x, ONE, "f32", 192000, 0.5)
    xt = [p for p, _ in t_out]
    bad = np.flatnonzero(~np.isfinite(xt[0]))
    print("non-finite MPX samples of stream 0 at", bad, "; pcm_nonfinite", t_out[0][1]["pcm_nonfinite"], r_out[0][1]["pcm_nonfinite"])
    assert t_out[0][1]["pcm_nonfinite"] == len(bad)
    for s in range(2):
        check(*r_out[s], xt[s], 192000, 0.5, "f32")
    assert same_bits(xt[1], clean[1]) and r_out[1][1]["pcm_nonfinite"] == 0
    assert not same_bits(xt[0], clean[0])


# ---- 6: the stage only reads -------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    """Audio, fmr_status, PPS events, RDS groups, monitor records and the output stage's PCM and records are bit-identical
    with and without the MPX output; without it none of its kernels runs."""
    blk, nb = 16384, 24
    n = blk * nb
    groups = rf.ps_groups(0xA0D1, "MPX-OUT!", n=int(n / FS / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / FS
    x = rf.fm_iq(rf.station_mpx(t, groups), FS).astype(np.complex64)
    outs = []
    for on in (False, True):
        ch = chain384(S=1, enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_output()
        if on:
            ch.enable_mpx_output(rate=192000)
        ch.enable_kernel_timing(1)
        audio, pps, names = [], [], set()
        for pos in range(0, n, 8 * blk):
            a, _ = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        pcm, recs, _ = ch.output_read(0)
        outs.append(dict(audio=np.concatenate(audio, axis=1), status=bytes(ch.status(0)), pps=pps, rds=ch.rds_groups(0),
                         mon=ch.monitor_records(0)[:3], pcm=pcm, recs=recs, names=names,
                         mpx=ch.mpx_output_read(0) if on else None))
        ch.close()
    a, b = outs
    assert same_bits(a["audio"], b["audio"]) and a["status"] == b["status"] and a["pps"] == b["pps"]
    assert len(a["rds"]) >= 2 and same_bits(a["rds"], b["rds"])
    assert len(a["mon"][0]) >= 6 and all(same_bits(u, v) for u, v in zip(a["mon"], b["mon"]))
    assert len(a["pcm"]) > 30000 and same_bits(a["pcm"], b["pcm"]) and same_bits(a["recs"], b["recs"])
    assert not any(k.startswith("mpx_") for k in a["names"]) and {"mpx_rate", "mpx_hist"} <= b["names"]
    pcm, info = b["mpx"]
    assert len(pcm) == n // 2 and info["samples_in"] == n and pcm.any()


# ---- 7: bank, pipelined and in_order -----------------------------------------------------------------------------------
F_BANK, OFFS = 2.5e6, [-700_000, 250_000, 600_000]
BANK_CALLS = [[BLK] * 6, [BLK, 1000], [BLK] * 8, [7], [BLK] * 7]


def bank_x():
    if "bank" not in _cache:
        _cache["bank"] = cb.composite(sum(map(sum, BANK_CALLS)), F_BANK, OFFS, [3, 4, 5], [0.3, 0.2, 0.25])
    return _cache["bank"]


def bank(**kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=F_BANK, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
                     channel_offsets_hz=OFFS, **kw)


def bank_tap():
    if "bank_tap" not in _cache:
        ch = bank()
        ch.enable_mpx_output(format="f32", rate=384000, gain=1.0)
        feed(ch, bank_x(), BANK_CALLS)
        _cache["bank_tap"] = [ch.mpx_output_read(s)[0] for s in range(3)]
        ch.close()
    return _cache["bank_tap"]


def test_three_channel_bank():
    """Each channel's ring at 192000 against the fixture on that channel's own 384000 tap from a twin bank; the taps
    against oracle_mpx of the capture."""
    x = bank_tap()
    ch = bank()
    ch.enable_mpx_output(rate=192000)
    feed(ch, bank_x(), BANK_CALLS)
    out = [ch.mpx_output_read(s) for s in range(3)]
    ch.close()
    ref = om.oracle_mpx(bank_x(), [b for c in BANK_CALLS for b in c], F_BANK, offsets_hz=OFFS)
    for s in range(3):
        assert len(x[s]) == len(ref[s]) > 50000
        check(*out[s], x[s], 192000, 0.5, "s16")
        d = np.abs(x[s][SETTLED:].astype(np.float64) - ref[s][SETTLED:]).max()
        print(f"channel {s}: largest |tap - oracle_mpx| after {SETTLED} samples: {d:.3e} (measured {BANK_MEASURED}, bound {BANK_BOUND})")
        assert d <= BANK_BOUND
    assert not same_bits(x[0], x[1]) and not same_bits(x[1], x[2])
    _cache["bank_192"] = [p for p, _ in out]


def test_pipelined_against_in_order():
    """The bank's calls as asynchronous device calls and one fmr_synchronize (pipelined: the tail runs a call late), and the
    in_order bank: the same rings, and the fixture's on the tap."""
    import torch
    x = bank_x()
    tapx = bank_tap()
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    stride = 2 * 8 * 2200
    got = []
    for in_order in (False, True):
        ch = bank(in_order=in_order)
        ch.enable_mpx_output(rate=171000)
        d_a = torch.zeros((len(BANK_CALLS), 3, stride), dtype=torch.float64, device="cuda")
        pos = 0
        for i, ll in enumerate(BANK_CALLS):
            ch.process_blocks_device(d_x.data_ptr() + 8 * pos, len(x), ll, d_a[i].data_ptr(), stride, sync=False)
            pos += sum(ll)
        ch.synchronize()
        got.append([ch.mpx_output_read(s) for s in range(3)])
        ch.close()
    for s in range(3):
        check(*got[0][s], tapx[s], 171000, 0.5, "s16")
        assert same_bits(got[0][s][0], got[1][s][0]) and got[0][s][1] == got[1][s][1]


# ---- 8: lifecycle ------------------------------------------------------------------------------------------------------
def test_lifecycle(am_narrow):
    live0 = fmr.debug_live_resources()
    ch = chain384(S=1)
    with pytest.raises(fmr.FmrError, match=r"error -2.*no MPX output"):
        ch.mpx_output_read(0)
    with pytest.raises(fmr.FmrError, match=r"error -2.*rate"):
        ch.enable_mpx_output(rate=100001)
    ch.enable_mpx_output(rate=228000, format="f32")
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_mpx_output()
    with pytest.raises(fmr.FmrError, match=r"error -2.*stream"):
        ch.mpx_output_read(1)
    pcm, info = ch.mpx_output_read(0)
    assert len(pcm) == 0 and pcm.dtype == np.float32 and (info["L"], info["M"], info["samples_in"]) == (19, 32, 0)
    ch.close()
    ch = chain384(S=1)
    ch.process_blocks(rows()[:1, :4096], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_mpx_output()
    ch.close()
    ch = fmr.Chain(mode=fmr.MODE_AM, input_rate=48e3, filter_coeff=am_narrow, max_block_len=2048, max_blocks=8)
    with pytest.raises(fmr.FmrError, match=r"error -3.*MPX"):
        ch.enable_mpx_output()
    ch.close()
    cz = fmr.Channelizer(F_BANK, OFFS, max_block_len=BLK, max_blocks=8)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        cz.enable_mpx_output()
    cz.close()
    assert fmr.debug_live_resources() == live0


def test_facade_smoke(tmp_path):
    """tests/mpx_output_smoke.cpp through the facade: FmDecoder (192 kHz S16, then a WAV file) and a two-channel
    ChannelBank (171 kHz F32)."""
    import os
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / "mpx_output_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "mpx_output_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe, str(tmp_path / "mpx.wav")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("fm frames", "bank0 frames", "bank1 frames", "wav bytes"):
        assert tag in r.stdout, r.stdout

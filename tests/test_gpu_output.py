"""Output stage on the GPU (fmr_enable_output): the PCM and the block records of a chain against tests/output_fixture.py
run on the audio the chain itself returned and on the if_rms the records themselves carry.  Stage and oracle see the
same doubles, and the fixture adds in the stage's order: block, first_frame, n_frames, channels, gate_open, if_level,
audio_level, n_clipped, n_nonfinite and every PCM sample must be equal bit for bit; audio_rms and audio_mean may differ by
one float32 ulp (the sums are fp64, only the final narrowing can land either side).  if_rms itself is held to the
oracle decoders at the tolerance tests/test_gpu_parity.py uses for it (rel = 1e-5: its lines 170, 342 and 473), and the
last record of a call to that call's fmr_status.if_rms bitwise.

Inputs: tests/siggen.py signals of unit amplitude with the carrier amplitude stepped per block between 0.3 and 0.003, and
squelch_level = 0.03.  A step down is taken LEAD samples before the block's end: the front end's filters are causal, so
what they still hold of the strong carrier then falls into the strong block, not into the weak one behind it (with the
step on the boundary the first weak block reads ~0.04: inside a factor 3 of the level).  Every test asserts on its
records that no block's if_rms lies within a factor 3 of the level."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import oracle_py as ora
import output_fixture as of
import rds_fixture as rf
import siggen
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

LEVEL, HI, LO = 0.03, 0.3, 0.003
BIT_FIELDS = ("block", "first_frame", "n_frames", "channels", "if_rms", "gate_open", "if_level", "audio_level", "n_clipped",
              "n_nonfinite")
F10, BLK = 10e6, 65536
AMPS7 = [HI, HI, LO, LO, HI, LO, HI]
LEAD = 4096


def stepped(unit, amps, blk, lead, sigma, seed=11):
    """unit (a unit-amplitude signal) times amps[b] over block b -- a step down taken `lead` samples early -- plus noise."""
    a = np.repeat(np.asarray(amps, dtype=np.float64), blk)
    for b in range(len(amps) - 1):
        if amps[b + 1] < amps[b] and lead:
            a[(b + 1) * blk - lead:(b + 1) * blk] = amps[b + 1]
    return (unit[:len(a)].astype(np.complex128) * a + siggen._noise(len(a), sigma, seed)).astype(np.complex64)


_cache = {}


def fm10():
    """7 x 65536 samples of FM stereo at 10 MS/s, stepped."""
    if "fm10" not in _cache:
        _cache["fm10"] = stepped(siggen.fm_stereo_iq(7 * BLK, F10, amplitude=1.0, sigma=0.0), AMPS7, BLK, LEAD, 1e-3)
    return _cache["fm10"]


# the same input in ragged calls: every 65536-region starts a block, so that no block straddles a step; blocks of 1 (most
# yield no IF sample, the others one IF sample and no audio), 511, 513, 4096 and 65536.  The first region is one block: the
# chain's very first IF samples are the filters' rise from nothing; so is a region behind a step up, which starts with a
# long block for the same reason, and whose short blocks lie in front of the LEAD samples at its end that already carry
# the weak carrier of the region behind it (the block that holds them is half strong: 0.21).
def _region(head):
    return head + [BLK - sum(head)]


RAGGED = [[BLK], _region([1] * 40 + [511, 513, 4096]), _region([4096, 511] + [1] * 30 + [513]) + [BLK],
          [BLK - 1026 - 8192, 513, 1, 1, 511, 8192] + _region([1, 4096]), [BLK]]
ONE = [[BLK] * 7]


def oracle_if(x, lens, F=F10, decode=True):
    """IF samples per block (oracle IfResampler) and the oracle FmDecoder's get_if_rms after each block that has some."""
    key = ("if", id(x), tuple(lens), decode)
    if key not in _cache:
        r = ora.IfResampler(F, 384e3)
        fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, np.load(os.path.join(ROOT, "tests", "golden", "filters",
                                                                                        "jj1bdx_48khz_fmaudio.npy")))
        n_if, rms, o = [], [], 0
        for bl in lens:
            u = r.process(x[o:o + bl])
            o += bl
            n_if.append(len(u))
            if len(u) and decode:
                fm.process(u)
                rms.append(fm.get_if_rms())
        _cache[key] = (n_if, np.array(rms))
    return _cache[key]


def feed(ch, x, calls):
    """x [rows, n] through process_blocks, one call per entry of `calls`: the audio [S, m], the doubles per block, and
    fmr_status.if_rms of stream 0 after every call."""
    x = np.atleast_2d(x)
    audio, alen, st, pos = [], [], [], 0
    for ll in calls:
        m = int(sum(ll))
        a, al = ch.process_blocks(x[:, pos:pos + m], ll)
        audio.append(a)
        alen += [int(v) for v in al]
        st.append(np.float32(ch.status(0).if_rms))
        pos += m
    return np.concatenate(audio, axis=1), alen, st


def oracle(recs, audio, alen, has_if, nch, level=LEVEL, gain=0.5, fmt=of.PCM_S16):
    """The fixture on this stream's audio, block by block, with the if_rms of the records."""
    assert len(recs) == sum(has_if), (len(recs), sum(has_if))
    blocks, o, k = [], 0, 0
    for n, h in zip(alen, has_if):
        if not h:
            assert n == 0
            blocks.append((None, np.zeros(0)))
            continue
        blocks.append((recs["if_rms"][k], audio[o:o + n]))
        o += n
        k += 1
    assert o == len(audio)
    return of.run(blocks, nch, level, gain, fmt)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(recs, pcm, ref, ref_pcm, level=LEVEL):
    print("if_rms:", recs["if_rms"].tolist())
    for k in BIT_FIELDS:
        assert same_bits(recs[k], ref[k]), (k, recs[k][:8], ref[k][:8])
    for k in ("audio_rms", "audio_mean"):
        d = np.abs(recs[k].astype(np.float64) - ref[k].astype(np.float64))
        print(k, "worst deviation in float32 ulps:", float(np.max(d / np.spacing(np.abs(ref[k])), initial=0.0)))
        assert np.all(d <= np.spacing(np.abs(ref[k]))), k
    assert same_bits(pcm, ref_pcm), (pcm.shape, ref_pcm.shape, int(np.sum(pcm != ref_pcm)))
    if level > 0:
        r = recs["if_rms"].astype(np.float64)
        assert np.all((r >= 3 * level) | (r <= level / 3)), r


def check(ch, stream, audio, alen, has_if, nch, level=LEVEL, gain=0.5, fmt=of.PCM_S16):
    pcm, recs, info = ch.output_read(stream)
    ref, ref_pcm = oracle(recs, audio, alen, has_if, nch, level, gain, fmt)
    compare(recs, pcm, ref, ref_pcm, level)
    assert info["frames_dropped"] == 0 and info["blocks_dropped"] == 0 and info["frames_waiting"] == 0 and info["blocks_waiting"] == 0
    assert info["first_frame"] == 0 and info["channels"] == nch and info["format"] == fmt
    return recs, pcm


def chain10(max_blocks=8, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=F10, enable_resampler=True, stereo=True, max_block_len=BLK,
                     max_blocks=max_blocks, **kw)


def run10(calls, fused):
    x = fm10()
    lens = [b for c in calls for b in c]
    n_if, ref_rms = oracle_if(x, lens)
    has_if = [n > 0 for n in n_if]
    ch = chain10(max_blocks=max(len(c) for c in calls))
    ch.enable_output(squelch_level=LEVEL)
    audio, alen, st = feed(ch, x, calls)
    assert ("fused" in ch.front_end_forms()) == fused, ch.front_end_forms()      # fmr_resampler_info(6)
    recs, pcm = check(ch, 0, audio[0], alen, has_if, 2)
    ch.close()
    assert np.allclose(recs["if_rms"], ref_rms, rtol=1e-5, atol=0), np.max(np.abs(recs["if_rms"] / ref_rms - 1))   # tests/test_gpu_parity.py:170
    # the last record of every call against that call's fmr_status.if_rms, bitwise
    ends = np.cumsum([sum(has_if[sum(map(len, calls[:i])):sum(map(len, calls[:i + 1]))]) for i in range(len(calls))])
    for e, s in zip(ends, st):
        assert e > 0 and recs["if_rms"][e - 1].tobytes() == s.tobytes(), (e, recs["if_rms"][e - 1], s)
    return recs, pcm, alen, has_if


def test_fm_stereo_fused_front_end_one_call_and_ragged_calls():
    """10 MS/s behind the fused front end: one call of 7 x 65536, and the same input in ragged calls (blocks without IF
    samples, blocks with IF samples and no audio).  Each cut against its own audio; the integer fields across the cuts."""
    one, pcm1, _, _ = run10(ONE, True)
    assert one["gate_open"].tolist() == [int(a == HI) for a in AMPS7] and one["block"].tolist() == list(range(7))
    # (the first block's audio is short by the audio filters' delay)
    assert np.all(one["n_frames"][1:] >= 314) and np.all(one["n_frames"] <= 315) and one["n_frames"][0] > 200 and one["n_clipped"].sum() == 0
    rag, pcm2, alen, has_if = run10(RAGGED, True)
    lens = [b for c in RAGGED for b in c]
    assert not all(has_if) and np.any(rag["n_frames"] == 0) and len(rag) == sum(has_if) < len(lens)
    assert rag["block"].tolist() == [b for b, h in enumerate(has_if) if h]
    region = np.cumsum([0] + lens)[rag["block"].astype(np.int64)] // BLK
    for g in range(7):      # frames and gate per 65536-region: the same in both cuts
        sel = region == g
        assert rag["n_frames"][sel].sum() == one["n_frames"][g] and np.all(rag["gate_open"][sel] == one["gate_open"][g]), g
    assert len(pcm1) == len(pcm2) == one["n_frames"].sum()
    closed = np.repeat(one["gate_open"] == 0, one["n_frames"])
    assert not pcm1[closed].any() and not pcm2[closed].any() and pcm1[~closed].any(axis=1).mean() > 0.9


def test_three_kernel_front_end(monkeypatch):
    monkeypatch.setenv("FMR_NO_FUSED", "1")
    recs, _, _, _ = run10(ONE, False)
    assert recs["gate_open"].tolist() == [int(a == HI) for a in AMPS7]


@pytest.mark.parametrize("mode", ["nbfm", "am"])
def test_nbfm_and_am_at_48k(mode, nbfm_default, nbfm_audio, am_narrow):
    """No resampler, 2048-sample blocks, 12 blocks in two calls, the squelch closing in the middle (the IF RMS of these
    modes is taken behind the IF filter: the early step keeps its tail out of the weak blocks)."""
    blk, amps, lead = 2048, [HI] * 4 + [LO] * 4 + [HI] * 4, 512
    assert lead > max(len(nbfm_default), len(am_narrow))
    n = 12 * blk
    if mode == "nbfm":
        x = stepped(siggen.nbfm_iq(n, 48e3, level=1.0, sigma=0.0), amps, blk, lead, 1e-4)
        ch = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                       nbfm_freq_dev=8000.0, max_block_len=blk, max_blocks=8)
        dec = ora.NbfmDecoder(nbfm_default, 8000.0, nbfm_audio)
    else:
        x = stepped(siggen.am_iq(n, 48e3, level=1.0, sigma=0.0), amps, blk, lead, 1e-4)
        ch = fmr.Chain(mode=fmr.MODE_AM, input_rate=48e3, filter_coeff=am_narrow, max_block_len=blk, max_blocks=8)
        dec = ora.AmDecoder(am_narrow, ora.MODE_AM)
    ch.enable_output(squelch_level=LEVEL)
    audio, alen, st = feed(ch, x, [[blk] * 5, [blk] * 7])
    recs, pcm = check(ch, 0, audio[0], alen, [True] * 12, 1)
    ch.close()
    ref_rms = []
    for b in siggen.blocks(x, blk):
        dec.process(b)
        ref_rms.append(dec.get_if_rms())
    assert np.allclose(recs["if_rms"], ref_rms, rtol=1e-5, atol=0), (recs["if_rms"], ref_rms)   # tests/test_gpu_parity.py:342,473
    assert recs["gate_open"].tolist() == [1] * 4 + [0] * 4 + [1] * 4 and recs["n_frames"].tolist() == [blk] * 12
    assert recs["if_rms"][4].tobytes() == st[0].tobytes() and recs["if_rms"][11].tobytes() == st[1].tobytes()
    assert not pcm[4 * blk:8 * blk].any() and pcm[:4 * blk].any() and pcm[8 * blk:].any()


def chain384(stereo=True, max_blocks=8, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=384e3, enable_resampler=False, stereo=stereo, max_block_len=16384,
                     max_blocks=max_blocks, **kw)


@pytest.mark.parametrize("stereo,fmt", [(False, "s16"), (False, "f32"), (True, "f32")])
def test_mono_chain_and_f32(stereo, fmt):
    """stereo = 0 (channels = 1) and the F32 format, at 384 kHz (no resampler: a block's if_rms is its own samples')."""
    blk, amps = 16384, [HI, LO, HI, HI, LO, LO]
    calls = [[blk, 1000, blk - 1000], [blk], [1, 2, blk - 3], [blk, blk]]
    x = stepped(siggen.fm_stereo_iq(6 * blk, 384e3, amplitude=1.0, sigma=0.0), amps, blk, 0, 1e-3)
    ch = chain384(stereo=stereo)
    ch.enable_output(format=fmt, squelch_level=LEVEL)
    audio, alen, _ = feed(ch, x, calls)
    nch, f = (2 if stereo else 1), (of.PCM_F32 if fmt == "f32" else of.PCM_S16)
    recs, pcm = check(ch, 0, audio[0], alen, [True] * len(alen), nch, fmt=f)
    ch.close()
    assert pcm.dtype == (np.float32 if fmt == "f32" else np.int16) and pcm.shape == (len(audio[0]) // nch, nch)
    assert np.all(recs["channels"] == nch) and np.any(recs["n_frames"] == 0) and sorted(set(recs["gate_open"].tolist())) == [0, 1]


def test_two_channel_bank():
    """A two-channel bank at 2.5 MS/s with unlike amplitudes: one channel squelched, the other open, in the same blocks."""
    F, blk, offs = 2.5e6, 16384, [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 4, [7]]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 4], [HI, LO])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                   channel_offsets_hz=offs)
    ch.enable_output(squelch_level=LEVEL)
    audio, alen, _ = feed(ch, x, calls)
    lens = [b for c in calls for b in c]
    has_if = [n > 0 for n in oracle_if(x, lens, F, decode=False)[0]]       # (the count law knows no offsets)
    got = [check(ch, s, audio[s], alen, has_if, 2) for s in range(2)]
    ch.close()
    assert np.all(got[0][0]["gate_open"] == 1) and np.all(got[1][0]["gate_open"] == 0)
    assert got[0][1].any() and not got[1][1].any() and len(got[0][1]) == len(got[1][1]) > 2000
    for k in ("block", "first_frame", "n_frames"):
        assert np.array_equal(got[0][0][k], got[1][0][k])


@pytest.mark.parametrize("calls", [[[BLK]] * 7, ONE], ids=["seven_calls", "one_call_longer_than_the_ring"])
def test_ring_overrun(calls):
    """max_frames = 1024 under 7 x 315 frames and max_blocks = 4 under 7 records, read once at the end."""
    x = fm10()
    ch = chain10()
    ch.enable_output(squelch_level=LEVEL, max_frames=1024, max_blocks=4)
    audio, alen, _ = feed(ch, x, calls)
    total = len(audio[0]) // 2
    _, _, info = ch.output_read(0, cap_frames=0, cap_blocks=0)
    first, dropped = of.ring_window(total, 1024)
    assert (info["frames_waiting"], info["frames_dropped"], info["first_frame"]) == (1024, dropped, first) and total > 2 * 1024
    assert (info["blocks_waiting"], info["blocks_dropped"]) == (4, 3)
    pcm, recs, info = ch.output_read(0)
    assert info["first_frame"] == total - 1024 and info["frames_waiting"] == 0 and info["frames_dropped"] == total - 1024
    # the oracle needs all seven if_rms: the three dropped records' from a second chain that keeps them
    full = chain10()
    full.enable_output(squelch_level=LEVEL)
    audio2, _, _ = feed(full, x, calls)
    pcm_all, recs_all, _ = full.output_read(0)
    full.close()
    assert same_bits(audio, audio2)
    ref, ref_pcm = oracle(recs_all, audio[0], alen, [True] * 7, 2)
    compare(recs_all, pcm_all, ref, ref_pcm)
    compare(recs, pcm, ref[-4:], ref_pcm[-1024:])
    # the ring goes on: one more block, read in two pieces
    a3, al3, _ = feed(ch, x[:BLK], [[BLK]])
    p1, r1, i1 = ch.output_read(0, cap_frames=100, cap_blocks=0)
    p2, r2, i2 = ch.output_read(0)
    ch.close()
    assert len(p1) == 100 and len(r1) == 0 and i1["first_frame"] == total and i1["frames_waiting"] == len(a3[0]) // 2 - 100
    assert i2["first_frame"] == total + 100 and len(r2) == 1 and r2["block"][0] == 7 and r2["first_frame"][0] == total
    assert i2["frames_dropped"] == total - 1024 and i2["blocks_dropped"] == 3
    y = a3[0] * (0.5 if r2["gate_open"][0] else 0.0)
    assert same_bits(np.concatenate([p1, p2]), of.to_s16(y)[0].reshape(-1, 2))


def test_pipelined_against_in_order():
    """Four asynchronous device calls of 2 x 65536 at 10 MS/s (pipelined: the tail runs a call late) and one
    fmr_synchronize, against the in_order chain: records and PCM bit for bit, and against the oracle on the audio in the
    device buffers."""
    import torch
    per = 2
    x = np.concatenate([fm10(), fm10()[:BLK]])
    kw = dict(mode=fmr.MODE_FM, input_rate=F10, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_output(squelch_level=LEVEL)
    audio, alen, _ = feed(ref_ch, x, [[BLK] * per] * 4)
    ref_recs, ref_pcm = check(ref_ch, 0, audio[0], alen, [True] * 8, 2)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_output(squelch_level=LEVEL)
    stride = 2 * 2048
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(4 * stride, dtype=torch.float64, device="cuda")
    al = []
    for i in range(4):
        al += [int(v) for v in ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * BLK, len(x), [BLK] * per,
                                                         d_a.data_ptr() + 8 * i * stride, stride, sync=False)]
    ch.synchronize()
    pcm, recs, info = ch.output_read(0)
    ch.close()
    assert al == alen and info["frames_dropped"] == 0
    h_a = d_a.cpu().numpy()
    dev_audio = np.concatenate([h_a[i * stride:i * stride + sum(al[per * i:per * i + per])] for i in range(4)])
    ref2, ref2_pcm = oracle(recs, dev_audio, al, [True] * 8, 2)
    compare(recs, pcm, ref2, ref2_pcm)
    for k in BIT_FIELDS:
        assert same_bits(recs[k], ref_recs[k]), k
    assert same_bits(pcm, ref_pcm)


def test_nothing_else_moves():
    """Audio, fmr_status, PPS events, RDS groups and the records of all three monitors are bit-identical with the stage
    on and off; a chain without it runs none of its kernels."""
    F, blk = 10e6, 65536
    n = 10 * blk * 16
    groups = rf.ps_groups(0xA0D1, "SQUELCH!", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    x = rf.fm_iq(rf.station_mpx(t, groups), F).astype(np.complex64)
    outs = []
    for on in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_loudness()
        ch.enable_rf_monitor()
        if on:
            ch.enable_output(squelch_level=LEVEL)
        ch.enable_kernel_timing(1)
        audio, alen, pps, names = [], [], [], set()
        for pos in range(0, n, 8 * blk):
            a, al = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            alen += [int(v) for v in al]
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        outs.append((np.concatenate(audio, axis=1), bytes(ch.status(0)), pps, ch.rds_groups(0), names,
                     ch.monitor_records(0)[:3], ch.loudness_records(0)[:1], ch.rf_monitor_records(0)[:3],
                     ch.output_read(0) if on else None, alen))
        ch.close()
    assert same_bits(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert len(outs[0][3]) >= 3 and same_bits(outs[0][3], outs[1][3])
    for m in (5, 6, 7):
        assert len(outs[0][m][0]) >= 4
        for a, b in zip(outs[0][m], outs[1][m]):
            assert same_bits(a, b), m
    assert not any(k.startswith("out_") for k in outs[0][4]) and {"out_pcm", "out_blocks"} <= outs[1][4]
    pcm, recs, _ = outs[1][8]
    ref, ref_pcm = oracle(recs, outs[1][0][0], outs[1][9], [True] * len(outs[1][9]), 2)
    compare(recs, pcm, ref, ref_pcm, level=0.0)            # (a steady carrier: the factor-3 rule has nothing to say)
    assert len(recs) == 160 and np.all(recs["gate_open"] == 1)


def test_clipping_at_gain_one():
    """gain = 1.0 on an over-deviated station (150 kHz peak: the audio reaches about 1.9): the exact count of saturated
    samples."""
    blk = 16384
    x = siggen.fm_mono_iq(4 * blk, 384e3, dev=150000.0)
    ch = chain384()
    ch.enable_output(gain=1.0)
    audio, alen, _ = feed(ch, x, [[blk] * 4])
    assert np.abs(audio[0]).max() > 1.2
    recs, pcm = check(ch, 0, audio[0], alen, [True] * 4, 2, level=0.0, gain=1.0)
    ch.close()
    r = np.rint(audio[0] * 32767.0)
    want = int(np.sum(r > 32767.0) + np.sum(r < -32768.0))
    print("n_clipped:", recs["n_clipped"].tolist())
    assert recs["n_clipped"].sum() == want > 1000 and np.all(recs["gate_open"] == 1)
    assert pcm.max() == 32767 and pcm.min() == -32768


def test_refusals_with_a_device():
    fe = fmr.Channelizer(2.5e6, [-700_000, 250_000], max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_output()
    fe.close()
    fe = fmr.Chain(mode=fmr.MODE_NONE, input_rate=10e6, enable_resampler=True, max_block_len=16384)
    with pytest.raises(fmr.FmrError, match=r"error -3.*front-end-only"):
        fe.enable_output()
    fe.close()
    ch = chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no output stage"):
        ch.output_read(0)
    ch.enable_output()
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_output()
    with pytest.raises(fmr.FmrError, match=r"error -2.*stream"):
        ch.output_read(1)
    L = ch._L
    assert L.fmr_output_read(ch.h, 0, None, 16, None, 0, None, None, 0) == fmr.ERR_BAD_ARG and "pcm is null" in L.fmr_last_error().decode()
    pcm, recs, info = ch.output_read(0)
    assert len(pcm) == 0 and len(recs) == 0 and info["frames_waiting"] == 0 and info["first_frame"] == 0
    ch.close()
    ch = chain384()
    ch.process_blocks(siggen.fm_stereo_iq(4096, 384e3)[None, :], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_output()
    ch.close()


def test_facade_smoke(tmp_path):
    """tests/output_smoke.cpp through the facade: FmDecoder, NbfmDecoder, AmDecoder and a two-channel ChannelBank."""
    exe = str(tmp_path / "output_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "output_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe, str(tmp_path / "out.wav")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("fm frames", "nbfm frames", "am frames", "bank0 frames", "bank1 frames", "wav bytes"):
        assert tag in r.stdout, r.stdout

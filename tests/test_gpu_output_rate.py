"""Output stage at other rates and mono on the GPU (fmr_set_output_rate): the PCM ring, the stream totals and the block
records of a chain against tests/output_rate_fixture.py run on the audio the chain itself returned and on the if_rms its
records carry, with the library's exported taps -- the method and the helpers of tests/test_gpu_output.py.  Stage and
oracle see the same doubles and add in the same order: every PCM sample, both totals and every field of every record
must be equal bit for bit, and the ring must have received ceil(F L / M) frames."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import output_fixture as of
import output_rate_fixture as orf
import rds_fixture as rf
import siggen
import test_gpu_output as tg
from conftest import ROOT
from test_gpu_output import BLK, F10, HI, LEVEL, LO, ONE, RAGGED, same_bits

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

_taps = {}


def taps(rate):
    if rate not in _taps:
        _taps[rate] = fmr.output_rate_taps(rate)
    return _taps[rate]


def blocks_of(recs, audio, alen, has_if):
    """(if_rms, audio) per block handed in, as the fixtures take them: the if_rms of the records."""
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
    return blocks


def rate_oracle(recs, audio, alen, has_if, nch, rate, mono, level=LEVEL, gain=0.5, fmt=of.PCM_S16):
    h, L, M, T = taps(rate)
    return orf.run(blocks_of(recs, audio, alen, has_if), nch, level, gain, fmt, L, M, T, h, mono)


def compare(recs, pcm, ref, ref_pcm, level=LEVEL):
    """tests/test_gpu_output.py's compare, and then every record field bit for bit."""
    tg.compare(recs, pcm, ref, ref_pcm, level)
    assert same_bits(recs, ref.astype(recs.dtype)), [k for k in ref.dtype.names if not same_bits(recs[k], ref[k])]


def check(ch, stream, audio, alen, has_if, nch, rate, mono, level=LEVEL, gain=0.5, fmt=of.PCM_S16):
    """Drains `stream` and holds ring, records, totals and both infos against the fixture."""
    pcm, recs, info = ch.output_read(stream)
    ri = ch.output_rate_info(stream)
    ref, ref_pcm, cl, nf = rate_oracle(recs, audio, alen, has_if, nch, rate, mono, level, gain, fmt)
    compare(recs, pcm, ref, ref_pcm, level)
    h, L, M, T = taps(rate)
    och = 1 if mono else nch
    F = len(audio) // nch
    print("frames in", F, "ring frames", len(pcm), "totals", ri["pcm_clipped"], ri["pcm_nonfinite"])
    assert len(pcm) == -(-F * L // M) and pcm.shape[1] == och
    assert (ri["pcm_clipped"], ri["pcm_nonfinite"]) == (cl, nf)
    assert (ri["rate"], ri["channels"], ri["L"], ri["M"], ri["taps_per_phase"], ri["frames_in"]) == (rate, och, L, M, T, F)
    assert ri["delay_frames"] == ((T * L - 1) / (2.0 * M) if T > 1 else 0.0)
    assert info["frames_dropped"] == 0 and info["blocks_dropped"] == 0 and info["frames_waiting"] == 0 and info["blocks_waiting"] == 0
    assert info["first_frame"] == 0 and info["channels"] == och and info["format"] == fmt
    # the header's mapping: the ring frames made from block k start at ceil(first_frame L / M)
    assert [fmr.output_frame_of(f, rate) for f in recs["first_frame"][:4]] == [-(-int(f) * L // M) for f in recs["first_frame"][:4]]
    return recs, pcm


@pytest.mark.parametrize("calls,rate,fmt,mono", [(RAGGED, 8000, "s16", False), (ONE, 44100, "s16", False), (RAGGED, 32000, "f32", True)],
                         ids=["8000_s16_ragged", "44100_s16_one_call", "32000_f32_mono_ragged"])
def test_fm_stereo_at_10_msps(calls, rate, fmt, mono):
    """7 x 65536 at 10 MS/s with the stepped carrier.  RAGGED: T - 1 = 853 frames of history exceed a block's 315 frames and
    whole calls, and there are blocks without IF samples and blocks with IF samples and no audio.  44100: 147 phases."""
    x = tg.fm10()
    lens = [b for c in calls for b in c]
    has_if = [n > 0 for n in tg.oracle_if(x, lens, decode=False)[0]]
    ch = tg.chain10(max_blocks=max(len(c) for c in calls))
    ch.enable_output(format=fmt, squelch_level=LEVEL, rate=rate, mono=mono)
    audio, alen, _ = tg.feed(ch, x, calls)
    recs, pcm = check(ch, 0, audio[0], alen, has_if, 2, rate, mono, fmt=of.PCM_F32 if fmt == "f32" else of.PCM_S16)
    ch.close()
    T = taps(rate)[3]
    assert sorted(set(recs["gate_open"].tolist())) == [0, 1] and pcm.any()
    if calls is RAGGED:
        assert np.any(recs["n_frames"] == 0) and not all(has_if)
    if rate == 8000:      # the history is longer than any block and than whole calls
        per_call = [sum(alen[sum(map(len, calls[:i])):sum(map(len, calls[:i + 1]))]) // 2 for i in range(len(calls))]
        assert T - 1 > recs["n_frames"].max() and min(per_call) < T - 1, per_call


CALLS384 = [[16384, 1000, 16384 - 1000], [16384], [1, 2, 16384 - 3], [16384, 16384]]


def x384():
    if "x384" not in tg._cache:
        tg._cache["x384"] = tg.stepped(siggen.fm_stereo_iq(6 * 16384, 384e3, amplitude=1.0, sigma=0.0), [HI, LO, HI, HI, LO, LO],
                                       16384, 0, 1e-3)
    return tg._cache["x384"]


@pytest.mark.parametrize("stereo,rate,mono", [(True, 16000, True), (False, 16000, True), (True, 48000, True)],
                         ids=["stereo_chain_mono_16000", "mono_chain_mono_ignored", "downmix_without_a_filter"])
def test_chain384_mono(stereo, rate, mono):
    ch = tg.chain384(stereo=stereo)
    ch.enable_output(format="f32", squelch_level=LEVEL, rate=rate, mono=mono)
    audio, alen, _ = tg.feed(ch, x384(), CALLS384)
    nch = 2 if stereo else 1
    recs, pcm = check(ch, 0, audio[0], alen, [True] * len(alen), nch, rate, mono and stereo, fmt=of.PCM_F32)
    ch.close()
    assert pcm.shape[1] == 1 and np.all(recs["channels"] == nch) and np.any(recs["n_frames"] == 0)
    assert sorted(set(recs["gate_open"].tolist())) == [0, 1]


def test_rate_48000_stereo_leaves_the_stage_as_it_is():
    """rate = 48000, mono = 0: the bytes of a chain that never called the new entry, from the same kernels."""
    got = []
    for call in (False, True):
        ch = tg.chain384()
        ch.enable_output(squelch_level=LEVEL)
        if call:
            ch.set_output_rate(48000, False)
        ch.enable_kernel_timing(1)
        audio, alen, _ = tg.feed(ch, x384(), CALLS384)
        names = {k for k, _ in ch.kernel_times()}
        ri = ch.output_rate_info(0)
        pcm, recs, info = ch.output_read(0)
        ch.close()
        got.append((audio, pcm, recs, info, names))
        assert (ri["rate"], ri["channels"], ri["L"], ri["M"], ri["delay_frames"], ri["frames_in"]) == (48000, 2, 1, 1, 0.0, len(pcm))
        assert "out_pcm" in names and not names & {"out_rate", "out_z", "out_hist"}
    for a, b in zip(got[0][:3], got[1][:3]):
        assert same_bits(a, b)
    assert got[0][3] == got[1][3] and got[0][1].any()


@pytest.mark.parametrize("rate", [16000, 8000])
@pytest.mark.parametrize("mode", ["nbfm", "am"])
def test_nbfm_and_am_at_48k(mode, rate, nbfm_default, nbfm_audio, am_narrow):
    """12 x 2048 in two calls, the squelch closing in the middle: the closed stretch is exactly zero T frames after it
    begins."""
    blk, amps, lead = 2048, [HI] * 4 + [LO] * 4 + [HI] * 4, 512
    n = 12 * blk
    if mode == "nbfm":
        x = tg.stepped(siggen.nbfm_iq(n, 48e3, level=1.0, sigma=0.0), amps, blk, lead, 1e-4)
        ch = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                       nbfm_freq_dev=8000.0, max_block_len=blk, max_blocks=8)
    else:
        x = tg.stepped(siggen.am_iq(n, 48e3, level=1.0, sigma=0.0), amps, blk, lead, 1e-4)
        ch = fmr.Chain(mode=fmr.MODE_AM, input_rate=48e3, filter_coeff=am_narrow, max_block_len=blk, max_blocks=8)
    ch.enable_output(squelch_level=LEVEL, rate=rate)
    audio, alen, _ = tg.feed(ch, x, [[blk] * 5, [blk] * 7])
    recs, pcm = check(ch, 0, audio[0], alen, [True] * 12, 1, rate, False)
    ch.close()
    _, L, M, T = taps(rate)
    assert recs["gate_open"].tolist() == [1] * 4 + [0] * 4 + [1] * 4 and recs["n_frames"].tolist() == [blk] * 12 and T < 4 * blk
    q = (np.arange(len(pcm)) * M) // L
    silent = (q - (T - 1) >= 4 * blk) & (q < 8 * blk)
    assert silent.sum() > 100 and pcm[silent].tobytes() == bytes(pcm[silent].nbytes)
    assert pcm[q < 4 * blk].any() and pcm[q >= 8 * blk].any() and pcm[(q >= 4 * blk) & (q < 4 * blk + T // 2)].any()


def test_two_channel_bank():
    """tests/test_gpu_output.py::test_two_channel_bank's input at 16000 mono: one channel open, the other all zeros."""
    F, blk, offs = 2.5e6, 16384, [-700_000, 250_000]
    calls = [[blk] * 5, [blk, 1000], [blk] * 4, [7]]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 4], [HI, LO])
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                   channel_offsets_hz=offs)
    ch.enable_output(squelch_level=LEVEL, rate=16000, mono=True)
    audio, alen, _ = tg.feed(ch, x, calls)
    lens = [b for c in calls for b in c]
    has_if = [n > 0 for n in tg.oracle_if(x, lens, F, decode=False)[0]]
    got = [check(ch, s, audio[s], alen, has_if, 2, 16000, True) for s in range(2)]
    ch.close()
    assert np.all(got[0][0]["gate_open"] == 1) and np.all(got[1][0]["gate_open"] == 0)
    assert got[0][1].any() and not got[1][1].any() and len(got[0][1]) == len(got[1][1]) > 600


@pytest.mark.parametrize("calls", [[[BLK]] * 7, ONE], ids=["seven_calls", "one_call_longer_than_the_ring"])
def test_ring_overrun(calls):
    """max_frames = 256 at 8000 Hz under 7 x 315 decoder frames (about 367 ring frames), read once at the end; then one
    more block read in two pieces."""
    x = tg.fm10()
    rate, depth = 8000, 256
    _, L, M, T = taps(rate)
    ch = tg.chain10()
    ch.enable_output(squelch_level=LEVEL, max_frames=depth, rate=rate)
    audio, alen, _ = tg.feed(ch, x, calls)
    F = len(audio[0]) // 2
    total = -(-F * L // M)
    _, _, info = ch.output_read(0, cap_frames=0, cap_blocks=0)
    first, dropped = of.ring_window(total, depth)
    assert total > depth and (info["frames_waiting"], info["frames_dropped"], info["first_frame"]) == (depth, dropped, first)
    pcm, recs, info = ch.output_read(0)
    assert info["first_frame"] == total - depth and info["frames_waiting"] == 0 and info["frames_dropped"] == total - depth
    assert len(recs) == 7 and len(pcm) == depth
    a3, al3, _ = tg.feed(ch, x[:BLK], [[BLK]])
    F2 = F + len(a3[0]) // 2
    total2 = -(-F2 * L // M)
    p1, r1, i1 = ch.output_read(0, cap_frames=20, cap_blocks=0)
    p2, r2, i2 = ch.output_read(0)
    ri = ch.output_rate_info(0)
    ch.close()
    assert len(p1) == 20 and len(r1) == 0 and i1["first_frame"] == total and i1["frames_waiting"] == total2 - total - 20
    assert i2["first_frame"] == total + 20 and len(r2) == 1 and r2["block"][0] == 7 and r2["first_frame"][0] == F
    assert i2["frames_dropped"] == total - depth and i2["blocks_dropped"] == 0 and 20 < total2 - total <= depth
    # the oracle on all eight blocks: the ring's window of the first seven, then the eighth's frames whole
    recs_all = np.concatenate([recs, r2])
    audio_all = np.concatenate([audio[0], a3[0]])
    ref, ref_pcm, cl, nf = rate_oracle(recs_all, audio_all, alen + al3, [True] * 8, 2, rate, False)
    compare(recs_all, np.concatenate([pcm, p1, p2]), ref, ref_pcm[total - depth:])
    assert len(ref_pcm) == total2 and (ri["pcm_clipped"], ri["pcm_nonfinite"], ri["frames_in"]) == (cl, nf, F2)


def test_pipelined_against_in_order():
    """Four asynchronous device calls of 2 x 65536 at 10 MS/s (pipelined: the tail runs a call late) and one
    fmr_synchronize, against the in_order chain, at 44100: records, PCM and totals bit for bit, and against the oracle on
    the audio in the device buffers."""
    import torch
    per, rate = 2, 44100
    x = np.concatenate([tg.fm10(), tg.fm10()[:BLK]])
    kw = dict(mode=fmr.MODE_FM, input_rate=F10, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_output(squelch_level=LEVEL, rate=rate)
    audio, alen, _ = tg.feed(ref_ch, x, [[BLK] * per] * 4)
    ref_ri = ref_ch.output_rate_info(0)
    ref_recs, ref_pcm = check(ref_ch, 0, audio[0], alen, [True] * 8, 2, rate, False)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_output(squelch_level=LEVEL, rate=rate)
    stride = 2 * 2048
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(4 * stride, dtype=torch.float64, device="cuda")
    al = []
    for i in range(4):
        al += [int(v) for v in ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * BLK, len(x), [BLK] * per,
                                                         d_a.data_ptr() + 8 * i * stride, stride, sync=False)]
    ch.synchronize()
    ri = ch.output_rate_info(0)
    pcm, recs, info = ch.output_read(0)
    ch.close()
    assert al == alen and info["frames_dropped"] == 0 and ri == ref_ri
    h_a = d_a.cpu().numpy()
    dev_audio = np.concatenate([h_a[i * stride:i * stride + sum(al[per * i:per * i + per])] for i in range(4)])
    ref2, ref2_pcm, cl, nf = rate_oracle(recs, dev_audio, al, [True] * 8, 2, rate, False)
    compare(recs, pcm, ref2, ref2_pcm)
    assert same_bits(recs, ref_recs) and same_bits(pcm, ref_pcm) and (ri["pcm_clipped"], ri["pcm_nonfinite"]) == (cl, nf)


def test_nothing_else_moves():
    """Audio, fmr_status, PPS events, RDS groups, the three monitors' records and the output records are bit-identical with
    and without fmr_set_output_rate; out_rate is absent from the kernel names without it."""
    F, blk = 10e6, 65536
    n = 10 * blk * 16
    groups = rf.ps_groups(0xA0D1, "RATE16K!", n=int(n / F / (104 * rf.TD)) + 2)
    t = np.arange(n, dtype=np.float64) / F
    x = rf.fm_iq(rf.station_mpx(t, groups), F).astype(np.complex64)
    outs = []
    for on in (False, True):
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=8,
                       enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_loudness()
        ch.enable_rf_monitor()
        ch.enable_output(squelch_level=LEVEL, **({"rate": 16000, "mono": True} if on else {}))
        ch.enable_kernel_timing(1)
        audio, alen, pps, names = [], [], [], set()
        for pos in range(0, n, 8 * blk):
            a, al = ch.process_blocks(x[None, pos:pos + 8 * blk], [blk] * 8)
            audio.append(a)
            alen += [int(v) for v in al]
            pps += ch.pps_events(0)
            names |= {k for k, _ in ch.kernel_times()}
        ri = ch.output_rate_info(0)
        pcm, recs, _ = ch.output_read(0)
        outs.append((np.concatenate(audio, axis=1), bytes(ch.status(0)), pps, ch.rds_groups(0), recs,
                     ch.monitor_records(0)[:3], ch.loudness_records(0)[:1], ch.rf_monitor_records(0)[:3], names, pcm, alen, ri))
        ch.close()
    assert same_bits(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
    assert len(outs[0][3]) >= 3 and same_bits(outs[0][3], outs[1][3])
    assert len(outs[0][4]) == 160 and same_bits(outs[0][4], outs[1][4])
    for m in (5, 6, 7):
        assert len(outs[0][m][0]) >= 4
        for a, b in zip(outs[0][m], outs[1][m]):
            assert same_bits(a, b), m
    assert not outs[0][8] & {"out_rate", "out_z", "out_hist"} and {"out_pcm", "out_blocks", "out_rate", "out_z", "out_hist"} <= outs[1][8]
    audio, alen, recs, pcm, ri = outs[1][0][0], outs[1][10], outs[1][4], outs[1][9], outs[1][11]
    ref, ref_pcm, cl, nf = rate_oracle(recs, audio, alen, [True] * len(alen), 2, 16000, True, level=LEVEL)
    compare(recs, pcm, ref, ref_pcm, level=0.0)
    assert (ri["pcm_clipped"], ri["pcm_nonfinite"]) == (cl, nf) and len(pcm) == -(-(len(audio) // 2) // 3)


def test_clipping_at_gain_one():
    """gain = 1.0 on the over-deviated station of tests/test_gpu_output.py::test_clipping_at_gain_one, at 32000: the
    fixture's count of saturated ring samples, and both rails."""
    blk = 16384
    x = siggen.fm_mono_iq(4 * blk, 384e3, dev=150000.0)
    ch = tg.chain384()
    ch.enable_output(gain=1.0, rate=32000)
    audio, alen, _ = tg.feed(ch, x, [[blk] * 4])
    assert np.abs(audio[0]).max() > 1.2
    ri = ch.output_rate_info(0)
    recs, pcm = check(ch, 0, audio[0], alen, [True] * 4, 2, 32000, False, level=0.0, gain=1.0)
    ch.close()
    print("pcm_clipped:", ri["pcm_clipped"], "n_clipped of the records:", recs["n_clipped"].tolist())
    assert ri["pcm_clipped"] > 0 and pcm.max() == 32767 and pcm.min() == -32768 and np.all(recs["gate_open"] == 1)


def test_refusals_with_a_device():
    ch = tg.chain384()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no output stage"):
        ch.set_output_rate(16000)
    with pytest.raises(fmr.FmrError, match=r"error -2.*no output stage"):
        ch.output_rate_info(0)
    ch.enable_output()
    with pytest.raises(fmr.FmrError, match=r"error -2.*rate"):
        ch.set_output_rate(8001)
    ch.set_output_rate(16000, True)
    with pytest.raises(fmr.FmrError, match=r"error -2.*already set"):
        ch.set_output_rate(16000, True)
    with pytest.raises(fmr.FmrError, match=r"error -2.*stream"):
        ch.output_rate_info(1)
    with pytest.raises(fmr.FmrError, match=r"error -2.*stream"):
        ch.output_rate_info(-1)
    ri = ch.output_rate_info(0)
    assert (ri["rate"], ri["channels"], ri["L"], ri["M"], ri["taps_per_phase"], ri["frames_in"]) == (16000, 1, 1, 3, 428, 0)
    pcm, recs, info = ch.output_read(0)
    assert pcm.shape == (0, 1) and len(recs) == 0 and info["channels"] == 1
    ch.close()
    ch = tg.chain384()
    ch.enable_output()
    ch.process_blocks(siggen.fm_stereo_iq(4096, 384e3)[None, :], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.set_output_rate(16000)
    ch.close()
    ch = tg.chain384()
    ch.enable_output()
    ch.set_output_rate(0, False)                 # accepted, and counts as the one call
    with pytest.raises(fmr.FmrError, match=r"error -2.*already set"):
        ch.set_output_rate(16000)
    ch.close()


def test_facade_smoke(tmp_path):
    """tests/output_rate_smoke.cpp through the facade: FmDecoder (16 kHz mono F32), NbfmDecoder (8 kHz) and a two-channel
    ChannelBank (44.1 kHz)."""
    exe = str(tmp_path / "output_rate_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "output_rate_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe, str(tmp_path / "out.wav")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("fm frames", "nbfm frames", "bank0 frames", "bank1 frames", "wav bytes"):
        assert tag in r.stdout, r.stdout

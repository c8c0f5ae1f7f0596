"""Output stage at the call shape it is built for: more than 64 blocks per call (k_out_blocks walks a call's blocks 64 at
a time and carries if_level, audio_level and the record counter from group to group), more than 384 behind b_first (k_stats
takes a second load) and more than 400 blocks with IF samples (the blocks in front of k_stats's b_first get their IF RMS
from a loop of their own).  The method and the helpers are those of tests/test_gpu_output.py and tests/test_gpu_output_rate.py: the
fixtures run on the audio the chain returned and on the if_rms of its records; every PCM sample, every integer and level
field of every record and both stream totals bit for bit, audio_rms / audio_mean within one float32 ulp, if_rms against
the oracle decoders at rtol = 1e-5 (tests/test_gpu_parity.py:170, 342, 473).

Inputs: the carrier alternates between 0.3 and 0.003 over regions whose edges lie at the lanes 63 | 64 | 65 of the first
group of 64 and at the blocks 382 | 383 | 384; squelch_level = 0.03.  k_stats loads 384 blocks at a time from b_first on:
in a call of 450 blocks (b_first = 0) the second load begins at block 384, on that edge; in the calls of 520 and 470
blocks (b_first = 64) it begins at block 448, two blocks in front of the edge at 450, and no gate changes there -- the
second load is then held by every block's if_rms against the oracle and by the status.  With these block lengths and
leads the oracle decoders give exactly that gate pattern and no block's IF RMS within a factor 3 of the level (every test
asserts both on its records, which are held to the oracle's if_rms).

Every test prints what it covered (blocks per call, front-end forms, blocks in front of b_first, gate pattern) and
asserts that it reached the path it is there for."""
import importlib

import numpy as np
import pytest

import oracle_py as ora
import output_fixture as of
import siggen
import test_gpu_output as tg
import test_gpu_output_rate as tr
from test_gpu_output import BIT_FIELDS, BLK, F10, HI, LEVEL, LO, RAGGED, feed, oracle, oracle_if, same_bits, stepped

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

BLK10, LEAD10 = 4608, 2304      # (4096-sample blocks: the first has 116 IF samples, and the call falls off the tiled forms)
BLK48, LEAD48 = 512, 256
EDGES520 = [0, 60, 64, 65, 130, 383, 384, 450, 520]
EDGES470 = [0, 60, 64, 65, 130, 383, 384, 450, 470]


def amps_of(edges):
    """HI and LO in turn over the regions between the edges, HI first."""
    return [a for i in range(len(edges) - 1) for a in [HI if i % 2 == 0 else LO] * (edges[i + 1] - edges[i])]


def gates_of(amps):
    return [int(a == HI) for a in amps]


AMPS130 = amps_of(EDGES520[:5])
AMPS541 = amps_of(EDGES520) + [HI] * 21             # (the 3-block call reopens the gate; the ring overrun takes 21 blocks)
AMPS523 = AMPS541[:523]
AMPS600 = amps_of(EDGES470) + AMPS130               # (the calls of 65 start the pattern again)
GATES520, GATES523, GATES600 = gates_of(AMPS523[:520]), gates_of(AMPS523), gates_of(AMPS600)


def cached(key, make):
    if key not in tg._cache:
        tg._cache[key] = make()
    return tg._cache[key]


def fm541():
    """541 x 4608 samples of FM stereo at 10 MS/s, stepped (the tests but one take the first 520 or 523 blocks)."""
    return cached("fm541", lambda: stepped(siggen.fm_stereo_iq(541 * BLK10, F10, amplitude=1.0, sigma=0.0), AMPS541, BLK10, LEAD10, 1e-3))


def nbfm600():
    return cached("nbfm600", lambda: stepped(siggen.nbfm_iq(600 * BLK48, 48e3, level=1.0, sigma=0.0), AMPS600, BLK48, LEAD48, 1e-4))


def am600():
    return cached("am600", lambda: stepped(siggen.am_iq(600 * BLK48, 48e3, level=1.0, sigma=0.0), AMPS600, BLK48, LEAD48, 1e-4))


def fm384x3():
    """260 x 2048 at 384 kHz, three rows: the strong, the weak and the stepped carrier (twice the first 130 blocks' pattern)."""
    def make():
        unit = siggen.fm_stereo_iq(260 * 2048, 384e3, amplitude=1.0, sigma=0.0)
        return np.stack([stepped(unit, a, 2048, 0, 1e-3, seed) for a, seed in (([HI] * 260, 11), ([LO] * 260, 12), (AMPS130 * 2, 13))])
    return cached("fm384x3", make)


def b_first(n_if):
    """k_stats's rule on a call's IF block lengths: from the last group of 64 blocks down to the second, the first group
    at which 400 blocks with IF samples have been seen (0: the walk takes the whole call)."""
    seen = 0
    for b0 in range(((len(n_if) - 1) // 64) * 64, 0, -64):
        seen += sum(1 for n in n_if[b0:b0 + 64] if n)
        if seen >= 400:
            return b0
    return 0


def runs_of(gates):
    g = [int(v) for v in gates]
    cut = [0] + [i for i in range(1, len(g)) if g[i] != g[i - 1]] + [len(g)]
    return " ".join(f"{'open' if g[a] else 'closed'} x {b - a}" for a, b in zip(cut, cut[1:]))


CALLS523 = [[BLK10] * 520, [BLK10] * 3]
INT_FIELDS = ("block", "first_frame", "n_frames", "gate_open", "n_clipped")


def report(n_if_calls, forms, gates):
    """Prints what a test covered; returns b_first of every call (the blocks in front of it take k_stats's own loop)."""
    bf = [b_first(n) for n in n_if_calls]
    print("blocks per call:", [len(n) for n in n_if_calls], "| front-end forms:", sorted(forms), "| blocks in front of b_first:", bf,
          "| tail lanes of the last group of 64:", [len(n) % 64 for n in n_if_calls])
    print("gate pattern (open x n / closed x n):", runs_of(gates))
    return bf


def split(v, calls):
    o, out = 0, []
    for c in calls:
        out.append(list(v[o:o + len(c)]))
        o += len(c)
    return out


def chain10(max_blocks, max_block_len=BLK10, **kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=F10, enable_resampler=True, stereo=True, max_block_len=max_block_len,
                     max_blocks=max_blocks, **kw)


def run10(x, calls, fused, max_block_len=BLK10):
    """tests/test_gpu_output.py's run10 on x: fixture, oracle if_rms, and the last record of every call against that call's
    fmr_status.if_rms; the front-end forms are read behind the first call."""
    lens = [b for c in calls for b in c]
    n_if, ref_rms = oracle_if(x, lens)
    has_if = [n > 0 for n in n_if]
    ch = chain10(max(len(c) for c in calls), max_block_len)
    ch.enable_output(squelch_level=LEVEL)
    audio, alen, st = feed(ch, x, calls[:1])
    forms = ch.front_end_forms()
    if len(calls) > 1:
        a2, al2, st2 = feed(ch, x[sum(calls[0]):], calls[1:])
        audio, alen, st = np.concatenate([audio, a2], axis=1), alen + al2, st + st2
    print("front-end forms behind the first call:", sorted(forms), "| behind all:", sorted(ch.front_end_forms()))
    assert ("fused" in forms) == fused and ("fused" in ch.front_end_forms()) == fused, (forms, ch.front_end_forms())
    recs, pcm = tg.check(ch, 0, audio[0], alen, has_if, 2)
    ch.close()
    bf = report(split(n_if, calls), forms, recs["gate_open"])
    assert np.allclose(recs["if_rms"], ref_rms, rtol=1e-5, atol=0), np.max(np.abs(recs["if_rms"] / ref_rms - 1))   # tests/test_gpu_parity.py:170
    ends = np.cumsum([sum(h) for h in split(has_if, calls)])
    for e, s in zip(ends, st):
        assert e > 0 and recs["if_rms"][e - 1].tobytes() == s.tobytes(), (e, recs["if_rms"][e - 1], s)
    return dict(recs=recs, pcm=pcm, audio=audio, alen=alen, has_if=has_if, b_first=bf)


def base():
    """Test 1's chain, once: tests 3, 5 and 8 compare with its records."""
    return cached("calls_base", lambda: run10(fm541(), CALLS523, True))


def closed_frames(recs):
    return np.repeat(recs["gate_open"] == 0, recs["n_frames"].astype(np.int64))


def test_fm_stereo_fused_front_end_520_blocks_in_one_call():
    """520 x 4608 at 10 MS/s in one call, then 3 blocks that carry the levels on.  b_first = 64: the records of the blocks
    0-63 (60-63 closed) come from k_stats's loop for the blocks in front of b_first, the status from its walk behind it."""
    got = base()
    recs, pcm = got["recs"], got["pcm"]
    assert got["b_first"] == [64, 0] and all(got["has_if"])
    assert recs["gate_open"].tolist() == GATES523 and recs["block"].tolist() == list(range(523))
    assert recs["n_clipped"].sum() == 0 and len(pcm) == recs["n_frames"].sum() > 11000
    closed = closed_frames(recs)
    assert not pcm[closed].any() and pcm[~closed].any(axis=1).mean() > 0.9


def test_three_kernel_front_end_520_blocks_in_one_call(monkeypatch):
    """The same with FMR_NO_FUSED = 1: k_stats reads the per-block arrays (part == nullptr), also in front of b_first."""
    monkeypatch.setenv("FMR_NO_FUSED", "1")
    got = run10(fm541(), CALLS523, False)
    assert got["b_first"] == [64, 0] and got["recs"]["gate_open"].tolist() == GATES523


@pytest.mark.parametrize("cuts,tails,reload_at", [((63, 64, 65, 129, 199), [63, 0, 1, 1, 7], None), ((450, 70), [2, 6], 384)],
                         ids=["63_64_65_129_199", "450_70"])
def test_fm_stereo_520_blocks_in_shorter_calls(cuts, tails, reload_at):
    """The first 520 blocks cut so that the last group of 64 has 63, 0, 1, 1 and 7 lanes; and in calls of 450 and 70: with
    b_first = 0 k_stats takes its second load at block 384, where the gate opens behind the one closed block 383.  Each
    cut against its own audio, and the integer fields against the one call's."""
    one = base()["recs"][:520]
    calls = [[BLK10] * n for n in cuts]
    got = run10(fm541(), calls, True)
    recs = got["recs"]
    assert [n % 64 for n in cuts] == tails and got["b_first"] == [0] * len(cuts) and sum(cuts) == 520
    if reload_at:     # k_stats: for (b0 = b_first; b0 < nb; b0 += FMR_STATS_THREADS), FMR_STATS_THREADS = 384
        assert got["b_first"][0] + 384 == reload_at < cuts[0] and GATES520[reload_at - 2:reload_at + 1] == [1, 0, 1]
        print("k_stats's second load begins at block", reload_at, "of the first call; gates 382-384:", recs["gate_open"][382:385].tolist())
    assert recs["gate_open"].tolist() == GATES520
    for k in INT_FIELDS:
        assert same_bits(recs[k], one[k]), k


# tests/test_gpu_output.py's RAGGED with its second and third call in one, and its run of one-sample blocks (nearly all
# without an IF sample: the front end takes one of 26.04) lengthened and cut by a 27-sample block after every three: those
# have one or two IF samples and hardly ever audio.  The run lies over the block indices 20-79 of the call, the 27-sample
# blocks at 23, 27, ..., 63, 67, ...: the first group of 64 ends on a block with IF samples and the second begins with
# three without.  The call goes on through the weak region 2 into region 3.
LONG = tg._region([513] * 20 + ([1] * 3 + [27]) * 15 + [511, 513, 4096]) + RAGGED[2]
RAGGED_LONG = [RAGGED[0], LONG, RAGGED[3], RAGGED[4]]


def test_ragged_call_of_119_blocks():
    """tests/test_gpu_output.py's 7 x 65536 with a ragged call of 119 blocks: records of the blocks with IF samples only, in
    order, and if_level / audio_level carried over the blocks without, across the groups of 64."""
    assert len(LONG) == 119 and sum(LONG) == 3 * BLK and sum(map(sum, RAGGED_LONG)) == 7 * BLK
    got = run10(tg.fm10(), RAGGED_LONG, True, max_block_len=BLK)
    recs, has_if, alen = got["recs"], got["has_if"], got["alen"]
    h, al = np.array(has_if[1:120]), np.array(alen[1:120])
    print("the long call, blocks 56-72: has IF samples", h[56:73].astype(int).tolist(), "audio samples", al[56:73].tolist())
    assert 0 < h[56:64].sum() < 8 and 0 < h[64:72].sum() < 8 and np.any(h[56:72] & (al[56:72] == 0)) and h[63] and not h[64]
    assert h[64:].sum() > 0 and len(recs) == sum(has_if) < len(has_if)
    assert recs["block"].tolist() == [b for b, v in enumerate(has_if) if v] and np.any(recs["n_frames"] == 0)
    region = np.cumsum([0] + [b for c in RAGGED_LONG for b in c])[recs["block"].astype(np.int64)] // BLK
    for g, a in enumerate(tg.AMPS7):
        assert np.all(recs["gate_open"][region == g] == int(a == HI)), g


@pytest.mark.parametrize("max_blocks", [64, 65, 100])
def test_record_ring_smaller_than_the_call(max_blocks):
    """520 records into a ring of 64, 65 or 100 (keep_from in k_out_blocks: records a later record of the call lands on are
    not written), then 3 more: the newest survive, bit-identical to the one call's, and blocks_dropped is exact."""
    one, x = base(), fm541()
    ch = chain10(520)
    ch.enable_output(squelch_level=LEVEL, max_blocks=max_blocks)
    a1, _, _ = feed(ch, x, CALLS523[:1])
    forms = ch.front_end_forms()
    _, _, info = ch.output_read(0, cap_frames=0, cap_blocks=0)
    assert (info["blocks_waiting"], info["blocks_dropped"]) == (max_blocks, 520 - max_blocks)
    a2, _, _ = feed(ch, x[520 * BLK10:], CALLS523[1:])
    pcm, recs, info = ch.output_read(0)
    ch.close()
    report([[1] * 520, [1] * 3], forms, recs["gate_open"])
    assert "fused" in forms and same_bits(np.concatenate([a1, a2], axis=1), one["audio"])
    assert len(recs) == max_blocks and (info["blocks_dropped"], info["blocks_waiting"], info["frames_dropped"]) == (523 - max_blocks, 0, 0)
    assert same_bits(recs, one["recs"][523 - max_blocks:]) and same_bits(pcm, one["pcm"])
    assert recs["block"].tolist() == list(range(523 - max_blocks, 523))


@pytest.mark.parametrize("mode", ["nbfm", "am"])
def test_nbfm_and_am_470_blocks_in_one_call(mode, nbfm_default, nbfm_audio, am_narrow):
    """48 kHz, 512-sample blocks: 470 in one call (b_first = 64, k_stats's second load at 384), then 130 in calls of 65
    (a tail of one lane) whose carrier starts the pattern again."""
    calls = [[BLK48] * 470, [BLK48] * 65, [BLK48] * 65]
    if mode == "nbfm":
        x = nbfm600()
        ch = fmr.Chain(mode=fmr.MODE_NBFM, input_rate=48e3, enable_resampler=False, filter_coeff=nbfm_default,
                       nbfm_freq_dev=8000.0, max_block_len=BLK48, max_blocks=470)
        dec = ora.NbfmDecoder(nbfm_default, 8000.0, nbfm_audio)
    else:
        x = am600()
        ch = fmr.Chain(mode=fmr.MODE_AM, input_rate=48e3, filter_coeff=am_narrow, max_block_len=BLK48, max_blocks=470)
        dec = ora.AmDecoder(am_narrow, ora.MODE_AM)
    ch.enable_output(squelch_level=LEVEL, max_frames=1 << 19)       # (600 x 512 frames: more than the default ring's 2^18)
    audio, alen, st = feed(ch, x, calls)
    forms = ch.front_end_forms()
    recs, pcm = tg.check(ch, 0, audio[0], alen, [True] * 600, 1)
    ch.close()
    bf = report([[BLK48] * len(c) for c in calls], forms, recs["gate_open"])
    assert bf == [64, 0, 0] and not forms       # (no IF resampler at 48 kHz: k_stats reads the per-block arrays)
    ref_rms = []
    for b in siggen.blocks(x, BLK48):
        dec.process(b)
        ref_rms.append(dec.get_if_rms())
    assert np.allclose(recs["if_rms"], ref_rms, rtol=1e-5, atol=0), np.max(np.abs(recs["if_rms"] / np.array(ref_rms) - 1))   # tests/test_gpu_parity.py:342,473
    assert recs["gate_open"].tolist() == GATES600 and recs["n_frames"].tolist() == [BLK48] * 600
    for e, s in zip((470, 535, 600), st):
        assert recs["if_rms"][e - 1].tobytes() == s.tobytes(), e
    closed = closed_frames(recs)
    assert not pcm[closed].any() and pcm[~closed].any(axis=1).mean() > 0.9


def test_pipelined_against_in_order_130_blocks_per_call():
    """Four asynchronous device calls of 130 x 4608 at 10 MS/s (pipelined: the tail runs a call late) and one
    fmr_synchronize, against the in_order chain: records and PCM bit for bit, and against the fixture on the audio in the
    device buffers."""
    import torch
    per = 130
    x = fm541()[:520 * BLK10]
    kw = dict(mode=fmr.MODE_FM, input_rate=F10, enable_resampler=True, stereo=True, max_block_len=BLK10, max_blocks=per)
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_output(squelch_level=LEVEL)
    audio, alen, _ = feed(ref_ch, x, [[BLK10] * per] * 4)
    ref_recs, ref_pcm = tg.check(ref_ch, 0, audio[0], alen, [True] * 520, 2)
    ref_ch.close()
    ch = fmr.Chain(**kw)
    ch.enable_output(squelch_level=LEVEL)
    stride = 2 * 8192
    assert stride >= 2 * max(sum(alen[per * i:per * i + per]) for i in range(4))
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(4 * stride, dtype=torch.float64, device="cuda")
    al = []
    for i in range(4):
        al += [int(v) for v in ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * BLK10, len(x), [BLK10] * per,
                                                         d_a.data_ptr() + 8 * i * stride, stride, sync=False)]
    ch.synchronize()
    forms = ch.front_end_forms()
    pcm, recs, info = ch.output_read(0)
    ch.close()
    report([[1] * per] * 4, forms, recs["gate_open"])
    assert "fused" in forms and al == alen and info["frames_dropped"] == 0 and info["blocks_dropped"] == 0
    h_a = d_a.cpu().numpy()
    dev_audio = np.concatenate([h_a[i * stride:i * stride + sum(al[per * i:per * i + per])] for i in range(4)])
    ref2, ref2_pcm = oracle(recs, dev_audio, al, [True] * 520, 2)
    tg.compare(recs, pcm, ref2, ref2_pcm)
    for k in BIT_FIELDS:
        assert same_bits(recs[k], ref_recs[k]), k
    assert same_bits(pcm, ref_pcm) and recs["gate_open"].tolist() == GATES520


@pytest.mark.parametrize("rate,fmt,mono", [(16000, "s16", True), (44100, "s16", False), (32000, "f32", False)],
                         ids=["16000_s16_mono", "44100_s16_stereo", "32000_f32_stereo"])
def test_rate_converter_520_blocks_in_one_call(rate, fmt, mono):
    """The rate converter behind the 520-block call and its 3-block successor; 32000 F32 stereo runs k_out_rate<1, 2>
    (8-byte frames)."""
    one, x = base(), fm541()
    ch = chain10(520)
    ch.enable_output(format=fmt, squelch_level=LEVEL, rate=rate, mono=mono)
    audio, alen, _ = feed(ch, x, CALLS523)
    forms = ch.front_end_forms()
    f = of.PCM_F32 if fmt == "f32" else of.PCM_S16
    recs, pcm = tr.check(ch, 0, audio[0], alen, [True] * 523, 2, rate, mono, fmt=f)
    ch.close()
    report([[1] * 520, [1] * 3], forms, recs["gate_open"])
    assert "fused" in forms and recs["gate_open"].tolist() == GATES523 and pcm.any()
    assert pcm.dtype == (np.float32 if fmt == "f32" else np.int16) and pcm.shape[1] == (1 if mono else 2)
    assert same_bits(audio, one["audio"])
    for k in BIT_FIELDS:      # the records know nothing of the ring's rate (F32 counts |y| > 1, S16 the saturated: none here)
        assert same_bits(recs[k], one["recs"][k]), k


def test_ring_overrun_f32_stereo_at_32000():
    """max_frames = 256 at 32000 Hz F32 stereo (float2 frames): the 520-block call laps the ring 30 times, a call of 20
    open blocks behind it once more (~295 ring frames: keep_from in k_out_rate on frames that are not zero), read once at
    the end -- the window lies in the open blocks; then one more block read in two pieces
    (tests/test_gpu_output_rate.py::test_ring_overrun)."""
    x = fm541()
    rate, depth = 32000, 256
    _, L, M, T = tr.taps(rate)
    calls = [[BLK10] * 520, [BLK10] * 20]
    ch = chain10(520)
    ch.enable_output(format="f32", squelch_level=LEVEL, max_frames=depth, rate=rate)
    audio, alen, _ = feed(ch, x, calls[:1])
    forms = ch.front_end_forms()
    total1 = -(-(len(audio[0]) // 2) * L // M)
    _, _, info = ch.output_read(0, cap_frames=0, cap_blocks=0)       # (counts only: nothing is drained)
    assert total1 > 20 * depth and (info["frames_waiting"], info["frames_dropped"], info["first_frame"]) == (depth, total1 - depth, total1 - depth)
    a2, al2, _ = feed(ch, x[520 * BLK10:], calls[1:])
    audio, alen = np.concatenate([audio, a2], axis=1), alen + al2
    F = len(audio[0]) // 2
    total = -(-F * L // M)
    _, _, info = ch.output_read(0, cap_frames=0, cap_blocks=0)
    first, dropped = of.ring_window(total, depth)
    assert total - total1 > depth and (info["frames_waiting"], info["frames_dropped"], info["first_frame"]) == (depth, dropped, first)
    pcm, recs, info = ch.output_read(0)
    assert info["first_frame"] == total - depth and info["frames_waiting"] == 0 and info["frames_dropped"] == total - depth
    assert len(recs) == 540 and pcm.shape == (depth, 2) and pcm.dtype == np.float32
    assert recs["gate_open"].tolist() == GATES520 + [1] * 20 and "fused" in forms
    print("window: frames without a zero sample", int(pcm.all(axis=1).sum()), "of", depth, "| left != right in", int((pcm[:, 0] != pcm[:, 1]).sum()))
    assert pcm.all(axis=1).mean() > 0.9       # (left == right here: the test below has the two halves of a frame unlike)
    a3, al3, _ = feed(ch, x[540 * BLK10:], [[BLK10]])
    F2 = F + len(a3[0]) // 2
    total2 = -(-F2 * L // M)
    p1, r1, i1 = ch.output_read(0, cap_frames=5, cap_blocks=0)
    p2, r2, i2 = ch.output_read(0)
    ri = ch.output_rate_info(0)
    ch.close()
    report([[1] * 520, [1] * 20, [1]], forms, np.concatenate([recs["gate_open"], r2["gate_open"]]))
    assert len(p1) == 5 and len(r1) == 0 and i1["first_frame"] == total and i1["frames_waiting"] == total2 - total - 5
    assert i2["first_frame"] == total + 5 and len(r2) == 1 and r2["block"][0] == 540 and r2["first_frame"][0] == F
    assert i2["frames_dropped"] == total - depth and i2["blocks_dropped"] == 0 and 5 < total2 - total <= depth
    assert r2["gate_open"][0] == 1 and p1.any() and p2.all(axis=1).mean() > 0.9
    # the fixture on all 541 blocks: the ring's window of the first 540, then the last block's frames whole
    recs_all = np.concatenate([recs, r2])
    audio_all = np.concatenate([audio[0], a3[0]])
    ref, ref_pcm, cl, nf = tr.rate_oracle(recs_all, audio_all, alen + al3, [True] * 541, 2, rate, False, fmt=of.PCM_F32)
    tr.compare(recs_all, np.concatenate([pcm, p1, p2]), ref, ref_pcm[total - depth:])
    assert len(ref_pcm) == total2 and (ri["pcm_clipped"], ri["pcm_nonfinite"], ri["frames_in"]) == (cl, nf, F2)


def test_ring_overrun_f32_stereo_left_and_right_differ():
    """The 10 MS/s input above is too short for the pilot PLL to declare stereo (0.67 s of pilot): left and right are the
    same doubles there, and a float2 frame with its halves swapped would pass.  The strong row of the three-stream input at
    384 kHz is stereo from about block 93 on: two calls of 130 x 2048 into the same ring of 256 F32 frames at 32000 Hz, read
    once at the end -- every frame of the window has left != right."""
    blk, per, rate, depth = 2048, 130, 32000, 256
    _, L, M, T = tr.taps(rate)
    x = fm384x3()[0]
    ch = tg.chain384(max_blocks=per)
    ch.enable_output(format="f32", squelch_level=LEVEL, max_frames=depth, rate=rate)
    audio, alen, _ = feed(ch, x, [[blk] * per] * 2)
    forms, stereo = ch.front_end_forms(), ch.status(0).stereo_detected
    total = -(-(len(audio[0]) // 2) * L // M)
    pcm, recs, info = ch.output_read(0)
    ri = ch.output_rate_info(0)
    ch.close()
    report([[blk] * per] * 2, forms, recs["gate_open"])
    print("window: left != right in", int((pcm[:, 0] != pcm[:, 1]).sum()), "of", len(pcm), "frames | stereo_detected", stereo)
    assert not forms and total > 100 * depth and len(recs) == 2 * per and np.all(recs["gate_open"] == 1)
    assert (info["first_frame"], info["frames_dropped"], info["frames_waiting"]) == (total - depth, total - depth, 0)
    assert pcm.shape == (depth, 2) and pcm.dtype == np.float32 and np.all(pcm[:, 0] != pcm[:, 1]) and pcm.all()
    ref, ref_pcm, cl, nf = tr.rate_oracle(recs, audio[0], alen, [True] * (2 * per), 2, rate, False, fmt=of.PCM_F32)
    tr.compare(recs, pcm, ref, ref_pcm[total - depth:])
    assert len(ref_pcm) == total and (ri["pcm_clipped"], ri["pcm_nonfinite"], ri["frames_in"]) == (cl, nf, len(audio[0]) // 2)


def test_three_streams_in_a_plain_chain(pilotcut):
    """n_streams = 3 at 384 kHz (no bank), 2 calls of 130 x 2048: a strong, a weak and the stepped carrier in the same
    blocks -- every stream against its own audio and its own oracle decoder; the gates do not leak between the streams."""
    blk, per = 2048, 130
    x = fm384x3()
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=384e3, enable_resampler=False, stereo=True, max_block_len=blk, max_blocks=per,
                   n_streams=3)
    ch.enable_output(squelch_level=LEVEL)
    audio, alen, _ = feed(ch, x, [[blk] * per] * 2)
    forms = ch.front_end_forms()
    got = [tg.check(ch, s, audio[s], alen, [True] * (2 * per), 2) for s in range(3)]
    ch.close()
    for s in range(3):
        report([[blk] * per] * 2, forms, got[s][0]["gate_open"])
        assert not forms       # (384 kHz in: no IF resampler, k_stats reads the per-block arrays)
        fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
        ref_rms = []
        for b in siggen.blocks(x[s], blk):
            fm.process(b)
            ref_rms.append(fm.get_if_rms())
        assert np.allclose(got[s][0]["if_rms"], ref_rms, rtol=1e-5, atol=0), s       # tests/test_gpu_parity.py:170
    want = gates_of(AMPS130 * 2)
    assert np.all(got[0][0]["gate_open"] == 1) and np.all(got[1][0]["gate_open"] == 0) and got[2][0]["gate_open"].tolist() == want
    assert got[0][1].any(axis=1).mean() > 0.9
    assert not got[1][1].any() and len(got[0][1]) == len(got[1][1]) == len(got[2][1]) > 30000
    closed = closed_frames(got[2][0])
    assert not got[2][1][closed].any() and got[2][1][~closed].any(axis=1).mean() > 0.9
    for k in ("block", "first_frame", "n_frames"):
        assert np.array_equal(got[0][0][k], got[1][0][k]) and np.array_equal(got[0][0][k], got[2][0][k])


def test_gate_at_equality():
    """squelch_level = a block's own if_rms: open ((double)float >= double holds at equality).  The next float32 above it,
    and a double between the two (a compare in float would round it down and open): closed, its frames all zero.  The other
    blocks' gates by the same compare, from the fixture."""
    blk, k = 2048, 4
    x = tg.stepped(siggen.fm_stereo_iq(8 * blk, 384e3, amplitude=1.0, sigma=0.0), [HI] * 8, blk, 0, 1e-3)

    def run(level):
        ch = tg.chain384(max_blocks=8)
        ch.enable_output(squelch_level=level)
        audio, alen, _ = feed(ch, x, [[blk] * 8])
        forms = ch.front_end_forms()
        pcm, recs, info = ch.output_read(0)
        ch.close()
        ref, ref_pcm = oracle(recs, audio[0], alen, [True] * 8, 2, level)
        tg.compare(recs, pcm, ref, ref_pcm, level=0.0)       # (the level lies on a block: the factor-3 rule is not for this test)
        report([[blk] * 8], forms, recs["gate_open"])
        assert not forms
        lo, n = int(recs["first_frame"][k]), int(recs["n_frames"][k])
        return recs, pcm[lo:lo + n]

    r0, p0 = run(0.0)
    rms = r0["if_rms"]
    at = float(rms[k])
    up = float(np.nextafter(rms[k], np.float32(np.inf)))
    between = 0.5 * (at + up)
    assert at < between < up and np.float32(between) == rms[k] and np.all(r0["gate_open"] == 1) and p0.any()
    print("if_rms:", [v.hex() for v in map(float, rms)], "levels:", at.hex(), between.hex(), up.hex())
    for level, want in ((at, 1), (up, 0), (between, 0)):
        recs, p = run(level)
        assert same_bits(recs["if_rms"], rms), (recs["if_rms"], rms)      # the same input, the same cut: the same bits
        assert recs["gate_open"].tolist() == [int(float(v) >= level) for v in rms] and recs["gate_open"][k] == want
        assert len(p) > 200 and (p.any() if want else not p.any())
        if want:
            assert same_bits(p, p0)

"""DC-offset and IQ-imbalance correction on the GPU (fmr_enable_iq_correction) against tests/iqcorr_fixture.py, bit for
bit.

The capture (iqcorr_fixture.capture): station 3 at -250 kHz (0.3) and station 4 at +250 kHz (0.03) at 2.5 MS/s, 122
intervals of 4096 samples, through the receiver model with g = 1.05, phi = 3 degrees and an offset of 0.01 - 0.006j, W = 4,
R = 8, with everything tests/test_iqcorr_fixture.py lists planted: non-finite, skipped and denormal samples, a -0.0 in
interval 0, all-zero and all-skipped stretches that empty the window, and two level steps.  Everything here is an equality
of bits: the stage's rows (tap 7) and records against the fixture's, and the chain's outputs against a twin chain without
the stage that is fed the fixture's corrected capture with the same cut into calls."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import blanker_fixture as bf
import iqcorr_fixture as qf
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

F, BLK, OFFS, N, Q = qf.F, qf.BLK, qf.OFFS, qf.N, qf.Q
CALLS, RAGGED = qf.CALLS, qf.RAGGED
IQC = dict(average_intervals=qf.CFG["W"], record_intervals=qf.CFG["R"])
NB = dict(gate_samples=2, max_run_samples=16, average_intervals=4, record_intervals=8)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def capture():
    return cached("x", qf.capture)


def fixture(x=None, key="main", **kw):
    """The fixture over one row (the main capture by default), computed once per key."""
    return cached(("fix", key), lambda: qf.run(capture() if x is None else x, **{**qf.CFG, **kw}))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bank(**kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
                     channel_offsets_hz=OFFS, **kw)


def feed(ch, x, calls, rows=0, resample=False, tap=7, rows6=0):
    """x [rows, n] through process_blocks (or resample_blocks), one call per entry of `calls`.  Returns a dict: out [S, m]
    (audio or IQ), lens, status (bytes per call and stream), pps, rows (tap 7 of every call joined, per input row, when
    rows > 0) and rows6 (tap 6 likewise)."""
    x = np.atleast_2d(x)
    S = ch.n_streams
    o = {"out": [], "lens": [], "status": [], "pps": [], "rows": [[] for _ in range(rows)], "rows6": [[] for _ in range(rows6)]}
    pos = 0
    for ll in calls:
        m = int(sum(ll))
        a, al = (ch.resample_blocks if resample else ch.process_blocks)(x[:, pos:pos + m], ll)
        o["out"].append(a)
        o["lens"] += [int(v) for v in al]
        if not resample:
            o["status"].append([bytes(ch.status(s)) for s in range(S)])
            o["pps"].append([ch.pps_events(s) for s in range(S)])
        for r in range(rows):
            o["rows"][r].append(ch.debug_read(tap, stream=r, cap=m + 16))
        for r in range(rows6):
            o["rows6"][r].append(ch.debug_read(6, stream=r, cap=m + 16))
        pos += m
    o["out"] = np.concatenate(o["out"], axis=1)
    o["rows"] = [np.concatenate(r) for r in o["rows"]]
    o["rows6"] = [np.concatenate(r) for r in o["rows6"]]
    return o


def check_records(recs, ref, first=0):
    assert len(recs) == len(ref) - first, (len(recs), len(ref), first)
    for k in qf.RECORD.names:
        assert same_bits(recs[k], ref[k][first:]), (k, recs[k][:16], ref[k][first:][:16])


def same_outputs(a, b):
    assert a["lens"] == b["lens"]
    assert same_bits(a["out"], b["out"])
    assert a["status"] == b["status"] and a["pps"] == b["pps"]


def twin_of(make, x_fixed, calls, **kw):
    ch = make()
    try:
        return feed(ch, x_fixed, calls, **kw)
    finally:
        ch.close()


def test_measure_mode_moves_nothing():
    """A bank with RDS and all three monitors: audio, status, PPS, RDS groups and monitor records are bit-identical with
    the measuring stage and without any; the stage's records are the fixture's; the apply kernel is never launched."""
    outs = []
    for on in (False, True):
        ch = bank(enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_loudness()
        ch.enable_rf_monitor()
        if on:
            ch.enable_iq_correction(act=False, **IQC)
        ch.enable_kernel_timing(1)
        names = set()
        o = {"out": [], "status": [], "pps": []}
        pos = 0
        for ll in CALLS:
            m = sum(ll)
            a, _ = ch.process_blocks(capture()[None, pos:pos + m], ll)
            o["out"].append(a)
            o["status"].append([bytes(ch.status(s)) for s in range(2)])
            o["pps"].append([ch.pps_events(s) for s in range(2)])
            names |= {k for k, _ in ch.kernel_times()}
            pos += m
        o["out"] = np.concatenate(o["out"], axis=1)
        o["rds"] = [ch.rds_groups(s) for s in range(2)]
        o["mon"] = [ch.monitor_records(s)[:3] + ch.loudness_records(s)[:1] + ch.rf_monitor_records(s)[:3] for s in range(2)]
        if on:
            recs, info = ch.iq_correction_records(0)
            with pytest.raises(fmr.FmrError, match=r"error -2.*tap 7"):
                ch.debug_read(7)
        ch.close()
        outs.append((o, names))
    (a, na), (b, nb) = outs
    assert same_bits(a["out"], b["out"]) and a["status"] == b["status"] and a["pps"] == b["pps"]
    for s in range(2):
        assert same_bits(a["rds"][s], b["rds"][s])
        assert len(a["mon"][s][0]) >= 1
        for u, v in zip(a["mon"][s], b["mon"][s]):
            assert same_bits(u, v)
    assert not any(k.startswith("iqc_") for k in na)
    assert {"iqc_moments", "iqc_coef", "iqc_records"} <= nb and "iqc_apply" not in nb
    check_records(recs, fixture()["records"])
    assert info["rows"] == 1 and info["mode"] == fmr.IQC_MEASURE and info["intervals_complete"] == N // Q
    assert (info["correct"], info["average_intervals"], info["record_intervals"], info["max_records"]) == (3, 4, 8, 1024)
    lv = fmr.iq_correction_levels(recs)
    ref = qf.derive(fixture()["records"])
    assert lv["n_skipped"] == 2 + 6 * Q and lv["n_nonfinite"] == 2 and lv["n_refused"] == 0
    for k, v in ref.items():
        assert lv[k] == v or abs(lv[k] - v) <= 1e-12 * abs(v), (k, lv[k], v)


def test_act_mode_bank():
    """The two-channel bank, acting: tap 7 is the fixture's corrected capture, the records are the fixture's, and audio,
    status and PPS are those of a twin without the stage fed the fixture's corrected capture with the same cut.  Tap 6
    stays refused: the chain has no blanker."""
    fx = fixture()
    ch = bank()
    ch.enable_iq_correction(act=True, **IQC)
    got = feed(ch, capture(), CALLS, rows=1)
    recs, info = ch.iq_correction_records(0)
    with pytest.raises(fmr.FmrError, match=r"error -2.*tap 6"):
        ch.debug_read(6)
    ch.close()
    assert same_bits(got["rows"][0], fx["out"])
    check_records(recs, fx["records"])
    assert info["mode"] == fmr.IQC_ACT
    same_outputs(got, twin_of(bank, fx["out"], CALLS))


def test_cut_independence():
    """One call against ragged calls (blocks of 1, 7, 4095, 4097, 16384 and a few hundred, several per call) and the
    regular cut on a channelizer: records and corrected rows are equal bit for bit, and equal to the fixture's; the IQ rows
    are the twin's."""
    assert sum(map(sum, RAGGED)) == N and max(map(len, RAGGED)) <= 8
    fx = fixture()
    for calls, blk, nblk in (([[N]], N, 1), (RAGGED, BLK, 8), (CALLS, BLK, 8)):
        make = lambda: fmr.Channelizer(F, OFFS, max_block_len=blk, max_blocks=nblk)
        ch = make()
        ch.enable_iq_correction(act=True, **IQC)
        got = feed(ch, capture(), calls, rows=1, resample=True)
        recs, _ = ch.iq_correction_records(0)
        ch.close()
        assert same_bits(got["rows"][0], fx["out"]), len(calls)
        check_records(recs, fx["records"])
        if calls is CALLS:
            tw = twin_of(make, fx["out"], CALLS, resample=True)
            assert got["lens"] == tw["lens"] and same_bits(got["out"], tw["out"]) and got["out"].shape[1] > 70000


SHAPES = {
    "two_streams_unlike_rows": dict(mode=fmr.MODE_FM, stereo=True, n_streams=2),
    "front_end_only": dict(mode=fmr.MODE_NONE),
    "fourth_down": dict(mode=fmr.MODE_FM, stereo=True, fourth_down=True),
    "r8b": dict(mode=fmr.MODE_FM, stereo=True, resampler_class=fmr.RESAMPLER_R8B),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_chain_shapes(shape):
    """Plain chains, acting, against their twins on the fixture's corrected rows: two streams with unlike rows (the second
    is iqcorr_fixture.second_row: another gain, phase and offset), a front-end-only chain, enable_fourth_down, the R8B
    class."""
    kw = SHAPES[shape]
    S = kw.get("n_streams", 1)
    resample = kw["mode"] == fmr.MODE_NONE
    rows = [capture()]
    fxs = [fixture()]
    if S == 2:
        rows.append(cached("x2", qf.second_row))
        fxs.append(fixture(rows[1], key="row2"))
        assert not same_bits(fxs[0]["coef"], fxs[1]["coef"])
    make = lambda: fmr.Chain(input_rate=F, enable_resampler=True, max_block_len=BLK, max_blocks=8, **kw)
    ch = make()
    ch.enable_iq_correction(act=True, **IQC)
    got = feed(ch, np.stack(rows), CALLS, rows=S, resample=resample)
    recs = [ch.iq_correction_records(r)[0] for r in range(S)]
    ch.close()
    for r in range(S):
        assert same_bits(got["rows"][r], fxs[r]["out"]), r
        check_records(recs[r], fxs[r]["records"])
    tw = twin_of(make, np.stack([f["out"] for f in fxs]), CALLS, resample=resample)
    same_outputs(got, tw)
    assert got["out"].shape[1] > 5000


@pytest.mark.parametrize("correct", ["DC", "BALANCE"])
def test_correct_selects_one_part(correct):
    mask = getattr(fmr, "IQC_" + correct)
    fx = fixture(key=correct, correct=mask)
    assert not same_bits(fx["out"], fixture()["out"])
    ch = fmr.Channelizer(F, OFFS, max_block_len=BLK, max_blocks=8)
    ch.enable_iq_correction(act=True, correct=mask, **IQC)
    got = feed(ch, capture(), CALLS, rows=1, resample=True)
    recs, info = ch.iq_correction_records(0)
    ch.close()
    assert info["correct"] == mask
    assert same_bits(got["rows"][0], fx["out"])
    check_records(recs, fx["records"])
    zero = ("w_re", "w_im") if correct == "DC" else ("dc_re", "dc_im")
    assert not any(recs[k].any() for k in zero)


def test_improper_row_is_refused_and_passes():
    """A real-valued capture (noise on Q): every interval with a window is refused; with BALANCE alone the rows pass bit
    for bit, with both parts they are the fixture's (the offset is still removed)."""
    x = cached("improper", qf.improper_row)
    for mask, key in ((fmr.IQC_BALANCE, "imp_b"), (0, "imp")):
        fx = fixture(x, key=key, correct=mask)
        ch = fmr.Channelizer(F, OFFS, max_block_len=BLK, max_blocks=8)
        ch.enable_iq_correction(act=True, correct=mask, **IQC)
        got = feed(ch, x, CALLS, rows=1, resample=True)
        recs, _ = ch.iq_correction_records(0)
        ch.close()
        check_records(recs, fx["records"])
        assert recs["n_refused"].tolist() == [7] + [8] * 14 and not recs["w_re"].any() and not recs["w_im"].any()
        assert same_bits(got["rows"][0], fx["out"])
        if mask == fmr.IQC_BALANCE:
            assert same_bits(got["rows"][0], x)


@pytest.mark.parametrize("order", ["corrector_first", "blanker_first"])
def test_both_stages_acting(order):
    """Corrector and blanker acting on a bank, enabled in either order: tap 7 is the corrector fixture's output, tap 6 the
    blanker fixture's run over that, and the outputs are those of a blanker-only chain fed the corrected capture."""
    fx = fixture()
    nbx = cached("nb", lambda: bf.run(fx["out"], G=2, M=16, W=4, threshold_db=12.0, R=8))
    assert nbx["blank"].sum() > 0 and np.isfinite(nbx["out"]).all() and not np.isfinite(fx["out"]).all()
    ch = bank()
    if order == "corrector_first":
        ch.enable_iq_correction(act=True, **IQC)
        ch.enable_blanker(act=True, **NB)
    else:
        ch.enable_blanker(act=True, **NB)
        ch.enable_iq_correction(act=True, **IQC)
    got = feed(ch, capture(), CALLS, rows=1, rows6=1)
    recs, _ = ch.iq_correction_records(0)
    nrecs, _ = ch.blanker_records(0)
    ch.close()
    assert same_bits(got["rows"][0], fx["out"])
    assert same_bits(got["rows6"][0], nbx["out"])
    check_records(recs, fx["records"])
    for k in bf.RECORD.names:
        assert same_bits(nrecs[k], nbx["records"][k]), k

    def blanker_only():
        c = bank()
        c.enable_blanker(act=True, **NB)
        return c
    same_outputs(got, twin_of(blanker_only, fx["out"], CALLS))


def device_feed(ch, rows, lens, taps=()):
    """rows [2, n] from a device buffer whose rows start one complex sample behind a 16-byte boundary and lie an odd
    number of samples apart, through resample_blocks_device, one call of one block per entry of `lens`.  Returns the IQ
    rows of all calls joined and, per tap, per input row, the tap of every call joined."""
    import torch
    n = rows.shape[1]
    stride = n + 65
    buf = np.zeros(1 + 2 * stride + 64, dtype=np.complex64)
    for r in range(2):
        buf[1 + r * stride:1 + r * stride + n] = rows[r]
    d_x = torch.from_numpy(buf.view(np.float32)).cuda()
    assert d_x.data_ptr() % 16 == 0 and stride % 2 == 1
    ocap = max(lens) + 64
    d_o = torch.zeros(2 * 2 * ocap, dtype=torch.float32, device="cuda")
    out, got = [], {t: [[], []] for t in taps}
    pos = 0
    for m in lens:
        ol = ch.resample_blocks_device(d_x.data_ptr() + 8 * (1 + pos), stride, [m], d_o.data_ptr(), ocap, sync=True)
        out.append(d_o.cpu().numpy().view(np.complex64).reshape(2, ocap)[:, :int(ol.sum())].copy())
        for t in taps:
            for r in range(2):
                got[t][r].append(ch.debug_read(t, stream=r, cap=m + 16))
        pos += m
    return np.concatenate(out, axis=1), {t: [np.concatenate(g) for g in got[t]] for t in taps}


def test_both_stages_acting_on_unaligned_device_rows():
    """What the two capture stages share, where the other tests do not go together: a two-stream front-end-only chain,
    both stages acting, fed from device rows off the 16-byte phase and an odd stride apart in five calls of 8209, 1, 4095,
    8192 and 4097 samples (they straddle intervals, one brings a single sample, and from the third on a call waits for the
    records kernel of two calls before).  Taps 7 and 6 and the records are the fixtures', and the IQ rows are those of a
    twin without the stages fed the fixtures' output the same way."""
    lens = [8209, 1, 4095, 8192, 4097]
    n = sum(lens)
    rows = np.stack([capture()[:n], cached("x2", qf.second_row)[:n]])
    rows[0, [17000, 20496, 20497, 24000]] = np.complex64(30 - 20j)       # impulses for the blanker, behind its first window:
    rows[1, [16500, 20479, 20480, 22222]] = np.complex64(-25 + 35j)      # a gate across a call's edge, one across an interval's
    fxs =[fixture(rows[r], key=("corner", r), R=1) for r in range(2)]
    nbxs = [bf.run(fx["out"], G=2, M=16, W=4, threshold_db=12.0, R=1) for fx in fxs]
    assert all(x["blank"].sum() > 0 for x in nbxs) and len(fxs[0]["records"]) == n // Q == 6
    make = lambda: fmr.Chain(mode=fmr.MODE_NONE, input_rate=F, enable_resampler=True, n_streams=2, max_block_len=BLK, max_blocks=1)
    ch = make()
    ch.enable_iq_correction(act=True, **{**IQC, "record_intervals": 1})
    ch.enable_blanker(act=True, **{**NB, "record_intervals": 1})
    out, taps = device_feed(ch, rows, lens, taps=(7, 6))
    recs = [(ch.iq_correction_records(r)[0], ch.blanker_records(r)[0]) for r in range(2)]
    ch.close()
    for r in range(2):
        assert same_bits(taps[7][r], fxs[r]["out"]), r
        assert same_bits(taps[6][r], nbxs[r]["out"]), r
        check_records(recs[r][0], fxs[r]["records"])
        for k in bf.RECORD.names:
            assert same_bits(recs[r][1][k], nbxs[r]["records"][k]), (r, k)
    ch = make()
    tw, _ = device_feed(ch, np.stack([x["out"] for x in nbxs]), lens)
    ch.close()
    assert same_bits(out, tw) and out.shape[1] > 3000


@pytest.mark.parametrize("pipeline", ["pipelined", "in_order"])
def test_fused_front_end_at_10ms(pipeline, monkeypatch):
    """The benchmark's station at 10 MS/s (the fused front end), impaired, 8 x 65536 samples in two calls, the defaults
    but records of 32 intervals: rows, records and audio against the fixture and the twin, pipelined and FMR_PIPELINE=0."""
    if pipeline == "in_order":
        monkeypatch.setenv("FMR_PIPELINE", "0")
    x = cached("x10", qf.capture10)
    fx = fixture(x, key="x10", W=64, R=32)
    assert fx["coef"][1:].all() and not fx["refused"].any()
    blk = qf.BLK10
    calls = [[blk] * 4] * 2
    make = lambda: fmr.Chain(mode=fmr.MODE_FM, input_rate=qf.F10, enable_resampler=True, stereo=True, max_block_len=blk,
                             max_blocks=4)
    ch = make()
    ch.enable_iq_correction(act=True, record_intervals=32)
    got = feed(ch, x, calls, rows=1)
    recs, info = ch.iq_correction_records(0)
    ch.close()
    assert info["average_intervals"] == 64 and info["max_records"] == 1024
    assert same_bits(got["rows"][0], fx["out"])
    check_records(recs, fx["records"])
    same_outputs(got, twin_of(make, fx["out"], calls))
    assert len(recs) == 4 and got["out"].shape[1] > 2000


def test_long_calls_over_several_coefficient_tiles():
    """k_iqc_coef works in tiles of 512 pieces and sums what lies more than two tiles in front again: a call of 1600
    intervals and 100 samples (four tiles, the last with such a front) and one of 718 more (two tiles, the first piece on
    top of the open interval), W = 64 across the tile edges, against the fixture over the capture repeated 19 times."""
    x = cached("xlong", lambda: np.tile(capture(), 19))
    fx = fixture(x, key="long", W=64, R=256)
    n1 = 1600 * Q + 100
    calls = [[1 << 20] * 6 + [n1 - 6 * (1 << 20)], [1 << 20] * 2 + [len(x) - n1 - 2 * (1 << 20)]]
    assert sum(map(sum, calls)) == len(x) == 2318 * Q and all(0 < b <= 1 << 20 for c in calls for b in c)
    ch = fmr.Chain(mode=fmr.MODE_NONE, input_rate=F, enable_resampler=True, max_block_len=1 << 20, max_blocks=8)
    ch.enable_iq_correction(act=True, average_intervals=64)
    got = feed(ch, x, calls, rows=1, resample=True)
    recs, _ = ch.iq_correction_records(0)
    ch.close()
    check_records(recs, fx["records"])
    assert len(recs) == 9 and same_bits(got["rows"][0], fx["out"])


def test_records_and_ring():
    """Records of R = 8 intervals in a ring of 4: 15 complete, 11 dropped in all, the last four read; cap = 0 counts."""
    ch = fmr.Channelizer(F, OFFS, max_block_len=BLK, max_blocks=8)
    ch.enable_iq_correction(act=False, max_records=4, **IQC)
    pos = 0
    for ll in CALLS[:3]:                       # 164840 samples: 40 intervals, 5 records
        ch.resample_blocks(capture()[pos:pos + sum(ll)], ll)
        pos += sum(ll)
    info = fmr.IqCorrectionInfo()
    assert ch._L.fmr_iq_correction_read(ch.h, 0, None, 0, C.byref(info), 0) == 4
    assert (info.records_complete, info.records_dropped, info.first_unread, info.records_ready) == (5, 1, 1, 4)
    recs, info = ch.iq_correction_records(0, cap=1)
    assert recs["index"].tolist() == [1] and info["records_ready"] == 3
    for ll in CALLS[3:]:
        ch.resample_blocks(capture()[pos:pos + sum(ll)], ll)
        pos += sum(ll)
    recs, info = ch.iq_correction_records(0)
    ch.close()
    assert recs["index"].tolist() == [11, 12, 13, 14]
    assert info["records_complete"] == 15 and info["records_dropped"] == 1 + 9 and info["records_ready"] == 0
    check_records(recs, fixture()["records"], first=11)


def test_refusals_with_a_device():
    live = fmr.debug_live_resources()
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, max_block_len=BLK, input_format=fmr.IQ_S16)
    held = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError, match=r"error -3.*raw input format"):
        ch.enable_iq_correction()
    assert fmr.debug_live_resources() == held
    ch.close()
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=384000.0, enable_resampler=False, max_block_len=BLK)
    held = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError, match=r"error -3.*IF resampler"):
        ch.enable_iq_correction()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no IQ corrector"):
        ch.iq_correction_records(0)
    assert fmr.debug_live_resources() == held
    ch.close()
    ch = bank()
    held = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError, match=r"error -2.*average_intervals"):
        ch.enable_iq_correction(average_intervals=1025)
    assert fmr.debug_live_resources() == held
    ch.enable_iq_correction(act=True)
    grown = fmr.debug_live_resources()
    assert grown > held
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_iq_correction()
    assert fmr.debug_live_resources() == grown
    with pytest.raises(fmr.FmrError, match=r"error -2.*input rows"):
        ch.iq_correction_records(1)
    recs, info = ch.iq_correction_records(0)
    assert len(recs) == 0 and info["records_complete"] == 0 and info["average_intervals"] == 64 and info["correct"] == 3
    assert len(ch.debug_read(7)) == 0
    ch.close()
    ch = bank()
    ch.process_blocks(capture()[None, :4096], [4096])
    held = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_iq_correction()
    assert fmr.debug_live_resources() == held
    ch.close()
    assert fmr.debug_live_resources() == live


def test_facade_smoke(tmp_path):
    """tests/iqcorr_smoke.cpp through the facade: FmDecoder, AmDecoder, NbfmDecoder, IfResampler, ChannelBank and
    Channelizer with the corrector acting."""
    exe = str(tmp_path / "iqcorr_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "iqcorr_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("fm corrected", "am corrected", "nbfm corrected", "ifr corrected", "bank corrected", "channelizer corrected"):
        assert tag in r.stdout, r.stdout

"""Impulse blanker on the GPU (fmr_enable_blanker) against tests/blanker_fixture.py, bit for bit.

The capture (blanker_fixture.capture25): two FM stereo stations at 2.5 MS/s, 122 intervals of 4096 samples, G = 2, M = 16,
W = 4, R = 8, with bursts of 8.0 (16 to 27 times the carriers) on both sides of an interval edge, on the last sample of a
call and the first of the next, within G of each other, as a run of triggers every other sample for 3 M samples and again
after three open samples, one NaN, one Inf, one burst in interval 0 and a +20 dB step.  tests/test_blanker_cases.py holds
the fixture alone to the margins these comparisons rest on.  Everything here is an equality of bits: the stage's rows and
records against the fixture's, and the chain's outputs against a twin chain without the stage that is fed the fixture's
blanked capture with the same cut into calls."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import blanker_fixture as bf
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

F, BLK, OFFS, N, Q = bf.F25, bf.BLK25, bf.OFFS25, bf.N25, bf.Q
CALLS = bf.CALLS25
NB = dict(gate_samples=bf.CFG25["G"], max_run_samples=bf.CFG25["M"], average_intervals=bf.CFG25["W"],
          record_intervals=bf.CFG25["R"])
# blocks of 1, 7, 4095, 4097, 16384 and a few hundred samples, several blocks per call
RAGGED = [[1], [7, 300], [4095], [4097, 1], [BLK] * 3, [777], [4096, 4096, 123], [1, 1, 2], [BLK, 4095, 4097, 555]]
while sum(map(sum, RAGGED)) + 8 * BLK < N:
    RAGGED.append([BLK] * 8)
RAGGED.append([])
while sum(map(sum, RAGGED)) < N:
    RAGGED[-1].append(min(BLK, N - sum(map(sum, RAGGED))))
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def capture(clean=False):
    return cached(("x", clean), lambda: bf.capture25(clean))


def fixture(x=None, key="main", **kw):
    """The fixture over one row (the main capture by default), computed once per key."""
    return cached(("fix", key), lambda: bf.run(capture() if x is None else x, **{**bf.CFG25, **kw}))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bank(**kw):
    return fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=8,
                     channel_offsets_hz=OFFS, **kw)


def feed(ch, x, calls, rows=0, resample=False, taps=()):
    """x [rows, n] through process_blocks (or resample_blocks), one call per entry of `calls`.  Returns a dict: out [S, m]
    (audio or IQ), lens, status (bytes per call and stream), pps, rows (tap 6 of every call joined, per input row, when
    rows > 0) and the taps asked for (per call and stream)."""
    x = np.atleast_2d(x)
    S = ch.n_streams
    o = {"out": [], "lens": [], "status": [], "pps": [], "rows": [[] for _ in range(rows)], "taps": []}
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
            o["rows"][r].append(ch.debug_read(6, stream=r, cap=m + 16))
        o["taps"].append([[ch.debug_read(t, stream=s, cap=1 << 18) for t in taps] for s in range(S)])
        pos += m
    o["out"] = np.concatenate(o["out"], axis=1)
    o["rows"] = [np.concatenate(r) for r in o["rows"]]
    return o


def check_records(recs, ref, first=0):
    assert len(recs) == len(ref) - first, (len(recs), len(ref), first)
    for k in bf.RECORD.names:
        assert same_bits(recs[k], ref[k][first:]), (k, recs[k][:16], ref[k][first:][:16])


def same_outputs(a, b):
    assert a["lens"] == b["lens"]
    assert same_bits(a["out"], b["out"])
    assert a["status"] == b["status"] and a["pps"] == b["pps"]


def twin_of(make, x_blanked, calls, **kw):
    ch = make()
    try:
        return feed(ch, x_blanked, calls, **kw)
    finally:
        ch.close()


def test_measure_mode_moves_nothing():
    """A bank with RDS and all three monitors: audio, status, PPS, RDS groups and monitor records are bit-identical with
    the measuring stage and without any; the stage's records are the fixture's."""
    outs = []
    for on in (False, True):
        ch = bank(enable_rds=True)
        ch.enable_monitor(interval_samples=38400)
        ch.enable_loudness()
        ch.enable_rf_monitor()
        if on:
            ch.enable_blanker(act=False, **NB)
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
            recs, info = ch.blanker_records(0)
            with pytest.raises(fmr.FmrError, match=r"error -2.*tap 6"):
                ch.debug_read(6)
        ch.close()
        outs.append((o, names))
    (a, na), (b, nb) = outs
    assert same_bits(a["out"], b["out"]) and a["status"] == b["status"] and a["pps"] == b["pps"]
    for s in range(2):
        assert same_bits(a["rds"][s], b["rds"][s])
        assert len(a["mon"][s][0]) >= 1
        for u, v in zip(a["mon"][s], b["mon"][s]):
            assert same_bits(u, v)
    assert not any(k.startswith("nb_") for k in na) and {"nb_level", "nb_apply", "nb_records"} <= nb
    check_records(recs, fixture()["records"])
    assert info["rows"] == 1 and info["mode"] == fmr.NB_MEASURE and info["intervals_complete"] == N // Q
    assert (info["gate_samples"], info["max_run_samples"], info["average_intervals"], info["record_intervals"],
            info["max_records"]) == (2, 16, 4, 8, 1024)
    lv = fmr.blanker_levels(recs, F)
    ref = fixture()["records"]
    assert lv["n_blanked"] == ref["n_blanked"].sum() > 0 and lv["n_nonfinite"] == 2
    assert lv["blanked_share"] == ref["n_blanked"].sum() / (len(ref) * 8 * Q)


def act_bank():
    def make():
        ch = bank()
        ch.enable_blanker(act=True, **NB)
        try:
            o = feed(ch, capture(), CALLS, rows=1)
            o["recs"], o["info"] = ch.blanker_records(0)
            return o
        finally:
            ch.close()
    return cached("act_bank", make)


def test_act_mode_bank():
    """The two-channel bank, acting: tap 6 is the fixture's blanked capture, the records are the fixture's, and audio,
    status and PPS are those of a twin without the stage fed the fixture's blanked capture with the same cut."""
    fx = fixture()
    got = act_bank()
    assert same_bits(got["rows"][0], fx["out"])
    check_records(got["recs"], fx["records"])
    assert fx["blank"].sum() > 30 and not np.isfinite(capture()).all() and np.isfinite(fx["out"]).all()
    same_outputs(got, twin_of(bank, fx["out"], CALLS))
    assert np.isfinite(got["out"]).all()


def test_clean_capture_act_mode():
    """Nothing triggers on the clean capture: acting, everything is bit-identical to the twin without the stage."""
    x = capture(clean=True)
    ch = bank()
    ch.enable_blanker(act=True, **NB)
    got = feed(ch, x, CALLS, rows=1)
    recs, _ = ch.blanker_records(0)
    ch.close()
    assert same_bits(got["rows"][0], x)
    assert recs["n_triggers"].sum() == 0 and recs["n_blanked"].sum() == 0 and len(recs) == N // Q // 8
    check_records(recs, fixture(x, key="clean")["records"])
    same_outputs(got, twin_of(bank, x, CALLS))


def test_cut_independence():
    """One call against ragged calls (blocks of 1, 7, 4095, 4097, 16384 and a few hundred, several per call) on a
    channelizer: records and blanked rows are equal bit for bit, and equal to the fixture's."""
    assert sum(map(sum, RAGGED)) == N and max(map(len, RAGGED)) <= 8
    fx = fixture()
    for calls, blk, nblk in (([[N]], N, 1), (RAGGED, BLK, 8)):
        ch = fmr.Channelizer(F, OFFS, max_block_len=blk, max_blocks=nblk)
        ch.enable_blanker(act=True, **NB)
        got = feed(ch, capture(), calls, rows=1, resample=True)
        recs, _ = ch.blanker_records(0)
        ch.close()
        assert same_bits(got["rows"][0], fx["out"]), len(calls)
        check_records(recs, fx["records"])


def test_channelizer_rows():
    """A Channelizer, acting: its IQ rows are the twin's on the fixture's blanked capture, bit for bit."""
    fx = fixture()
    make = lambda: fmr.Channelizer(F, OFFS, max_block_len=BLK, max_blocks=8)
    ch = make()
    ch.enable_blanker(act=True, **NB)
    got = feed(ch, capture(), CALLS, rows=1, resample=True)
    ch.close()
    tw = twin_of(make, fx["out"], CALLS, resample=True)
    assert got["lens"] == tw["lens"] and same_bits(got["out"], tw["out"]) and got["out"].shape[1] > 70000


SHAPES = {
    "two_streams_unlike_rows": dict(mode=fmr.MODE_FM, stereo=True, n_streams=2),
    "am": dict(mode=fmr.MODE_AM),
    "fourth_down": dict(mode=fmr.MODE_FM, stereo=True, fourth_down=True),
    "r8b": dict(mode=fmr.MODE_FM, stereo=True, resampler_class=fmr.RESAMPLER_R8B),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_chain_shapes(shape):
    """Plain chains, acting, against their twins on the fixture's blanked rows: two streams with unlike rows (the second
    row is the capture turned by 12345 samples and halved), an AM chain, enable_fourth_down, the R8B class."""
    kw = SHAPES[shape]
    S = kw.get("n_streams", 1)
    rows = [capture()]
    fxs = [fixture()]
    if S == 2:
        with np.errstate(invalid="ignore"):
            rows.append(cached("x2", lambda: (np.roll(capture(), 12345) * np.float32(0.5)).astype(np.complex64)))
        fxs.append(fixture(rows[1], key="row2"))
        assert not same_bits(fxs[0]["blank"], fxs[1]["blank"])
    make = lambda: fmr.Chain(input_rate=F, enable_resampler=True, max_block_len=BLK, max_blocks=8, **kw)
    ch = make()
    ch.enable_blanker(act=True, **NB)
    got = feed(ch, np.stack(rows), CALLS, rows=S)
    recs = [ch.blanker_records(r)[0] for r in range(S)]
    ch.close()
    for r in range(S):
        assert same_bits(got["rows"][r], fxs[r]["out"]), r
        check_records(recs[r], fxs[r]["records"])
    same_outputs(got, twin_of(make, np.stack([f["out"] for f in fxs]), CALLS))
    assert got["out"].shape[1] > 5000


def test_async_device_calls_at_10ms():
    """Four asynchronous device calls of 2 x 65536 at 10 MS/s on the pipelined chain, acting with the defaults (G = 8,
    M = 64), and one fmr_synchronize, against the in_order chain fed from the host: audio and records bit for bit, the
    records the fixture's, and the audio that of an in_order twin without the stage on the fixture's blanked capture."""
    import torch
    per, blk = 2, bf.BLK10
    x = cached("x10", bf.capture10)
    fx = fixture(x, key="x10", G=8, M=64, W=16, R=256)
    assert fx["blank"].sum() >= 60 * 8
    kw = dict(mode=fmr.MODE_FM, input_rate=bf.F10, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=per)
    calls = [[blk] * per] * 4
    ref_ch = fmr.Chain(in_order=True, **kw)
    ref_ch.enable_blanker(act=True, record_intervals=32)
    ref = feed(ref_ch, x, calls, rows=1)
    ref_recs, info = ref_ch.blanker_records(0)
    ref_ch.close()
    assert (info["gate_samples"], info["max_run_samples"], info["average_intervals"]) == (8, 64, 16)
    assert same_bits(ref["rows"][0], fx["out"])
    fx32 = fixture(x, key="x10r32", G=8, M=64, W=16, R=32)
    check_records(ref_recs, fx32["records"])
    tw = twin_of(lambda: fmr.Chain(in_order=True, **kw), fx["out"], calls)
    assert ref["lens"] == tw["lens"] and same_bits(ref["out"], tw["out"])
    ch = fmr.Chain(**kw)
    ch.enable_blanker(act=True, record_intervals=32)
    stride = 2 * 2048
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_a = torch.zeros(4 * stride, dtype=torch.float64, device="cuda")
    al = []
    for i in range(4):
        al += [int(v) for v in ch.process_blocks_device(d_x.data_ptr() + 8 * i * per * blk, len(x), [blk] * per,
                                                         d_a.data_ptr() + 8 * i * stride, stride, sync=False)]
    ch.synchronize()
    recs, _ = ch.blanker_records(0)
    last = ch.debug_read(6, cap=per * blk + 16)
    ch.close()
    assert al == ref["lens"]
    h_a = d_a.cpu().numpy()
    dev_audio = np.concatenate([h_a[i * stride:i * stride + sum(al[per * i:per * i + per])] for i in range(4)])
    assert same_bits(dev_audio, ref["out"][0])
    check_records(recs, fx32["records"])
    assert same_bits(last, fx["out"][3 * per * blk:])


def test_nan_in_a_bank():
    """A 10 MS/s bank (its stage B widens a NaN to a tile of IF samples) with the blanker acting: the NaN reaches neither
    IF nor audio, and IF and audio equal the twin's on the fixture's zeroed capture."""
    import chanbank_fixture as cb
    F10, blk, offs = 10e6, 65536, [-1_200_000, 800_000]
    n = 6 * blk
    x = cached("x10bank", lambda: cb.composite(n, F10, offs, [3, 4], [0.3, 0.2]))
    x = x.copy()
    x[3 * blk + 1234] = np.complex64(complex(np.nan, np.nan))
    z = bf.run(x, *bf.defaults(F10))["out"]          # (the NaN and the seven samples behind it: the gate is 0.8 us)
    assert np.count_nonzero(z != x) == 8 and not z[3 * blk + 1234:3 * blk + 1242].any()
    make = lambda: fmr.Chain(mode=fmr.MODE_FM, input_rate=F10, enable_resampler=True, stereo=True, max_block_len=blk,
                             max_blocks=2, channel_offsets_hz=offs)
    calls = [[blk, blk]] * 3
    ch = make()
    ch.enable_blanker(act=True)
    got = feed(ch, x, calls, rows=1, taps=(0,))
    ch.close()
    assert same_bits(got["rows"][0], z)
    tw = twin_of(make, z, calls, taps=(0,))
    same_outputs(got, tw)
    assert np.isfinite(got["out"]).all()
    for c in range(3):
        for s in range(2):
            assert np.isfinite(got["taps"][c][s][0]).all() and len(got["taps"][c][s][0]) > 1000
            assert same_bits(got["taps"][c][s][0], tw["taps"][c][s][0])


def test_records_and_ring():
    """Records of R = 8 intervals in a ring of 4: 15 complete, 11 dropped, the last four read; cap = 0 counts."""
    ch = fmr.Channelizer(F, OFFS, max_block_len=BLK, max_blocks=8)
    ch.enable_blanker(act=False, max_records=4, **NB)
    pos = 0
    for ll in CALLS[:3]:                       # 164840 samples: 40 intervals, 5 records
        ch.resample_blocks(capture()[pos:pos + sum(ll)], ll)
        pos += sum(ll)
    info = fmr.BlankerInfo()
    assert ch._L.fmr_blanker_read(ch.h, 0, None, 0, C.byref(info), 0) == 4
    assert (info.records_complete, info.records_dropped, info.first_unread, info.records_ready) == (5, 1, 1, 4)
    recs, info = ch.blanker_records(0, cap=1)
    assert recs["index"].tolist() == [1] and info["records_ready"] == 3
    for ll in CALLS[3:]:
        ch.resample_blocks(capture()[pos:pos + sum(ll)], ll)
        pos += sum(ll)
    recs, info = ch.blanker_records(0)
    ch.close()
    assert recs["index"].tolist() == [11, 12, 13, 14]
    assert info["records_complete"] == 15 and info["records_dropped"] == 1 + 9 and info["records_ready"] == 0
    check_records(recs, fixture()["records"], first=11)


def test_refusals_with_a_device():
    live = fmr.debug_live_resources()
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, max_block_len=BLK, input_format=fmr.IQ_S16)
    held = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError, match=r"error -3.*raw input format"):
        ch.enable_blanker()
    assert fmr.debug_live_resources() == held
    ch.close()
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=384000.0, enable_resampler=False, max_block_len=BLK)
    with pytest.raises(fmr.FmrError, match=r"error -3.*IF resampler"):
        ch.enable_blanker()
    with pytest.raises(fmr.FmrError, match=r"error -2.*no blanker"):
        ch.blanker_records(0)
    ch.close()
    ch = bank()
    with pytest.raises(fmr.FmrError, match=r"error -2.*max_run_samples"):
        ch.enable_blanker(gate_samples=0, max_run_samples=1)          # (below the default gate of this chain's rate: 2)
    held = fmr.debug_live_resources()
    ch.enable_blanker(act=True)
    assert fmr.debug_live_resources() > held
    with pytest.raises(fmr.FmrError, match=r"error -2.*already enabled"):
        ch.enable_blanker()
    with pytest.raises(fmr.FmrError, match=r"error -2.*input rows"):
        ch.blanker_records(1)
    recs, info = ch.blanker_records(0)
    assert len(recs) == 0 and info["records_complete"] == 0 and info["gate_samples"] == 2 and info["max_run_samples"] == 16
    assert len(ch.debug_read(6)) == 0
    ch.close()
    ch = bank()
    ch.process_blocks(capture()[None, :4096], [4096])
    with pytest.raises(fmr.FmrError, match=r"error -2.*already taken samples"):
        ch.enable_blanker()
    ch.close()
    assert fmr.debug_live_resources() == live


def test_facade_smoke(tmp_path):
    """tests/blanker_smoke.cpp through the facade: FmDecoder, AmDecoder, NbfmDecoder, IfResampler, ChannelBank and
    Channelizer with the blanker."""
    exe = str(tmp_path / "blanker_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "blanker_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("fm blanked", "am blanked", "nbfm blanked", "ifr blanked", "bank blanked", "channelizer blanked"):
        assert tag in r.stdout, r.stdout

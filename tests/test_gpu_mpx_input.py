"""MPX input on the GPU (fmr_create_mpx_decoder): an FM chain fed composite PCM instead of IQ.

The design makes the feature exactly checkable.  Chain A is an IQ chain at 384 kHz without the resampler whose MPX output
(fmr_enable_mpx_output at 384000 F32, gain 1.0) is its discriminator output bit for bit; chain B is an MpxChain at 384000
F32 gain 1.0 fed A's ring with A's block lengths.  Everything behind the discriminator reads the MPX row and the block table
and nothing else, so B's audio, PPS events, RDS groups, status and monitor records must be A's bits -- no tolerance.  At the
other rates the front end is held to tests/mpx_input_fixture.py (the header's definition in numpy float64) bit for bit, and
the decoder behind it to an MpxChain at 384000 fed the fixture's floats.

Signals: siggen.fm_stereo_iq at 384 kHz, two unlike streams, 622592 samples in 76 blocks of 8192: the pilot's lock delay
is 192000 samples and the first PPS event needs 19000 pilot periods, 384000 samples, behind it -- 576000 in all (425984
samples, one PPS period behind the lock delay's start, end without an event: measured on the MI355X).  57344 samples of A's
MPX where the front end alone is checked."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mpx_input_fixture as mi
import mpx_output_fixture as mo
import rds_fixture as rf
import siggen
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

FS, BLK, N, NB = 384000.0, 8192, 622592, 76
SHORT = 57344
STATUS_BITS = ("stereo_detected", "pilot_level", "pll_freq_err", "baseband_mean", "baseband_level")
_cache = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rows():
    if "rows" not in _cache:
        _cache["rows"] = np.stack([siggen.fm_stereo_iq(N, FS, stream_id=0),
                                   siggen.fm_stereo_iq(N, FS, stream_id=3, amplitude=0.2, phase0=0.7)]).astype(np.complex64)
    return _cache["rows"]


def status_of(ch, s):
    st = ch.status(s)
    d = {k: np.array(getattr(st, k)).tobytes() for k in STATUS_BITS}
    d.update(if_rms=float(st.if_rms), if_agc_gain=float(st.if_agc_gain), agc=(st.agc_iterations, st.agc_fallback),
             mp=(st.multipath_error, st.multipath_resets), stereo=st.stereo_detected)
    return d


def collect(ch, audio, alen):
    S = ch.n_streams
    return {"audio": audio, "alen": alen, "pps": [ch.pps_events(s) for s in range(S)], "status": [status_of(ch, s) for s in range(S)]}


def chain_a(x=None, setup=None, **kw):
    """The IQ chain over x (default: rows()) in one call of 52 blocks, its MPX through the stage itself at 384000 F32, gain
    1.0.  setup(ch) may enable further stages; returns the results, the ring of every stream, and what `read` gives."""
    x = rows() if x is None else x
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, max_block_len=BLK, max_blocks=NB, n_streams=len(x),
                   **kw)
    ch.enable_mpx_output(format="f32", rate=384000, gain=1.0, max_frames=1 << 20)
    extra = setup(ch) if setup else None
    audio, alen = ch.process_blocks(x, [BLK] * NB)
    out = collect(ch, audio, alen)
    out["mpx"] = np.stack([ch.mpx_output_read(s)[0] for s in range(len(x))])
    return out, ch, extra


def chain_b(mpx, lens, rate=384000, fmt="f32", gain=1.0, setup=None, max_blocks=NB, **kw):
    ch = fmr.MpxChain(rate=rate, format=fmt, gain=gain, n_streams=len(mpx), max_block_len=max(max(lens), 1), max_blocks=max_blocks,
                      **kw)
    extra = setup(ch) if setup else None
    audio, alen = ch.process_blocks(mpx, lens)
    return collect(ch, audio, alen), ch, extra


def base():
    """A on rows(), stereo: cached."""
    if "A" not in _cache:
        out, ch, _ = chain_a(stereo=True)
        ch.close()
        _cache["A"] = out
    return _cache["A"]


def assert_same_decoder(a, b, what=""):
    assert same_bits(a["alen"], b["alen"]), what
    d = np.abs(a["audio"] - b["audio"]).max() if a["audio"].shape == b["audio"].shape and a["audio"].size else -1.0
    print(f"{what}: audio {a['audio'].shape}, largest |A - B| = {d:.3e}")
    assert same_bits(a["audio"], b["audio"]), what
    assert a["pps"] == b["pps"], what
    for sa, sb in zip(a["status"], b["status"]):
        for k in STATUS_BITS:
            assert sa[k] == sb[k], (what, k)


# ---- 1: round trip, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(stereo=True), dict(stereo=True, pilot_shift=True), dict(stereo=False)],
                         ids=["stereo", "pilot_shift", "mono"])
def test_round_trip_is_exact(kw):
    if kw == dict(stereo=True):
        a = base()
    else:
        a, ch, _ = chain_a(**kw)
        ch.close()
    assert a["mpx"].shape == (2, N) and a["mpx"].dtype == np.float32
    if kw.get("stereo"):
        assert all(st["stereo"] == 1 for st in a["status"]) and all(len(p) >= 1 for p in a["pps"]), (a["status"], a["pps"])
    b, ch, _ = chain_b(a["mpx"], [BLK] * NB, **kw)
    info = [ch.mpx_input_info(s) for s in range(2)]
    tap = ch.debug_read(1, stream=1, cap=1 << 20)
    ch.close()
    assert_same_decoder(a, b, str(kw))
    assert same_bits(tap, a["mpx"][1])
    for s in range(2):
        assert b["status"][s]["if_rms"] == 0.0 and b["status"][s]["if_agc_gain"] == 1.0
        assert b["status"][s]["agc"] == (0, 0) and b["status"][s]["mp"] == (0.0, 0)
        assert info[s] == mi.info(384000, 1.0, N, mi.PCM_F32), info[s]
    assert a["audio"].any() and not same_bits(a["audio"][0], a["audio"][1])


# ---- 2: RDS, exact ----------------------------------------------------------------------------------------------------
def test_rds_groups_are_exact():
    groups = rf.ps_groups(0xC0DE, "MPX  IN ", n=int(N / FS / (104 * rf.TD)) + 2)
    x = rf.mpx_iq(rf.known_mpx(N, groups, kind="stereo"))[None, :]

    def read(ch):
        return ch.rds_groups(0), ch.rds_status(0)

    a, cha, _ = chain_a(x, stereo=True, enable_rds=True)
    ga, sa = read(cha)
    cha.close()
    assert len(ga) >= 4, len(ga)
    b, chb, _ = chain_b(a["mpx"], [BLK] * NB, stereo=True, rds=True)
    gb, sb = read(chb)
    rho = chb.rds_reliabilities(0)
    chb.close()
    assert same_bits(ga, gb) and fmr.rds_pi(gb) == 0xC0DE
    assert (sa.synced, sa.blocks_bad, sa.groups_dropped) == (sb.synced, sb.blocks_bad, sb.groups_dropped)
    assert len(rho) > 0 and np.isfinite(rho).all()
    assert_same_decoder(a, b, "rds")


# ---- 3: bit parity of the front end -----------------------------------------------------------------------------------
def pcm_of(n, rate, fmt):
    """The first n samples of A's MPX, both streams, as the MPX output would archive them (its fixture, default gain 0.5)."""
    key = ("pcm", n, rate, fmt)
    if key not in _cache:
        mpx = base()["mpx"]
        _cache[key] = np.stack([mo.run(mpx[s, :n], rate, 0.5, mo.PCM_S16 if fmt == "s16" else mo.PCM_F32)[0] for s in range(2)])
    return _cache[key]


def feed(ch, pcm, calls, taps=True):
    """pcm [S, F] through process_blocks, one call per entry of `calls`: the audio, every audio_len, and the joined tap 1."""
    S = ch.n_streams
    audio, alens, tap, pos = [], [], [[] for _ in range(S)], 0
    for ll in calls:
        m = int(sum(ll))
        a, al = ch.process_blocks(pcm[:, pos:pos + m], ll)
        audio.append(a)
        alens += [int(v) for v in al]
        if taps:
            for s in range(S):
                tap[s].append(ch.debug_read(1, stream=s, cap=1 << 18) if m else np.zeros(0, np.float32))
        pos += m
    return np.concatenate(audio, axis=1), alens, [np.concatenate(t) if t else None for t in tap]


@pytest.mark.parametrize("rate,fmt", [(192000, "s16"), (171000, "s16"), (256000, "f32"), (96000, "f32")])
def test_front_end_bit_parity(rate, fmt):
    pcm = pcm_of(SHORT, rate, fmt)
    F = pcm.shape[1]
    L, M, T, K, delay = mi.geometry(rate)
    # blocks that are no multiple of anything, one workgroup and many, an empty one, in calls of several blocks
    lens = [4096, 1, 0, 777, 4095, 257] + [4096] * ((F - 9226) // 4096)
    lens.append(F - sum(lens))
    calls = [lens[:3], lens[3:6], lens[6:]]
    ch = fmr.MpxChain(rate=rate, format=fmt, gain=0.0, n_streams=2, max_block_len=4096, max_blocks=len(lens))
    audio, alens, tap = feed(ch, pcm, calls)
    info = [ch.mpx_input_info(s) for s in range(2)]
    ch.close()
    refs = []
    for s in range(2):
        ref, nf = mi.run(pcm[s], rate, 2.0)
        refs.append(ref)
        d = np.abs(tap[s].astype(np.float64) - ref).max() if len(tap[s]) == len(ref) else -1.0
        print(f"rate {rate} {fmt} stream {s}: {len(ref)} MPX samples, largest |tap - fixture| = {d:.3e}")
        assert same_bits(tap[s], ref)
        assert info[s] == mi.info(rate, 2.0, F, mi.PCM_S16 if fmt == "s16" else mi.PCM_F32, nf), info[s]
    assert info[0]["delay_samples"] == delay and info[0]["samples_out"] == len(refs[0])
    # per-block audio_len: what an MpxChain at 384000 makes of the fixture's floats in blocks of the count law's MPX counts
    cnt = [int(c) for c in mi.block_counts(lens, L, M)]
    assert sum(cnt) == len(refs[0]) and cnt[2] == 0
    ch = fmr.MpxChain(rate=384000, format="f32", gain=1.0, n_streams=2, max_block_len=max(cnt), max_blocks=len(cnt))
    audio2, alens2, _ = feed(ch, np.stack(refs), [cnt[:3], cnt[3:6], cnt[6:]], taps=False)
    ch.close()
    assert alens == alens2 and sum(alens) == audio.shape[1] and alens[2] == 0
    assert same_bits(audio, audio2)


# ---- 4: the decoder behind it, exact ----------------------------------------------------------------------------------
def test_decoder_behind_the_front_end_is_exact():
    """B at 192000 S16 against B' at 384000 F32 gain 1.0 fed the fixture's floats in blocks of B's per-block MPX counts."""
    rate = 192000
    pcm = pcm_of(N, rate, "s16")
    L, M, T, K, _ = mi.geometry(rate)
    lens = [BLK // 2] * (pcm.shape[1] // (BLK // 2))
    lens.append(pcm.shape[1] - sum(lens))
    lens = [v for v in lens if v]
    b, ch, _ = chain_b(pcm, lens, rate=rate, fmt="s16", gain=0.0, max_blocks=len(lens), stereo=True)
    ch.close()
    x = np.stack([mi.run(pcm[s], rate, 2.0)[0] for s in range(2)])
    cnt = [int(v) for v in mi.block_counts(lens, L, M)]
    b2, ch, _ = chain_b(x, cnt, max_blocks=len(cnt), stereo=True)
    ch.close()
    assert_same_decoder(b2, b, "192000 S16 against 384000 F32")
    assert all(st["stereo"] == 1 for st in b["status"]) and all(len(p) >= 1 for p in b["pps"])
    # the archive's decode is the IQ chain's audio, later by both filters' delay: same length law, same programme
    a = base()
    assert abs(int(b["alen"].sum()) - int(a["alen"].sum())) <= 2


# ---- 5: cuts ----------------------------------------------------------------------------------------------------------
def run_171(pcm, calls, max_blocks):
    ch = fmr.MpxChain(rate=171000, format="s16", gain=0.0, n_streams=2, max_block_len=4096, max_blocks=max_blocks)
    ch.enable_mpx_output(format="f32", rate=384000, gain=1.0, max_frames=1 << 17)
    audio, alens, _ = feed(ch, pcm, calls, taps=False)
    ring = np.stack([ch.mpx_output_read(s)[0] for s in range(2)])
    info = ch.mpx_input_info(0)
    ch.close()
    return audio, alens, ring, info


def test_cuts():
    """One call against ragged calls at 171000: the MPX (the ring at 384000 F32, gain 1.0) and the counters are equal bit for
    bit and equal to the fixture's, and every block's audio_len is the same.

    The audio of different groupings.  The decoder behind the front end solves its recurrences -- the pilot PLL, the DC
    block -- in chunks laid out from the start of each call (kernels_par.hpp), so two groupings of the same blocks round
    differently behind a bit-identical MPX: measured on the MI355X, 7.3e-12 at most, one call against 70 ragged calls and
    against calls of 7 blocks.  That is the decoder's, not the front end's: each grouping's audio is, bit for bit, the audio
    of an MpxChain at 384000 F32 fed the fixture's floats in the same grouping (asserted).  Across groupings the audio is
    held to the bound the project holds every chain's audio to against the serial reference, 1e-5:
    two groupings that each meet it lie within 2e-5 of each other."""
    rate = 171000
    L, M, T, K, _ = mi.geometry(rate)
    pcm = pcm_of(SHORT, rate, "s16")
    F = pcm.shape[1]
    head = [[1], [0, 5, 0]] + [[65]] * 64 + [[K - 2]]
    used = sum(sum(c) for c in head)
    rest = [4096] * ((F - used) // 4096)
    rest.append(F - used - sum(rest))
    ragged = head + [rest[:2], rest[2:]]
    blocks = [v for c in ragged for v in c]
    audio1, alens1, ring1, info1 = run_171(pcm, [blocks], len(blocks))
    audio2, alens2, ring2, info2 = run_171(pcm, ragged, len(blocks))
    ref = np.stack([mi.run(pcm[s], rate, 2.0)[0] for s in range(2)])
    assert same_bits(ring1, ref) and same_bits(ring2, ref)
    assert info1 == info2 == mi.info(rate, 2.0, F)
    assert alens1 == alens2
    # the same blocks grouped into different calls: the same audio
    regroup = [blocks[i:i + 7] for i in range(0, len(blocks), 7)]
    audio3, alens3, ring3, _ = run_171(pcm, regroup, len(blocks))
    d12 = np.abs(audio1 - audio2).max()
    d13 = np.abs(audio1 - audio3).max()
    print(f"cuts: largest audio difference one call / ragged calls {d12:.3e}, one call / calls of 7 blocks {d13:.3e}")
    assert same_bits(ring3, ref) and alens3 == alens1
    assert audio1.shape == audio2.shape == audio3.shape and audio1.any()
    assert d12 <= 2e-5 and d13 <= 2e-5
    # the front end adds nothing that depends on the calls: behind the same MPX in the same grouping, the same bits
    for calls, audio in ((ragged, audio2), (regroup, audio3)):
        cnt = [[int(c) for c in mi.block_counts(ll, L, M, frames_before=f0)] for ll, f0 in
               zip(calls, np.concatenate([[0], np.cumsum([sum(ll) for ll in calls])[:-1]]))]
        ch = fmr.MpxChain(rate=384000, format="f32", gain=1.0, n_streams=2, max_block_len=max(max(c) for c in cnt),
                          max_blocks=len(blocks))
        twin, alens_t, _ = feed(ch, ref, cnt, taps=False)
        ch.close()
        assert alens_t == alens1 and same_bits(twin, audio)


# ---- 6: non-finite input ----------------------------------------------------------------------------------------------
def test_nonfinite_input():
    rate = 192000
    clean = pcm_of(SHORT, rate, "f32")
    dirty = clean.copy()
    dirty[0, 1000] = np.nan
    dirty[0, 20001] = np.inf
    lens = [4096] * (clean.shape[1] // 4096)
    out = {}
    for name, pcm in (("clean", clean), ("dirty", dirty)):
        ch = fmr.MpxChain(rate=rate, format="f32", gain=0.0, n_streams=2, max_block_len=4096, max_blocks=len(lens))
        audio, alens, tap = feed(ch, pcm, [lens[:3], lens[3:]])
        out[name] = (audio, tap, [ch.mpx_input_info(s)["nonfinite_in"] for s in range(2)])
        ch.close()
    assert out["clean"][2] == [0, 0] and out["dirty"][2] == [2, 0]
    ref, nf = mi.run(dirty[0, :sum(lens)], rate, 2.0)
    assert nf == 2 and same_bits(out["dirty"][1][0], ref) and np.isfinite(ref).all()
    assert same_bits(out["dirty"][1][1], out["clean"][1][1]) and same_bits(out["dirty"][0][1], out["clean"][0][1])
    assert not same_bits(out["dirty"][1][0], out["clean"][1][0])


# ---- 7: stages --------------------------------------------------------------------------------------------------------
def _stages(ch):
    ch.enable_monitor(interval_samples=98304)
    ch.enable_loudness()
    ch.enable_analyser()
    ch.enable_weak_signal()
    ch.enable_output(format="s16")


def _stage_reads(ch):
    out = {}
    for s in range(ch.n_streams):
        recs, hist, psd, _ = ch.monitor_records(s)
        out[("mon", s)] = (recs, hist, psd)
        out[("ld", s)] = ch.loudness_records(s)[:1]
        out[("an", s)] = ch.analyser_records(s)[:2]
        out[("ws", s)] = ch.weak_signal_records(s)[:1]
        pcm, blocks, _ = ch.output_read(s)
        out[("out", s)] = (pcm, blocks)
    return out


def test_stages_return_what_they_return_on_the_iq_chain():
    a, cha, _ = chain_a(stereo=True, setup=_stages)
    ra = _stage_reads(cha)
    cha.close()
    assert same_bits(a["mpx"], base()["mpx"])
    b, chb, _ = chain_b(a["mpx"], [BLK] * NB, stereo=True, setup=_stages)
    rb = _stage_reads(chb)
    chb.close()
    assert_same_decoder(a, b, "stages")
    for key in ra:
        if key[0] == "out":
            (pa, ba), (pb, bb) = ra[key], rb[key]
            assert same_bits(pa, pb) and len(ba) == len(bb) == NB and pa.any()
            for f in ba.dtype.names:
                if f in ("if_rms", "if_level"):
                    assert not bb[f].any() and ba[f].all()
                else:
                    assert same_bits(ba[f], bb[f]), (key, f)
        else:
            assert len(ra[key][0]) >= 1 or key[0] == "ws", key
            for u, v in zip(ra[key], rb[key]):
                assert same_bits(u, v), key


def test_stage_refusals():
    ch = fmr.MpxChain(rate=192000, n_streams=1, max_block_len=BLK, max_blocks=2)
    L = ch._L
    for call, word in ((lambda: ch.enable_output(squelch_level=0.01), "squelch"), (ch.enable_rf_monitor, "RF monitor"),
                       (ch.enable_blanker, "blanker"), (ch.enable_iq_correction, "IQ corrector")):
        with pytest.raises(fmr.FmrError, match=word) as e:
            call()
        assert f"error {fmr.ERR_UNSUPPORTED}" in str(e.value) and ("MPX decoder" in str(e.value) or "composite" in str(e.value))
    ch.enable_output(squelch_level=0.0)
    for which in (0, 4, 6, 7, 5):
        with pytest.raises(fmr.FmrError):
            ch.debug_read(which, cap=16)
    with pytest.raises(fmr.FmrError, match="RDS"):
        ch.rds_groups(0)
    ch.close()


# ---- 8: lifecycle -----------------------------------------------------------------------------------------------------
def test_lifecycle():
    live = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError) as e:
        fmr.MpxChain(rate=100001)
    assert e.value.code == fmr.ERR_BAD_ARG and fmr.debug_live_resources() == live
    ch = fmr.MpxChain(rate=192000, format="s16", n_streams=1, max_block_len=4096, max_blocks=2)
    iq = fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, max_block_len=4096, max_blocks=2)
    assert fmr.debug_live_resources() > live
    import torch
    x = np.zeros(4096, dtype=np.complex64)
    pcm = np.zeros((1, 4096), dtype=np.int16)
    d_in = torch.zeros(4096 * 2, dtype=torch.float32, device="cuda")
    d_au = torch.zeros(4096, dtype=torch.float64, device="cuda")
    # the wrong process entry, in both directions
    for call in (lambda: fmr.Chain.process_blocks(ch, x, [4096]), lambda: fmr.Chain.process(ch, x), lambda: fmr.Chain.resample(ch, x),
                 lambda: fmr.Chain.resample_blocks(ch, x, [4096]),
                 lambda: fmr.Chain.process_blocks_device(ch, d_in.data_ptr(), 4096, [16], d_au.data_ptr(), 4096)):
        with pytest.raises(fmr.FmrError, match="MPX decoder"):
            call()
    for call in (lambda: fmr.MpxChain.process_blocks(_as_mpx(iq), pcm, [4096]),
                 lambda: fmr.MpxChain.process_blocks_device(iq, d_in.data_ptr(), 4096, [16], d_au.data_ptr(), 4096),
                 lambda: fmr.MpxChain.mpx_input_info(iq)):
        with pytest.raises(fmr.FmrError, match="fmr_create_mpx_decoder"):
            call()
    # capacity, then a call, then an enable after it
    with pytest.raises(fmr.FmrError):
        ch.process_blocks(np.zeros((1, 3 * 4096), dtype=np.int16), [4096] * 3)
    audio, alen = ch.process_blocks(pcm, [4096])
    assert audio.shape == (1, int(alen.sum())) and 0 < int(alen.sum()) <= 2 * (8192 // 8 + 1) and not audio.any()
    assert ch.mpx_input_info()["frames_in"] == 4096 and ch.mpx_input_info()["samples_out"] == 8192
    with pytest.raises(fmr.FmrError, match="already taken samples"):
        ch.enable_monitor()
    ch.close()
    iq.close()
    assert fmr.debug_live_resources() == live


def _as_mpx(iq):
    iq.format = fmr.PCM_S16
    return iq


# ---- 9: the C++ facade ------------------------------------------------------------------------------------------------
def test_facade_smoke(tmp_path):
    """FmDecoder -> 192 kHz S16 WAV -> MpxFileReader -> MpxDecoder -> audio (tests/mpx_input_smoke.cpp)."""
    fmr.build_library()
    exe = str(tmp_path / "mpx_input_smoke")
    pkg = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(pkg, 'host')}",
                    os.path.join(ROOT, "tests", "mpx_input_smoke.cpp"), "-o", exe, f"-L{pkg}", "-lfmradion_amd",
                    f"-Wl,-rpath,{pkg}"], check=True)
    r = subprocess.run([exe, str(tmp_path / "mpx.wav")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "OK" in r.stdout

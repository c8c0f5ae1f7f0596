"""Channel bank on the GPU (fmr_config.channel_offset_hz): K stations decoded out of one wideband capture, every channel
against the oracle chain fed u_s = the capture mixed down by its offset (tests/chanbank_fixture.py)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import oracle_py as ora
import siggen
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def ragged_calls(total, seed, short_at=(0, 17)):
    """Calls of up to 40 ragged blocks (70 % full 65536-sample blocks); the calls at the indices in short_at are one
    block of a few samples."""
    rng = np.random.default_rng(seed)
    calls, n, i = [], 0, 0
    while n < total:
        if i in short_at:
            ll = [3 + i % 5]
        else:
            ll = [65536 if rng.random() < 0.7 else int(rng.integers(1, 65537)) for _ in range(int(rng.integers(1, 41)))]
        calls.append(ll)
        n += sum(ll)
        i += 1
    return calls


def run_bank(ch, x, calls):
    got = [[] for _ in range(ch.n_streams)]
    alens, pos = [], 0
    for ll in calls:
        m = sum(ll)
        a, alen = ch.process_blocks(x[pos:pos + m], ll)
        for s in range(ch.n_streams):
            got[s].append(a[s])
        alens += list(alen)
        pos += m
    return [np.concatenate(g) for g in got], alens


FM6_OFFS = [-4_100_000, -2_300_000, -700_000, -300_000, 1_234_567, 4_450_000]
FM6_IDS = [2, 7, 13, 19, 26, 31]
FM6_AMPS = [0.3, 0.095, 0.2, 0.13, 0.25, 0.11]       # about 10 dB


@pytest.mark.parametrize("cls", ["fast", "r8b"])
def test_six_fm_stations_10m(cls, pilotcut, monkeypatch):
    """Six FM-stereo stations in one 10 MS/s capture (two 400 kHz apart, one offset whose phase period is the full 10^7
    samples), ragged calls of up to 40 blocks over 0.75 s, calls of a few samples that yield no IF sample among them."""
    F = 10e6
    r8b = cls == "r8b"
    if r8b:
        monkeypatch.setenv("FMR_DEBUG_TAPS", "1")     # (the IF tap sits behind k_ifr_poly5h's discriminator epilogue)
    calls = ragged_calls(7_500_000, 11)
    n = sum(map(sum, calls))
    x = cb.composite(n, F, FM6_OFFS, FM6_IDS, FM6_AMPS)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=65536, max_blocks=40,
                   resampler_class=fmr.RESAMPLER_R8B if r8b else fmr.RESAMPLER_FAST, channel_offsets_hz=FM6_OFFS)
    got, alens = run_bank(ch, x, calls)
    lens = [b for ll in calls for b in ll]
    assert ch.channel_bank_forms() == {"modtap"}
    assert not ({"fused", "decim16"} & ch.front_end_forms())
    assert ch._L.fmr_resampler_info(ch.h, 6) == 0          # a bank's stage A sets no FMR_FE_* bit
    for s, (f, i) in enumerate(zip(FM6_OFFS, FM6_IDS)):
        fm, out = cb.oracle_fm(cb.mix_down(x, f, F), F, lens, pilotcut, r8b=r8b, delay=fmr.DELAY_3TAPS)
        assert alens == [len(q) for q in out], s
        ref = np.concatenate(out)
        assert len(got[s]) == len(ref) > 60000
        err = rms(got[s] - ref)
        assert err < 1e-5, (s, err)
        st = ch.status(s)
        assert st.stereo_detected == int(fm.stereo_detected()) == 1, s
        assert st.if_rms == pytest.approx(fm.get_if_rms(), rel=1e-5)
        assert st.if_agc_gain == pytest.approx(fm.get_if_agc_gain(), rel=1e-4)
        assert st.pilot_level == pytest.approx(fm.get_pilot_level(), rel=4e-6)
        assert abs(cb.peak_hz(got[s][0::2][-24000:], 48000.0) - cb.left_tone(i)) < 3.0, s
    ch.close()


# (mode, F, class, offsets): FM 2.5 M both classes, 3 M R8B, 6 M FAST, NBFM 2.4 M -> 48 k, AM 1.48 M -> 48 k
SHAPES = [
    ("fm", 2.5e6, "fast", [-700_000, 250_000]),
    ("fm", 2.5e6, "r8b", [-500_000, 0, 1_000_000]),
    ("fm", 3e6, "r8b", [-1_200_000, 400_000]),
    ("fm", 6e6, "fast", [-2_000_000, 123_457, 2_500_000]),
    ("nbfm", 2.4e6, "fast", [-1_000_000, 33_333, 900_000]),
    ("am", 1.48e6, "fast", [-600_000, 200_000]),
    # eleven channels: two channel groups of k_ifr_chan (grid.y = 2, the second group zero-padded)
    ("fm", 10e6, "fast", [-4_500_000 + 900_000 * i + 7 * i for i in range(11)]),
]


@pytest.mark.parametrize("mode, F, cls, offs", SHAPES, ids=[f"{m}_{F / 1e6:g}M_{c}" for m, F, c, _ in SHAPES])
def test_if_of_other_shapes(mode, F, cls, offs, monkeypatch):
    """The IF of every channel against ora.IfResampler of u_s (rel RMS < 2e-6, test_gpu_parity's bound)."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    r8b = cls == "r8b"
    dec = 384e3 if mode == "fm" else 48e3
    n = 40 * 16384
    x = cb.composite(n, F, offs, list(range(3, 3 + len(offs))), [(0.3, 0.12, 0.2)[i % 3] for i in range(len(offs))])
    m = {"fm": fmr.MODE_FM, "nbfm": fmr.MODE_NBFM, "am": fmr.MODE_AM}[mode]
    coeff = None if mode == "fm" else fmr.filter_table("jj1bdx_nbfm_48khz_default" if mode == "nbfm" else "jj1bdx_am_48khz_default")
    ch = fmr.Chain(mode=m, input_rate=F, enable_resampler=True, stereo=True, filter_coeff=coeff, max_block_len=16384,
                   max_blocks=40, resampler_class=fmr.RESAMPLER_R8B if r8b else fmr.RESAMPLER_FAST, channel_offsets_hz=offs,
                   nbfm_freq_dev=0.0)
    ch.process_blocks(x, [16384] * 40)
    assert ch.channel_bank_forms() == {"modtap"}
    for s, f in enumerate(offs):
        r = ora.IfResampler(F, dec, 180.0, 0.98, True) if r8b else ora.IfResampler(F, dec)
        ref = np.concatenate([r.process(b) for b in siggen.blocks(cb.mix_down(x, f, F), 16384)])
        got = ch.debug_read(0, stream=s)
        assert len(got) == len(ref), (s, len(got), len(ref))
        rel = rms(got - ref) / rms(ref)
        assert rel < 2e-6, (s, rel)
    ch.close()


def test_quarter_rate_offset_equals_fourth_down(pilotcut):
    """A one-channel bank at +F/4 (2.4 MS/s) and a plain chain with enable_fourth_down both follow FourthConverterIQ(False)
    -> IfResampler -> FmDecoder."""
    F, blk, nb = 2.4e6, 16384, 60
    x = cb.composite(blk * nb, F, [600_000, -400_000], [4, 9], [0.3, 0.15])
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=nb)
    bank = fmr.Chain(channel_offsets_hz=[600_000], **kw)
    plain = fmr.Chain(fourth_down=True, **kw)
    a_bank, _ = bank.process_blocks(x, [blk] * nb)
    a_plain, _ = plain.process_blocks(x[None, :], [blk] * nb)
    f4, r = ora.FourthConverterIQ(False), ora.IfResampler(F, 384e3)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
    ref = np.concatenate([fm.process(r.process(f4.process(b))) for b in siggen.blocks(x, blk)])
    assert len(a_bank[0]) == len(a_plain[0]) == len(ref)
    assert rms(a_bank[0] - ref) < 1e-5 and rms(a_plain[0] - ref) < 1e-5
    bank.close(); plain.close()


def test_bank_equals_plain_chain_on_premixed_copies(monkeypatch):
    """Three channels, one at offset 0, against the plain 3-stream chain fed the mixed-down copies."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    F, blk, nb = 6e6, 65536, 24
    offs = [0, -1_500_000, 2_200_000]
    x = cb.composite(blk * nb, F, offs, [1, 5, 8], [0.3, 0.1, 0.2])
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=nb)
    bank = fmr.Chain(channel_offsets_hz=offs, **kw)
    plain = fmr.Chain(n_streams=3, **kw)
    a_bank, _ = bank.process_blocks(x, [blk] * nb)
    a_plain, _ = plain.process_blocks(np.stack([cb.mix_down(x, f, F) for f in offs]), [blk] * nb)
    for s in range(3):
        ib, ip = bank.debug_read(0, stream=s), plain.debug_read(0, stream=s)
        assert len(ib) == len(ip)
        assert rms(ib - ip) / rms(ip) < 2e-6, s
        assert rms(a_bank[s] - a_plain[s]) < 1e-5, s
    bank.close(); plain.close()


def test_nan_and_dropout(pilotcut, monkeypatch):
    """test_carrier_dropout_and_nan_samples's events in the capture.  Every channel follows its oracle through the cold
    start and the dropout and after the NaN, and no NaN reaches any channel's audio.  Around the NaN the bank's stage A
    must poison exactly what a plain chain's stage A poisons: the IF of every channel, NaN positions included, equals
    that of the plain 3-stream chain with the same stage B (k_ifr_poly4, FMR_NO_FUSED=1) fed the mixed-down copies, and so
    does the audio.  (That stage B widens a NaN to its banded tile, unlike the fused front end: DESIGN.md.)"""
    F, blk, nblk, batch = 10e6, 65536, 160, 40
    offs, ids = [-3_000_000, 0, 2_600_000], [3, 6, 12]
    x = cb.composite(nblk * blk, F, offs, ids, [0.3, 0.15, 0.2])
    k0 = 50 * blk + 777
    x[k0:k0 + 8000] = 0
    k1 = 85 * blk + 4321
    x[k1:k1 + 3] = np.complex64(complex(np.nan, np.nan))
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=batch)
    ch = fmr.Chain(channel_offsets_hz=offs, **kw)
    monkeypatch.setenv("FMR_NO_FUSED", "1")
    plain = fmr.Chain(n_streams=3, **kw)
    u = [cb.mix_down(x, f, F) for f in offs]
    got = [[] for _ in offs]
    pg = [[] for _ in offs]
    for c in range(nblk // batch):
        lo, hi = c * batch * blk, (c + 1) * batch * blk
        a, _ = ch.process_blocks(x[lo:hi], [blk] * batch)
        b, _ = plain.process_blocks(np.stack([v[lo:hi] for v in u]), [blk] * batch)
        for s in range(len(offs)):
            got[s].append(a[s])
            pg[s].append(b[s])
            if lo <= k1 < hi:          # the call that holds the NaN samples
                ib, ip = ch.debug_read(0, stream=s), plain.debug_read(0, stream=s)
                assert len(ib) == len(ip)
                nb_, np_ = ~np.isfinite(ib), ~np.isfinite(ip)
                assert nb_.any() and np.array_equal(nb_, np_), s
                assert rms(ib[~nb_] - ip[~np_]) / rms(ip[~np_]) < 2e-6, s
    lens = [blk] * nblk
    for s, f in enumerate(offs):
        fm, out = cb.oracle_fm(u[s], F, lens, pilotcut, delay=fmr.DELAY_3TAPS)
        ref = np.concatenate(out)
        g, p = np.concatenate(got[s]), np.concatenate(pg[s])
        assert len(g) == len(ref) == len(p)
        assert not np.isnan(g).any() and not np.isnan(ref).any()
        a0 = 2 * int((k1 / F - 0.002) * 48000)
        a1 = 2 * int((k1 / F + 0.35) * 48000)
        assert rms((g - ref)[:a0]) < 1e-5, s
        assert rms((g - ref)[a1:]) < 1e-5, s
        assert float(np.max(np.abs(g - p))) < 1e-3 and rms(g - p) < 1e-5, s
    ch.close(); plain.close()


def test_call_paths():
    """Host API == device API (one-row tensor, asynchronous calls); pipelined == in_order bit for bit; fmr_process on a
    one-channel bank == process_blocks."""
    import torch
    F, blk, nb, ncall = 10e6, 65536, 8, 4
    offs = [-1_000_000, 2_000_000]
    x = cb.composite(blk * nb * ncall, F, offs, [2, 4], [0.3, 0.2])
    kw = dict(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=nb,
              channel_offsets_hz=offs)
    calls = [[blk] * nb] * ncall
    host, _ = run_bank(fmr.Chain(**kw), x, calls)
    inord, _ = run_bank(fmr.Chain(in_order=True, **kw), x, calls)
    for s in range(2):
        assert np.array_equal(host[s], inord[s]), s
    dev = fmr.Chain(**kw)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    astride = 2 * (blk * nb // 20 + 64 * nb)
    d_a = torch.zeros((ncall, 2, astride), dtype=torch.float64, device="cuda")
    alens = []
    for c in range(ncall):
        off = c * blk * nb
        alens.append(dev.process_blocks_device(d_x.data_ptr() + 8 * off, 0, [blk] * nb, d_a[c].data_ptr(), astride))
    dev.synchronize()
    a = d_a.cpu().numpy()
    for s in range(2):
        g = np.concatenate([a[c, s, :int(alens[c].sum())] for c in range(ncall)])
        assert np.array_equal(g, host[s]), s
    one = fmr.Chain(**dict(kw, channel_offsets_hz=[offs[0]], max_blocks=1))
    two = fmr.Chain(**dict(kw, channel_offsets_hz=[offs[0]], max_blocks=1))
    p1 = np.concatenate([one.process(x[i * blk:(i + 1) * blk]) for i in range(nb)])
    p2 = np.concatenate([two.process_blocks(x[i * blk:(i + 1) * blk], [blk])[0][0] for i in range(nb)])
    assert len(p1) > 0 and np.array_equal(p1, p2)
    # fmr_process returns one audio row: a bank of more than one channel is refused there
    with pytest.raises(fmr.FmrError, match="fmr_process"):
        fmr.Chain(**dict(kw, max_blocks=1)).process(x[:blk])


def test_facade_channel_bank(tmp_path):
    """tests/channel_bank_smoke.cpp through the facade: a two-station capture, both channels report stereo."""
    exe = str(tmp_path / "channel_bank_smoke")
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}"]
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", *inc, os.path.join(ROOT, "tests", "channel_bank_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stereo 1 1" in r.stdout, r.stdout

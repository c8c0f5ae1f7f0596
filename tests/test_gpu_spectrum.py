"""Band spectrum on the GPU (fmr_spectrum_*) against the float64 Welch oracle of
tests/spectrum_fixture.py, and the scan -> channel bank flow.

Bound of the oracle comparison, per bin: |P - P_ref| <= 1e-4 P_ref + 1e-12 max P_ref (an fp32 FFT of log2 N passes,
input and twiddles rounded once to fp32: ~1e-6 expected)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import chanbank_fixture as cb
import spectrum_fixture as sf

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 10e6


def scene(n, rows=1, seed=0, noise=3e-2):
    """White noise plus tones (different per row), complex64 (rows, n).  The noise floor sits 50-60 dB below the
    strongest tone's bin: an fp32 FFT's error in a bin is of the order of eps times the strongest bin's amplitude, so
    a bin far further down than that is not resolved to 1e-4 of its own power in one segment."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    out = np.empty((rows, n), np.complex64)
    for r in range(rows):
        x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
        for k in range(3):
            f = rng.uniform(-0.45, 0.45) * F
            x = x + 10 ** rng.uniform(-2.5, -0.3) * np.exp(2j * np.pi * (f * t / F + rng.random()))
        out[r] = x.astype(np.complex64)
    return out


def run(sp, x, cuts):
    o = 0
    for c in cuts:
        sp.process(x[:, o:o + c])
        o += c
    assert o == x.shape[1]


def assert_oracle(sp, x, N, H, win, seg_lo=0, rel=1e-4):
    for r in range(x.shape[0]):
        mean, peak, cnt, skp = sf.welch(x[r], N, H, win, F, seg_lo=seg_lo)
        info = sp.info(r)
        assert info["segments"] == cnt and info["segments_skipped"] == skp, (r, info, cnt, skp)
        gm, gp = sp.psd(r), sp.peak_hold(r)
        assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gp))
        ok, worst = sf.close(gm, mean, rel)
        assert ok, ("mean", r, worst)
        ok, worst = sf.close(gp, peak, rel)
        assert ok, ("peak", r, worst)


@pytest.mark.parametrize("N", [256, 1024, 8192, 16384])
@pytest.mark.parametrize("win", [sf.HANN, sf.RECT, sf.BLACKMAN_HARRIS])
def test_mean_and_peak_against_oracle(N, win):
    for H in (N, N // 2, N // 4, 3 * N // 8):
        n = 24 * N + 17
        x = scene(n, rows=3, seed=N + H + win)
        sp = fmr.Spectrum(F, fft_size=N, hop=H, window=win, n_rows=3, max_call_len=n)
        run(sp, x, [n // 3, n - n // 3])
        assert_oracle(sp, x, N, H, win)
        info = sp.info(0)
        assert info["bin_hz"] == F / N and info["samples_seen"] == n
        w = sf.window(win, N)
        assert info["enbw_hz"] == pytest.approx(F * np.sum(w ** 2) / np.sum(w) ** 2, rel=1e-12)
        sp.close()


def test_scale_and_placement():
    N = 8192
    f = 1000 * F / N                                   # a bin centre
    n = 16 * N
    A = 0.5
    x = (A * np.exp(2j * np.pi * f * np.arange(n) / F)).astype(np.complex64)[None]
    sp = fmr.Spectrum(F, fft_size=N, hop=N, window=fmr.WINDOW_RECT, max_call_len=n)
    sp.process(x)
    p = sp.psd()
    assert int(np.argmax(p)) == N // 2 + 1000
    assert np.sum(p) * F / N == pytest.approx(A * A, rel=1e-5)
    assert sp.freqs()[N // 2 + 1000] == pytest.approx(f)
    # a -100 dBFS tone 1 MHz from a 0 dBFS one, Blackman-Harris: >= 20 dB above its neighbourhood
    f1, f2 = 1.5e6 + 0.3 * F / N, 2.5e6 + 0.3 * F / N
    t = np.arange(n)
    y = (np.exp(2j * np.pi * f1 * t / F) + 1e-5 * np.exp(2j * np.pi * f2 * t / F)).astype(np.complex64)[None]
    sp2 = fmr.Spectrum(F, fft_size=N, hop=N // 2, window=fmr.WINDOW_BLACKMAN_HARRIS, max_call_len=n)
    sp2.process(y)
    q = sp2.psd()
    k2 = N // 2 + int(round(f2 * N / F))
    near = np.concatenate([q[k2 - 60:k2 - 8], q[k2 + 8:k2 + 60]])
    assert 10 * np.log10(q[k2 - 2:k2 + 3].max() / np.median(near)) >= 20.0


CUTS = {
    "ragged": [5000, 77, 1, 1, 4000, 30000, 123, 9999, 2, 10797],
    "short": [300] * 200,
    "ones": [1] * 3000 + [57000],
}


def test_call_cuts():
    N, H = 1024, 384
    n = 60000
    x = scene(n, rows=2, seed=5)
    ref = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=2, max_call_len=n)
    ref.process(x)
    for name, cuts in CUTS.items():
        assert sum(cuts) == n, name
        outs = []
        for rep in range(2):
            sp = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=2, max_call_len=n)
            run(sp, x, cuts)
            outs.append([(sp.psd(r), sp.peak_hold(r)) for r in range(2)])
            sp.close()
        for r in range(2):
            np.testing.assert_array_equal(outs[0][r][1], ref.peak_hold(r), err_msg=name)
            m = ref.psd(r)
            assert np.all(np.abs(outs[0][r][0] - m) <= 1e-6 * m), name
            np.testing.assert_array_equal(outs[0][r][0], outs[1][r][0], err_msg=name)
            np.testing.assert_array_equal(outs[0][r][1], outs[1][r][1], err_msg=name)
    # a call that completes no segment changes nothing
    sp = fmr.Spectrum(F, fft_size=N, hop=H, max_call_len=n)
    sp.process(x[:1, :N - 1])
    assert sp.info()["segments"] == 0 and not np.any(sp.psd()) and not np.any(sp.peak_hold())
    sp.process(x[:1, N - 1:N])
    assert sp.info()["segments"] == 1


def test_device_path_and_raw_formats():
    import torch
    N, H, n = 2048, 1024, 50000
    x = scene(n, rows=2, seed=9)
    host = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=2, max_call_len=20000)
    dev = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=2, max_call_len=20000)
    stride = 20000 + 16
    d = torch.zeros((2, stride * 3), dtype=torch.complex64, device="cuda")
    cuts = [20000, 17, 19983, 10000]
    o = 0
    for c in cuts:
        host.process(x[:, o:o + c])
        d[:, :c] = torch.from_numpy(x[:, o:o + c].copy()).cuda()
        torch.cuda.synchronize()
        dev.process_device(d.data_ptr(), c, stride=d.shape[1], sync=False)
        dev.synchronize()
        o += c
    for r in range(2):
        np.testing.assert_array_equal(dev.psd(r), host.psd(r))
        np.testing.assert_array_equal(dev.peak_hold(r), host.peak_hold(r))
    # FMR_ERR_CAPACITY leaves the object as it was; the retry goes through
    before = (dev.psd(0), dev.info(0))
    with pytest.raises(fmr.FmrError, match="-4"):
        dev.process_device(d.data_ptr(), 20001, stride=d.shape[1])
    with pytest.raises(fmr.FmrError, match="-4"):
        dev.process(np.zeros((2, 20001), np.complex64))
    np.testing.assert_array_equal(dev.psd(0), before[0])
    assert dev.info(0) == before[1]
    dev.process_device(d.data_ptr(), 20000, stride=d.shape[1])
    host.process(d[:, :20000].cpu().numpy())
    np.testing.assert_array_equal(dev.psd(1), host.psd(1))
    # raw rows equal cf32 rows converted by the documented rule, bit for bit
    rng = np.random.default_rng(3)
    m = 30000
    raws = {
        fmr.IQ_S16: (rng.integers(-32768, 32768, (2, m, 2)).astype(np.int16), lambda v: v.astype(np.float32) / 32768.0),
        fmr.IQ_U8: (rng.integers(0, 256, (2, m, 2)).astype(np.uint8), lambda v: (v.astype(np.float32) - 128.0) / 128.0),
        fmr.IQ_S8: (rng.integers(-128, 128, (2, m, 2)).astype(np.int8), lambda v: v.astype(np.float32) / 128.0),
    }
    for fmt, (raw, conv) in raws.items():
        a = fmr.Spectrum(F, fft_size=1024, hop=300, n_rows=2, input_format=fmt, max_call_len=m)
        b = fmr.Spectrum(F, fft_size=1024, hop=300, n_rows=2, max_call_len=m)
        a.process(raw[:, :777])
        a.process(raw[:, 777:])
        f = conv(raw)
        b.process((f[..., 0] + 1j * f[..., 1]).astype(np.complex64))
        for r in range(2):
            np.testing.assert_array_equal(a.psd(r), b.psd(r), err_msg=str(fmt))
            np.testing.assert_array_equal(a.peak_hold(r), b.peak_hold(r), err_msg=str(fmt))


def test_non_finite_samples():
    N, H, n = 1024, 512, 40000
    x = scene(n, rows=2, seed=11)
    x[0, 5000] = np.nan
    x[0, 20000 + 700] = np.inf                           # inside the overlap of two segments
    x[1, 33333] = complex(0, -np.inf)
    x[1, 2] = complex(np.nan, 0)
    sp = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=2, max_call_len=n)
    run(sp, x, [7000, 13701, 19299])
    assert_oracle(sp, x, N, H, sf.HANN)
    assert sp.info(0)["segments_skipped"] == 2 + 2 and sp.info(1)["segments_skipped"] == 1 + 2


def test_reset():
    N, H, n = 1024, 256, 50000
    x = scene(n, rows=1, seed=12)
    sp = fmr.Spectrum(F, fft_size=N, hop=H, window=fmr.WINDOW_BLACKMAN_HARRIS, max_call_len=n)
    sp.process(x[:, :20000])
    done = sp.info()["segments"]
    sp.reset()
    assert sp.info()["segments"] == 0 and not np.any(sp.psd())
    assert sp.info()["first_segment"] == done
    sp.process(x[:, 20000:])
    assert_oracle(sp, x, N, H, sf.BLACKMAN_HARRIS, seg_lo=done)


def run_split(N, H, rows, max_call_len, n_seg):
    """(runs, segments per run) of one call as the engine splits it (fmradion_amd.hip, fmr_spectrum::init / run): about
    one workgroup per slot the chip holds at N (LDS and threads of k_spec_seg), shared by the rows, no more than a call's
    segments."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    logn = N.bit_length() - 1
    T = min(1024, N // 4)
    lds = (N + (N >> 5)) * 8
    occ = max(1, min(163840 // lds, 2048 // T))
    smax = (max_call_len + H - 1) // H + 1
    rmax = max(1, min(smax, (n_cu * occ + rows - 1) // rows))
    runs = min(n_seg, rmax)
    per_run = -(-n_seg // runs)
    assert logn >= 8
    return -(-n_seg // per_run), per_run


@pytest.mark.parametrize("N,H,rows,n", [(16384, 8192, 8, 100 * 8192), (256, 96, 1, 96 * 20000 + 160)])
def test_runs_of_many_segments_against_oracle(N, H, rows, n):
    """One call whose workgroups each take several segments (registers accumulate across the run, the LDS is reused
    segment after segment), with non-finite samples that skip segments in the middle of runs."""
    n_seg = (n - N) // H + 1
    runs, per_run = run_split(N, H, rows, n, n_seg)
    assert per_run >= 2, (runs, per_run)
    x = scene(n, rows=rows, seed=N + rows)
    mid = (runs // 2) * per_run + per_run // 2         # a segment inside a run, not its first
    x[0, mid * H + N // 2] = np.nan
    x[rows - 1, (mid + 1) * H + 3] = complex(np.inf, 0)
    x[rows - 1, n - 1] = np.nan                         # the call's last segment
    sp = fmr.Spectrum(F, fft_size=N, hop=H, window=fmr.WINDOW_HANN, n_rows=rows, max_call_len=n)
    sp.process(x)
    assert_oracle(sp, x, N, H, sf.HANN)
    assert sp.info(0)["segments_skipped"] >= 1 and sp.info(rows - 1)["segments_skipped"] >= 2


def test_runs_of_many_segments_call_cuts():
    """The same input as one call (several segments per workgroup), two halves, and calls of at most 50000 samples:
    bit-identical peak hold, the mean within 1e-6, the same cut twice gives the same bits."""
    N, H, rows, n = 1024, 384, 2, 1_200_000
    n_seg = (n - N) // H + 1
    assert run_split(N, H, rows, n, n_seg)[1] >= 2
    x = scene(n, rows=rows, seed=31)
    x[1, 400_000] = np.nan
    cuts = {"one": [n], "halves": [n // 2, n - n // 2], "small": [50000] * (n // 50000)}
    assert all(sum(c) == n for c in cuts.values())
    out = {}
    for name, cut in cuts.items():
        sp = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=rows, max_call_len=n)
        run(sp, x, cut)
        out[name] = [(sp.psd(r), sp.peak_hold(r), sp.info(r)["segments"], sp.info(r)["segments_skipped"]) for r in range(rows)]
        sp.close()
    sp = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=rows, max_call_len=n)
    run(sp, x, cuts["one"])
    for r in range(rows):
        np.testing.assert_array_equal(sp.psd(r), out["one"][r][0])
        np.testing.assert_array_equal(sp.peak_hold(r), out["one"][r][1])
        for name in ("halves", "small"):
            np.testing.assert_array_equal(out[name][r][1], out["one"][r][1], err_msg=name)
            m = out["one"][r][0]
            assert np.all(np.abs(out[name][r][0] - m) <= 1e-6 * m), name
            assert out[name][r][2:] == out["one"][r][2:], name
    assert_oracle(sp, x, N, H, sf.HANN)


def test_peak_hold_deep_bins():
    """Peak hold on bins 60-70 dB under the strongest tone's bin (noise 1e-2).  One segment's fp32 FFT is good there to
    the error model of DESIGN.md section 10: an amplitude error of at most e |X_max| per bin, e = log2(N) 2^-24, so
    |P - P_ref| <= 1e-4 P_ref + 2 e sqrt(P_ref max P_ref) + e^2 max P_ref (the 1e-4 term alone is met by the mean)."""
    for N in (8192, 16384):
        H = N // 2
        n = 24 * N
        x = scene(n, rows=2, seed=N + 7, noise=1e-2)
        x = (x + 0.5 * np.exp(2j * np.pi * 1.2345e6 * np.arange(n) / F)).astype(np.complex64)   # one tone at -6 dBFS
        sp = fmr.Spectrum(F, fft_size=N, hop=H, window=fmr.WINDOW_RECT, n_rows=2, max_call_len=n)
        sp.process(x)
        e = np.log2(N) * 2.0 ** -24
        for r in range(2):
            mean, peak, _, _ = sf.welch(x[r], N, H, sf.RECT, F)
            mx = peak.max()
            assert 10 * np.log10(mx / np.median(peak)) > 58.0          # most bins are that deep
            ok, worst = sf.close(sp.psd(r), mean)
            assert ok, ("mean", N, r, worst)
            bound = 1e-4 * peak + 2 * e * np.sqrt(peak * mx) + e * e * mx
            err = np.abs(sp.peak_hold(r) - peak)
            assert np.all(err <= bound), ("peak", N, r, float(np.max(err / bound)))


# six stations on the 100 kHz raster offset by 50 kHz, -10 .. -40 dB
SCAN_OFFS = [-3450000, -2150000, -850000, 650000, 1950000, 3750000]
SCAN_IDS = [1, 2, 3, 4, 5, 6]
SCAN_DB = [-10, -16, -22, -28, -34, -40]
README_RULE = dict(raster_hz=100000, raster_offset_hz=50000, bandwidth_hz=200000, threshold_db=10.0)


def test_scan_then_decode():
    n = 1 << 23
    amps = [10 ** (d / 20) for d in SCAN_DB]
    x = cb.composite(n, F, SCAN_OFFS, SCAN_IDS, amps)
    rng = np.random.default_rng(21)
    x = (x + 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    sp = fmr.Spectrum(F, fft_size=8192, max_call_len=n)
    sp.process(x)
    st = fmr.find_stations(sp.psd(), F, **README_RULE)
    offs = [s["offset_hz"] for s in st]
    assert offs == SCAN_OFFS, st
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=65536, max_blocks=128,
                   channel_offsets_hz=offs)
    audio, _ = ch.process_blocks(x[None, :n], [65536] * 128)
    for s, i in enumerate(SCAN_IDS):
        assert abs(cb.peak_hz(audio[s][0::2][-24000:], 48000.0) - cb.left_tone(i)) < 3.0, s
    ch.close()


def test_facade_spectrum_monitor(tmp_path):
    exe = str(tmp_path / "spectrum_smoke")
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(libdir, 'host')}", os.path.join(ROOT, "tests", "spectrum_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "stations -1150000 350000 2050000" in r.stdout and "bank channels 3" in r.stdout, r.stdout

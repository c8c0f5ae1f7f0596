"""The band spectrum's waterfall on the GPU (fmr_spectrum_create_waterfall / fmr_spectrum_read_waterfall, DESIGN.md
section 10) against the float64 oracle of tests/waterfall_fixture.py, and its cut independence bit for bit.

Bound of the oracle comparison: spectrum_fixture.close at its default (|P - P_ref| <= 1e-4 P_ref + 1e-12 max P_ref), the
bound the peak-hold tests apply to the same fp32 per-segment powers.  A MEAN line adds R of them in fp32, in sub-blocks of
8: at most 8 + R / 8 roundings of 2^-24 on one path (R = 1000: 133 x 6e-8 = 8e-6), well inside 1e-4.

Test signal (scene): a line of few segments shows single segments' powers, which the peak hold over a whole capture does
not.  An fp32 FFT's amplitude error in a bin is of the order of one rounding of the strongest bin, 2^-24 |X_max| (DESIGN.md
section 10), so a bin's power is good to 1e-4 of itself only down to 20 log10(1e-4 / 2^-23) = 58.5 dB under the strongest
bin.  The noise bins of a line are gamma distributed (the mean of R exponentials): among the M = rows x lines x N values a
test compares, the deepest is expected where M (R q)^R / R! = 1, that is -10 log10 q dB under the floor's mean (R = 1,
M = 3584: 35.5 dB; R = 2, M = 98304: 26.5 dB; R = 1000, M = 1024: 4.4 dB).  scene() therefore sets the noise so that the floor's mean
sits 58.5 dB less that figure under the strongest tone's bin, for every shape by the same rule."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import spectrum_fixture as sf
import waterfall_fixture as wf

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 10e6
WHICH = [wf.MEAN, wf.PEAK]


DEPTH_DB = 20 * np.log10(1e-4 / 2.0 ** -23)       # 58.5 dB: where 2^-24 |X_max| of amplitude is 1e-4 of a bin's power


def floor_db(N, H, R, n, rows, compared=None):
    """dB from the strongest tone's bin down to the noise floor's mean (the module docstring's rule); compared = M, the
    values a test holds to the oracle, where that is not every line of every row."""
    lines = max(1, ((n - N) // H + 1) // R)
    M = rows * lines * N if compared is None else compared
    log_q = (math.lgamma(R + 1) - math.log(M)) / R - math.log(R)
    return DEPTH_DB - max(0.0, -10 * log_q / math.log(10))


def scene(n, N, H, R, rows=1, seed=0, win=sf.HANN, compared=None):
    """White noise plus three tones per row (the kind test_gpu_spectrum.scene makes), the noise level by floor_db: a
    tone of amplitude A has the bin amplitude A sum w, the floor's mean power is sigma^2 sum w^2."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    w = sf.window(win, N)
    down = 10 ** (floor_db(N, H, R, n, rows, compared) / 20)
    out = np.empty((rows, n), np.complex64)
    for r in range(rows):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
        amps = []
        tones = np.zeros(n, np.complex128)
        for k in range(3):
            f = rng.uniform(-0.45, 0.45) * F
            amps.append(10 ** rng.uniform(-2.5, -0.3))
            tones = tones + amps[-1] * np.exp(2j * np.pi * (f * t / F + rng.random()))
        sigma = max(amps) * np.sum(w) / (np.sqrt(np.sum(w * w)) * down)
        out[r] = (sigma * x + tones).astype(np.complex64)
    return out


def length(N, H, R, lines, extra=17):
    """Samples that complete exactly `lines` lines, plus `extra` (< H: no further segment)."""
    return (lines * R - 1) * H + N + extra


def make(N, H, R, L, which, n, rows=1, win=sf.HANN, fmt=None):
    return fmr.Spectrum(F, fft_size=N, hop=H, window=win, n_rows=rows, max_call_len=n, waterfall_segments=R,
                        waterfall_lines=L, waterfall_which=which, **({} if fmt is None else {"input_format": fmt}))


def feed(sp, x, cuts):
    o = 0
    for c in cuts:
        sp.process(x[:, o:o + c])
        o += c
    assert o == x.shape[1]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,H,R,lines,win", [
    (256, 128, 3, 5, sf.HANN), (256, 256, 1, 7, sf.HANN), (1024, 100, 4, 4, sf.HANN), (1024, 100, 4, 4, sf.BLACKMAN_HARRIS),
    (16384, 8192, 2, 3, sf.HANN), (256, 32, 1000, 2, sf.HANN)])
def test_lines_against_oracle(N, H, R, lines, win, which):
    n = length(N, H, R, lines)
    x = scene(n, N, H, R, rows=2, seed=N + H + R, win=win)
    sp = make(N, H, R, lines + 1, which, n, rows=2, win=win)
    feed(sp, x, [n // 3, n - n // 3])
    for r in range(2):
        got, cnt, info = sp.waterfall(r)
        ref, rcnt = wf.lines(x[r], N, H, win, F, R, which)
        assert got.shape == (lines, N) and got.dtype == np.float32 and len(ref) == lines
        assert info["first_line"] == 0 and info["lines_ready"] == 0 and info["lines_dropped"] == 0
        assert info["line_seconds"] == R * H / F
        np.testing.assert_array_equal(cnt, rcnt)
        assert np.all(cnt == R)
        ok, worst = wf.close(got, ref)
        print("waterfall oracle", N, H, R, win, which, "row", r, "worst ratio", worst)
        assert ok, (N, H, R, which, r, worst)
    sp.close()


CUT_HEAD = [1, 127, 128, 129, 1000, 5]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,H,R", [(256, 128, 3), (256, 32, 20)])
def test_cut_independence_bit_for_bit(N, H, R, which):
    """One call against [1, 127, 128, 129, 1000, 5, rest] and a second cut.  At (256, 128, 3) a line is 384 samples: the
    1000-sample call completes the lines 0, 1 and 2, the calls of 1 and 5 samples are shorter than a hop, and the second
    cut has calls that end exactly on the last sample of line 0 (512 samples) and of line 1 (a one-sample call).  At
    (256, 32, 20) a line has sub-blocks of 8, 8 and 4 segments and the calls end inside them."""
    lines = 9
    n = length(N, H, R, lines, extra=0)                   # the input ends exactly on the last line's last sample
    x = scene(n, N, H, R, rows=2, seed=7 + R)
    end0, end1 = length(N, H, R, 1, 0), length(N, H, R, 2, 0)
    cuts = {"one": [n], "issue": CUT_HEAD + [n - sum(CUT_HEAD)],
            "line_ends": [end0, end1 - end0 - 1, 1, 2000, n - end1 - 2000]}
    out = {}
    for name, cut in cuts.items():
        sp = make(N, H, R, lines, which, n, rows=2)
        feed(sp, x, cut)
        out[name] = [sp.waterfall(r) for r in range(2)]
        sp.close()
    for r in range(2):
        ref, rcnt = wf.lines(x[r], N, H, sf.HANN, F, R, which)
        assert out["one"][r][0].shape == (lines, N)
        assert wf.close(out["one"][r][0], ref)[0]
        for name in ("issue", "line_ends"):
            np.testing.assert_array_equal(out[name][r][0], out["one"][r][0], err_msg=name)
            np.testing.assert_array_equal(out[name][r][1], out["one"][r][1], err_msg=name)
            np.testing.assert_array_equal(out[name][r][1], rcnt, err_msg=name)


def test_many_segments_call_cuts():
    """The shapes of test_gpu_spectrum.test_runs_of_many_segments_call_cuts (3123 segments per row): one call, two halves
    and calls of 50000 samples give the same lines and counts bit for bit, MEAN and PEAK; a NaN costs its line the segments that cover it."""
    N, H, rows, n, R = 1024, 384, 2, 1_200_000, 100
    x = scene(n, N, H, R, rows=rows, seed=31)
    x[1, 400_000] = np.nan
    cuts = {"one": [n], "halves": [n // 2, n - n // 2], "small": [50000] * (n // 50000)}
    nlines = ((n - N) // H + 1) // R
    for which in WHICH:
        out = {}
        for name, cut in cuts.items():
            sp = make(N, H, R, nlines, which, n, rows=rows)
            feed(sp, x, cut)
            out[name] = [sp.waterfall(r) for r in range(rows)]
            sp.close()
        for r in range(rows):
            ref, rcnt = wf.lines(x[r], N, H, sf.HANN, F, R, which)
            assert len(ref) == nlines == len(out["one"][r][0])
            np.testing.assert_array_equal(out["one"][r][1], rcnt)
            ok, worst = wf.close(out["one"][r][0], ref)
            assert ok, (which, r, worst)
            for name in ("halves", "small"):
                np.testing.assert_array_equal(out[name][r][0], out["one"][r][0], err_msg=name)
                np.testing.assert_array_equal(out[name][r][1], out["one"][r][1], err_msg=name)
        # row 1: the NaN sits in the segments ceil((p - N + 1) / H) .. floor(p / H) = 1040, 1041, both of line 10
        cover = 400_000 // H + (N - 1 - 400_000) // H + 1
        assert cover == 2 and rcnt[10] == R - cover and np.sum(rcnt != R) == 1


@pytest.mark.parametrize("R", [1, 20])
def test_call_split_into_launches(R):
    """One call whose sub-blocks exceed what one launch of the segment pass takes: the engine takes a call in launches of
    at most 128 MiB / (rows N 16 bytes) runs per row, here 1024 (rows = 8, N = 1024), one run per sub-block.  2100 lines
    of R = 1 (2100 runs) and 700 lines of R = 20 (sub-blocks of 8, 8, 4: 2100 runs) take three launches each; at R = 20
    the launches end after run 1023 (line 341, sub-block 0) and run 2047 (line 682, sub-block 1): both inside a line,
    whose partial goes from one launch to the next.  Every line of every row against the same input in calls of 20000
    samples (626 runs at the most: one launch each) bit for bit; against the oracle the first and last two lines and the
    four around each launch boundary, of the rows 0 and 7 (M = 2 x 12 x 1024 for the scene's floor: with all 17 million
    values of R = 1 the deepest noise bin alone would lie 72 dB under the floor); and with a ring of 37 lines, whose slots
    a later launch of the same call overwrites.  The accumulators add up over the launches: peak hold bit for bit, mean PSD to fp64 rounding."""
    N, H, rows = 1024, 32, 8
    lines = 2100 if R == 1 else 700
    room = (128 << 20) // (rows * N * 16)
    assert lines * -(-R // 8) > 2 * room and 20000 // H + 2 <= room
    n = length(N, H, R, lines)
    bounds = [room // -(-R // 8), 2 * room // -(-R // 8)]              # the lines the launches end in (or before)
    spans = [(0, 2)] + [(b - 2, b + 2) for b in bounds] + [(lines - 2, lines)]
    x = scene(n, N, H, R, rows=rows, seed=41 + R, compared=2 * 12 * N)
    small_cuts = [20000] * (n // 20000) + [n % 20000]
    for which in WHICH:
        one = make(N, H, R, lines, which, n, rows=rows)
        small = make(N, H, R, lines, which, 20000, rows=rows)
        shallow = make(N, H, R, 37, which, n, rows=rows)
        feed(one, x, [n])
        feed(small, x, small_cuts)
        feed(shallow, x, [n])
        for r in range(rows):
            g, c, i = one.waterfall(r)
            sg, sc, si = small.waterfall(r)
            assert g.shape == (lines, N) and i == si and i["first_line"] == 0 and i["lines_dropped"] == 0
            np.testing.assert_array_equal(g, sg)
            np.testing.assert_array_equal(c, sc)
            assert np.all(c == R)
            tg, tc, ti = shallow.waterfall(r)
            assert ti["first_line"] == lines - 37 and ti["lines_dropped"] == lines - 37 and ti["lines_ready"] == 0
            np.testing.assert_array_equal(tg, g[lines - 37:])
            np.testing.assert_array_equal(tc, c[lines - 37:])
            if r in (0, rows - 1):
                for lo, hi in spans:
                    ref, rcnt = wf.lines(x[r], N, H, sf.HANN, F, R, which, line_lo=lo, line_hi=hi)
                    np.testing.assert_array_equal(c[lo:hi], rcnt)
                    ok, worst = wf.close(g[lo:hi], ref)
                    print("waterfall launches", R, which, "row", r, "lines", lo, hi, "worst ratio", worst)
                    assert ok, (R, which, r, lo, worst)
            np.testing.assert_array_equal(one.peak_hold(r), small.peak_hold(r))
            m = small.psd(r)
            assert np.all(np.abs(one.psd(r) - m) <= 1e-12 * m)
            assert one.info(r) == small.info(r)
        for sp in (one, small, shallow):
            sp.close()


def spectrum_scene(n, rows=1, seed=0, noise=3e-2):
    """test_gpu_spectrum.scene as it stands: the floor 50-60 dB (N = 16384, Hann: up to 65 dB) under the strongest bin."""
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


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,H,R,lines", [(16384, 8192, 2, 3), (8192, 4096, 1, 4)])
def test_deep_bins_error_model(N, H, R, lines, which):
    """Lines of one and two segments on the spectrum test's own scene, whose deepest bins lie 70 dB and more under the
    strongest (at (16384, 8192, 2), seed 24578, the PEAK line of row 1 has a bin 69.7 dB down that is off by 1.26e-4 of
    itself).  The bound is the fp32 FFT's error model of DESIGN.md section 10, as test_peak_hold_deep_bins applies it to
    single segments: an amplitude error of at most e |X_max| per bin, e = log2(N) 2^-24, so per segment
    |P - P_ref| <= 1e-4 P_ref + 2 e sqrt(P_ref mx) + e^2 mx with mx the largest power of any segment of the row.  The
    bound is concave and increasing in P_ref, so it holds for the maximum and for the mean of R segments as it stands."""
    n = length(N, H, R, lines)
    x = spectrum_scene(n, rows=2, seed=N + H + R)
    sp = make(N, H, R, lines, which, n, rows=2)
    feed(sp, x, [n // 3, n - n // 3])
    e = np.log2(N) * 2.0 ** -24
    for r in range(2):
        got, cnt, _ = sp.waterfall(r)
        ref, rcnt = wf.lines(x[r], N, H, sf.HANN, F, R, which)
        mx = wf.lines(x[r], N, H, sf.HANN, F, R, wf.PEAK)[0].max()
        assert got.shape == ref.shape
        np.testing.assert_array_equal(cnt, rcnt)
        bound = 1e-4 * ref + 2 * e * np.sqrt(ref * mx) + e * e * mx
        err = np.abs(got.astype(np.float64) - ref)
        print("waterfall deep bins", N, R, which, "row", r, "worst err / bound", float(np.max(err / bound)),
              "deepest bin dB", float(10 * np.log10(ref.min() / mx)), "worst ratio to 1e-4", wf.close(got, ref)[1])
        assert np.all(err <= bound), (N, R, which, r, float(np.max(err / bound)))
    sp.close()


def test_rows_strides_and_device_path():
    import torch
    N, H, R, rows = 512, 200, 5, 3
    n = length(N, H, R, 60)
    x = scene(n, N, H, R, rows=rows, seed=3)
    cuts = [10000 - 3, 7, n - 10008, 4]
    mcl = max(cuts)
    for which in WHICH:
        host = make(N, H, R, 80, which, mcl, rows=rows)
        dev = make(N, H, R, 80, which, mcl, rows=rows)
        stride = mcl + 24
        d = torch.zeros((rows, stride), dtype=torch.complex64, device="cuda")
        o = 0
        for c in cuts:
            host.process(x[:, o:o + c])
            d[:, :c] = torch.from_numpy(x[:, o:o + c].copy()).cuda()
            torch.cuda.synchronize()
            dev.process_device(d.data_ptr(), c, stride=stride, sync=False)
            dev.synchronize()                                 # (the next copy into d waits for the call that reads it)
            o += c
        # a last call with sync = 0 followed by the read alone: the read synchronises
        tail = scene(3 * R * H, N, H, R, rows=rows, seed=4)[:, :mcl]
        host.process(tail)
        d[:, :tail.shape[1]] = torch.from_numpy(tail.copy()).cuda()
        torch.cuda.synchronize()
        dev.process_device(d.data_ptr(), tail.shape[1], stride=stride, sync=False)
        full = np.concatenate([x, tail], axis=1)
        for r in range(rows):
            g, c, i = dev.waterfall(r)
            hg, hc, hi = host.waterfall(r)
            np.testing.assert_array_equal(g, hg)
            np.testing.assert_array_equal(c, hc)
            assert i == hi and len(g) == 63
            ref, rcnt = wf.lines(full[r], N, H, sf.HANN, F, R, which)
            assert len(ref) == len(g) and wf.close(g, ref)[0]
            np.testing.assert_array_equal(c, rcnt)
        host.close()
        dev.close()


def test_raw_formats_equal_converted_cf32():
    rng = np.random.default_rng(3)
    m, N, H, R = 30000, 1024, 300, 3
    raws = {
        fmr.IQ_S16: (rng.integers(-32768, 32768, (2, m, 2)).astype(np.int16), lambda v: v.astype(np.float32) / 32768.0),
        fmr.IQ_U8: (rng.integers(0, 256, (2, m, 2)).astype(np.uint8), lambda v: (v.astype(np.float32) - 128.0) / 128.0),
    }
    for which in WHICH:
        for fmt, (raw, conv) in raws.items():
            a = make(N, H, R, 64, which, m, rows=2, fmt=fmt)
            b = make(N, H, R, 64, which, m, rows=2)
            a.process(raw[:, :777])
            a.process(raw[:, 777:])
            f = conv(raw)
            b.process((f[..., 0] + 1j * f[..., 1]).astype(np.complex64))
            for r in range(2):
                la, ca, _ = a.waterfall(r)
                lb, cb, _ = b.waterfall(r)
                assert len(la) == ((m - N) // H + 1) // R
                np.testing.assert_array_equal(la, lb, err_msg=str(fmt))
                np.testing.assert_array_equal(ca, cb, err_msg=str(fmt))
            a.close()
            b.close()


@pytest.mark.parametrize("which", WHICH)
def test_non_finite_samples(which):
    """N = 256, H = 128, R = 4: segment j covers [128 j, 128 j + 256).  Sample 704 lies in the segments 4 and 5 (line 1:
    two of its four are left); samples 1736 and 1992 lie in 12, 13 and 14, 15: line 3 has none left."""
    N, H, R, lines = 256, 128, 4, 5
    n = length(N, H, R, lines)
    x = scene(n, N, H, R, rows=2, seed=11)
    x[0, 704] = np.nan
    x[0, 1736] = complex(np.inf, 0)
    x[0, 1992] = complex(0, -np.inf)
    sp = make(N, H, R, lines, which, n, rows=2)
    feed(sp, x, [700, 1100, n - 1800])
    got, cnt, _ = sp.waterfall(0)
    ref, rcnt = wf.lines(x[0], N, H, sf.HANN, F, R, which)
    np.testing.assert_array_equal(cnt, [4, 2, 4, 0, 4])
    np.testing.assert_array_equal(cnt, rcnt)
    assert not np.any(got[3]) and np.all(np.isfinite(got))
    ok, worst = wf.close(got, ref)
    assert ok, worst
    got1, cnt1, _ = sp.waterfall(1)
    assert np.all(cnt1 == R) and wf.close(got1, wf.lines(x[1], N, H, sf.HANN, F, R, which)[0])[0]
    # segments_skipped keeps its meaning: the segments left out of the accumulators
    _, _, counted, skipped = sf.welch(x[0], N, H, sf.HANN, F)
    assert skipped == 6
    assert sp.info(0)["segments_skipped"] == skipped and sp.info(0)["segments"] == counted
    assert sp.info(1)["segments_skipped"] == 0


def test_ring_overrun_and_cap_zero():
    N, H, R = 256, 256, 2
    n = length(N, H, R, 5, extra=100)
    x = scene(n, N, H, R, seed=13)
    for which in WHICH:
        sp = make(N, H, R, 2, which, n)
        feed(sp, x, [n // 2, n - n // 2])
        L = fmr.lib()
        info = fmr.WaterfallInfo()
        canary = np.full(N, -7.0, np.float32)
        rc = L.fmr_spectrum_read_waterfall(sp.h, 0, canary.ctypes.data_as(C.POINTER(C.c_float)), None, 0, C.byref(info))
        assert rc == 2 and np.all(canary == -7.0)
        assert (info.first_line, info.lines_ready, info.lines_dropped) == (3, 2, 3)
        got, cnt, i = sp.waterfall()
        assert i["first_line"] == 3 and i["lines_dropped"] == 3 and i["lines_ready"] == 0 and len(got) == 2
        ref, rcnt = wf.lines(x[0], N, H, sf.HANN, F, R, which, line_lo=3)
        assert wf.close(got, ref)[0]
        np.testing.assert_array_equal(cnt, rcnt)
        got, cnt, i = sp.waterfall()
        assert len(got) == 0 and len(cnt) == 0 and i["first_line"] == 5 and i["lines_dropped"] == 3
        sp.close()


def test_partial_reads_per_row_and_reset():
    N, H, R, rows = 256, 100, 3, 2
    n = length(N, H, R, 5)
    x = scene(n, N, H, R, rows=rows, seed=17)
    more = scene(4 * R * H, N, H, R, rows=rows, seed=18)
    full = np.concatenate([x, more], axis=1)
    sp = make(N, H, R, 16, wf.MEAN, n, rows=rows)
    whole = make(N, H, R, 16, wf.MEAN, n, rows=rows)          # the same input, never reset, read at the end
    sp.process(x)
    whole.process(x)
    a, _, ia = sp.waterfall(0, cap=2)
    assert len(a) == 2 and ia["first_line"] == 0 and ia["lines_ready"] == 3
    b, _, ib = sp.waterfall(1)
    assert len(b) == 5 and ib["first_line"] == 0 and ib["lines_ready"] == 0
    # reset: the accumulators start again, the unread lines and the line grid stay
    sp.reset()
    assert sp.info(0)["segments"] == 0
    c, cc, ic = sp.waterfall(0, cap=1)
    assert len(c) == 1 and ic["first_line"] == 2 and ic["lines_ready"] == 2 and ic["lines_dropped"] == 0
    sp.process(more)
    whole.process(more)
    d, _, idd = sp.waterfall(0)
    assert idd["first_line"] == 3
    ref = whole.waterfall(0)[0]
    np.testing.assert_array_equal(np.concatenate([a, c, d]), ref)
    np.testing.assert_array_equal(np.concatenate([b, sp.waterfall(1)[0]]), whole.waterfall(1)[0])
    assert wf.close(ref, wf.lines(full[0], N, H, sf.HANN, F, R, wf.MEAN)[0])[0] and len(ref) == 9
    assert sp.info(0)["first_segment"] == 5 * R and sp.info(0)["segments"] == 4 * R


@pytest.mark.parametrize("N,H,R,n", [(1024, 384, 7, 60000), (256, 96, 1, 96 * 3000 + 160), (16384, 8192, 64, 40 * 8192)])
def test_accumulators_unmoved(N, H, R, n):
    """Same input and cut through a waterfall object and a plain one: the peak hold bit for bit, the counts equal, the
    mean PSD within 1e-12 relative (its fp64 partial sums are cut into other runs)."""
    x = scene(n, N, H, R, rows=2, seed=N + R)
    x[1, n // 2] = np.nan
    cut = [n // 3, 1, n - n // 3 - 1]
    a = make(N, H, R, 4, wf.MEAN, n, rows=2)
    b = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=2, max_call_len=n)
    feed(a, x, cut)
    feed(b, x, cut)
    for r in range(2):
        np.testing.assert_array_equal(a.peak_hold(r), b.peak_hold(r))
        m = b.psd(r)
        assert np.all(np.abs(a.psd(r) - m) <= 1e-12 * m), float(np.max(np.abs(a.psd(r) - m) / m))
        assert a.info(r) == b.info(r)
    with pytest.raises(fmr.FmrError, match="-2"):
        b.waterfall()
    assert fmr.lib().fmr_spectrum_read_waterfall(b.h, 0, None, None, 0, None) == fmr.ERR_BAD_ARG


def test_facade_spectrum_monitor_waterfall(tmp_path):
    exe = str(tmp_path / "waterfall_smoke")
    raw = str(tmp_path / "input.cf32")
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(libdir, 'host')}", os.path.join(ROOT, "tests", "waterfall_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe, raw], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    rows = [ln.split() for ln in r.stdout.splitlines()]
    head = [t for t in rows if t[0] == "waterfall"][0]      # waterfall <N> <hop> <R> <first_line> <lines>
    N, H, R, first, nl = (int(v) for v in head[1:6])
    got = np.array([[float.fromhex(v) for v in t[3:]] for t in rows if t[0] == "line"], dtype=np.float32)
    gcnt = np.array([int(t[2]) for t in rows if t[0] == "line"])
    x = np.fromfile(raw, dtype=np.complex64)[None]
    sp = make(N, H, R, 64, wf.MEAN, x.shape[1])
    sp.process(x)
    lines, cnt, info = sp.waterfall()
    assert first == 0 and nl == len(lines) >= 3 and got.shape == lines.shape
    np.testing.assert_array_equal(got, lines)
    np.testing.assert_array_equal(gcnt, cnt)

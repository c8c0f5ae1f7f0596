"""CPU-side checks of fmr_set_output_rate / fmr_get_output_rate / fmr_output_rate_taps (include/fmradion_amd.h): the
struct layouts of header and binding, every configuration refusal by name before the chain is looked at, the prototype
filters against their specification, and a 16 kHz mono file through AudioFileWriter."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
from scipy.io import wavfile

from cheader import header_struct as _header_struct
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.OutputRateConfig(C.sizeof(fmr.OutputRateConfig), 16000, 0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _set(L, cfg, size=None, chain=None):
    rc = L.fmr_set_output_rate(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [("fmr_output_rate_config", "OutputRateConfig", 16),
                                               ("fmr_output_rate_info", "OutputRateInfo", 56)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


@pytest.mark.parametrize("field,value", [("rate", 7999), ("rate", 48001), ("rate", 8001), ("rate", -16000), ("mono", 2),
                                         ("mono", -1), ("reserved", 1)])
def test_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _set(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_set_output_rate" in msg and field in msg and "chain" not in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _set(L, _cfg(), size=C.sizeof(fmr.OutputRateConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_output_rate_config" in msg, msg
    rc, msg = _set(L, _cfg(struct_size=C.sizeof(fmr.OutputRateConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_set_output_rate(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    info = fmr.OutputRateInfo()
    assert L.fmr_get_output_rate(None, 0, C.byref(info), 0) == fmr.ERR_BAD_ARG
    assert "fmr_get_output_rate" in L.fmr_last_error().decode()


@pytest.mark.parametrize("kw", [{}, {"rate": 0}, {"rate": 48000, "mono": 1}, {"rate": 8000}, {"rate": 44100, "mono": 1},
                                {"rate": 11025}, {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _set(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_set_output_rate", "fmr_get_output_rate", "fmr_output_rate_taps"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- the prototype filters ---------------------------------------------------------------------------------------------
GEOM = {8000: (1, 6), 11025: (147, 640), 16000: (1, 3), 22050: (147, 320), 32000: (2, 3), 44100: (147, 160)}


@pytest.mark.parametrize("rate", sorted(GEOM))
def test_taps_meet_the_specification(L, rate):
    """L, M, T L; symmetry bit for bit; sum h = L; pass band 0 .. 0.9 rate / 2 within +-0.001 dB and stop band from
    rate / 2 on >= 100 dB down, read off a zero-padded FFT of the library's taps (grid: 16 points per main-lobe width
    48000 L / (T L) at least)."""
    l, m, t = C.c_int(), C.c_int(), C.c_int()
    n = L.fmr_output_rate_taps(rate, None, 0, C.byref(l), C.byref(m), C.byref(t))
    assert (l.value, m.value) == GEOM[rate] and n == t.value * l.value > 0
    small = np.full(4, 7.0)
    assert L.fmr_output_rate_taps(rate, small.ctypes.data_as(C.POINTER(C.c_double)), 4, None, None, None) == n
    assert np.all(small == 7.0)                      # cap too small: nothing written
    h, l2, m2, t2 = fmr.output_rate_taps(rate)
    assert (l2, m2, t2) == (l.value, m.value, t.value) and len(h) == n
    assert h.tobytes() == h[::-1].tobytes()
    ll = l.value
    assert abs(float(np.sum(h)) - ll) <= 1e-12 * ll, float(np.sum(h)) - ll
    nfft = 1 << int(np.ceil(np.log2(16 * n)))
    H = np.abs(np.fft.rfft(h, nfft)) / ll
    f = np.arange(len(H)) * (48000.0 * ll / nfft)
    pb = 20 * np.log10(H[f <= 0.9 * rate / 2])
    sb = 20 * np.log10(np.maximum(H[f >= rate / 2], 1e-300))
    print(f"rate {rate}: L {ll} M {m.value} T {t.value}; pass band {pb.min():+.2e} .. {pb.max():+.2e} dB; "
          f"stop band {sb.max():.2f} dB")
    assert np.abs(pb).max() <= 0.001 and sb.max() <= -100.0


def test_taps_of_48000_and_refused_rates(L):
    h, l, m, t = fmr.output_rate_taps(48000)
    assert (h.tolist(), l, m, t) == ([1.0], 1, 1, 1)
    assert fmr.output_rate_taps(0)[1:] == (1, 1, 1)
    for rate in (7999, 8001, 48001):
        assert L.fmr_output_rate_taps(rate, None, 0, None, None, None) == fmr.ERR_BAD_ARG
        with pytest.raises(fmr.FmrError, match="rate"):
            fmr.output_rate_taps(rate)


def test_output_frame_of():
    assert [fmr.output_frame_of(f, 16000) for f in (0, 1, 2, 3, 4, 315)] == [0, 1, 1, 1, 2, 105]
    assert fmr.output_frame_of(160, 44100) == 147 and fmr.output_frame_of(161, 44100) == 148
    assert fmr.output_frame_of(12345, 48000) == fmr.output_frame_of(12345, 0) == 12345


# ---- a 16 kHz mono file ------------------------------------------------------------------------------------------------
def test_16k_mono_file_round_trips(tmp_path):
    """The ring's int16 frames at 16 kHz, one channel, through AudioFileWriter::write_i16 and back."""
    exe = str(tmp_path / "output_fileio_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "output_fileio_check.cpp")], check=True)
    pcm = np.random.default_rng(5).integers(-32768, 32768, size=16000 + 123).astype(np.int16)
    pcm[:4] = [-32768, 32767, 0, -1]
    src, wav = str(tmp_path / "pcm.s16"), str(tmp_path / "a.wav")
    pcm.tofile(src)
    r = subprocess.run([exe, "write", "WAV_INT16", src, wav, "16000", "0", "1000"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["written", str(len(pcm)), "refused", "0"], r.stdout + r.stderr
    rate, data = wavfile.read(wav)
    assert rate == 16000 and data.dtype == np.int16 and data.shape == (len(pcm),) and np.array_equal(data, pcm)

"""CPU-side checks of the waterfall's entry points (include/fmradion_amd.h, fmr_spectrum_create_waterfall /
fmr_spectrum_read_waterfall): every refusal by name before a device is touched, the spectrum configuration refused
with fmr_spectrum_create's own code and words, FMR_ERR_NO_DEVICE for a valid pair without a device, the exports."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.SpectrumConfig()
    c.struct_size, c.device, c.n_rows, c.input_rate, c.input_format = C.sizeof(c), 0, 1, 10e6, fmr.IQ_CF32
    c.fft_size, c.hop, c.window, c.max_call_len = 8192, 0, fmr.WINDOW_HANN, 1 << 16
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _wf(**kw):
    w = fmr.WaterfallConfig(C.sizeof(fmr.WaterfallConfig), 4, 16, fmr.WATERFALL_MEAN)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _create(L, cfg, wf, wf_size=None, cfg_size=None):
    h = C.c_void_p()
    rc = L.fmr_spectrum_create_waterfall(C.byref(cfg), C.sizeof(cfg) if cfg_size is None else cfg_size, C.byref(wf),
                                         C.sizeof(wf) if wf_size is None else wf_size, C.byref(h))
    if rc == 0:
        L.fmr_spectrum_destroy(h)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("field,value", [
    ("segments_per_line", 0), ("segments_per_line", -1), ("segments_per_line", 65537), ("max_lines", 0), ("max_lines", -3),
    ("which", 2), ("which", -1),
])
def test_waterfall_refusals_name_the_field(L, field, value):
    rc, msg = _create(L, _cfg(), _wf(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_spectrum_create_waterfall" in msg and field in msg, msg


def test_waterfall_refuses_a_larger_struct(L):
    rc, msg = _create(L, _cfg(), _wf(), wf_size=C.sizeof(fmr.WaterfallConfig) + 4)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_waterfall_config" in msg, msg
    rc, msg = _create(L, _cfg(), _wf(struct_size=C.sizeof(fmr.WaterfallConfig) + 4))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_waterfall_config" in msg, msg


def test_waterfall_refuses_a_ring_above_one_gib(L):
    # n_rows L N 4 bytes: 1 x 16384 x 16384 x 4 = 1 GiB passes the check, one line more does not
    rc, msg = _create(L, _cfg(fft_size=16384), _wf(max_lines=16385))
    assert rc == fmr.ERR_BAD_ARG and "max_lines" in msg and "1 GiB" in msg, msg
    rc, msg = _create(L, _cfg(fft_size=256, n_rows=4), _wf(max_lines=(1 << 30) // (4 * 256 * 4) + 1))
    assert rc == fmr.ERR_BAD_ARG and "max_lines" in msg, msg
    rc, msg = _create(L, _cfg(fft_size=16384, n_rows=65535), _wf(max_lines=2 ** 31 - 1))
    assert rc == fmr.ERR_BAD_ARG and "max_lines" in msg, msg


@pytest.mark.parametrize("field,value", [("fft_size", 1000), ("hop", -1), ("window", 3), ("input_format", 4),
                                         ("input_rate", 0.0), ("n_rows", 0), ("max_call_len", 0)])
def test_spectrum_config_is_refused_in_the_plain_entry_points_words(L, field, value):
    h = C.c_void_p()
    cfg = _cfg(**{field: value})
    rc0 = L.fmr_spectrum_create(C.byref(cfg), C.sizeof(cfg), C.byref(h))
    msg0 = L.fmr_last_error().decode()
    rc, msg = _create(L, cfg, _wf(segments_per_line=0))      # the spectrum configuration is checked first
    assert rc0 == fmr.ERR_BAD_ARG and rc == rc0 and msg == msg0 and field in msg, (rc0, msg0, rc, msg)


def test_larger_spectrum_struct_is_refused_in_the_plain_entry_points_words(L):
    h = C.c_void_p()
    cfg = _cfg()
    big = C.sizeof(fmr.SpectrumConfig) + 8
    rc0 = L.fmr_spectrum_create(C.byref(cfg), big, C.byref(h))
    msg0 = L.fmr_last_error().decode()
    rc, msg = _create(L, cfg, _wf(), cfg_size=big)
    assert rc0 == fmr.ERR_BAD_ARG and rc == rc0 and msg == msg0 and "struct_size" in msg, (msg0, msg)


def test_null_arguments(L):
    h = C.c_void_p()
    cfg, wf = _cfg(), _wf()
    assert L.fmr_spectrum_create_waterfall(None, 0, C.byref(wf), 0, C.byref(h)) == fmr.ERR_BAD_ARG
    assert L.fmr_spectrum_create_waterfall(C.byref(cfg), 0, None, 0, C.byref(h)) == fmr.ERR_BAD_ARG
    assert L.fmr_spectrum_create_waterfall(C.byref(cfg), 0, C.byref(wf), 0, None) == fmr.ERR_BAD_ARG
    assert L.fmr_spectrum_read_waterfall(None, 0, None, None, 0, None) == fmr.ERR_BAD_ARG


def test_valid_pair_opens_the_device_next(L):
    """Every check passed: without a GPU the answer is FMR_ERR_NO_DEVICE, with one the object is made."""
    import torch
    want = fmr.OK if torch.cuda.is_available() else fmr.ERR_NO_DEVICE
    for ckw, wkw in (({}, {}), ({"fft_size": 256, "hop": 256}, {"segments_per_line": 1, "max_lines": 1, "which": fmr.WATERFALL_PEAK}),
                     ({"fft_size": 16384, "n_rows": 1}, {"segments_per_line": 65536, "max_lines": 16}),
                     ({"fft_size": 1024, "n_rows": 3, "input_format": fmr.IQ_U8}, {"struct_size": 0})):
        rc, msg = _create(L, _cfg(**ckw), _wf(**wkw))
        assert rc == want, (ckw, wkw, rc, msg)
        if want == fmr.ERR_NO_DEVICE:
            assert "no HIP device" in msg, msg
            assert L.fmr_debug_live_resources() == 0       # (the failed create left nothing behind)


def test_struct_layout_and_exports(L):
    assert C.sizeof(fmr.WaterfallConfig) == 16
    assert C.sizeof(fmr.WaterfallInfo) == 32
    for name in ("fmr_spectrum_create_waterfall", "fmr_spectrum_read_waterfall"):
        assert name in fmr.EXPORTS
        assert hasattr(L, name)
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T fmr_spectrum_create_waterfall" in out and " T fmr_spectrum_read_waterfall" in out
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmradion_amd.h")).read()
    assert "fmr_spectrum_create_waterfall(" in hdr and "fmr_spectrum_read_waterfall(" in hdr
    assert "FMR_WATERFALL_MEAN = 0, FMR_WATERFALL_PEAK = 1" in hdr

"""CPU-side checks of fmr_enable_mpx_output / fmr_mpx_output_read / fmr_mpx_output_taps (include/fmradion_amd.h): the struct
layouts of header and binding, every configuration refusal by name before the chain is looked at, and the exports."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.MpxOutputConfig(C.sizeof(fmr.MpxOutputConfig), fmr.PCM_S16, 192000, 0.5, 4096)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_mpx_output(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [("fmr_mpx_output_config", "MpxOutputConfig", 32),
                                               ("fmr_mpx_output_info", "MpxOutputInfo", 88)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


@pytest.mark.parametrize("field,value", [("format", 2), ("format", -1), ("rate", 95999), ("rate", 384001), ("rate", 100001),
                                         ("rate", -192000), ("rate", 48000), ("gain", -0.5), ("gain", float("inf")),
                                         ("gain", float("nan")), ("max_frames", (1 << 26) + 1)])
def test_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_mpx_output" in msg and field in msg and "chain" not in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.MpxOutputConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_mpx_output_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.MpxOutputConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_mpx_output(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    info, got = fmr.MpxOutputInfo(), C.c_size_t(7)
    assert L.fmr_mpx_output_read(None, 0, None, 0, C.byref(got), C.byref(info), 0) == fmr.ERR_BAD_ARG and got.value == 0
    assert "fmr_mpx_output_read" in L.fmr_last_error().decode()


@pytest.mark.parametrize("kw", [{}, {"rate": 0}, {"rate": 384000, "format": fmr.PCM_F32}, {"rate": 96000}, {"rate": 171000},
                                {"rate": 228000}, {"rate": 256000}, {"gain": 0.0}, {"gain": 4.0}, {"max_frames": 0},
                                {"max_frames": 1}, {"max_frames": 1 << 26}, {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_mpx_output", "fmr_mpx_output_read", "fmr_mpx_output_taps"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


def test_taps_entry(L):
    """The contract of fmr_output_rate_taps: the count with taps = NULL or cap too small (nothing written then), L, M, T."""
    l, m, t = C.c_int(), C.c_int(), C.c_int()
    n = L.fmr_mpx_output_taps(171000, None, 0, C.byref(l), C.byref(m), C.byref(t))
    assert (l.value, m.value) == (57, 128) and n == t.value * 57 > 0
    small = np.full(4, 7.0)
    assert L.fmr_mpx_output_taps(171000, small.ctypes.data_as(C.POINTER(C.c_double)), 4, None, None, None) == n
    assert np.all(small == 7.0)
    h, l2, m2, t2 = fmr.mpx_output_taps(171000)
    assert (l2, m2, t2) == (57, 128, t.value) and len(h) == n
    for rate in (95999, 384001, 100001):
        assert L.fmr_mpx_output_taps(rate, None, 0, None, None, None) == fmr.ERR_BAD_ARG
        assert "rate" in L.fmr_last_error().decode()

"""CPU-side checks of the MPX input's C-ABI (include/fmradion_amd.h, fmr_create_mpx_decoder): the struct layouts of header
and binding, the exports, fmr_mpx_input_geometry against the fixture, the shape step of the create, and every refusal of the
create by code and field name -- all of them made before a device is opened, so none of this needs one."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

import mpx_input_fixture as mi
from cheader import header_struct as _header_struct

fmr = importlib.import_module("airspy-fmradion_amd")

NEW = ("fmr_create_mpx_decoder", "fmr_process_mpx_blocks", "fmr_process_mpx_blocks_device", "fmr_get_mpx_input_info",
       "fmr_mpx_input_geometry", "fmr_debug_mpx_chain_shape")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _configs(**kw):
    a = dict(rate=192000, format="s16", gain=0.0, n_streams=2, stereo=True, deemphasis_us=50.0, pilot_shift=False, rds=False,
             max_block_len=8192, max_blocks=4, device=0)
    a.update({k: v for k, v in kw.items() if k in a})
    cfg, m, keep = fmr._mpx_configs(**a)
    for k, v in kw.items():
        if k.startswith("cfg_"):
            setattr(cfg, k[4:], v)
        elif k.startswith("in_"):
            setattr(m, k[3:], v)
    return cfg, m, keep


def _create(L, cfg, m, in_size=None):
    h = C.c_void_p(7)
    rc = L.fmr_create_mpx_decoder(C.byref(cfg), C.sizeof(fmr.Config), C.byref(m), C.sizeof(m) if in_size is None else in_size,
                                  C.byref(h))
    return rc, L.fmr_last_error().decode(), h


@pytest.mark.parametrize("name,binding,size", [("fmr_mpx_input_config", "MpxInputConfig", 32),
                                               ("fmr_mpx_input_info", "MpxInputInfo", 72)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out
    assert issubclass(fmr.MpxChain, fmr.Chain)


@pytest.mark.parametrize("rate", [96000, 171000, 192000, 228000, 256000])
def test_geometry_entry_agrees_with_the_fixture(L, rate):
    assert fmr.mpx_input_geometry(rate) == mi.geometry(rate)
    assert fmr.mpx_input_geometry(rate)[3] == 143
    k = C.c_int()
    assert L.fmr_mpx_input_geometry(rate, None, None, None, C.byref(k), None) == fmr.OK and k.value == 143


def test_geometry_entry_edges(L):
    assert fmr.mpx_input_geometry(384000) == fmr.mpx_input_geometry(0) == (1, 1, 1, 1, 0.0)
    for rate in (100001, 95999, 384001, -192000):
        with pytest.raises(fmr.FmrError, match="rate"):
            fmr.mpx_input_geometry(rate)
    assert L.fmr_mpx_input_geometry(100001, None, None, None, None, None) == fmr.ERR_BAD_ARG


def test_shape_of_an_accepted_create():
    """The shape step alone: the MPX-input form, in order, max_if = ceil(max_in M / L) + 4, nothing of the IF resampler."""
    sh = fmr.mpx_chain_shape(rate=171000, format="f32", n_streams=2, max_block_len=8192, max_blocks=4)
    assert (sh["mpx_in"], sh["mpx_format"], sh["mpx_L"], sh["mpx_M"], sh["mpx_K"]) == (1, fmr.PCM_F32, 57, 128, 143)
    assert sh["mpx_T"] == mi.geometry(171000)[2]
    assert sh["max_if"] == -(-(8192 * 4) * 128 // 57) + 4 and sh["max_au"] > 0
    assert (sh["pipelined"], sh["D"], sh["stage_b"], sh["fused"], sh["fir"], sh["qa"]) == (0, 0, 0, 0, 0, 0)
    sh = fmr.mpx_chain_shape(rate=0, max_block_len=1000, max_blocks=1)
    assert (sh["mpx_in"], sh["mpx_L"], sh["mpx_M"], sh["mpx_T"], sh["mpx_K"], sh["max_if"]) == (1, 1, 1, 1, 1, 1008 + 4)
    # an IQ chain's shape says it is not that form
    iq = fmr.chain_shape_config(fmr._make_config(fmr.MODE_FM, 384000.0, False, False, False, None, True, 50.0, False, 0, 8192, 4,
                                                 1, 0, 0.0, 0, 0.0, fmr.RESAMPLER_FAST, False, None)[0])
    assert iq.max_if == 8192 * 4


@pytest.mark.parametrize("kw,code,field", [
    ({"cfg_mode": fmr.MODE_AM}, fmr.ERR_UNSUPPORTED, "mode"),
    ({"cfg_mode": fmr.MODE_NONE}, fmr.ERR_UNSUPPORTED, "mode"),
    ({"cfg_fmfilter_enable": 1}, fmr.ERR_UNSUPPORTED, "fmfilter_enable"),
    ({"cfg_multipath_stages": 2}, fmr.ERR_UNSUPPORTED, "multipath_stages"),
    ({"cfg_input_format": fmr.IQ_S16}, fmr.ERR_UNSUPPORTED, "input_format"),
    ({"cfg_enable_fourth_down": 1}, fmr.ERR_UNSUPPORTED, "enable_fourth_down"),
    ({"cfg_enable_resampler": 1}, fmr.ERR_BAD_ARG, "enable_resampler"),
    ({"cfg_input_rate": 384000.0}, fmr.ERR_BAD_ARG, "input_rate"),
    ({"in_format": 2}, fmr.ERR_BAD_ARG, "format"),
    ({"in_format": -1}, fmr.ERR_BAD_ARG, "format"),
    ({"in_rate": 100001}, fmr.ERR_BAD_ARG, "rate"),
    ({"in_rate": 95999}, fmr.ERR_BAD_ARG, "rate"),
    ({"in_rate": 384001}, fmr.ERR_BAD_ARG, "rate"),
    ({"in_rate": 48000}, fmr.ERR_BAD_ARG, "rate"),
    ({"in_gain": -1.0}, fmr.ERR_BAD_ARG, "gain"),
    ({"in_gain": float("nan")}, fmr.ERR_BAD_ARG, "gain"),
    ({"in_gain": float("inf")}, fmr.ERR_BAD_ARG, "gain"),
    ({"in_rds": 2}, fmr.ERR_BAD_ARG, "rds"),
])
def test_create_refusals_name_the_field_and_open_no_device(L, kw, code, field):
    cfg, m, _keep = _configs(**kw)
    live = fmr.debug_live_resources()
    rc, msg, h = _create(L, cfg, m)
    assert rc == code, (kw, rc, msg)
    assert "fmr_create_mpx_decoder" in msg and field in msg, msg
    assert h.value is None and fmr.debug_live_resources() == live
    # the shape step gives the same answer
    o = fmr.ChainShapeInfo()
    assert L.fmr_debug_mpx_chain_shape(C.byref(cfg), C.sizeof(fmr.Config), C.byref(m), C.sizeof(m), C.byref(o), C.sizeof(o)) == code
    assert field in L.fmr_last_error().decode()


def test_channel_offsets_are_refused(L):
    cfg, m, _keep = _configs()
    offs = (C.c_int32 * 2)(0, 100000)
    cfg.channel_offset_hz = offs
    rc, msg, _ = _create(L, cfg, m)
    assert rc == fmr.ERR_BAD_ARG and "channel_offset_hz" in msg, msg


def test_input_rate_may_state_the_pcm_rate():
    assert fmr.mpx_chain_shape(rate=192000)["mpx_in"] == 1
    cfg, m, _keep = _configs(cfg_input_rate=192000.0)
    o = fmr.ChainShapeInfo()
    assert fmr.lib().fmr_debug_mpx_chain_shape(C.byref(cfg), C.sizeof(fmr.Config), C.byref(m), C.sizeof(m), C.byref(o), C.sizeof(o)) == fmr.OK


def test_larger_struct_and_null_arguments(L):
    cfg, m, _keep = _configs()
    rc, msg, _ = _create(L, cfg, m, in_size=C.sizeof(fmr.MpxInputConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_mpx_input_config" in msg, msg
    cfg, m, _keep = _configs(in_struct_size=C.sizeof(fmr.MpxInputConfig) + 8)
    rc, msg, _ = _create(L, cfg, m)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    h = C.c_void_p()
    assert L.fmr_create_mpx_decoder(None, 0, C.byref(m), 0, C.byref(h)) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_create_mpx_decoder(C.byref(cfg), 0, None, 0, C.byref(h)) == fmr.ERR_BAD_ARG and "in is null" in L.fmr_last_error().decode()
    assert L.fmr_create_mpx_decoder(C.byref(cfg), 0, C.byref(m), 0, None) == fmr.ERR_BAD_ARG
    bl = np.array([16], dtype=np.uint32)
    pcm = np.zeros(16, dtype=np.int16)
    u32p = C.POINTER(C.c_uint32)
    assert L.fmr_process_mpx_blocks(None, pcm.ctypes.data, 16, bl.ctypes.data_as(u32p), 1, None, 0, None) == fmr.ERR_BAD_ARG
    assert "fmr_process_mpx_blocks" in L.fmr_last_error().decode()
    assert L.fmr_process_mpx_blocks_device(None, pcm.ctypes.data, 16, bl.ctypes.data_as(u32p), 1, None, 0, None, 1) == fmr.ERR_BAD_ARG
    info = fmr.MpxInputInfo()
    assert L.fmr_get_mpx_input_info(None, 0, C.byref(info), 0) == fmr.ERR_BAD_ARG
    assert "fmr_get_mpx_input_info" in L.fmr_last_error().decode()

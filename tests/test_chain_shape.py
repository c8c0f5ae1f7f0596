"""What a create decides before it builds anything (fmr.chain_shape / fmr_debug_chain_shape: plan_create() of
csrc/chain_shape.hpp run by itself).  No device is opened, so everything here runs without a GPU:
  * every form a row of RATE_CASES lists is one its chain's shape permits, and the shape's design is the product's;
  * every refusal of a create -- the raw-format rows, the rules of the lifecycle test, the equaliser's bound, unknown
    class / format, a missing filter, every refused row of the channel-bank and channelizer argument tests -- comes
    with the create's code and words and without a device;
  * the stage-B ladder at its edges, against the ladder restated here from the design numbers alone.
"""
import ctypes as C
import importlib

import pytest

import test_channel_bank_args as bank_args
import test_channelizer_args as chz_args
from test_front_end_rate_table import (FAST, R8B, RATE_CASES, REFUSED_CASES, assert_forms_permitted, chain_kwargs, design)

fmr = importlib.import_module("airspy-fmradion_amd")


def refusal(**kw):
    """(code, message) with which chain_shape refuses Chain(**kw); the library must hold nothing afterwards that it did not before."""
    before = fmr.debug_live_resources()
    with pytest.raises(fmr.FmrError) as e:
        fmr.chain_shape(**kw)
    assert fmr.debug_live_resources() == before
    return e.value.code, e.value.message


def shape_of(case):
    return fmr.chain_shape(**chain_kwargs(case, 4))


# ------------------------------------------------------------------ the rows of the source-rate table
@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: c.name)
def test_rate_case_forms_are_permitted_by_the_shape(case):
    assert_forms_permitted(case.forms, shape_of(case))


@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: c.name)
def test_rate_case_design_is_the_products(case):
    want = dict(design(case)[2])
    if want["D"] == 1:
        want["NA"] = 1                              # stage A is a copy: one unit tap
    assert shape_of(case).design == want


@pytest.mark.parametrize("case", REFUSED_CASES, ids=lambda c: c.name)
def test_raw_format_rows_are_refused_without_a_device(case):
    code, msg = refusal(**chain_kwargs(case, 4))
    assert code == fmr.ERR_UNSUPPORTED, (code, msg)
    D = design(case)[2]["D"]
    assert msg == ("input_format != cf32 needs the FAST resampler class and a source rate with integer pre-decimation >= 2 "
                   f"({case.fin:.0f} -> {case.fout:.0f} Hz gives D = {D}): convert on the host or use cf32 input"), msg


# ------------------------------------------------------------------ the other refusals of a create
FM10 = dict(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, max_block_len=65536, max_blocks=4)


@pytest.mark.parametrize("kw, code, words", [
    # the two of tests/test_gpu_lifecycle.py::test_create_that_is_refused_before_the_device_is_opened
    (dict(FM10, input_format=fmr.IQ_S16, resampler_class=fmr.RESAMPLER_R8B), fmr.ERR_UNSUPPORTED,
     "input_format != cf32 needs the FAST resampler class and a source rate with integer pre-decimation >= 2 "
     "(10000000 -> 384000 Hz gives D = 10): convert on the host or use cf32 input"),
    (dict(FM10, mode=fmr.MODE_NONE, input_rate=5e9), fmr.ERR_UNSUPPORTED,
     "resampling ratio 5e+09 -> 384000 is outside the supported design range"),
    (dict(mode=fmr.MODE_FM, input_rate=384e3, stereo=True, max_block_len=512, max_blocks=106, multipath_stages=320),
     fmr.ERR_UNSUPPORTED, "multipath_stages 320 is above 319: the equaliser holds 4 stages + 1 taps, 1280 at most"),
    (dict(FM10, resampler_class=7), fmr.ERR_BAD_ARG, "unknown resampler_class 7"),
    (dict(FM10, input_format=7), fmr.ERR_BAD_ARG, "input_format 7 unknown"),
    (dict(mode=fmr.MODE_FM, input_format=fmr.IQ_U8), fmr.ERR_UNSUPPORTED,
     "input_format != cf32 is converted inside the front-end kernel: enable_resampler must be set"),
    (dict(FM10, mode=9), fmr.ERR_UNSUPPORTED, "mode 9 is not on the hot path (FM, AM, DSB only)"),
    (dict(FM10, max_blocks=0), fmr.ERR_BAD_ARG, "bad capacity / n_streams"),
], ids=["s16_r8b", "ratio", "multipath_320", "resampler_class", "input_format", "raw_without_resampler", "mode", "capacity"])
def test_refused_without_a_device_in_the_creates_words(kw, code, words):
    assert refusal(**kw) == (code, words)


@pytest.mark.parametrize("mode", [fmr.MODE_FM, fmr.MODE_AM, fmr.MODE_NBFM], ids=["fm", "am", "nbfm"])
def test_decoder_without_filter_coeff_is_refused(mode):
    cfg = fmr.Config()
    cfg.n_streams, cfg.mode, cfg.input_rate, cfg.max_block_len, cfg.max_blocks = 1, mode, 384e3 if mode == fmr.MODE_FM else 48e3, 4096, 2
    with pytest.raises(fmr.FmrError) as e:
        fmr.chain_shape_config(cfg)
    assert (e.value.code, e.value.message) == (fmr.ERR_BAD_ARG, "filter_coeff missing")
    cfg.mode = fmr.MODE_NONE                         # a front-end-only chain has no filter
    assert fmr.chain_shape_config(cfg).max_if == 4096 * 2


def test_a_refusal_comes_before_the_device_index_is_looked_at():
    """The one intended difference from a create that validated as it built: where the configuration is refused and the
    device index is bad as well, the configuration's error is the one reported."""
    with pytest.raises(fmr.FmrError, match=r"fmr_create failed \(-2\): input_format 7 unknown"):
        fmr.Chain(**dict(FM10, input_format=7, device=12345))


# ------------------------------------------------------------------ channel bank and channelizer: every refused row
@pytest.mark.parametrize("kw, code, words", bank_args.REFUSALS, ids=bank_args.REFUSAL_IDS)
def test_channel_bank_rows_refused_without_a_device(kw, code, words):
    got, msg = refusal(channel_offsets_hz=[0, 20000], **kw)
    assert got == code and "channel bank" in msg and words in msg, (got, msg)
    assert (got, msg) == bank_args._create(channel_offsets_hz=[0, 20000], **kw)      # (and fmr_create says the same)


@pytest.mark.parametrize("mode, F, f", bank_args.OFFSETS_BEYOND)
def test_channel_bank_offsets_refused_without_a_device(mode, F, f):
    kw = dict(bank_args.FM10, mode=mode, input_rate=F, channel_offsets_hz=[0, f])
    got, msg = refusal(**kw)
    assert got == fmr.ERR_BAD_ARG and "channel_offset_hz[1]" in msg and "(input_rate - decoder rate) / 2" in msg, (got, msg)
    assert (got, msg) == bank_args._create(**kw)


def chz_shape(input_rate, offsets, **kw):
    """(rc, message) of chain_shape for the channelizer configuration of test_channelizer_args._config."""
    cfg, _arr = chz_args._config(input_rate, offsets, **kw)
    try:
        fmr.chain_shape_config(cfg, channelizer=True)
    except fmr.FmrError as e:
        return e.code, e.message
    return fmr.OK, ""


@pytest.mark.parametrize("over, code, words", chz_args.RULES, ids=chz_args.RULE_IDS)
def test_channelizer_rules_refused_without_a_device(over, code, words):
    over = dict(over)
    F = over.pop("input_rate", 10e6)
    rc, msg = chz_shape(F, [0, 20000], **over)
    assert rc == code and msg.startswith("channelizer:") and words in msg, (rc, msg)
    assert (rc, msg) == chz_args._create(F, [0, 20000], **over)


def test_channelizer_without_offsets_refused_without_a_device():
    rc, msg = chz_shape(10e6, [])
    assert rc == fmr.ERR_BAD_ARG and msg.startswith("channelizer:") and "channel_offset_hz" in msg, (rc, msg)


@pytest.mark.parametrize("F, out", chz_args.OFFSET_RATES)
def test_channelizer_offsets_refused_without_a_device(F, out):
    edge = int((F - out) // 2)
    assert chz_shape(F, [0, -edge], output_rate=out) == (fmr.OK, "")
    for f in (edge + 1, -edge - 1):
        rc, msg = chz_shape(F, [0, f], output_rate=out)
        assert rc == fmr.ERR_BAD_ARG and "channel_offset_hz[1]" in msg and "(input_rate - output_rate) / 2" in msg, (rc, msg)
        assert (rc, msg) == chz_args._create(F, [0, f], output_rate=out)


@pytest.mark.parametrize("F, out, cls", chz_args.STAGE_A,
                         ids=[f"{F / 1e6:g}M_{o / 1e3:g}k_{'r8b' if c else 'fast'}" for F, o, c in chz_args.STAGE_A])
def test_channelizer_stage_a_rule_without_a_device(F, out, cls):
    v, D, NA = chz_args._verdict(F, out, cls)
    rc, msg = chz_shape(F, [0], output_rate=out, resampler_class=cls)
    if v == "ok":
        assert rc == fmr.OK, (rc, msg)
        return
    assert rc == fmr.ERR_UNSUPPORTED, (rc, msg)
    if v == "design":
        assert "design range" in msg, msg
    else:
        assert msg.startswith("channelizer:") and f"D = {D}" in msg and "outside the bank kernel's range" in msg, msg
    assert (rc, msg) == chz_args._create(F, [0], output_rate=out, resampler_class=cls)


# ------------------------------------------------------------------ the stage-B ladder
# Restated from the design numbers alone (DESIGN.md "Creating a chain"): output position q of a period of LB starts
# off[q] = q MB / LB mid samples in; a tile of 64 periods stages tl samples.  poly2 needs tl in 96 KB of LDS; poly3 also the
# shift among four consecutive positions inside the rows' zero padding (32 - 8) and 64 samples of slack; poly4 / poly4_am
# need what poly3 needs, poly5h what poly2 needs plus room for its fp16 planes and tap chunks in 160 KB.
def ladder(info):
    LB, MB, TB = info["LB"], info["MB"], info["TB"]
    if info["LT"]:
        return "poly_frac"
    off = [q * MB // LB for q in range(LB)]
    tl = 64 * MB + off[-1] + TB
    poly2 = tl * 8 <= 98304 and LB <= 4096
    dmax = max(off[min(g + 3, LB - 1)] - off[g] for g in range(0, LB, 4))
    poly3 = poly2 and dmax <= 24 and (tl + 64) * 8 <= 98304
    if poly2 and (LB, MB) == (48, 125) and TB != 210 and TB % 2 == 0:
        nkb = -(-((off[47] + TB + 31) // 32) // 4) * 4
        x_len = -(-(tl + 64) // 128) * 128 + 96
        if 8 * x_len + 2 * 4 * 3 * 2 * 64 * 16 <= 160 * 1024 - 64 and 63 * 125 + 32 * nkb <= x_len <= 48 * 256:
            return "poly5h"
    if poly3 and (LB, MB, TB) == (3, 8, 214):
        return "poly4_am"
    if poly3 and (LB, MB, TB) == (48, 125, 210):
        return "poly4"
    return "poly3" if poly3 else "poly2" if poly2 else "poly"


@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: c.name)
def test_base_stage_b_is_the_ladders(case):
    assert shape_of(case).stage_b == ladder(design(case)[2])


def _row(name):
    return next(c for c in RATE_CASES if c.name == name)


def test_ladder_edges():
    # poly2 fits and poly3 does not: 66 / 185 / 226 stages 64 * 185 + 182 + 226 = 12248 samples (97 984 bytes), 64 more do not fit
    c = _row("lds_edge_1m48_am")
    info = design(c)[2]
    assert (info["LB"], info["MB"], info["TB"]) == (66, 185, 226)
    tl = 64 * 185 + 65 * 185 // 66 + 226
    assert tl * 8 <= 98304 < (tl + 64) * 8
    assert shape_of(c).stage_b == "poly2"
    # nothing tiled fits: 192 / 625 stages 40 000 samples and more -> poly; a ppm-corrected rate (LT != 0) -> poly_frac
    c = _row("airspy_2m5_fm_fast")
    assert (design(c)[2]["LB"], design(c)[2]["MB"], design(c)[2]["LT"]) == (192, 625, 0)
    assert shape_of(c).stage_b == "poly"
    c = _row("rtl_2m4_ppm37_fm_u8_f4")
    assert design(c)[2]["LT"] != 0 and shape_of(c).stage_b == "poly_frac"
    # 48 / 125: TB == 210 (FAST class) -> poly4, any other even TB (R8B class: 3122) -> poly5h
    fast, r8b = _row("airspy_6m_fm_fast"), _row("airspy_3m_fm_r8b")
    assert design(fast)[2] == dict(design(fast)[2], LB=48, MB=125, TB=210)
    assert design(r8b)[2] == dict(design(r8b)[2], LB=48, MB=125, TB=3122)
    assert shape_of(fast).stage_b == "poly4" and shape_of(r8b).stage_b == "poly5h"


def test_upgrades_of_the_10ms_shapes():
    """The bench chain (10 MS/s, FAST: D = 10, NA = 103 in front of poly4) takes the fused front end, with the discriminator
    as its epilogue unless the IF filter or the equaliser sits between them; FMR_NO_FUSED and a channel bank switch it off."""
    assert fmr.chain_shape(**FM10).fused == "disc" and fmr.chain_shape(**FM10).pipelined
    s = fmr.chain_shape(**dict(FM10, fmfilter_enable=True, filter_coeff=[0.0] * 63 + [1.0] + [0.0] * 63))
    assert s.fused == "if_only" and s.fir == "poly4_disc"
    assert fmr.chain_shape(**dict(FM10, multipath_stages=2)).fused == "if_only"
    assert fmr.chain_shape(**dict(FM10, fourth_down=True)).fused is None
    assert fmr.chain_shape(**dict(FM10, channel_offsets_hz=[0, 200000])).fused is None
    assert not fmr.chain_shape(**dict(FM10, in_order=True)).pipelined
    r8b = fmr.chain_shape(**dict(FM10, resampler_class=R8B))
    assert r8b.decim16 and r8b.poly5h_disc and r8b.qa == 24
    assert fmr.chain_shape(**dict(FM10, resampler_class=FAST)).qa == 16


def test_no_fused_switch_takes_the_upgrades_away(monkeypatch):
    monkeypatch.setenv("FMR_NO_FUSED", "1")
    s = fmr.chain_shape(**FM10)
    assert s.fused is None and s.stage_b == "poly4"
    r8b = fmr.chain_shape(**dict(FM10, resampler_class=R8B))
    assert not r8b.decim16 and not r8b.poly5h_disc and r8b.stage_b == "poly5h"
    assert shape_of(_row("rtl_2m048_fm_u8_f4")).stage_b == "poly3"      # (poly4_am is the switch's as well)


def test_out_size_newer_than_library_refused():
    L = fmr.lib()
    cfg = fmr.Config()
    out = (C.c_char * (C.sizeof(fmr.ChainShapeInfo) + 8))()
    L.fmr_debug_chain_shape.restype = C.c_int
    L.fmr_debug_chain_shape.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    assert L.fmr_debug_chain_shape(C.byref(cfg), 0, 0, out, C.sizeof(fmr.ChainShapeInfo) + 8) == fmr.ERR_BAD_ARG
    assert "newer than the library" in L.fmr_last_error().decode()

"""Channelizer (fmr_create_channelizer) without a GPU: the new entry points are declared and exported, every rule of the
channel bank is applied by name before the device is opened (with output_rate as the target rate), the facade's
Channelizer compiles, and IqFileWriter -> IqFileReader is bit-exact."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")

NEW = ["fmr_create_channelizer", "fmr_resample_blocks", "fmr_resample_blocks_device"]


def _config(input_rate, offsets, output_rate=0.0, resampler_class=fmr.RESAMPLER_FAST, **over):
    """(fmr_config of a channelizer, the offsets it points to); the fields in `over` are set after the channelizer's own."""
    cfg = fmr.Config()
    cfg.n_streams, cfg.mode, cfg.input_rate, cfg.enable_resampler = len(offsets) or 1, fmr.MODE_NONE, float(input_rate), 1
    cfg.output_rate, cfg.resampler_class = float(output_rate), int(resampler_class)
    cfg.max_block_len, cfg.max_blocks = 65536, 4
    arr = (C.c_int32 * max(1, len(offsets)))(*[int(f) for f in offsets])
    if offsets:
        cfg.channel_offset_hz = arr
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg, arr


def _create(input_rate, offsets, output_rate=0.0, resampler_class=fmr.RESAMPLER_FAST, **over):
    """(rc, message) of fmr_create_channelizer for _config(...)."""
    L = fmr.lib()
    cfg, _arr = _config(input_rate, offsets, output_rate, resampler_class, **over)
    h = C.c_void_p()
    rc = L.fmr_create_channelizer(C.byref(cfg), 0, C.byref(h))
    msg = L.fmr_last_error().decode()
    if rc == fmr.OK:
        L.fmr_destroy(h)
    return rc, msg


def _accepted(rc, msg):
    return rc == fmr.OK or (rc == fmr.ERR_NO_DEVICE and "no HIP device" in msg)


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in fmr.EXPORTS
        assert hasattr(fmr.lib(), name), name
    # the reference interface the batched form generalises is named where it is declared
    decl = hdr[hdr.index("int fmr_resample_blocks(") - 800:hdr.index("int fmr_resample_blocks(")]
    assert "IfResampler.h:35-38" in decl


def _shape(F, out, cls):
    _, d = fmr.design_taps_class(F, out, cls, 0)
    return d["D"], d["NA"]


# (input rate, output rate): the reference's SDR source rates to the FM IF rate, 2.4 MS/s to the AM rate, and rates that
# are neither (250 kHz takes the 3/8 stage-B shape, 200 kHz a generic one, 240 kHz D = 16)
RATES = [(10e6, 384e3), (6e6, 384e3), (2.5e6, 384e3), (2.4e6, 48e3), (10e6, 250e3), (6e6, 200e3), (10e6, 240e3)]


@pytest.mark.parametrize("cls", [fmr.RESAMPLER_FAST, fmr.RESAMPLER_R8B], ids=["fast", "r8b"])
@pytest.mark.parametrize("F, out", RATES, ids=[f"{F / 1e6:g}M_{o / 1e3:g}k" for F, o in RATES])
def test_valid_configs_reach_the_device(F, out, cls):
    D, NA = _shape(F, out, cls)
    assert 2 <= D <= 24 and NA <= 400, (D, NA)      # (the list holds shapes in the kernel's range only)
    edge = int((F - out) // 2)
    rc, msg = _create(F, [-edge, 0, 12345, edge], output_rate=out, resampler_class=cls)
    assert _accepted(rc, msg), (rc, msg)


def test_output_rate_zero_is_384k():
    edge = int((10e6 - 384e3) // 2)
    assert _accepted(*_create(10e6, [edge]))
    rc, msg = _create(10e6, [edge + 1])
    assert rc == fmr.ERR_BAD_ARG and "(input_rate - output_rate) / 2" in msg, (rc, msg)


RULES = [
    (dict(mode=fmr.MODE_FM), fmr.ERR_UNSUPPORTED, "mode = -1"),
    (dict(mode=fmr.MODE_AM), fmr.ERR_UNSUPPORTED, "mode = -1"),
    (dict(enable_resampler=0), fmr.ERR_UNSUPPORTED, "enable_resampler = 1"),
    (dict(input_format=fmr.IQ_S16), fmr.ERR_UNSUPPORTED, "input_format"),
    (dict(input_format=fmr.IQ_U8), fmr.ERR_UNSUPPORTED, "input_format"),
    (dict(enable_fourth_down=1), fmr.ERR_BAD_ARG, "enable_fourth_down"),
    (dict(input_rate=2.4e6 * (1 + 37e-6)), fmr.ERR_UNSUPPORTED, "whole number of hertz"),
]
RULE_IDS = ["fm_mode", "am_mode", "no_resampler", "s16", "u8", "fourth_down", "ppm_rate"]


@pytest.mark.parametrize("over, code, words", RULES, ids=RULE_IDS)
def test_rules_refused_by_name(over, code, words):
    over = dict(over)
    rc, msg = _create(over.pop("input_rate", 10e6), [0, 20000], **over)
    assert rc == code, (rc, msg)
    assert msg.startswith("channelizer:") and words in msg, msg


def test_no_offsets_refused():
    rc, msg = _create(10e6, [])
    assert rc == fmr.ERR_BAD_ARG and msg.startswith("channelizer:") and "channel_offset_hz" in msg, (rc, msg)


OFFSET_RATES = [(10e6, 384e3), (2.4e6, 48e3), (10e6, 250e3)]


@pytest.mark.parametrize("F, out", OFFSET_RATES)
def test_offset_beyond_half_the_band_refused(F, out):
    edge = int((F - out) // 2)
    assert _accepted(*_create(F, [0, -edge], output_rate=out))
    for f in (edge + 1, -edge - 1):
        rc, msg = _create(F, [0, f], output_rate=out)
        assert rc == fmr.ERR_BAD_ARG, (rc, msg)
        assert "channel_offset_hz[1]" in msg and "(input_rate - output_rate) / 2" in msg, msg


# Output rates of 10, 6 and 2.4 MS/s captures over a wide range (the R8B class passes NA = 400 between 192 and 160 kHz at
# 10 MS/s).  The verdict each one must get is derived from the design inside the tests: nothing here may load the
# library while pytest collects (conftest.py: torch's HIP context comes up first on the GPU box).
STAGE_A = [(F, out, cls) for F in (10e6, 6e6, 2.4e6)
           for out in (4e6, 2e6, 1e6, 500e3, 384e3, 300e3, 200e3, 192e3, 180e3, 176.4e3, 170e3, 160e3, 150e3, 120e3,
                       100e3, 96e3, 60e3, 48e3, 44.1e3, 32e3, 24e3) if out < F
           for cls in (fmr.RESAMPLER_FAST, fmr.RESAMPLER_R8B)]


def _verdict(F, out, cls):
    """"ok", "D" (outside 2 .. 24), "NA" (over 400) or "design" (no design at this ratio) from fmr_design_taps_class."""
    try:
        D, NA = _shape(F, out, cls)
    except fmr.FmrError:
        return "design", None, None
    return ("ok" if 2 <= D <= 24 and NA <= 400 else "D" if D < 2 or D > 24 else "NA"), D, NA


def test_stage_a_cases_cover_every_verdict():
    verdicts = {_verdict(*c)[0] for c in STAGE_A}
    assert {"ok", "D", "NA"} <= verdicts, verdicts


@pytest.mark.parametrize("F, out, cls", STAGE_A,
                         ids=[f"{F / 1e6:g}M_{o / 1e3:g}k_{'r8b' if c else 'fast'}" for F, o, c in STAGE_A])
def test_stage_a_shape_rule(F, out, cls):
    """Accept / refuse follows the design (fmr_design_taps_class): D = 2 .. 24 and NA <= 400."""
    v, D, NA = _verdict(F, out, cls)
    rc, msg = _create(F, [0], output_rate=out, resampler_class=cls)
    if v == "ok":
        assert _accepted(rc, msg), (rc, msg)
    elif v == "design":
        assert rc == fmr.ERR_UNSUPPORTED and "design range" in msg, (rc, msg)
    else:
        assert rc == fmr.ERR_UNSUPPORTED, (rc, msg)
        assert msg.startswith("channelizer:") and f"D = {D}" in msg and "outside the bank kernel's range" in msg, msg


def test_decoder_bank_rules_keep_their_words():
    """fmr_create still refuses a front-end-only bank, in the channel bank's words."""
    with pytest.raises(fmr.FmrError, match=r"fmr_create failed \(-3\): channel bank: .*mode != -1"):
        fmr.Chain(mode=fmr.MODE_NONE, input_rate=10e6, enable_resampler=True, channel_offsets_hz=[0, 1000])


def test_cfg_size_newer_than_library_refused():
    L = fmr.lib()
    cfg = fmr.Config()
    h = C.c_void_p()
    assert L.fmr_create_channelizer(C.byref(cfg), C.sizeof(cfg) + 8, C.byref(h)) == fmr.ERR_BAD_ARG
    assert "newer than the library" in L.fmr_last_error().decode()


def _compile(tmp_path, src, name):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(libdir, 'host')}", os.path.join(ROOT, "tests", src), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_facade_channelizer_compiles(tmp_path):
    """The facade's Channelizer builds with -Wall -Werror; without a GPU the program stops loudly with "no HIP device"."""
    exe = _compile(tmp_path, "channelizer_smoke.cpp", "channelizer_smoke")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0 and "channels 3" in r.stdout) or (r.returncode != 0 and "no HIP device" in r.stderr), \
        (r.returncode, r.stdout, r.stderr)


def test_iq_file_writer_round_trip(tmp_path):
    """IqFileWriter -> IqFileReader is bit-exact (NaN, infinities, denormals, signed zeros included), and the file on
    disk is a valid 2-channel IEEE-float WAV after every write."""
    exe = _compile(tmp_path, "channelizer_smoke.cpp", "channelizer_smoke")
    r = subprocess.run([exe, str(tmp_path), "--fileio"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "iq round trip ok" in r.stdout, r.stdout

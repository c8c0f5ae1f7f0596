"""Channel bank (fmr_config.channel_offset_hz) without a GPU: the refusal rules of fmr_create, the header's contract and
the sign convention of the composite fixture the GPU tests build on (tests/test_gpu_channel_bank.py)."""
import importlib
import os
import re

import numpy as np
import pytest

import chanbank_fixture as cb
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")


def _create(**kw):
    """(rc, message) of fmr_create for a Chain(**kw); rc = 0 when it succeeded (a GPU is present)."""
    try:
        ch = fmr.Chain(**kw)
    except fmr.FmrError as e:
        m = re.match(r"fmr_create failed \((-?\d+)\): (.*)", str(e))
        assert m, str(e)
        return int(m.group(1)), m.group(2)
    ch.close()
    return 0, ""


FM10 = dict(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, max_block_len=65536, max_blocks=4)


REFUSALS = [
    (dict(FM10, enable_resampler=False), fmr.ERR_UNSUPPORTED, "enable_resampler"),
    (dict(FM10, mode=fmr.MODE_NONE), fmr.ERR_UNSUPPORTED, "mode != -1"),
    (dict(FM10, input_format=fmr.IQ_U8), fmr.ERR_UNSUPPORTED, "input_format"),
    (dict(FM10, fourth_down=True), fmr.ERR_BAD_ARG, "enable_fourth_down"),
    (dict(FM10, input_rate=2.4e6 * (1 + 37e-6)), fmr.ERR_UNSUPPORTED, "whole number of hertz"),
    (dict(FM10, input_rate=1.152e6), fmr.ERR_UNSUPPORTED, "D = 1"),
    (dict(FM10, input_rate=912e3), fmr.ERR_UNSUPPORTED, "D = 1"),
    (dict(FM10, input_rate=456e3), fmr.ERR_UNSUPPORTED, "D = 1"),
    (dict(FM10, mode=fmr.MODE_AM), fmr.ERR_UNSUPPORTED, "D = 80"),
]
REFUSAL_IDS = ["no_resampler", "front_end_only", "raw_format", "fourth_down", "ppm_rate", "d1_1m152", "d1_912k", "d1_456k",
               "d80_10m_am"]


@pytest.mark.parametrize("kw, code, words", REFUSALS, ids=REFUSAL_IDS)
def test_refusals(kw, code, words):
    rc, msg = _create(channel_offsets_hz=[0, 20000], **kw)
    assert rc == code, (rc, msg)
    assert "channel bank" in msg and words in msg, msg


OFFSETS_BEYOND = [(fmr.MODE_FM, 10e6, 4_808_001), (fmr.MODE_FM, 10e6, -4_808_001),
                  (fmr.MODE_AM, 2.4e6, 1_176_001), (fmr.MODE_NBFM, 1.48e6, -716_001)]


@pytest.mark.parametrize("mode, F, f", OFFSETS_BEYOND)
def test_offset_beyond_half_the_band_refused(mode, F, f):
    rc, msg = _create(**dict(FM10, mode=mode, input_rate=F), channel_offsets_hz=[0, f])
    assert rc == fmr.ERR_BAD_ARG, (rc, msg)
    assert "channel_offset_hz[1]" in msg and "(input_rate - decoder rate) / 2" in msg, msg


# every other shape of the source-rate table: D = 2 .. 19, NA <= 367, both classes
VALID = [(fmr.MODE_FM, F, cls) for F in (2.5e6, 3e6, 6e6, 10e6) for cls in (fmr.RESAMPLER_FAST, fmr.RESAMPLER_R8B)] + \
        [(m, F, cls) for m in (fmr.MODE_NBFM, fmr.MODE_AM) for F in (2.4e6, 1.48e6, 1.152e6, 912e3)
         for cls in (fmr.RESAMPLER_FAST, fmr.RESAMPLER_R8B)]


@pytest.mark.parametrize("mode, F, cls", VALID)
def test_valid_bank_passes_validation(mode, F, cls):
    dec = 384e3 if mode == fmr.MODE_FM else 48e3
    edge = int((F - dec) // 2)
    rc, msg = _create(**dict(FM10, mode=mode, input_rate=F, resampler_class=cls), channel_offsets_hz=[-edge, 0, edge])
    # without a GPU the chain gets past every bank rule and fails where the device is opened
    assert rc == fmr.OK or (rc == fmr.ERR_NO_DEVICE and "no HIP device" in msg), (rc, msg)


def test_header_contract():
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    body = hdr[hdr.index("typedef struct {\n  int device;"):hdr.index("} fmr_config;")]
    fields = re.findall(r"^\s+(?:const\s+)?[\w ]+?\s\*?(\w+);", body, re.M)
    assert fields[-2:] == ["in_order", "channel_offset_hz"], fields[-3:]
    assert "const int32_t *channel_offset_hz;" in body
    cbs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"FMR_CB_(\w+)\s*=\s*1\s*<<\s*(\d+)", hdr))
    assert {k.lower(): 1 << v for k, v in cbs.items()} == fmr.CB_FORMS
    fes = {m.group(1).lower(): 1 << int(m.group(2)) for m in re.finditer(r"FMR_FE_(\w+)\s*=\s*1\s*<<\s*(\d+)", hdr)}
    assert fes == fmr.FE_FORMS            # no new FMR_FE_* bit
    assert [n for n, _ in fmr.Config._fields_][-1] == "channel_offset_hz"
    assert b"0.4" in fmr.lib().fmr_version()


def test_fixture_sign_convention(pilotcut):
    """The oracle, decoding u_s from the composite, hears station s's own left tone: offsets point at +f in the spectrum."""
    F, n = 2.5e6, 2_000_000
    offs, ids, amps = [-700_000, 0, 450_000], [3, 11, 22], [0.3, 0.12, 0.2]
    x = cb.composite(n, F, offs, ids, amps)
    lens = [65536] * (n // 65536)
    for f, i in zip(offs, ids):
        fm, out = cb.oracle_fm(cb.mix_down(x, f, F), F, lens, pilotcut, delay=fmr.DELAY_3TAPS)
        a = np.concatenate(out)
        assert fm.stereo_detected()
        left = a[0::2][-24000:]
        assert abs(cb.peak_hz(left, 48000.0) - cb.left_tone(i)) < 3.0, (f, i, cb.peak_hz(left, 48000.0))


def test_facade_channel_bank_compiles(tmp_path):
    """The facade's ChannelBank builds with g++ -std=c++17; without a GPU the program stops loudly with "no HIP device"."""
    import subprocess
    exe = str(tmp_path / "channel_bank_smoke")
    libdir = os.path.join(ROOT, "airspy-fmradion_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(libdir, 'host')}", os.path.join(ROOT, "tests", "channel_bank_smoke.cpp"), "-o", exe,
                    f"-L{libdir}", "-lfmradion_amd", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0 and "stereo 1 1" in r.stdout) or (r.returncode != 0 and "no HIP device" in r.stderr), \
        (r.returncode, r.stdout, r.stderr)

"""CPU-side checks of the output stage's entry points (include/fmradion_amd.h, fmr_enable_output / fmr_output_read /
fmr_squelch_level_from_db): the struct layouts of header and binding, every configuration refusal by name before the
chain is looked at, and AudioFileWriter::write_i16 read back from the container."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest
from scipy.io import wavfile

import output_fixture as of
from cheader import header_struct as _header_struct
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.OutputConfig(C.sizeof(fmr.OutputConfig), 0, 0.0, 0.0, 0, 0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_output(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_output_config", "OutputConfig", 32), ("fmr_output_block", "OutputBlock", 56), ("fmr_output_info", "OutputInfo", 56)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_output_block")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.OUTPUT_BLOCK, of.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 56
    assert (fmr.PCM_S16, fmr.PCM_F32) == (of.PCM_S16, of.PCM_F32) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    assert "enum { FMR_PCM_S16 = 0, FMR_PCM_F32 = 1 };" in hdr


@pytest.mark.parametrize("field,value", [
    ("format", 2), ("format", -1), ("squelch_level", -1e-9), ("squelch_level", float("nan")), ("squelch_level", float("inf")),
    ("gain", -0.5), ("gain", float("nan")), ("gain", float("inf")), ("max_frames", (1 << 26) + 1), ("max_blocks", 65537)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_output" in msg and field in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.OutputConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_output_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.OutputConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_output(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    got = C.c_size_t(77)
    assert L.fmr_output_read(None, 0, None, 0, None, 0, C.byref(got), None, 0) == fmr.ERR_BAD_ARG
    assert got.value == 0 and "fmr_output_read" in L.fmr_last_error().decode()


@pytest.mark.parametrize("kw", [{}, {"format": 1, "squelch_level": 0.03, "gain": 1.0, "max_frames": 1, "max_blocks": 1},
                                {"max_frames": 1 << 26, "max_blocks": 65536}, {"struct_size": 0}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_a_shorter_struct_takes_the_defaults(L):
    """A caller that knows only struct_size and format: everything else is zero = default; the chain is looked at next."""
    rc, msg = _enable(L, _cfg(struct_size=8, max_frames=(1 << 26) + 1), size=8)
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, msg


def test_squelch_level_from_db(L):
    got = fmr.squelch_level_from_db(20.0)
    assert abs(got - 0.1) <= np.spacing(0.1), got
    assert fmr.squelch_level_from_db(0.0) == 1.0
    for db in (-6.0, 3.0, 40.0, 150.0):
        assert abs(fmr.squelch_level_from_db(db) - of.squelch_level_from_db(db)) <= np.spacing(of.squelch_level_from_db(db))


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_output", "fmr_output_read", "fmr_squelch_level_from_db"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- AudioFileWriter::write_i16 --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("output_fileio")
    out = os.path.join(d, "output_fileio_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(ROOT, "tests", "output_fileio_check.cpp")], check=True)
    return out


def _write(exe, fmt, src, dst, rate, stereo, piece):
    r = subprocess.run([exe, "write", fmt, src, dst, str(rate), str(int(stereo)), str(piece)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [int(v) for v in r.stdout.split()[1::2]]


@pytest.mark.parametrize("stereo,n", [(True, 2 * 5000), (False, 4321)])
def test_write_i16_round_trips(exe, tmp_path, stereo, n):
    pcm = np.random.default_rng(3).integers(-32768, 32768, size=n).astype(np.int16)
    pcm[:4] = [-32768, 32767, 0, -1]
    src = str(tmp_path / "pcm.s16")
    pcm.tofile(src)
    raw, wav = str(tmp_path / "a.raw"), str(tmp_path / "a.wav")
    assert _write(exe, "RAW_INT16", src, raw, 48000, stereo, 777) == [n, 0]
    assert np.array_equal(np.fromfile(raw, dtype=np.int16), pcm)                  # the bytes as they are
    assert _write(exe, "WAV_INT16", src, wav, 48000, stereo, 1000) == [n, 0]
    rate, data = wavfile.read(wav)
    assert rate == 48000 and data.dtype == np.int16 and np.array_equal(data.reshape(-1), pcm)
    assert data.shape == ((n // 2, 2) if stereo else (n,))
    if stereo:      # the reader of the project itself (IqFileReader: two-channel WAV, sf_read_float's x / 32768)
        dump = str(tmp_path / "dump.cf32")
        r = subprocess.run([exe, "read", wav, dump], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == ["rate", "48000", "samples", str(n // 2)], r.stdout + r.stderr
        assert np.array_equal(np.fromfile(dump, dtype=np.float32), (pcm / 32768.0).astype(np.float32))


def test_write_i16_is_refused_on_a_float_container(exe, tmp_path):
    src = str(tmp_path / "pcm.s16")
    np.arange(100, dtype=np.int16).tofile(src)
    assert _write(exe, "WAV_FLOAT32", src, str(tmp_path / "f.wav"), 48000, True, 50) == [0, 1]

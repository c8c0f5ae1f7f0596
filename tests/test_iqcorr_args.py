"""CPU-side checks of the IQ corrector's entry points (include/fmradion_amd.h, fmr_enable_iq_correction /
fmr_iq_correction_read / fmr_iq_correction_derive): the struct layouts of header and binding, every refusal that can be
reached without a chain, by field name and before the chain is looked at, the exports, and the host-only derive call on
hand-made records."""
import ctypes as C
import importlib
import math
import subprocess

import numpy as np
import pytest

import cheader
import iqcorr_fixture as qf

fmr = importlib.import_module("airspy-fmradion_amd")
Q = qf.Q


def _header_struct(name):
    cheader.CT.setdefault("int64_t", C.c_int64)          # (the record is the header's first struct with signed 64-bit sums)
    return cheader.header_struct(name)


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


def _cfg(**kw):
    c = fmr.IqCorrectionConfig(struct_size=C.sizeof(fmr.IqCorrectionConfig))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _enable(L, cfg, size=None, chain=None):
    rc = L.fmr_enable_iq_correction(chain, C.byref(cfg), C.sizeof(cfg) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("name,binding,size", [
    ("fmr_iq_correction_config", "IqCorrectionConfig", 28), ("fmr_iq_correction_info", "IqCorrectionInfo", 72),
    ("fmr_iq_correction_levels", "IqCorrectionLevels", 120)])
def test_header_and_ctypes_layouts_agree(name, binding, size):
    h, b = _header_struct(name), getattr(fmr, binding)
    assert [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_] == \
           [(n, getattr(b, n).offset, getattr(b, n).size) for n, _ in b._fields_]
    assert C.sizeof(h) == C.sizeof(b) == size


def test_record_layout_agrees_with_the_numpy_types():
    h = _header_struct("fmr_iq_correction_record")
    want = [(n, getattr(h, n).offset, getattr(h, n).size) for n, _ in h._fields_]
    for dt in (fmr.IQ_CORRECTION_RECORD, qf.RECORD):
        assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == want
        assert dt.itemsize == C.sizeof(h) == 112
        assert all(dt.fields[k][0] == np.int64 for k in qf.SUMS)


def test_constants_agree_with_the_fixture():
    assert (fmr.IQC_MEASURE, fmr.IQC_ACT) == (0, 1) and (fmr.IQC_DC, fmr.IQC_BALANCE) == (qf.DC, qf.BALANCE) == (1, 2)
    assert fmr.NB_Q == qf.Q == 4096


@pytest.mark.parametrize("field,value", [
    ("mode", 2), ("mode", -1), ("correct", 4), ("correct", -1), ("average_intervals", -1), ("average_intervals", 1025),
    ("record_intervals", -1), ("record_intervals", 4097), ("max_records", -1), ("max_records", 65537)])
def test_config_refusals_name_the_field_before_the_chain_is_looked_at(L, field, value):
    rc, msg = _enable(L, _cfg(**{field: value}))
    assert rc == fmr.ERR_BAD_ARG, (field, value, rc, msg)
    assert "fmr_enable_iq_correction" in msg and field in msg, msg


def test_larger_struct_and_null_arguments(L):
    rc, msg = _enable(L, _cfg(), size=C.sizeof(fmr.IqCorrectionConfig) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "fmr_iq_correction_config" in msg, msg
    rc, msg = _enable(L, _cfg(struct_size=C.sizeof(fmr.IqCorrectionConfig) + 8))
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, msg
    assert L.fmr_enable_iq_correction(None, None, 0) == fmr.ERR_BAD_ARG and "cfg" in L.fmr_last_error().decode()
    assert L.fmr_iq_correction_read(None, 0, None, 0, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_iq_correction_derive(None, 1, None, 0) == fmr.ERR_BAD_ARG
    assert L.fmr_debug_read(None, 0, 7, None, 0) == fmr.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [
    {}, {"struct_size": 0}, {"mode": 1, "correct": 1, "average_intervals": 1, "record_intervals": 1, "max_records": 1},
    {"correct": 2}, {"correct": 3, "average_intervals": 1024, "record_intervals": 4096, "max_records": 65536}])
def test_valid_config_with_a_null_chain_names_the_chain(L, kw):
    rc, msg = _enable(L, _cfg(**kw))
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, (kw, rc, msg)


def test_a_shorter_struct_takes_the_defaults_for_the_rest(L):
    # a caller that knows only struct_size and mode
    rc, msg = _enable(L, _cfg(struct_size=8, average_intervals=-5), size=8)
    assert rc == fmr.ERR_BAD_ARG and "chain is null" in msg, msg


def test_exports(L):
    out = subprocess.run(["nm", "-D", "--defined-only", fmr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("fmr_enable_iq_correction", "fmr_iq_correction_read", "fmr_iq_correction_derive"):
        assert name in fmr.EXPORTS and hasattr(L, name) and f" T {name}" in out


# ---- fmr_iq_correction_derive --------------------------------------------------------------------------------------
def _hand_made():
    """Two records of 2 intervals: I = +-1/2, Q = +-3/8 in quadrature (g = 3/4, w = 1/7), on top of a DC of (1/8, -1/16)"""
    r = np.zeros(2, dtype=fmr.IQ_CORRECTION_RECORD)
    n = 2 * Q
    r["index"], r["first_interval"], r["n_intervals"], r["n_usable"] = [3, 4], [6, 8], 2, n
    one = 1 << 36
    r["sum_re"], r["sum_im"] = n * one // 8, -n * one // 16
    r["sum_rr"] = n * (one // 4 + one // 64)
    r["sum_ii"] = n * (9 * one // 64 + one // 256)
    r["sum_ri"] = -n * one // 128
    r["n_skipped"], r["n_nonfinite"], r["n_refused"] = [1, 2], [0, 5], [0, 1]
    return r


def test_derive_on_hand_made_records():
    got = fmr.iq_correction_levels(_hand_made())
    assert (got["n_intervals"], got["n_usable"], got["n_skipped"], got["n_nonfinite"], got["n_refused"]) == (4, 4 * Q, 3, 5, 1)
    assert got["usable_share"] == 1.0 and got["refused"] == 0
    assert (got["dc_re"], got["dc_im"]) == (0.125, -0.0625)
    assert abs(got["dc_dbfs"] - 20 * math.log10(math.hypot(0.125, 0.0625))) < 1e-12
    assert abs(got["w_re"] - 1 / 7) < 1e-15 and got["w_im"] == 0.0
    assert abs(got["image_rejection_db"] - 20 * math.log10(7)) < 1e-12
    assert abs(got["gain_imbalance_db"] - 20 * math.log10(0.75)) < 1e-12 and got["phase_error_deg"] == 0.0
    ref = qf.derive(_hand_made().astype(qf.RECORD))
    for k, v in ref.items():
        assert got[k] == v or abs(got[k] - v) < 1e-12, k


def test_derive_of_a_balanced_row_a_short_one_and_refusals(L):
    r = _hand_made()[:1]
    r["sum_ii"], r["sum_ri"], r["sum_re"], r["sum_im"] = r["sum_rr"], 0, 0, 0
    got = fmr.iq_correction_levels(r)
    assert got["w_re"] == 0.0 and got["w_im"] == 0.0 and got["image_rejection_db"] == math.inf
    assert got["gain_imbalance_db"] == 0.0 and got["phase_error_deg"] == 0.0 and got["dc_dbfs"] == -math.inf
    # fewer than Q / 2 usable samples: nothing is estimated
    r = _hand_made()[:1]
    r["n_usable"] = Q // 2 - 1
    got = fmr.iq_correction_levels(r)
    assert got["dc_re"] == 0.0 and got["w_re"] == 0.0 and got["image_rejection_db"] == math.inf
    assert got["usable_share"] == (Q // 2 - 1) / (2 * Q)
    # an improper pool: g = 1/4 gives w = 0.6, reported as refused
    r = _hand_made()[:1]
    r["sum_re"], r["sum_im"], r["sum_ri"] = 0, 0, 0
    r["sum_rr"], r["sum_ii"] = 2 * Q * (1 << 34), 2 * Q * (1 << 30)
    got = fmr.iq_correction_levels(r)
    assert got["refused"] == 1 and got["w_re"] == 0.0 and got["image_rejection_db"] == math.inf
    out = fmr.IqCorrectionLevels()
    bad = _hand_made()
    bad["n_intervals"][1] = 0
    assert L.fmr_iq_correction_derive(bad.ctypes.data, 2, C.byref(out), 0) == fmr.ERR_BAD_ARG
    assert "n_intervals" in L.fmr_last_error().decode()
    good = _hand_made()
    for n in (0, -1):
        assert L.fmr_iq_correction_derive(good.ctypes.data, n, C.byref(out), 0) == fmr.ERR_BAD_ARG
        assert "n < 1" in L.fmr_last_error().decode()
    # a caller that knows a shorter struct gets that many bytes
    out.dc_im = 123.0
    assert L.fmr_iq_correction_derive(good.ctypes.data, 2, C.byref(out), 16) == fmr.OK
    assert out.dc_im == 123.0 and out.struct_size == C.sizeof(fmr.IqCorrectionLevels) and out.dc_re == 0.125

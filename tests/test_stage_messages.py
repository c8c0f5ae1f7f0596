"""The refusals of the record stages' entry points that need no chain, text and return code, held verbatim.

Seven stages write records into a ring: modulation monitor, RF monitor, audio monitor, analyser, weak-signal handling,
impulse blanker, IQ correction.  Their fmr_enable_* / fmr_*_read / fmr_*_derive share one reader, one field check and one
derive front in the library; what a caller sees of them -- fmr_last_error() and the return code -- is recorded in
tests/golden/stage_messages.json and compared here case by case.  `python tests/test_stage_messages.py` writes the fixture
from the library it finds (it was recorded from a build of the commit before the shared helpers)."""
import ctypes as C
import importlib
import json
import math
import os

import numpy as np
import pytest

fmr = importlib.import_module("airspy-fmradion_amd")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_messages.json")
NAN, INF = math.nan, math.inf


def _below(x):
    return float(np.nextafter(x, -INF))


def _above(x):
    return float(np.nextafter(x, INF))


# stage -> (config type, [(field, values one step below and above its range, and what else its check tells apart)])
STAGES = {
    "monitor": ("MonitorConfig", [
        ("interval_samples", [511, 513, (1 << 30) + 512]), ("hist_bins", [-1, 1, 1025]),
        ("hist_range", [_below(0.0), -2.0, INF, NAN]), ("max_records", [-1, 4097])]),
    "rf_monitor": ("RfMonitorConfig", [("interval_samples", [511, 513, (1 << 30) + 512]), ("max_records", [-1, 4097])]),
    "loudness": ("LoudnessConfig", [("step_samples", [32, 47, 56, (1 << 20) + 16]), ("max_records", [-1, 65537])]),
    "analyser": ("AnalyserConfig", [
        ("fft_size", [-1, 512, 1000, 16384]), ("interval_samples", [1024, 2049, (1 << 24) + 2048]), ("max_records", [-1, 4097])]),
    "weak_signal": ("WeakSignalConfig", [
        ("mode", [-1, 2]), ("actions", [8, 0xffffffff]), ("record_intervals", [-1, 1001]), ("max_records", [-1, 65537]),
        ("attack_ms", [_below(0.0), _above(60000.0), NAN]), ("release_ms", [_below(0.0), _above(60000.0), NAN]),
        ("blend_lo_db", [-23.0, INF, NAN]), ("blend_hi_db", [-40.0, INF]), ("highcut_lo_db", [-15.0, NAN]),
        ("highcut_hi_db", [-30.0, -INF]), ("mute_lo_db", [-9.0, NAN]), ("mute_hi_db", [-20.0, NAN]),
        ("highcut_hz", [_below(500.0), _above(15000.0), -1.0, NAN]), ("mute_floor_db", [_above(0.0), 3.0, -INF, NAN])]),
    "blanker": ("BlankerConfig", [
        ("mode", [-1, 2]), ("threshold_db", [_below(6.0), _above(40.0), -12.0, NAN]), ("gate_samples", [-1, 257]),
        ("max_run_samples", [-1, 1025]), ("average_intervals", [-1, 65]), ("record_intervals", [-1, 4097]),
        ("max_records", [-1, 65537])]),
    "iq_correction": ("IqCorrectionConfig", [
        ("mode", [-1, 2]), ("correct", [-1, 4]), ("average_intervals", [-1, 1025]), ("record_intervals", [-1, 4097]),
        ("max_records", [-1, 65537])]),
}
# two fields together, where a check reads both
PAIRS = {"blanker": [{"gate_samples": 16, "max_run_samples": 15}, {"gate_samples": 256, "max_run_samples": 255}],
         "weak_signal": [{"blend_lo_db": -20.0, "blend_hi_db": -20.0}, {"mute_lo_db": 1.0, "mute_hi_db": 0.5}]}
# fmr_*_read(chain = null, ...): the arguments behind the chain
READ_ARGS = {"monitor": (0, None, None, None, 0, None, 0), "rf_monitor": (0, None, None, None, 0, None, 0),
             "loudness": (0, None, 0, None, 0), "analyser": (0, None, None, 0, None, 0), "weak_signal": (0, None, 0, None, 0),
             "blanker": (0, None, 0, None, 0), "iq_correction": (0, None, 0, None, 0)}
RECORDS = {"monitor": "MONITOR_RECORD", "rf_monitor": "RF_MONITOR_RECORD", "loudness": "LOUDNESS_RECORD",
           "analyser": "ANALYSER_RECORD", "weak_signal": "WEAK_SIGNAL_RECORD", "blanker": "BLANKER_RECORD",
           "iq_correction": "IQ_CORRECTION_RECORD"}
LEVELS = {"monitor": "MonitorLevels", "rf_monitor": "RfMonitorLevels", "loudness": "LoudnessLevels", "analyser": "AnalyserLevels",
          "weak_signal": "WeakSignalLevels", "blanker": "BlankerLevels", "iq_correction": "IqCorrectionLevels"}


def _derive(L, stage, recs, n, out):
    """fmr_<stage>_derive on recs (an address or None) with the other arguments valid."""
    f = getattr(L, f"fmr_{stage}_derive")
    o = C.byref(out) if out is not None else None
    if stage == "monitor":
        return f(recs, None, n, o, 0)
    if stage == "rf_monitor":
        return f(recs, None, None, n, o, 0)
    if stage == "loudness":
        return f(recs, n, -60.0, o, 0)
    if stage == "blanker":
        return f(recs, n, 2.5e6, o, 0)
    if stage == "analyser":
        spectra = np.zeros(3 * 2049)
        return f(recs, spectra.ctypes.data, n, None, 0, o, 0)
    return f(recs, n, o, 0)


def _cases(L):
    """[(case id, thunk -> return code)] in a fixed order."""
    out = []
    for stage, (cfg_name, fields) in STAGES.items():
        T = getattr(fmr, cfg_name)
        enable = getattr(L, f"fmr_enable_{stage}")

        def en(kw, size=None, enable=enable, T=T):
            cfg = T(struct_size=C.sizeof(T))
            for k, v in kw.items():
                setattr(cfg, k, v)
            return enable(None, C.byref(cfg), C.sizeof(T) if size is None else size)

        out.append((f"{stage}.enable.null_cfg", lambda enable=enable: enable(None, None, 0)))
        out.append((f"{stage}.enable.cfg_size_larger", lambda en=en, T=T: en({}, C.sizeof(T) + 8)))
        out.append((f"{stage}.enable.struct_size_larger", lambda en=en, T=T: en({"struct_size": C.sizeof(T) + 8})))
        for field, values in fields:
            for v in values:
                out.append((f"{stage}.enable.{field}={v!r}", lambda en=en, field=field, v=v: en({field: v})))
        for kw in PAIRS.get(stage, []):
            out.append((f"{stage}.enable.{kw!r}", lambda en=en, kw=kw: en(kw)))
        out.append((f"{stage}.enable.null_chain", lambda en=en: en({})))
        out.append((f"{stage}.enable.null_chain.struct_size_0", lambda en=en: en({"struct_size": 0})))
        read = getattr(L, f"fmr_{stage}_read")
        out.append((f"{stage}.read.null_chain", lambda read=read, stage=stage: read(None, *READ_ARGS[stage])))
        dt = getattr(fmr, RECORDS[stage])
        lv = getattr(fmr, LEVELS[stage])
        out.append((f"{stage}.derive.null_recs", lambda stage=stage, lv=lv: _derive(L, stage, None, 1, lv())))
        out.append((f"{stage}.derive.null_out",
                    lambda stage=stage, dt=dt: _derive(L, stage, np.zeros(1, dtype=dt).ctypes.data, 1, None)))
        out.append((f"{stage}.derive.n=0", lambda stage=stage, dt=dt, lv=lv: _derive(L, stage, np.zeros(1, dtype=dt).ctypes.data, 0, lv())))
        if "n_intervals" in dt.names:      # a hand-made record no read has filled, behind one that looks filled
            def unfilled(stage=stage, dt=dt, lv=lv):
                r = np.zeros(2, dtype=dt)
                r["n_intervals"] = [4, 0]
                return _derive(L, stage, r.ctypes.data, 2, lv())
            out.append((f"{stage}.derive.n_intervals=0", unfilled))
    for tap in (6, 7):
        out.append((f"debug_read.tap{tap}.null_chain", lambda tap=tap: L.fmr_debug_read(None, 0, tap, None, 0)))
    return out


def _sentinel(L):
    """A refusal of an entry point none of the cases use: a case that sets no message of its own shows this one."""
    assert L.fmr_get_output_rate(None, 0, None, 0) == fmr.ERR_BAD_ARG
    return L.fmr_last_error().decode()


def collect(L):
    got = {}
    for cid, thunk in _cases(L):
        _sentinel(L)
        rc = int(thunk())
        got[cid] = {"rc": rc, "error": L.fmr_last_error().decode()}
    return got


@pytest.fixture(scope="module")
def L():
    fmr.build_library()
    return fmr.lib()


@pytest.fixture(scope="module")
def got(L):
    return collect(L)


WANT = {}
if os.path.exists(GOLDEN):
    with open(GOLDEN) as _f:
        WANT = json.load(_f)


def test_the_fixture_holds_exactly_the_cases(got):
    assert list(got) == list(WANT)


@pytest.mark.parametrize("cid", list(WANT))
def test_message_and_return_code(got, cid):
    assert got[cid] == WANT[cid]


def test_every_case_is_a_refusal_and_all_but_the_debug_taps_name_their_function(L, got):
    quiet = _sentinel(L)
    for cid, g in got.items():
        assert g["rc"] < 0, (cid, g)
        if cid.startswith("debug_read"):
            assert g["error"] == quiet, (cid, g)       # (fmr_debug_read refuses a null chain without a message)
        else:
            stage, what = cid.split(".")[:2]
            assert g["error"].startswith(f"fmr_enable_{stage}: " if what == "enable" else f"fmr_{stage}_{what}: "), (cid, g)


if __name__ == "__main__":
    fmr.build_library()
    with open(GOLDEN, "w") as f:
        json.dump(collect(fmr.lib()), f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}")

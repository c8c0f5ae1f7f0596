"""The IF resampler at the source rates the reference's SDR sources deliver (CPU side; the table is shared with
tests/test_gpu_front_end_rates.py).

The chain picks one of about a dozen kernel forms for each stage of the IF resampler, at create from the design shape
(D, NA, LB, MB, TB, LT of csrc/design.hpp), the class, input_format and enable_fourth_down, and on every call from its
size.  RATE_CASES holds the sources of the reference (main.cpp:685-699 block sizes; RtlSdrSource.cpp:77-93,261 U8 with
Fs/4) with the forms each one reaches; the GPU file runs every row against the fp64 oracle and asserts that exactly
these forms ran (Chain.front_end_forms()).  What this file checks without a GPU:
  * product design == oracle design (info and taps, both classes) for every row -- the GPU comparison rests on it;
  * the rows together reach every FMR_FE_* form (two are covered by named tests elsewhere);
  * the raw-format refusals are refusals of the documented rule, and no case row falls under it (the create refuses
    them before it opens a device: tests/test_chain_shape.py asserts that here, without one);
  * the call schedules hold the edge lengths the GPU rows are meant to exercise;
  * the IF parity check itself trips on one sample shifted by 1e-4 x rms.
"""
import collections
import importlib
import os
import re

import numpy as np
import pytest

import oracle_py as ora
from conftest import ROOT, load_filter

fmr = importlib.import_module("airspy-fmradion_amd")

FAST, R8B = fmr.RESAMPLER_FAST, fmr.RESAMPLER_R8B
CF32, U8 = fmr.IQ_CF32, fmr.IQ_U8

Case = collections.namedtuple("Case", "name source fin fout cls fmt f4 blk mode forms")


def _c(name, source, fin, fout, cls, fmt, f4, blk, mode, forms):
    return Case(name, source, float(fin), float(fout), cls, fmt, bool(f4), int(blk), mode, frozenset(forms.split()))


# name, source, source rate, output rate, class, input format, Fs/4, block length, decoder, forms that run (both stages)
RATE_CASES = [
    _c("airspy_2m5_fm_fast", "Airspy R2", 2.5e6, 384e3, FAST, CF32, 0, 65536, "fm", "decim2_16 poly"),
    _c("airspy_2m5_fm_r8b", "Airspy R2", 2.5e6, 384e3, R8B, CF32, 0, 65536, "fm", "decim2_24 poly"),
    _c("airspy_6m_fm_fast", "Airspy Mini", 6e6, 384e3, FAST, CF32, 0, 65536, "fm", "decim2_16 poly4"),
    _c("airspy_3m_fm_r8b", "Airspy Mini", 3e6, 384e3, R8B, CF32, 0, 65536, "fm", "decim2_24 poly5h poly5h_disc"),
    _c("airspy_10m_fm_r8b_short_long", "Airspy R2", 10e6, 384e3, R8B, CF32, 0, 65536, "fm",
       "decim16 decim2_24 poly5h poly5h_disc"),
    _c("airspy_10m_am_fast", "Airspy R2", 10e6, 48e3, FAST, CF32, 0, 65536, "am", "decim poly4"),
    _c("rtl_2m4_fm_u8_f4", "RTL-SDR", 2.4e6, 384e3, FAST, U8, 1, 16384, "fm", "decim2_16 poly3"),
    _c("rtl_2m4_ppm37_fm_u8_f4", "RTL-SDR -r 37", 2.4e6 * (1 + 37e-6), 384e3, FAST, U8, 1, 16384, "fm", "decim2_16 poly_frac"),
    _c("rtl_2m4_fm_r8b_f4", "RTL-SDR", 2.4e6, 384e3, R8B, CF32, 1, 16384, "fm", "decim2_24 poly3"),
    _c("rtl_2m048_fm_u8_f4", "RTL-SDR", 2.048e6, 384e3, FAST, U8, 1, 16384, "fm", "decim2_16 poly4_am"),
    _c("rtl_3m2_fm_u8_f4", "RTL-SDR", 3.2e6, 384e3, FAST, U8, 1, 16384, "fm", "decim2_16 poly3"),
    _c("rtl_1m152_fm_f4", "RTL-SDR", 1.152e6, 384e3, FAST, CF32, 1, 16384, "fm", "decim poly3"),
    _c("rtl_1m152_am_u8_f4", "RTL-SDR", 1.152e6, 48e3, FAST, U8, 1, 16384, "am", "decim2_16 poly4_am"),
    _c("rtl_1m152_am_r8b_f4", "RTL-SDR", 1.152e6, 48e3, R8B, CF32, 1, 16384, "am", "decim2_24 poly3"),
    _c("rtl_2m4_nbfm_f4", "RTL-SDR", 2.4e6, 48e3, FAST, CF32, 1, 16384, "nbfm", "decim poly3"),
    _c("airspyhf_912k_fm_r8b", "AirspyHF", 912e3, 384e3, R8B, CF32, 0, 2048, "fm", "decim poly3"),
    _c("airspyhf_912k_nbfm", "AirspyHF", 912e3, 48e3, FAST, CF32, 0, 2048, "nbfm", "decim2_16 poly3"),
    _c("airspyhf_456k_fm", "AirspyHF", 456e3, 384e3, FAST, CF32, 0, 2048, "fm", "decim poly3"),
    _c("lds_edge_1m48_am", "(LDS edge of k_ifr_poly2)", 1.48e6, 48e3, FAST, CF32, 0, 16384, "am", "decim2_16 poly2"),
]

# Forms no row here has to reach: the GPU test that covers each against the oracle.
COVERED_ELSEWHERE = {
    "fused": "tests/test_gpu_fused_levels.py::test_fused_front_end_at_amplitude",
    "poly4_am": "tests/test_gpu_parity.py::test_if_resampler_384k_matrix_core_form_against_the_vector_form",
}

# Raw formats are converted inside k_ifr_decim2's FAST form only: U8 needs the FAST class and 2 <= D <= 15.  These source
# configurations are refused at create (tests/test_chain_shape.py asserts it without a device, the GPU file with one); the
# reference converts them on the host.
REFUSED_CASES = [
    _c("rtl_1m152_fm_u8_d1", "RTL-SDR", 1.152e6, 384e3, FAST, U8, 1, 16384, "fm", ""),
    _c("rtl_2m4_nbfm_u8_d19", "RTL-SDR", 2.4e6, 48e3, FAST, U8, 1, 16384, "nbfm", ""),
    _c("rtl_2m4_fm_u8_r8b", "RTL-SDR", 2.4e6, 384e3, R8B, U8, 1, 16384, "fm", ""),
]


MODES = {"fm": fmr.MODE_FM, "am": fmr.MODE_AM, "nbfm": fmr.MODE_NBFM}
STAGE_B_FORMS = {"poly5h", "poly4", "poly4_am", "poly3", "poly2", "poly_frac", "poly"}
STAGE_B_UPGRADES = {"fused", "poly5h_disc"}


def chain_kwargs(case, max_blocks, n_streams=2, **kw):
    """Chain(...) / chain_shape(...) arguments of a row's decoder chain."""
    extra = {}
    if case.mode == "am":
        extra["filter_coeff"] = load_filter("jj1bdx_am_48khz_narrow")
    elif case.mode == "nbfm":
        extra["filter_coeff"] = load_filter("jj1bdx_nbfm_48khz_default")
    extra.update(kw)
    return dict(mode=MODES[case.mode], input_rate=case.fin, enable_resampler=True, fourth_down=case.f4, stereo=True,
                max_block_len=case.blk, max_blocks=max_blocks, n_streams=n_streams, input_format=case.fmt,
                resampler_class=case.cls, **extra)


def assert_forms_permitted(forms, shape):
    """Every kernel form in `forms` (a row's, or what a chain ran) is one the chain's shape (fmr.chain_shape) permits."""
    forms = set(forms)
    assert "decim16" not in forms or shape.decim16, (forms, shape)
    assert "poly5h_disc" not in forms or shape.poly5h_disc, (forms, shape)
    assert "fused" not in forms or shape.fused, (forms, shape)
    assert "decim2_16" not in forms or shape.qa == 16, (forms, shape)
    assert "decim2_24" not in forms or shape.qa == 24, (forms, shape)
    assert "decim" not in forms or shape.qa == 0, (forms, shape)      # (the generic stage A runs only where k_ifr_decim2 cannot)
    assert shape.stage_b in forms or forms & STAGE_B_UPGRADES, (forms, shape)
    assert forms & STAGE_B_FORMS <= {shape.stage_b}, (forms, shape)


def design(case, cls=None):
    """(stage-A taps, stage-B taps, info) of the product's design for the row (or another class)."""
    cls = case.cls if cls is None else cls
    ha, info = fmr.design_taps_class(case.fin, case.fout, cls, 0)
    hb, _ = fmr.design_taps_class(case.fin, case.fout, cls, 1)
    return ha, hb, info


def oracle_resampler(case, cls=None):
    """The oracle's design of the class (ora.Resampler) -- the same specification ora.IfResampler runs in fp64."""
    cls = case.cls if cls is None else cls
    return ora.Resampler(case.fin, case.fout, 180.0, 0.98, True) if cls == R8B else ora.Resampler(case.fin, case.fout, 140.0)


def oracle_if_resampler(case):
    return ora.IfResampler(case.fin, case.fout, 180.0, 0.98, True) if case.cls == R8B else ora.IfResampler(case.fin, case.fout)


def raw_format_refused(case, info):
    return case.fmt != CF32 and (case.cls != FAST or not 2 <= info["D"] <= 15)


# ------------------------------------------------------------------ call schedules
def call_schedule(case, D):
    """Calls (lists of block lengths) of one row: ragged calls of several blocks -- 1, < D, not a multiple of 4, a
    k_ifr_decim2 tile (256 mid samples) +- 1, a zero-length block -- and long calls of full blocks (the fused and
    matrix-core stage-A forms and the discriminator epilogue need those).  The 10 MS/s R8B row alternates short calls
    (< 2000 mid samples: k_ifr_decim2<.., 24>) and long ones (k_ifr_decim16)."""
    blk, t = case.blk, 256 * D
    if "decim16" in case.forms:
        short, long_ = [1, D - 1, 4097, 0, t + 1, t - 1], [blk] * 4
        return [short, long_] * 3
    sched = [[blk, 1, D - 1 if D > 1 else 2, blk - 3, 0, min(t + 1, blk)],
             [min(t - 1, blk), blk, blk],
             [5, blk // 2 + 7],
             [blk] * 4]
    n_if = sum(map(sum, sched)) * case.fout / case.fin
    reps = int(min(8, max(1, np.ceil(20000 / n_if))))
    return sched * reps


# ------------------------------------------------------------------ IF parity bounds
# FAST forms and the fp16 three-product stage B of the R8B class: the existing front-end bar (tests/test_gpu_parity.py).
REL_RMS_FAST = 2e-6
# R8B stage B in the vector forms accumulates TB taps per output in one fp32 fmaf chain.  A rounding of the running sum
# per tap, of size ~2^-24 |s_k|, over the ~TB/2 taps at which the partial sum has reached the output's size: rel RMS
# ~ 2^-24 sqrt(TB/2) / sqrt(3) ~ 0.4 * 2^-24 sqrt(TB) (a float32 model of the chain with the R8B taps gives 0.28-0.31).
# Bound: K_R8B * 2^-24 * sqrt(TB) with K_R8B = 1 (3.2e-6 at TB = 2848, 3.7e-6 at 3902) -- stage A's fp32 mid samples
# and the fp32 taps add to the accumulation's share.  Measured on the MI355X (parity report): rel RMS 0.9e-6 ... 1.1e-6
# (0.27 ... 0.30 x 2^-24 sqrt(TB), as the model says), max |err| 4.1e-6 ... 7.2e-6 x rms -- against 3.2e-6 ... 3.7e-6 and
# 30 x that.  FAST rows: rel RMS 1.8e-7 ... 6.9e-7 (D = 80: 1197 stage-A taps), max |err| 1.1e-6 ... 3.3e-6 x rms.
K_R8B = 1.0
# max |err| over every sample of a row <= MAX_OVER_RMS x the RMS bound x rms(ref): one wrong sample at a tile seam, a
# phase-table edge or an Fs/4 index would stand out by orders of magnitude; Gaussian accumulation noise does not reach it.
MAX_OVER_RMS = 30.0
VECTOR_FORMS_B = {"poly3", "poly2", "poly", "poly_frac"}


def rel_rms_bound(case, info):
    if case.cls == R8B and case.forms & VECTOR_FORMS_B:
        return K_R8B * 2.0 ** -24 * np.sqrt(info["TB"])
    return REL_RMS_FAST


def tile_b(case, info):
    """Output samples per tile of the row's stage-B form (for the failure message)."""
    f = case.forms
    if f & {"poly4", "poly4_am", "poly5h", "poly5h_disc"}:
        return 3072
    if f & {"poly3", "poly2"}:
        return 64 * info["LB"]
    return 256


def check_if_parity(got, ref, bound, tile, call_starts=()):
    """got / ref: the IF samples of one stream, all calls; bound: relative RMS bound.  Returns (rel RMS, max |err| / rms).
    The worst sample is reported with its call and its position in the call modulo the stage-B tile."""
    got, ref = np.asarray(got, dtype=np.complex128), np.asarray(ref, dtype=np.complex128)
    assert len(got) == len(ref), (len(got), len(ref))
    r = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    err = np.abs(got - ref)
    rel = float(np.sqrt(np.mean(err ** 2))) / r
    i = int(np.argmax(err))
    worst = float(err[i]) / r
    c = int(np.searchsorted(np.asarray(call_starts, dtype=np.int64), i, side="right")) - 1 if len(call_starts) else 0
    p = i - (int(call_starts[c]) if len(call_starts) else 0)
    where = f"worst sample {i} (call {c}, position {p} in the call, {p} mod tile {tile} = {p % tile})"
    assert rel <= bound, f"rel RMS {rel:.3e} > {bound:.3e}; {where}, |err| = {worst:.3e} x rms"
    assert worst <= MAX_OVER_RMS * bound, f"max |err| {worst:.3e} x rms > {MAX_OVER_RMS * bound:.3e}; {where}"
    return rel, worst


# ------------------------------------------------------------------ tests
def _header_forms():
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    return {m.group(1).lower(): 1 << int(m.group(2)) for m in re.finditer(r"FMR_FE_(\w+)\s*=\s*1\s*<<\s*(\d+)", hdr)}


def test_front_end_form_bits_mirror_the_header():
    assert _header_forms() == fmr.FE_FORMS
    assert len(set(fmr.FE_FORMS.values())) == len(fmr.FE_FORMS)


@pytest.mark.parametrize("case", RATE_CASES + REFUSED_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("cls", [FAST, R8B], ids=["fast", "r8b"])
def test_product_design_equals_the_oracle_design(case, cls):
    ha, hb, info = design(case, cls)
    rs = oracle_resampler(case, cls)
    oi = rs.info()
    assert info == {k: oi[k] for k in ("D", "NA", "LB", "MB", "TB", "LT")}
    assert np.array_equal(ha, rs.taps_a()) and np.array_equal(hb, rs.taps_b())


def test_the_rows_reach_every_form():
    reached = set().union(*(c.forms for c in RATE_CASES))
    assert reached <= set(fmr.FE_FORMS), reached - set(fmr.FE_FORMS)
    missing = set(fmr.FE_FORMS) - reached - set(COVERED_ELSEWHERE)
    assert not missing, f"no row reaches {sorted(missing)}"
    assert set(COVERED_ELSEWHERE) <= set(fmr.FE_FORMS)
    for tid in COVERED_ELSEWHERE.values():
        path, name = tid.split("::")
        assert re.search(rf"^def {name}\(", open(os.path.join(ROOT, path)).read(), re.M), tid
    names = [c.name for c in RATE_CASES + REFUSED_CASES]
    assert len(names) == len(set(names))


def test_the_rows_reach_the_shapes_they_are_named_for():
    """Stage-A and stage-B forms follow from the design shape; pin the shapes behind the rows (csrc/fmradion_amd.hip
    create): a design change that moves a row to another form must show up here first."""
    shape = {c.name: design(c)[2] for c in RATE_CASES}
    assert shape["airspy_2m5_fm_fast"] == dict(D=2, NA=21, LB=192, MB=625, TB=262, LT=0)
    assert shape["airspy_2m5_fm_r8b"]["TB"] == 3902
    assert shape["airspy_10m_am_fast"] == dict(D=80, NA=1197, LB=48, MB=125, TB=210, LT=0)
    assert (shape["rtl_1m152_fm_f4"]["D"], shape["rtl_1m152_fm_f4"]["LB"], shape["rtl_1m152_fm_f4"]["MB"]) == (1, 1, 3)
    assert (shape["rtl_2m048_fm_u8_f4"]["LB"], shape["rtl_2m048_fm_u8_f4"]["MB"], shape["rtl_2m048_fm_u8_f4"]["TB"]) == (3, 8, 214)
    assert (shape["rtl_2m4_fm_u8_f4"]["LB"], shape["rtl_2m4_fm_u8_f4"]["MB"]) == (8, 25)
    assert shape["rtl_2m4_ppm37_fm_u8_f4"]["LT"] > 0
    assert (shape["lds_edge_1m48_am"]["LB"], shape["lds_edge_1m48_am"]["MB"]) == (66, 185)
    assert shape["rtl_3m2_fm_u8_f4"]["D"] == 3 and shape["rtl_1m152_am_u8_f4"]["D"] == 9 and shape["airspyhf_912k_nbfm"]["D"] == 7
    for c in RATE_CASES:
        if c.forms & {"poly3"}:
            assert shape[c.name]["LB"] > 1 or c.name == "rtl_1m152_fm_f4", c.name
        if "decim" in c.forms:
            assert shape[c.name]["D"] == 1 or shape[c.name]["D"] > 15, c.name


def test_raw_format_refusals_are_listed_not_run():
    for c in REFUSED_CASES:
        assert raw_format_refused(c, design(c)[2]), c.name
    for c in RATE_CASES:
        assert not raw_format_refused(c, design(c)[2]), c.name


@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: c.name)
def test_call_schedules_hold_the_edge_lengths(case):
    D = design(case)[2]["D"]
    calls = call_schedule(case, D)
    lens = [n for c in calls for n in c]
    assert max(lens) <= case.blk and max(len(c) for c in calls) <= 6
    assert 0 in lens and 1 in lens and any(n % 4 for n in lens)
    assert D == 1 or D - 1 in lens
    t = 256 * D
    if t + 1 <= case.blk:
        assert t - 1 in lens and t + 1 in lens
    assert any(len(c) >= 3 and min(c) == case.blk for c in calls)
    if "decim16" in case.forms:
        mids = [sum(c) / D for c in calls]
        assert any(m < 2000 for m in mids) and any(m > 4 * 2000 for m in mids)


def test_the_parity_check_trips_on_one_shifted_sample():
    rng = np.random.default_rng(7)
    ref = (rng.standard_normal(30000) + 1j * rng.standard_normal(30000)).astype(np.complex128)
    got = ref + 1e-7 * (rng.standard_normal(30000) + 1j * rng.standard_normal(30000))
    r = np.sqrt(np.mean(np.abs(ref) ** 2))
    rel, worst = check_if_parity(got, ref, REL_RMS_FAST, 3072, [0, 10000])
    assert rel < REL_RMS_FAST and worst < MAX_OVER_RMS * REL_RMS_FAST
    bad = got.copy()
    bad[12345] += 1e-4 * r
    with pytest.raises(AssertionError, match=r"max \|err\|.*worst sample 12345 \(call 1, position 2345 in the call, 2345 mod tile 3072"):
        check_if_parity(bad, ref, REL_RMS_FAST, 3072, [0, 10000])

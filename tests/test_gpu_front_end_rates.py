"""The IF resampler at the source rates of the reference's SDR sources, against the fp64 oracle (GPU).

Every row of RATE_CASES (tests/test_front_end_rate_table.py) runs on a decoder chain of its mode with two streams of
different content -- seeded complex white noise plus an FM station, so that every tap and every phase matters; for U8
rows quantised, and converted on the oracle side with ora.iq_convert, then FourthConverterIQ where Fs/4 is on -- in
ragged calls of several blocks.  The IF samples of every call (fmr_debug_read 0, FMR_DEBUG_TAPS=1 where the
discriminator epilogue keeps them on chip) are held against ora.IfResampler of the row's class:
  * the same output counts, call by call (and block by block where the decoder's audio counts are the IF counts);
  * exactly the row's kernel forms ran (Chain.front_end_forms()), and the chain's shape (fmr.chain_shape) permits them;
  * relative RMS error <= 2e-6 (FAST forms), or K_R8B * 2^-24 * sqrt(TB) where the R8B class accumulates its thousands
    of stage-B taps in one fp32 chain; and max |err| <= 30 x that bound x rms(ref): one wrong sample at a tile seam,
    a phase-table edge or an Fs/4 index carried across an odd block fails the row.
End to end: the audio of six source configurations against the oracle's decoders at the 1e-5 RMS north star.
"""
import importlib

import numpy as np
import pytest

import oracle_py as ora
import siggen
from conftest import load_filter
from test_front_end_rate_table import (MAX_OVER_RMS, MODES, RATE_CASES, REFUSED_CASES, REL_RMS_FAST, U8, CF32, R8B, FAST,
                                       assert_forms_permitted, call_schedule, chain_kwargs, check_if_parity, design,
                                       oracle_if_resampler, rel_rms_bound, tile_b)
from test_gpu_parity import _report

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")
S = 2


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def broadband_iq(n, fin, stream, f4):
    """An FM station plus complex white noise over the whole band (seeded per stream); at +fs/4 for Fs/4 rows."""
    x = siggen.fm_stereo_iq(n, fin, stream_id=stream, amplitude=0.3, sigma=0.0).astype(np.complex128)
    rng = np.random.default_rng(1000 + stream)
    x = x + 0.08 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if f4:
        x = x * (1j ** (np.arange(n) % 4))
    return x.astype(np.complex64)


def u8_quantise(x):
    """RTL-SDR offset binary: (n, 2) uint8 I, Q."""
    q = lambda v: np.clip(np.round(v * 127.0 + 127.5), 0, 255)
    return np.stack([q(x.real), q(x.imag)], axis=1).astype(np.uint8)


def source(case, n):
    """(what the chain is fed: (S, n) complex64 or (S, n, 2) uint8, what the oracle's resampler is fed: S complex64)."""
    xs = [broadband_iq(n, case.fin, s, case.f4) for s in range(S)]
    if case.fmt == CF32:
        return np.stack(xs), xs
    raw = [u8_quantise(x) for x in xs]
    return np.stack(raw), [ora.iq_convert(case.fmt, r) for r in raw]


def make_chain(case, max_blocks, **kw):
    return fmr.Chain(**chain_kwargs(case, max_blocks, n_streams=S, **kw))


# ------------------------------------------------------------------ IF samples, every row
@pytest.mark.parametrize("case", RATE_CASES, ids=lambda c: c.name)
def test_if_samples_against_the_fp64_oracle(case, monkeypatch):
    if case.forms & {"fused", "poly5h_disc"}:
        monkeypatch.setenv("FMR_DEBUG_TAPS", "1")      # the IF samples stay on chip behind the discriminator epilogue
    _, _, info = design(case)
    calls = call_schedule(case, info["D"])
    n = sum(map(sum, calls))
    feed, xf = source(case, n)
    ch = make_chain(case, max(len(c) for c in calls))
    want = {k: info[k] for k in ("D", "NA", "LB", "MB", "TB", "LT")}
    if want["D"] == 1:
        want["NA"] = 1                              # stage A is a copy: one unit tap
    assert ch.resampler_info() == want
    rs = [oracle_if_resampler(case) for _ in range(S)]
    f4 = [ora.FourthConverterIQ(False) if case.f4 else None for _ in range(S)]
    got, ref = [[] for _ in range(S)], [[] for _ in range(S)]
    call_starts, n_if, pos = [], 0, 0
    for ll in calls:
        m = sum(ll)
        _, alen = ch.process_blocks(feed[:, pos:pos + m], ll)
        per_block = []
        for s in range(S):
            o, rb = pos, []
            for bl in ll:
                b = xf[s][o:o + bl]
                if f4[s] is not None:
                    b = f4[s].process(b)
                rb.append(rs[s].process(b))
                o += bl
            per_block.append([len(q) for q in rb])
            ref[s].append(np.concatenate(rb))
            got[s].append(ch.debug_read(0, stream=s))
            assert len(got[s][-1]) == len(ref[s][-1]), (case.name, s, ll, len(got[s][-1]), len(ref[s][-1]))
        assert per_block[0] == per_block[1]
        if case.mode != "fm":           # AmDecoder / NbfmDecoder: one audio sample per IF sample
            assert list(alen) == per_block[0], (case.name, ll)
        call_starts.append(n_if)
        n_if += len(ref[0][-1])
        pos += m
    forms = ch.front_end_forms()
    bound = rel_rms_bound(case, info)
    tile = tile_b(case, info)
    rels, worsts = [], []
    for s in range(S):
        g, q = np.concatenate(got[s]), np.concatenate(ref[s])
        assert len(q) > 2000
        try:
            rel, worst = check_if_parity(g, q, bound, tile, call_starts)
        except AssertionError as e:
            _report(f"front_end_rate_{case.name}", stream=s, failed=str(e), forms=sorted(forms), info=info)
            raise AssertionError(f"{case.name} stream {s}: {e}") from None
        rels.append(rel); worsts.append(worst)
    _report(f"front_end_rate_{case.name}", n_if=n_if, rel_rms=max(rels), max_err_over_rms=max(worsts),
            bound_rel_rms=bound, bound_max_err_over_rms=MAX_OVER_RMS * bound, forms=sorted(forms), expected_forms=sorted(case.forms),
            info=info, cls="r8b" if case.cls == R8B else "fast", fmt=case.fmt, fourth=case.f4, calls=len(calls))
    assert forms == set(case.forms), (case.name, sorted(forms), sorted(case.forms))
    assert_forms_permitted(forms, fmr.chain_shape(**chain_kwargs(case, max(len(c) for c in calls), n_streams=S)))
    # sensitivity on the measured arrays: one product sample off by 1e-4 x rms fails the max-error bound
    if bound == REL_RMS_FAST:
        g, q = np.concatenate(got[0]), np.concatenate(ref[0])
        g = g.astype(np.complex128)
        g[len(g) // 2 + 17] += 1e-4 * rms(q)
        with pytest.raises(AssertionError, match="max"):
            check_if_parity(g, q, bound, tile, call_starts)
    ch.close()


@pytest.mark.parametrize("case", REFUSED_CASES, ids=lambda c: c.name)
def test_raw_format_refusals(case):
    with pytest.raises(fmr.FmrError, match="input_format"):
        make_chain(case, 4)


# ------------------------------------------------------------------ end to end
def _ragged(blk, n_calls, rng, per_call=4):
    calls = []
    for _ in range(n_calls):
        ll = [blk] * per_call
        if rng.random() < 0.5:
            ll[int(rng.integers(per_call))] = int(rng.integers(1, blk))
        calls.append(ll)
    return calls


E2E = [
    # name, source rate, decoder, class, format, Fs/4, block length, calls of 4 blocks
    ("rtl_2m4_fm_stereo_u8_f4", 2.4e6, "fm", FAST, U8, True, 16384, 20),
    ("rtl_2m4_ppm37_fm_stereo_u8_f4", 2.4e6 * (1 + 37e-6), "fm", FAST, U8, True, 16384, 20),
    ("airspy_2m5_fm_stereo_r8b", 2.5e6, "fm", R8B, CF32, False, 65536, 5),
    ("rtl_1m152_am_u8_f4", 1.152e6, "am", FAST, U8, True, 16384, 12),
    ("airspyhf_912k_nbfm", 912e3, "nbfm", FAST, CF32, False, 2048, 60),
    ("airspy_10m_am_d80", 10e6, "am", FAST, CF32, False, 65536, 6),
]


@pytest.mark.parametrize("name,fin,mode,cls,fmt,f4,blk,n_calls", E2E, ids=[e[0] for e in E2E])
def test_end_to_end_audio_against_the_oracle(name, fin, mode, cls, fmt, f4, blk, n_calls, pilotcut):
    rng = np.random.default_rng(sum(map(ord, name)))
    calls = _ragged(blk, n_calls, rng)
    n = sum(map(sum, calls))
    xs = []
    for s in range(S):
        if mode == "fm":
            x = siggen.fm_stereo_iq(n, fin, stream_id=s)
        elif mode == "am":
            x = siggen.am_iq(n, fin, offset=37.0 + 11.0 * s, seed=3 + s) * 5.0
        else:
            x = siggen.nbfm_iq(n, fin, offset=120.0 + 15.0 * s, seed=5 + s)
        if f4:
            x = x * (1j ** (np.arange(n) % 4))
        xs.append(x.astype(np.complex64))
    if fmt == U8:
        raw = [u8_quantise(x) for x in xs]
        feed, xf = np.stack(raw), [ora.iq_convert(fmt, r) for r in raw]
    else:
        feed, xf = np.stack(xs), xs
    nbfm_default, nbfm_audio = load_filter("jj1bdx_nbfm_48khz_default"), load_filter("jj1bdx_48khz_nbfmaudio")
    am_narrow = load_filter("jj1bdx_am_48khz_narrow")
    kw = {"fm": {}, "am": {"filter_coeff": am_narrow}, "nbfm": {"filter_coeff": nbfm_default}}[mode]
    ch = fmr.Chain(mode=MODES[mode], input_rate=fin, enable_resampler=True, fourth_down=f4, stereo=True,
                   max_block_len=blk, max_blocks=4, n_streams=S, input_format=fmt, resampler_class=cls, **kw)
    decs = []
    for _ in range(S):
        r = ora.IfResampler(fin, 384e3 if mode == "fm" else 48e3, *((180.0, 0.98, True) if cls == R8B else ()))
        d = {"fm": lambda: ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut),
             "am": lambda: ora.AmDecoder(am_narrow),
             "nbfm": lambda: ora.NbfmDecoder(nbfm_default, 8000.0, nbfm_audio)}[mode]()
        decs.append((ora.FourthConverterIQ(False) if f4 else None, r, d))
    got, ref = [[] for _ in range(S)], [[] for _ in range(S)]
    pos = 0
    for ll in calls:
        m = sum(ll)
        a, alen = ch.process_blocks(feed[:, pos:pos + m], ll)
        for s in range(S):
            f4o, r, d = decs[s]
            o, lens = pos, []
            for bl in ll:
                b = xf[s][o:o + bl]
                if f4o is not None:
                    b = f4o.process(b)
                q = d.process(r.process(b))
                ref[s].append(q); lens.append(len(q))
                o += bl
            assert list(alen) == lens, (name, s, ll)
            got[s].append(a[s])
        pos += m
    errs, levels = [], []
    for s in range(S):
        g, q = np.concatenate(got[s]), np.concatenate(ref[s])
        assert len(g) == len(q) > 4000
        errs.append(rms(g - q)); levels.append(rms(q))
    st = ch.status(0)
    _report(f"front_end_rate_e2e_{name}", audio_rms_err=max(errs), audio_rms=min(levels), forms=sorted(ch.front_end_forms()),
            stereo_detected=st.stereo_detected if mode == "fm" else None)
    assert max(errs) < 1e-5, (name, errs)
    assert min(levels) > 1e-3, (name, levels)
    ch.close()

"""Error behaviour of the C-ABI on the device path (include/fmradion_amd.h): a refused call must leave the decoder state
untouched (the reference's process() cannot fail half way; a caller that sized its buffer wrongly must be able to
retry), empty blocks are legal (FmDecode.cpp:89-92), shapes the kernels cannot take are refused at create."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle_py as ora
import siggen

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def _raw_process(ch, iq, audio_cap):
    out = np.empty(max(audio_cap, 1), dtype=np.float64)
    n = C.c_size_t()
    rc = fmr.lib().fmr_process(ch.h, iq.ctypes.data_as(C.POINTER(C.c_float)), len(iq),
                               out.ctypes.data_as(C.POINTER(C.c_double)), audio_cap, C.byref(n))
    return rc, out[:n.value].copy()


def test_refused_calls_leave_the_state_untouched(pilotcut):
    fs, blk = 384e3, 2517
    x = siggen.fm_stereo_iq(40 * blk, fs)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs, stereo=True, max_block_len=blk, max_blocks=4)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
    got, ref = [], []
    for i, b in enumerate(siggen.blocks(x, blk)):
        if i == 7:                                         # audio buffer too small: refused, nothing consumed
            rc, a = _raw_process(ch, b, 8)
            assert rc == fmr.ERR_CAPACITY and len(a) == 0
        if i == 9:                                         # more blocks than the chain was built for
            with pytest.raises(fmr.FmrError):
                ch.process_blocks(np.tile(b, 5)[None, :], [blk] * 5)
        if i == 11:                                        # a block longer than max_block_len
            with pytest.raises(fmr.FmrError):
                ch.process_blocks(np.tile(b, 2)[None, :], [2 * blk])
        if i == 13:                                        # n_blocks = 0
            with pytest.raises(fmr.FmrError):
                ch.process_blocks(b[None, :], [])
        got.append(ch.process(b))
        ref.append(fm.process(b))
    assert [len(g) for g in got] == [len(r) for r in ref]
    assert rms(np.concatenate(got) - np.concatenate(ref)) < 1e-6
    ch.close()


def test_empty_blocks_inside_a_call(pilotcut):
    """Zero-length blocks between real ones (a source that delivered nothing): FmDecode.cpp:89-92 returns at once."""
    fs, blk = 10e6, 65536
    x = siggen.fm_stereo_iq(24 * blk, fs)
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=fs, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=16)
    r = ora.IfResampler(fs, 384e3)
    fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
    got, ref = [], []
    for c in range(2):
        seg = x[c * 12 * blk:(c + 1) * 12 * blk]
        lens = [blk, 0, blk, blk, 0, 0] + [blk] * 9 + [0]
        a, alen = ch.process_blocks(seg[None, :], lens)
        got.append(a[0])
        o, rl = 0, []
        for n in lens:
            q = fm.process(r.process(seg[o:o + n]))
            rl.append(len(q)); ref.append(q); o += n
        assert list(alen) == rl
    assert rms(np.concatenate(got) - np.concatenate(ref)) < 1e-5
    ch.close()


def test_unsupported_shapes_are_refused_at_create():
    # raw integer input needs the v2 front-end kernel, i.e. an integer pre-decimation >= 2: refused when the
    # chain is built, not on every call
    with pytest.raises(fmr.FmrError):
        fmr.Chain(mode=fmr.MODE_FM, input_rate=1.0e6, enable_resampler=True, input_format=fmr.IQ_U8, max_block_len=2048)
    with pytest.raises(fmr.FmrError):                     # raw input without the resampler in front
        fmr.Chain(mode=fmr.MODE_FM, input_rate=384e3, enable_resampler=False, input_format=fmr.IQ_S16, max_block_len=2048)
    with pytest.raises(fmr.FmrError):                     # a ratio outside the design range
        fmr.Chain(mode=fmr.MODE_NONE, input_rate=5e9, enable_resampler=True, max_block_len=2048)


# The record stages' refusals that need a chain, as the library words them: stage -> (enable, read, the stage's noun, what it
# counts from, the smallest chain that accepts it).
_FM = dict(mode=fmr.MODE_FM, input_rate=384e3, max_block_len=4096)
_FE = dict(mode=fmr.MODE_NONE, input_rate=2.5e6, enable_resampler=True, max_block_len=4096)
STAGES = {
    "monitor": ("enable_monitor", "monitor_records", "monitor", "MPX sample", _FM),
    "rf_monitor": ("enable_rf_monitor", "rf_monitor_records", "RF monitor", "IF sample", _FM),
    "loudness": ("enable_loudness", "loudness_records", "audio monitor", "audio sample", _FM),
    "analyser": ("enable_analyser", "analyser_records", "analyser", "audio sample", _FM),
    "weak_signal": ("enable_weak_signal", "weak_signal_records", "weak-signal stage", "MPX sample", _FM),
    "blanker": ("enable_blanker", "blanker_records", "blanker", "input sample", _FE),
    "iq_correction": ("enable_iq_correction", "iq_correction_records", "IQ corrector", "input sample", _FE),
}
CAPTURE = {"blanker": ("the blanker", 6, "tap 6 (blanked input rows) needs a chain with fmr_enable_blanker in FMR_NB_ACT, and an input row"),
           "iq_correction": ("the IQ corrector", 7, "tap 7 (corrected input rows) needs a chain with fmr_enable_iq_correction in "
                                                    "FMR_IQC_ACT, and an input row")}


def _refused(call, rc, msg):
    with pytest.raises(fmr.FmrError) as e:
        call()
    assert str(e.value) == f"fmradion_amd error {rc}: {msg}"


@pytest.mark.parametrize("stage", list(STAGES))
def test_record_stage_refusals_word_for_word(stage):
    """Every refusal of a record stage that needs a chain, text and code in full: the read before the enable, the second
    enable, the enable after a call of one block of 4096 samples; for the two stages on the capture also a row the chain
    does not have, the three chains they do not fit and their debug tap on a chain without them."""
    enable, read, noun, first, kw = STAGES[stage]
    fn, rd = f"fmr_{enable}", f"fmr_{stage}_read"
    block = np.full((1, 4096), 0.1, dtype=np.complex64)
    ch = fmr.Chain(**kw)
    _refused(getattr(ch, read), -2, f"{rd}: the chain has no {noun} ({fn})")
    if stage in CAPTURE:
        _refused(lambda: ch.debug_read(CAPTURE[stage][1]), -2, "fmr_debug_read: " + CAPTURE[stage][2])
    getattr(ch, enable)()
    _refused(getattr(ch, enable), -2, f"{fn}: the {noun} of this chain is already enabled")
    if stage in CAPTURE:
        _refused(lambda: getattr(ch, read)(5), -2, f"{rd}: row 5 is not one of the chain's 1 input rows")
    ch.close()
    ch = fmr.Chain(**kw)
    (ch.resample_blocks if kw is _FE else ch.process_blocks)(block, [4096])
    _refused(getattr(ch, enable), -2, f"{fn}: the chain has already taken samples (the {noun} counts from the chain's first {first})")
    ch.close()
    if stage not in CAPTURE:
        return
    the = CAPTURE[stage][0]
    for make, msg in (
            (lambda: fmr.MpxChain(), f"{the} works on an IQ capture; an MPX decoder (fmr_create_mpx_decoder) is fed composite PCM"),
            (lambda: fmr.Chain(mode=fmr.MODE_FM, input_rate=2.5e6, enable_resampler=True, max_block_len=16384, input_format=fmr.IQ_S16),
             f"{the} reads complex float samples (FMR_IQ_CF32); this chain takes a raw input format"),
            (lambda: fmr.Chain(**_FM), f"{the} sits in front of the IF resampler; this chain has none (enable_resampler = 0)")):
        ch = make()
        _refused(getattr(ch, enable), -3, f"{fn}: {msg}")
        ch.close()

"""Nothing is left behind: every path that makes device buffers, pinned blocks, events or streams gives all of them back.
fmr_debug_live_resources() counts what the library's owners hold in the process; each case reads it before, while its
objects are open (> before: the counter counts) and after everything is closed (== before; 0 in a fresh process).  Also:
a create that is refused and an enable that is refused leave the count -- and the chain -- as they were.
No case forces an allocation to fail (that takes a request of hundreds of gigabytes on a shared card): that a partly built
chain gives everything back rests on the owners (each member frees what it holds when the chain dies), and that a failed
enable leaves nothing behind on how enables are built (a local stage, moved into the chain on success)."""
import gc
import importlib

import numpy as np
import pytest

import siggen

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

BLK, NB = 65536, 4          # the smallest FM shape with the fused front end and ring slots 1 .. 3


def live():
    gc.collect()
    return fmr.debug_live_resources()


@pytest.fixture(scope="module")
def x_fm():
    x = siggen.fm_stereo_iq(2 * NB * BLK, 10e6)[None, :]
    x.setflags(write=False)
    return x


def full_chain(**kw):
    """Shape 1: FM at 10 MS/s, pipelined, made through the RDS create, every optional stage enabled."""
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=NB,
                   enable_rds=True, **kw)
    ch.enable_monitor(interval_samples=2048, max_records=8)
    ch.enable_rf_monitor(interval_samples=2048, max_records=8)
    ch.enable_loudness(step_samples=480, max_records=8)
    ch.enable_output(format="s16")
    ch.set_output_rate(44100, mono=True)
    return ch


def call(ch, x, k):
    return ch.process_blocks(x[:, k * NB * BLK:(k + 1) * NB * BLK], [BLK] * NB)


def read_every_reader(ch):
    assert len(ch.monitor_records(cap=1)[0]) == 1
    assert len(ch.rf_monitor_records(cap=1)[0]) == 1
    assert len(ch.loudness_records(cap=1)[0]) == 1
    ch.rds_groups()
    pcm, blocks, _ = ch.output_read(cap_blocks=1)
    assert len(pcm) > 0 and pcm.shape[1] == 1 and len(blocks) == 1


def test_fm_pipelined_with_every_stage(x_fm):
    before = live()
    ch = full_chain()
    assert live() > before
    for k in range(2):
        audio, _ = call(ch, x_fm, k)
        assert audio.shape[1] > 0
    read_every_reader(ch)
    ch.close()
    assert live() == before


def test_fm_in_order_with_if_filter(x_fm, fm_medium):
    """The streams of the chain that is not pipelined: side2 is a stream of its own."""
    before = live()
    ch = full_chain(in_order=True, fmfilter_enable=True, filter_coeff=fm_medium)
    assert live() > before
    call(ch, x_fm, 0)
    read_every_reader(ch)
    ch.close()
    assert live() == before


def test_am_48k_with_f32_output(am_narrow):
    before = live()
    ch = fmr.Chain(mode=fmr.MODE_AM, input_rate=48e3, filter_coeff=am_narrow, max_block_len=4096, max_blocks=4)
    ch.enable_output(format="f32")
    assert live() > before
    ch.process_blocks(siggen.am_iq(4 * 4096, 48e3)[None, :], [4096] * 4)
    pcm, blocks, _ = ch.output_read()
    assert pcm.dtype == np.float32 and len(pcm) > 0 and len(blocks) == 4
    ch.close()
    assert live() == before


def test_channelizer(x_fm):
    before = live()
    cz = fmr.Channelizer(10e6, [-1_000_000, 2_000_000], max_block_len=BLK, max_blocks=2)
    assert live() > before
    out, olen = cz.resample_blocks(x_fm[0, :2 * BLK], [BLK, BLK])
    assert out.shape[0] == 2 and int(olen.sum()) > 0
    cz.close()
    assert live() == before


def test_spectrum_with_waterfall(x_fm):
    before = live()
    sp = fmr.Spectrum(10e6, fft_size=256, n_rows=2, max_call_len=4096, waterfall_segments=4, waterfall_lines=4)
    assert live() > before
    sp.process(np.stack([x_fm[0, :4096], x_fm[0, 4096:8192]]))
    assert sp.psd(1).shape == (256,)
    assert len(sp.waterfall(row=1)[0]) > 0
    sp.close()
    assert live() == before


@pytest.mark.parametrize("kw, words", [
    (dict(input_format=fmr.IQ_S16, resampler_class=fmr.RESAMPLER_R8B), "needs the FAST resampler class"),
    (dict(mode=fmr.MODE_NONE, input_rate=5e9), "outside the supported design range"),
], ids=["s16_r8b", "ratio"])
def test_create_that_is_refused_before_the_device_is_opened(kw, words):
    """Both configurations used to be refused with the device open and streams made; the create now decides its shape
    first (plan_create) and refuses them before it opens the device (tests/test_chain_shape.py: the same refusals on a
    machine without one).  Either way nothing may be left behind."""
    before = live()
    cfg = dict(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, max_block_len=BLK, max_blocks=NB)
    cfg.update(kw)
    with pytest.raises(fmr.FmrError, match=words) as e:
        fmr.Chain(**cfg)
    assert f"({fmr.ERR_UNSUPPORTED})" in str(e.value)
    assert live() == before


def test_multipath_stages_are_bounded_by_the_equaliser_kernel():
    """MultipathFilter(stages) holds 4 stages + 1 taps and the widest equaliser kernel 1280: 320 stages are refused before
    anything is allocated, 319 (1277 taps) make a chain whose equaliser runs: its 100 warm-up blocks end inside the call, and
    the six blocks behind them push 3072 samples into its window, past the reference tap (3 stages + 1 = 958 samples back),
    from where on the constant-modulus error is not zero and the taps move."""
    before = live()
    cfg = dict(mode=fmr.MODE_FM, input_rate=384e3, stereo=True, max_block_len=512, max_blocks=106)
    with pytest.raises(fmr.FmrError, match="multipath_stages 320 is above 319") as e:
        fmr.Chain(multipath_stages=320, **cfg)
    assert f"({fmr.ERR_UNSUPPORTED})" in str(e.value)
    assert live() == before
    ch = fmr.Chain(multipath_stages=319, **cfg)
    audio, alen = ch.process_blocks(siggen.fm_stereo_iq(106 * 512, 384e3)[None, :], [512] * 106)
    assert int(alen.sum()) == audio.shape[1] > 0 and np.isfinite(audio).all()
    coeff = ch.multipath_coefficients()
    assert len(coeff) == 4 * 319 + 1 and np.isfinite(coeff).all()
    assert np.abs(coeff - (np.arange(len(coeff)) == 3 * 319 + 1)).max() > 0
    ch.close()
    assert live() == before


def test_refused_enables_leave_the_chain_as_it_was(x_fm):
    before = live()

    def make():
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, max_block_len=BLK,
                       max_blocks=NB)
        ch.enable_output(format="s16")
        return ch

    ch, twin = make(), make()
    held = live()
    with pytest.raises(fmr.FmrError, match="already enabled") as e:
        ch.enable_output(format="f32")
    assert f"error {fmr.ERR_BAD_ARG}:" in str(e.value) and live() == held
    for c in (ch, twin):
        c.set_output_rate(44100)
    held = live()
    assert held > before
    with pytest.raises(fmr.FmrError, match="already set") as e:
        ch.set_output_rate(32000, mono=True)
    assert f"error {fmr.ERR_BAD_ARG}:" in str(e.value) and live() == held
    first = [call(c, x_fm, 0)[0] for c in (ch, twin)]
    with pytest.raises(fmr.FmrError, match="already taken samples") as e:
        ch.enable_loudness()
    assert f"error {fmr.ERR_BAD_ARG}:" in str(e.value) and live() == held
    second = [call(c, x_fm, 1)[0] for c in (ch, twin)]
    assert first[0].shape[1] > 0 and second[0].shape[1] > 0
    assert np.array_equal(first[0], first[1]) and np.array_equal(second[0], second[1])
    pcm = [c.output_read()[0] for c in (ch, twin)]
    assert pcm[0].shape == pcm[1].shape and pcm[0].shape[1] == 2 and np.array_equal(pcm[0], pcm[1])
    assert ch.output_rate_info()["rate"] == 44100
    ch.close()
    twin.close()
    assert live() == before


def test_twelve_create_call_close_cycles(x_fm):
    before = live()
    for _ in range(12):
        ch = full_chain()
        call(ch, x_fm, 0)
        ch.close()
    assert live() == before

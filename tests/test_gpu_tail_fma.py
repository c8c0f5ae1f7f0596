"""The audio tail's FIRs as chains of fused multiply-adds.

Stage A, stage B and the pilot cut compute every output as acc = fma(h[k], x[top - k], acc), k ascending, in every
kernel form (fir_step, kernels.hpp): the oracle's tap order with one rounding per tap instead of two.  What is checked,
each bound against the parent commit (a multiply and an add per tap, the oracle's own arithmetic) on the same input in
the same session:

* oracle parity of the tail stage by stage: the chain's own de-emphasised 384 kHz signal (debug tap 3) through the
  oracle's audio resampler, pilot cut and DC block -- running on across the calls -- against the chain's mono audio, for
  FM at 10 MS/s in calls of 1, 3 and 4 blocks of 65536, a ragged call and one-block calls of 45 / 48 / 51 audio samples
  (cutting a), and for the same blocks cut into calls at other places (cutting b): what a call hands the next one -- the
  FIRs' history samples -- is checked against a filter that was never cut.  Bound: twice the parent's error.  Measured
  (MI355X, 6355 samples, audio rms 0.4355), rms (max):
      cutting a   parent 2.201e-12 (9.1e-12)   this commit 2.256e-12 (9.1e-12)
      cutting b   parent 2.460e-12 (9.1e-12)   this commit 2.274e-12 (9.1e-12)
  The serial environment's forms (FMR_SERIAL=1: k_aud_decim, the serial de-emphasis and DC block) get the same bound,
  that of the product's forms on the same input: the parent's serial environment IS the oracle's arithmetic (error
  0.0, measured), so any fused multiply-add moves it; this commit measures 1.293e-12 (7.3e-12) there -- the roundings
  of the FIRs behind the DC block, as in the product's forms;
* call cuts of the stereo chain behind the pilot lock: the decoder's Newton solves (IF AGC, pilot PLL) run per call, so
  two cuttings agree to the solves' 1e-7, not bit for bit (the parent neither; its mono chain at 384 kHz differs by
  3.7e-10 between cuttings, measured);
* one NaN IF sample: the non-finite audio samples do not outnumber the parent's count for the same input, which is
  none (the discriminator zeroes the sample's footprint, parent and this commit alike).
"""
import importlib
import os

import numpy as np
import pytest

import oracle_py as ora
import siggen

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")
BLK = 65536
LOCK_CALL = [BLK] * 110                     # 0.72 s: the pilot lock takes 0.67 s
CALLS = [LOCK_CALL, [BLK], [BLK] * 3, [BLK] * 4, [9375, 10000, 10625, 30000, 65000, 2000, 65536],
         [9375], [10000], [10625], [BLK] * 2]
# parent commit (mul + add per tap, the oracle's arithmetic), same session as this commit's figures
PARENT_STAGE_ERR = {"a": 2.201e-12, "b": 2.460e-12}          # the product's kernel forms, by cutting (CUTS below)
PARENT_NAN_COUNT = 0


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def _run(x, calls, *, in_rate=10e6, stereo=True, taps=False, serial=False, max_block_len=BLK):
    """Audio of every call (list), and with taps the de-emphasised 384 kHz mono signal of every call."""
    old = {k: os.environ.pop(k, None) for k in ("FMR_DEBUG_TAPS", "FMR_SERIAL")}
    if serial:
        os.environ["FMR_SERIAL"] = "1"
    if taps:
        os.environ["FMR_DEBUG_TAPS"] = "1"
    try:
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=in_rate, enable_resampler=in_rate != 384e3, stereo=stereo,
                       max_block_len=max_block_len, max_blocks=max(len(c) for c in calls))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    audio, alens, mono384, pos = [], [], [], 0
    for c in calls:
        n = sum(c)
        a, alen = ch.process_blocks(x[None, pos:pos + n], c)
        pos += n
        audio.append(np.array(a[0]))
        alens.append([int(v) for v in alen])
        if taps:
            mono384.append(ch.debug_read(3))
    st = ch.status(0)
    ch.close()
    return audio, alens, mono384, st


@pytest.fixture(scope="module")
def signal():
    x = siggen.fm_stereo_iq(sum(sum(c) for c in CALLS), 10e6)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def product(signal):
    return _run(signal, CALLS)


def test_stereo_call_cuts_agree_to_the_solves_tolerance(signal, product):
    """Other cuts of the calls behind the lock call: per-call Newton solves, so not bit for bit (the parent neither)."""
    got = np.concatenate(product[0][1:])
    calls = [LOCK_CALL, [BLK] * 5, [BLK] * 3, [9375, 10000, 10625, 30000, 65000], [2000, 65536, 9375], [10000, 10625],
             [BLK] * 2]
    assert sum(sum(c) for c in calls) == sum(sum(c) for c in CALLS)
    other, alen, _, st = _run(signal, calls)
    other = np.concatenate(other[1:])
    assert st.stereo_detected == 1 and product[3].stereo_detected == 1      # the L-R channel reaches the output
    assert got.shape == other.shape
    assert float(np.max(np.abs(got - other))) < 1e-7


def _regroup(calls, sizes):
    """The same blocks in the same order, cut into calls of sizes[0], sizes[1], ... blocks (cyclic)."""
    blocks = [b for c in calls for b in c]
    out, i, k = [], 0, 0
    while i < len(blocks):
        out.append(blocks[i:i + sizes[k % len(sizes)]])
        i += sizes[k % len(sizes)]
        k += 1
    return out


STAGE_CALLS = CALLS[1:8] + [[BLK] * 2, [BLK], [BLK] * 3, [BLK] * 2, [BLK]]
CUTS = {"a": STAGE_CALLS, "b": _regroup(STAGE_CALLS, [2, 5, 1, 3])}


@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("cut", ["a", "b"])
def test_tail_stages_against_the_oracle(signal, pilotcut, cut, serial):
    calls = CUTS[cut]
    n = sum(sum(c) for c in calls)
    audio, alen, mono384, _ = _run(signal[:n], calls, stereo=False, taps=True, serial=serial)
    rs = ora.Resampler(384e3, 48e3, 180.0)
    pc = ora.LowPassFilterFirAudio(pilotcut)
    hp = ora.HighPassFilterIir(0.0001)
    ref = []
    for al, m in zip(alen, mono384):
        a48 = rs.process(m)
        assert len(a48) == sum(al), (len(a48), al)
        o = 0
        for nb in al:                               # the pilot cut runs per audio block (its block-head path)
            ref.append(hp.process(pc.process(a48[o:o + nb])))
            o += nb
    got, ref = np.concatenate(audio), np.concatenate(ref)
    assert got.shape == ref.shape
    err = rms(got - ref)
    print(f"tail stages vs oracle (cut {cut}, serial environment: {serial}): rms err {err:.3e}, "
          f"max {float(np.max(np.abs(got - ref))):.3e}, audio rms {rms(ref):.4f}, {len(ref)} samples")
    assert err <= 2 * PARENT_STAGE_ERR[cut], (err, PARENT_STAGE_ERR[cut])


def test_one_nan_sample_stays_confined(signal):
    calls = [[BLK] * 4, [BLK] * 3]
    n = sum(sum(c) for c in calls)
    x = np.array(signal[:n])
    x[3 * BLK + 1234] = complex(np.nan, 0.0)
    a = np.concatenate(_run(x, calls, stereo=False)[0])
    bad = int(np.sum(~np.isfinite(a)))
    print(f"non-finite audio samples: {bad} of {len(a)}")
    assert bad <= PARENT_NAN_COUNT, (bad, PARENT_NAN_COUNT)
    assert np.isfinite(a[-300:]).all()

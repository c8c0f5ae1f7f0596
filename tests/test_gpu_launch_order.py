"""What a call launches, in which order and on which stream, for the shapes that take the different paths through the call
path (plan_call and the run_* stages of csrc/fmradion_amd.hip).  Four asynchronous calls with kernel timing in trace mode
(enable_kernel_timing(3)), one synchronise, then the (name, stream) pairs of kernel_trace() against the list recorded in
tests/golden/launch_order.json.  The trace is kept in the order the host enqueues, so it is deterministic; the time stamps
are not compared.

The trace covers the instrumented launches only (what the engine brackets with timed() / timed_on()).  Table copies, event
records and event waits leave no entry: they are covered by the tests that hold the audio bit-identical between the
pipelined and the in-order chain (test_gpu_pipeline.py) and across the launch-structure switches (test_gpu_configs.py).

The golden lists were recorded with this file's trace_of() against the engine as it was before the call path was rewritten
as a plan and job structs: they pin the order that engine had, not the order of the code under test."""
import importlib
import json
import os

import numpy as np
import pytest

import siggen
from conftest import GOLD, load_filter

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")
BLK = 65536                 # 10 MS/s: 2516 or 2517 IF samples per block
N_CALLS = 4
GOLDEN = os.path.join(GOLD, "launch_order.json")

FM10 = dict(mode=fmr.MODE_FM, input_rate=10e6, enable_resampler=True, stereo=True, max_block_len=BLK)
# name: (chain arguments, environment, block lengths of the four calls, signal).  N_if is the IF sample count of a call;
# plan_call's thresholds: 1536 (fused front end), 3072 (poly5h_disc, poly4_disc), 8192 (short-call round counts).
SHAPES = {
    # (a) fused front end with the discriminator epilogue, pipelined: N_if = 10066
    "fm_pipelined": (FM10, {}, [[BLK] * 4] * 4, "fm10"),
    # (b) the same in order: the mono channel beside the PLL (split_mono), the lock walk in its own call
    "fm_in_order": (FM10, {"FMR_PIPELINE": "0"}, [[BLK] * 4] * 4, "fm10"),
    # (c) the IF filter on the matrix cores with the discriminator epilogue (poly4_disc); the tail waits behind it
    "fm_if_filter": (dict(FM10, fmfilter_enable=True, filter="jj1bdx_fm_384kHz_medium"), {}, [[BLK] * 4] * 4, "fm10"),
    # (d) R8B class: decim16 + poly5h_disc, k_fe_post behind the first PLL pass
    "fm_r8b": (dict(FM10, resampler_class=fmr.RESAMPLER_R8B), {}, [[BLK] * 4] * 4, "fm10"),
    # (e) 384 kHz with the equaliser: 60 blocks of 160 samples (N_if = 9600), so that the equaliser's 100 warm-up blocks end
    # inside the second call and the AGC runs beside it from there on
    "fm_equaliser": (dict(mode=fmr.MODE_FM, input_rate=384e3, stereo=True, multipath_stages=8, max_block_len=160),
                     {}, [[160] * 60] * 4, "fm384"),
    # (f) AM at 48 kHz
    "am": (dict(mode=fmr.MODE_AM, input_rate=48e3, filter="jj1bdx_am_48khz_narrow", max_block_len=4096), {},
           [[4096] * 4] * 4, "am48"),
    # (g) (a) with N_if = 7549 <= 8192: three spare rounds, PLL chunks of kCPllSmall samples
    "fm_short_calls": (FM10, {}, [[BLK] * 3] * 4, "fm10"),
    # (h) (a) whose second call has blocks too short for the fused kernel: three-kernel front end, discriminator in the
    # decoder stage, its phase committed on the side stream (what the third call's front end then waits for)
    "fm_short_second_call": (FM10, {}, [[BLK] * 4, [1500, 2000, 1200], [BLK] * 4, [BLK] * 4], "fm10"),
    # (i) two mono streams: no PLL stage
    "fm_two_mono": (dict(FM10, stereo=False, n_streams=2), {}, [[BLK] * 4] * 4, "fm10"),
}


def make_signals():
    n = N_CALLS * 4 * BLK
    sig = {"fm10": np.stack([siggen.fm_stereo_iq(n, 10e6, stream_id=s) for s in range(2)]),
           "fm384": siggen.fm_stereo_iq(N_CALLS * 60 * 160, 384e3)[None, :],
           "am48": siggen.am_iq(N_CALLS * 4 * 4096, 48e3)[None, :]}
    for v in sig.values():
        v.setflags(write=False)
    return sig


@pytest.fixture(scope="module")
def signals():
    return make_signals()


def trace_of(name, signals, monkeypatch):
    """[(kernel name, stream)] of the four calls of shape `name`, in enqueue order."""
    import torch
    kw, env, calls, sig = SHAPES[name]
    kw = dict(kw)
    if "filter" in kw:
        kw["filter_coeff"] = load_filter(kw.pop("filter"))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S = kw.get("n_streams", 1)
    x = signals[sig][:S]
    n = x.shape[1]
    ch = fmr.Chain(max_blocks=max(len(c) for c in calls), **kw)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    d_x = torch.from_numpy(x.copy().view(np.float32).reshape(S, -1)).cuda()
    cap = 2 * (max(sum(c) for c in calls) + 64 * max(len(c) for c in calls))
    d_a = torch.zeros((len(calls), S, cap), dtype=torch.float64, device="cuda")
    ch.enable_kernel_timing(3)
    off = 0
    for i, c in enumerate(calls):
        alen = ch.process_blocks_device(d_x.data_ptr() + 8 * off, n, c, d_a[i].data_ptr(), cap, sync=False)
        assert int(alen.sum()) > 0
        off += sum(c)
    ch.synchronize()
    tr = [(nm, st) for nm, st, _, _ in ch.kernel_trace()]
    ch.close()
    return tr


@pytest.mark.parametrize("name", list(SHAPES))
def test_launch_order(name, signals, monkeypatch):
    with open(GOLDEN) as f:
        want = [tuple(e) for e in json.load(f)[name]]
    got = trace_of(name, signals, monkeypatch)
    assert len(want) > 0
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    assert got == want, f"{name}: first difference at entry {first}: got {got[first:first + 4]}, recorded {want[first:first + 4]}"

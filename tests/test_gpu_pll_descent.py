"""The second PLL pass's down-sweep as a descent through the Jacobian pass's tree, against the chain it replaced.

The Jacobian pass leaves the composites of its tree's inner nodes (pll_compose_tree's sink, csrc/pll_compose.hpp); the
pass behind it takes every chunk's start delta from them in five dependent levels (pll_descend_head, kernels_par.hpp)
where the chain head walks two groups of 32 chunks step by step.  FMR_X_PLL_CHAIN_HEAD=1 selects the chain head in the
same library: both forms run in this process, on the calls of tests/test_gpu_pll_sweeps.py (its chunk counts, its call
builder) plus 95 chunks (a wave whose second group is short) and 32 * 32 * 32 + 1 (a second batch of level 3), whole
chunks and ragged blocks, two streams, behind a warm-up call that brings the PLL into lock.  Same chunks, same
arithmetic, another association: decisions identical, audio to 1e-9, the second pass's boundary mismatch within a
factor 2, the audio within 1e-5 RMS of the oracle's FmDecoder -- the bounds of that file.

A call at noise sigma = 3e-2 needs its third pass: the descent runs in pass 2, k_pll_up and the chain in pass 3.  A call
of one chunk is accepted on its first pass: no down-sweep runs at all.
"""
import importlib
import os

import numpy as np
import pytest

import oracle_py as ora
import siggen
from conftest import ROOT
from test_gpu_pll_sweeps import COUNTS as SWEEP_COUNTS, FS, MISMATCH_FLOOR, S, WARM, call_of, chunks_of

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")

WANTED = [1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 1023, 1024, 1025]
COUNTS = SWEEP_COUNTS + [n for n in WANTED if n not in SWEEP_COUNTS]
BIG = 32 * 32 * 32 + 1                  # chunks: 33 level-2 sets, the second batch of level 3
BIG_BLOCK = 65536
NOISY = 1025                            # chunks of the call at sigma = 3e-2
SWITCH = "FMR_X_PLL_CHAIN_HEAD"


def _run(chain_head, xs, calls, max_block=8192):
    old = os.environ.pop(SWITCH, None)
    if chain_head:
        os.environ[SWITCH] = "1"
    try:
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=True, n_streams=S,
                       max_block_len=max_block, max_blocks=64)
        out, pos = [], 0
        for ll in calls:
            m = sum(ll)
            a, alen = ch.process_blocks(xs[:, pos:pos + m], ll)
            pos += m
            st = [ch.status(s) for s in range(S)]
            out.append([dict(audio=np.array(a[s]), alen=int(alen.sum()), locked=int(st[s].stereo_detected),
                             rounds=int(st[s].pll_iterations), fallback=int(st[s].pll_fallback),
                             mismatch=[float(v) for v in st[s].pll_mismatch_history]) for s in range(S)])
        ch.close()
        return out
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def _oracle(xs, calls):
    pilotcut = np.load(os.path.join(ROOT, "tests", "golden", "filters", "jj1bdx_48khz_fmaudio.npy"))
    ref = []
    for s in range(S):
        fm = ora.FmDecoder(False, fmr.DELAY_3TAPS, True, 50.0, False, 0, pilotcut)
        pos, per_call = 0, []
        for ll in calls:
            parts = []
            for b in ll:
                parts.append(np.asarray(fm.process(xs[s, pos:pos + b])))
                pos += b
            per_call.append(np.concatenate(parts))
        ref.append(per_call)
    return ref


def _both(calls, sigma=None, max_block=8192):
    total = sum(sum(ll) for ll in calls)
    kw = {} if sigma is None else dict(sigma=sigma)
    xs = np.stack([siggen.fm_stereo_iq(total, FS, stream_id=s, **kw) for s in range(S)])
    return _run(False, xs, calls, max_block), _run(True, xs, calls, max_block), _oracle(xs, calls)


def _compare(tag, n, c, desc, chain, ref):
    """The assertions of tests/test_gpu_pll_sweeps.py between the two forms, for call c of n chunks."""
    for s in range(S):
        t, v = desc[c][s], chain[c][s]
        m_t = t["mismatch"][1] if len(t["mismatch"]) > 1 else 0.0
        m_v = v["mismatch"][1] if len(v["mismatch"]) > 1 else 0.0
        err = float(np.max(np.abs(t["audio"] - v["audio"]))) if t["audio"].size == v["audio"].size and t["audio"].size else 0.0
        e_ref = t["audio"] - ref[s][c] if t["audio"].size == ref[s][c].size else np.array([np.inf])
        rms = float(np.sqrt(np.mean(e_ref ** 2))) if e_ref.size else 0.0
        print(f"{tag} chunks {n:5d} stream {s}: rounds {t['rounds']}/{v['rounds']} fallback {t['fallback']}/{v['fallback']} "
              f"locked {t['locked']}/{v['locked']} audio {t['alen']}/{v['alen']} mismatch[1] {m_t:.3e}/{m_v:.3e} "
              f"|descent - chain| {err:.2e} rms vs oracle {rms:.2e}")
        assert (t["rounds"], t["fallback"], t["locked"], t["alen"]) == (v["rounds"], v["fallback"], v["locked"], v["alen"]), (n, s)
        assert t["audio"].shape == v["audio"].shape
        assert err < 1e-9, (n, s, err)
        if t["rounds"] >= 2 and max(m_t, m_v) > MISMATCH_FLOOR:      # (a call accepted on its first pass has no second entry)
            assert m_v / 2 <= m_t <= m_v * 2, (n, s, m_t, m_v)
        assert rms < 1e-5, (n, s, rms)


@pytest.fixture(scope="module")
def runs():
    """Both layouts in one sequence of calls per chain: warm-up, the whole-chunk calls, the ragged calls.  Descent head, chain
    head and the oracle, once for all tests."""
    calls = [WARM] + [call_of(n, False) for n in COUNTS] + [call_of(n, True) for n in COUNTS]
    assert [chunks_of(ll) for ll in calls[1:]] == COUNTS + COUNTS
    assert all(n in COUNTS for n in WANTED)
    return (calls,) + _both(calls)


@pytest.mark.parametrize("ragged", [False, True], ids=["whole_chunks", "ragged_blocks"])
def test_descent_head_equals_chain_head(runs, ragged):
    calls, desc, chain, ref = runs
    assert all(desc[0][s]["locked"] == 1 for s in range(S))          # the warm-up call brought the PLL into lock
    first = 1 + (len(COUNTS) if ragged else 0)
    for c in range(first, first + len(COUNTS)):
        _compare("ragged" if ragged else "whole", COUNTS[c - first], c, desc, chain, ref)


def test_one_chunk_is_accepted_without_a_down_sweep(runs):
    calls, desc, chain, ref = runs
    c = 1 + COUNTS.index(1)
    for s in range(S):
        assert desc[c][s]["rounds"] == 1 and chain[c][s]["rounds"] == 1, (desc[c][s]["rounds"], chain[c][s]["rounds"])
        assert np.array_equal(desc[c][s]["audio"], chain[c][s]["audio"])      # (nothing of the two forms ran)


def test_second_batch_of_level_3():
    blocks = [BIG_BLOCK] * (BIG // (BIG_BLOCK // 64)) + [64]
    assert sum(-(-b // 64) for b in blocks) == BIG
    calls = [WARM, blocks]
    desc, chain, ref = _both(calls, max_block=BIG_BLOCK)
    assert all(desc[0][s]["locked"] == 1 for s in range(S))
    _compare("level 3", BIG, 1, desc, chain, ref)


def test_third_pass_keeps_the_chain():
    calls = [WARM, call_of(NOISY, False)]
    desc, chain, ref = _both(calls, sigma=3e-2)
    for s in range(S):
        assert desc[1][s]["rounds"] >= 3, desc[1][s]["rounds"]      # pass 2: the descent; pass 3: k_pll_up and the chain
    _compare("sigma 3e-2", NOISY, 1, desc, chain, ref)

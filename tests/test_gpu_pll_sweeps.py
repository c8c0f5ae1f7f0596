"""The node pass's sweeps inside the PLL's integration passes, at every level's edge.

The Jacobian pass composes its chunks' maps as a balanced tree out of the registers (pll_compose_tree, kernels_par.hpp),
the second pass runs the down-sweep in its head.  A group is 32 chunks, a wave 64, a level-2 set 1024: calls of 1, 2, 3,
31, 32, 33, 63, 64, 65, 127, 129, 1023, 1024, 1025 and 2049 chunks straddle every one of those edges, once with whole
chunks and once with ragged blocks (every block ends in a short chunk), on two streams, behind one warm-up call that
brings the PLL into lock.  The partner is the chain form: FMR_PLL_V1=1, seven launches a round, every sweep a dependent
chain (tests/test_gpu_pll_forms.py).  Same chunks, same arithmetic, another association: decisions identical, audio to
1e-9 (that test's bound), the second round's boundary mismatch within a factor 2 (a wrong composite shows as orders of
magnitude, or as an extra round), and the audio within 1e-5 RMS of the oracle's FmDecoder.

Chunk lengths are the library's: 64 samples, 16 in calls of up to 8192 samples (fmradion_amd.hip, kSmallCall).  The
calls below are built to the chunk COUNT: a call that would be too short for 64-sample chunks is made of 16-sample ones.
"""
import importlib
import os

import numpy as np
import pytest

import oracle_py as ora
import siggen
from conftest import ROOT

pytestmark = pytest.mark.gpu

fmr = importlib.import_module("airspy-fmradion_amd")

FS, S = 384e3, 2
COUNTS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 129, 1023, 1024, 1025, 2049]
WARM = [8192] * 64                      # 1.37 s: the lock flag needs 0.67 s of pilot
SMALL_CALL, MAX_BLOCK = 8192, 8192
# The mismatch is counted in units of 1e-7 rad of phase (the acceptance rule's unit; a pass is accepted at 16).  One Newton
# round solves a call of two chunks exactly, so its second mismatch is the rounding of the last operation: 0.0 in one
# form, 1.3e-13 in the other, and no factor holds between those.  Below 16 last bits of a phase of 2 pi in that unit
# (16 * 2 pi * 2^-52 * 1e7 = 2.2e-7 units) both values are rounding and only have to stay there.
MISMATCH_FLOOR = 16 * 2 * np.pi * 2.0 ** -52 * 1e7


def chunks_of(blocks):
    """The library's chunk count of a call (k_chunk_tab and the rule for short calls)."""
    c = 16 if sum(blocks) <= SMALL_CALL else 64
    return sum(-(-b // c) for b in blocks)


def call_of(n, ragged):
    """Block lengths of a call of n chunks.  ragged: blocks of 40 chunks whose last is short (2517 = 39 * 64 + 21 samples
    with chunks of 64), and a last block of the chunks left over, also ending short."""
    for c, tail in ((64, 21), (16, 5)):
        per = 40 if ragged else MAX_BLOCK // c
        short = tail if ragged else c
        blocks = [(per - 1) * c + short] * (n // per)
        if n % per:
            blocks.append((n % per - 1) * c + short)
        if chunks_of(blocks) == n:
            return blocks
    raise AssertionError(n)


def _run(v1, xs, calls):
    old = os.environ.pop("FMR_PLL_V1", None)
    if v1:
        os.environ["FMR_PLL_V1"] = "1"
    try:
        ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=FS, enable_resampler=False, stereo=True, n_streams=S,
                       max_block_len=MAX_BLOCK, max_blocks=64, ab=bool(v1))
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
        os.environ.pop("FMR_PLL_V1", None)
        if old is not None:
            os.environ["FMR_PLL_V1"] = old


@pytest.fixture(scope="module")
def runs():
    """Both layouts in one sequence of calls per chain: warm-up, the whole-chunk calls, the ragged calls.  The product, its
    chain-form partner and the oracle, once for all tests."""
    calls = [WARM] + [call_of(n, False) for n in COUNTS] + [call_of(n, True) for n in COUNTS]
    assert [chunks_of(ll) for ll in calls[1:]] == COUNTS + COUNTS
    assert all(ll[-1] % 64 == 21 or ll[-1] % 16 == 5 for ll in calls[1 + len(COUNTS):])
    total = sum(sum(ll) for ll in calls)
    xs = np.stack([siggen.fm_stereo_iq(total, FS, stream_id=s) for s in range(S)])
    tree, chain = _run(False, xs, calls), _run(True, xs, calls)
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
    return calls, tree, chain, ref


@pytest.mark.parametrize("ragged", [False, True], ids=["whole_chunks", "ragged_blocks"])
def test_tree_sweeps_equal_chain_sweeps(runs, ragged):
    calls, tree, chain, ref = runs
    assert all(tree[0][s]["locked"] == 1 for s in range(S))          # the warm-up call brought the PLL into lock
    first = 1 + (len(COUNTS) if ragged else 0)
    for c in range(first, first + len(COUNTS)):
        n = COUNTS[c - first]
        for s in range(S):
            t, v = tree[c][s], chain[c][s]
            m_t, m_v = t["mismatch"][1], v["mismatch"][1]
            err = float(np.max(np.abs(t["audio"] - v["audio"]))) if t["audio"].size == v["audio"].size and t["audio"].size else 0.0
            e_ref = t["audio"] - ref[s][c] if t["audio"].size == ref[s][c].size else np.array([np.inf])
            rms = float(np.sqrt(np.mean(e_ref ** 2))) if e_ref.size else 0.0
            print(f"chunks {n:4d} ragged {int(ragged)} stream {s}: rounds {t['rounds']}/{v['rounds']} fallback "
                  f"{t['fallback']}/{v['fallback']} locked {t['locked']}/{v['locked']} audio {t['alen']}/{v['alen']} "
                  f"mismatch[1] {m_t:.3e}/{m_v:.3e} |tree - chain| {err:.2e} rms vs oracle {rms:.2e}")
            assert (t["rounds"], t["fallback"], t["locked"], t["alen"]) == (v["rounds"], v["fallback"], v["locked"], v["alen"]), (n, s)
            assert t["audio"].shape == v["audio"].shape
            assert err < 1e-9, (n, s, err)
            if t["rounds"] >= 2 and max(m_t, m_v) > MISMATCH_FLOOR:  # (a call accepted on its first pass has no second entry)
                assert m_v / 2 <= m_t <= m_v * 2, (n, s, m_t, m_v)
            assert rms < 1e-5, (n, s, rms)

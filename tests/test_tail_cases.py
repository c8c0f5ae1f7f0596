"""tests/tail_cases.py pinned on the CPU: the stage oracle IS the oracle (bit for bit), K_STATE is the bound of
tests/test_gpu_tail_fma.py in units of the DC block's state, and every case of tests/test_gpu_tail_stereo.py lies in the
regime it is named for -- computed from block lengths alone and from the oracle's own lock decisions."""
import math

import numpy as np
import pytest

import oracle_py as ora
import siggen
import tail_cases as tc

# the constants the regimes are computed from, where the product defines them
assert tc.C_DC == 64            # airspy-fmradion_amd/csrc/fmradion_amd.hip:74    constexpr int ... C_DC = 64
assert tc.FMR_DC_K == 32        # airspy-fmradion_amd/csrc/kernels_par.hpp:219    #define FMR_DC_K 32
assert tc.FMR_DC_MAXW == 8      # airspy-fmradion_amd/csrc/kernels_par.hpp:220    #define FMR_DC_MAXW 8


@pytest.fixture(scope="module")
def pilotcut():
    return tc.load_pilotcut()


@pytest.mark.parametrize("stereo,pilot_shift", [(True, False), (True, True), (False, False)])
def test_stage_oracle_is_the_oracle(pilotcut, stereo, pilot_shift):
    """FmDecoder block by block at 384 kHz through the lock-in; after every block the stage oracle on the decoder's own
    de-emphasised signals and lock flag returns exactly the decoder's audio."""
    blocks = [2048] * 60 + [1, 7, 8, 400, 0] * 3 + [2048] * 40 + [0, 400, 8, 7, 1] * 2 + [2048] * 4
    x = tc.fm_iq(sum(blocks))
    (alens, locked, taps), = tc.oracle_blocks(x, [blocks], pilotcut, stereo=stereo, pilot_shift=pilot_shift, want_taps=True)
    so = tc.stage_oracle(pilotcut, stereo=stereo)
    n = 0
    for (a, m384, d384), al, lk in zip(taps, alens, locked):
        r = so.process_call(m384, d384 if stereo else None, [al], [lk], pilot_shift)
        assert np.array_equal(r.audio, a)
        assert len(r.st_m) == al and (not stereo or len(r.st_d) == al)
        n += len(a)
    assert n == (2 if stereo else 1) * tc.cum_audio(sum(blocks)) > 26000
    if stereo:
        assert not locked[0] and locked[-1] and sum(alens[i] > 0 and not locked[i] for i in range(len(blocks))) > 50
    # several blocks in one call: the resampler runs over the call, pilot cut and mux per block
    so2 = tc.stage_oracle(pilotcut, stereo=stereo)
    got, i = [], 0
    for k in [7, 1, 60, 3, 200]:
        sel = range(i, min(i + k, len(blocks)))
        r = so2.process_call(np.concatenate([taps[j][1] for j in sel]),
                             np.concatenate([taps[j][2] for j in sel]) if stereo else None,
                             [alens[j] for j in sel], [locked[j] for j in sel], pilot_shift)
        got.append(r.audio)
        i += k
    assert np.array_equal(np.concatenate(got), np.concatenate([t[0] for t in taps]))


def test_units_count_the_locked_blocks_only(pilotcut):
    x = tc.fm_iq(8 * 2048)
    (alens, _, taps), = tc.oracle_blocks(x, [[2048] * 8], pilotcut, want_taps=True)
    m, d = np.concatenate([t[1] for t in taps]), np.concatenate([t[2] for t in taps])
    r = tc.stage_oracle(pilotcut).process_call(m, d, alens, [False, True] * 4)
    u = r.units()
    lk = np.repeat([False, True] * 4, alens)
    assert u["mid"] == (tc.ULP * tc.rms(r.st_m), tc.ULP * tc.amax(r.st_m))
    assert u["side"][0] == tc.STEREO_GAIN * tc.ULP * tc.rms(r.st_d * lk)
    assert u["out"][0] == u["mid"][0] + u["side"][0] and u["out"][1] == u["mid"][1] + u["side"][1]
    lo, hi = sum(alens[:2]), sum(alens[:3])             # an unlocked block by itself: only u_m counts
    assert r.units(lo, hi)["side"] == (0.0, 0.0) and r.units(lo, hi)["out"] == r.units(lo, hi)["mid"]
    rp = tc.stage_oracle(pilotcut).process_call(m, d, alens, [False, True] * 4, pilot_shift=True)
    assert rp.units()["out"] == (tc.ULP * tc.rms(rp.st_d * lk), tc.ULP * tc.amax(rp.st_d * lk))
    assert np.all(rp.audio[0::2][~lk] == 0.0) and np.array_equal(rp.audio[0::2][lk], rp.d[lk])


def test_k_state(pilotcut):
    """K_STATE = the bound test_gpu_tail_fma.py asserts on its mono cutting "a" (2 x 2.201e-12), in units of
    u = 2^-52 x rms(DC-block state) of the ORACLE's mono chain on that test's input and calls."""
    blk = 65536
    calls = [[blk] * 110, [blk], [blk] * 3, [blk] * 4, [9375, 10000, 10625, 30000, 65000, 2000, 65536], [9375], [10000],
             [10625], [blk] * 2]                                            # test_gpu_tail_fma.py: CALLS (the signal's length)
    stage_calls = calls[1:8] + [[blk] * 2, [blk], [blk] * 3, [blk] * 2, [blk]]         # ... STAGE_CALLS = CUTS["a"]
    n = tc.n_samples(stage_calls)
    x = siggen.fm_stereo_iq(tc.n_samples(calls), 10e6)[:n]
    so = tc.stage_oracle(pilotcut, stereo=False)
    st = []
    for alens, _, taps in tc.oracle_blocks(x, stage_calls, pilotcut, in_rate=10e6, stereo=False, want_taps=True):
        for (a, m384, _), al in zip(taps, alens):
            r = so.process_call(m384, None, [al])
            assert np.array_equal(r.audio, a)
            st.append(r.st_m)
    st = np.concatenate(st)
    u = tc.ULP * tc.rms(st)
    print(f"oracle mono chain on test_gpu_tail_fma's input: {len(st)} audio samples, rms(state) {tc.rms(st):.2f}, "
          f"max|state| {tc.amax(st):.2f}, u = {u:.5e}, bound / u = {tc.TAIL_FMA_BOUND / u:.3f}")
    assert len(st) == 6355
    assert u == pytest.approx(tc.TAIL_FMA_U, rel=1e-4)
    assert math.ceil(tc.TAIL_FMA_BOUND / u) == tc.K_STATE


ALL_CASES = ["CASE1_A", "CASE1_B", "CASE2", "CASE3", "CASE4", "CASE5A", "CASE5B"]


@pytest.mark.parametrize("name", ALL_CASES)
def test_audio_lens_from_block_lengths(name):
    """cum_audio against the oracle's resampler (the counts do not depend on the samples)."""
    calls = getattr(tc, name)
    if name == "CASE4":
        calls = [calls[0], calls[1][:20], calls[1][20:40]]
    rs = ora.Resampler(tc.FS_IF, tc.FS_AU, 180.0)
    assert [[len(rs.process(np.zeros(b))) for b in c] for c in calls] == tc.audio_lens(calls)


def test_regime_arithmetic():
    r = tc.regime([8192] * 129)
    assert (r["n_audio"], r["chunks"], r["waves"], r["passes"], r["tile"], r["tiles"]) == (1056768, 16512, 8, 2, 1280, 7)
    r = tc.regime([320, 0, 7])
    assert (r["chunks"], r["waves"], r["passes"], r["tile"], r["tiles_per_block"]) == (6, 1, 1, 320, [1, 0, 1])
    assert tc.regime([321])["tile"] == 1280 and tc.regime([1281])["tiles"] == 2
    assert tc.regime([64] * 2048)["waves"] == 1 and tc.regime([64] * 2048 + [1])["waves"] == 2
    assert tc.regime([64] * 16384)["passes"] == 1 and tc.regime([64] * 16384 + [1])["passes"] == 2


def test_case1_shapes():
    al = tc.audio_lens(tc.CASE1_A)
    assert [sum(a) for a in al[1:4]] == [314, 944, 2517] and [len(a) for a in al[1:4]] == [1, 3, 8]
    assert al[4][0] == 50 and al[4][4] == 0 and al[4][7] == 0 and sorted(al[4][1:4]) == [0, 1, 1]      # 400, 1, 7, 8, 0, ..
    assert [a for a in al[5:8]] == [[45], [48], [51]]
    assert all(tc.regime(a)["tile"] == 320 for a in al[1:])             # the product's form of the pilot cut
    assert [b for c in tc.CASE1_A for b in c] == [b for c in tc.CASE1_B for b in c]
    assert tc.CASE1_A[0] == tc.CASE1_B[0] == tc.LOCK and tc.CASE1_A[1:] != tc.CASE1_B[1:]
    # the L-R halos (58 + 280 / 3 mid-rate and 126 audio samples) reach over three and more blocks of the ragged call
    assert sum(al[4][1:5]) < 126


def test_case2_regimes():
    al = tc.audio_lens(tc.CASE2)
    assert [a[0] for a in al[1:7]] == tc.PCUT_AUDIO and al[7] == tc.PCUT_AUDIO
    for a, want in zip(al[1:], tc.CASE2_REGIME):
        r = tc.regime(a)
        assert (r["au_max"], r["tile"], r["tiles"]) == want
    r = tc.regime(al[8])                                                # short blocks in the 1280-tile form, one tile each
    assert r["tile"] == 1280 and r["tiles_per_block"] == [1, 1, 1, 3, 1] and sorted(al[8])[:4] <= [315] * 4


@pytest.mark.parametrize("name", ["CASE3", "CASE4"])
def test_node_pass_regimes(name):
    al = tc.audio_lens(getattr(tc, name))
    for i, want in getattr(tc, name + "_REGIME").items():
        r = tc.regime(al[i])
        assert (r["n_audio"], r["chunks"], r["waves"], r["passes"]) == want
        assert tc.regime(al[i + 1])["waves"] == 1                       # the call behind it is short: the carried state
    if name == "CASE3":
        assert al[3][-1] == 1 or sum(al[3]) % 64 == 1                   # chunk 2176 holds one sample
        assert (2177 - 2048) // tc.FMR_DC_K == 4 and (2177 - 2048) % tc.FMR_DC_K == 1      # lane 4 of wave 1, one chunk
        assert 4608 - 2 * 2048 == 512                                   # the third wave: 16 of its 64 lanes
    else:
        assert 16512 - 8 * 2048 == 128                                  # the second pass


def _runs(flags):
    out = []
    for f in flags:
        if not out or out[-1] != f:
            out.append(f)
    return out


@pytest.mark.parametrize("pilot_shift", [False, True])
def test_lock_transition_cases_hold_both_flags_in_one_call(pilotcut, pilot_shift):
    x = tc.fm_iq(tc.n_samples(tc.CASE5A))
    (alens, locked), = tc.oracle_blocks(x, tc.CASE5A, pilotcut, pilot_shift=pilot_shift)
    ne = [lk for lk, a in zip(locked, alens) if a > 0]
    assert ne.count(False) >= 2 and ne.count(True) >= 2 and _runs(ne) == [False, True]
    i = locked.index(True)
    assert tc.CASE5A[0][i - 2:i + 1] == [5, 0, 63] and alens[i - 1] == 0 and alens[i] in (7, 8)
    assert sum(alens[:i]) % 64 != 0 and sum(alens[:i + 1]) % 64 != 0    # the flag changes inside a 64-sample chunk
    x = tc.pilot_drop_iq(tc.n_samples(tc.CASE5B))
    (alens, locked), = tc.oracle_blocks(x, tc.CASE5B, pilotcut, pilot_shift=pilot_shift)
    assert min(alens) > 0
    assert _runs(locked) == [False, True, False, True]                  # locked -> unlocked -> locked inside the call
    assert all(locked.count(f) >= 2 for f in (False, True))
    edges = [i for i in range(1, len(locked)) if locked[i] != locked[i - 1]]
    assert all(sum(alens[:i]) % 64 != 0 for i in edges)


def test_case6_shapes(pilotcut):
    """1 MS/s behind the IF resampler: three pilot-cut tiles per product block, the lock inside the first call."""
    x = siggen.fm_stereo_iq(tc.n_samples(tc.CASE6_1M), 1e6)
    res = tc.oracle_blocks(x, tc.CASE6_1M, pilotcut, in_rate=1e6)
    assert res[0][1][-1] and all(all(lk) for _, lk in res[1:])
    assert all(3140 <= a <= 3150 for a in res[2][0]) and tc.regime(res[2][0])["tiles"] == 3
    assert [len(c) for c in tc.CASE6_1M] == [16] + [len(c) for c in tc.CASE1_A[1:]]
    assert 0 in res[4][0] and [sum(a) for a, _ in res[5:8]] == [45, 48, 51]


def test_node_pass_model_shows_what_the_powers_cost(pilotcut):
    """The finding behind the fix in make_dc_coef / k_dc_nodes, on the CPU: a float64 model of the DC block's multiple shooting
    against the oracle's serial recurrence on the same pilot-cut output, a cold call and a steady one that starts from a
    carried state.  With A^2048 from a chain of double products (4e-10 wrong) and every product rounded by itself the model
    is where the product was measured, over 100 u; with the powers from long double and one rounding per row it is at the
    oracle's own distance from a long-double evaluation, inside K_STATE."""
    assert np.finfo(np.longdouble).nmant >= 63
    n = 6 * 65536 + 20 * 8192
    x = tc.fm_iq(n)
    ((_, _, taps),) = tc.oracle_blocks(x, [[n]], pilotcut, stereo=False, want_taps=True)
    v = ora.LowPassFilterFirAudio(pilotcut).process(ora.Resampler(tc.FS_IF, tc.FS_AU, 180.0).process(taps[0][1]))
    hp = ora.HighPassFilterIir(0.0001)
    coef = (hp.s.b0, hp.s.b1, hp.s.b2, hp.s.a1, hp.s.a2)
    y, st = np.empty(len(v)), np.empty(len(v))
    for i, s in enumerate(v.tolist()):
        y[i] = hp._step(hp.s, s)
        st[i] = hp.s.x1
    (ach, _), (agp0, *_) = tc.dc_powers(coef[3], coef[4], False)
    (ach_x, _), (agp0_x, *_) = tc.dc_powers(coef[3], coef[4], True)
    rel = float(np.max(np.abs(agp0[0] / agp0_x[0] - 1.0)))
    print(f"A^2048 by 2048 double products: {rel:.1e} relative")
    assert 1e-10 < rel < 1e-9 and np.max(np.abs(ach[0] / ach_x[0] - 1.0)) < 1e-13
    for lo, hi in [(0, 49152), (49152, len(v))]:
        carry = (float(st[lo - 1]), float(st[lo - 2])) if lo else (0.0, 0.0)
        u, umax = tc.ULP * tc.rms(st[lo:hi]), tc.ULP * tc.amax(st[lo:hi])
        fig = {}
        for exact in (False, True):
            e = tc.dc_scan_model(v[lo:hi], coef, carry, exact) - y[lo:hi]
            fig[exact] = (tc.rms(e) / u, tc.amax(e) / umax)
            print(f"samples {lo} .. {hi}, {'long double powers, one rounding per row' if exact else 'double products':42s}: "
                  f"rms {tc.rms(e):.2e} = {fig[exact][0]:.2f} u, max {tc.amax(e):.2e} = {fig[exact][1]:.2f} u_max")
        assert fig[False][0] > 100 and fig[False][1] > 100
        assert fig[True][0] <= 1.5 and fig[True][1] <= tc.K_STATE

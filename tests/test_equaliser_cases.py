"""The conditions every case of tests/test_gpu_equaliser_edges.py relies on, proved by the oracle alone (no GPU)."""
import numpy as np
import pytest

import equaliser_cases as ec
import oracle_py as ora

TAP_TOL = 2e-6          # what the GPU tests hold the discriminator output to, per block


def failed_blocks(r):
    return [b for b in range(len(r.if_len)) if r.failed(b)]


@pytest.mark.parametrize("name", ec.NAMES)
def test_equaliser_is_active_where_the_case_looks(name):
    """Up to the 100th non-empty IF block the decoder's MPX is that of a decoder without equaliser, bit for bit; from the
    101st on it differs in every block that did not fail.  No case needs more than 400 k IF samples."""
    c = ec.case(name)
    for s in range(c.n_streams):
        r, u = ec.reference(name, s), ec.unequalised(name, s)
        af = r.active_from
        assert af is not None and r.if_len == u.if_len
        assert sum(1 for n in r.if_len[:af] if n) == ec.WARM and r.if_len[af] > 0
        assert all(np.array_equal(p, q) for p, q in zip(r.disc[:af], u.disc[:af]))
        live = [b for b in range(af, len(c.lens)) if r.if_len[b] and not r.failed(b)]
        assert len(live) >= 8
        assert not [b for b in live if np.array_equal(r.disc[b], u.disc[b])]
        assert len(failed_blocks(r)) == r.resets and u.resets == 0
        assert len(r.coeff) == c.order
        assert sum(r.if_len) <= 400_000
        assert len(c.lens) - af >= 10 and max(len(k) for k in c.calls) <= 20


@pytest.mark.parametrize("name", ec.NAMES)
def test_the_projects_bound_is_a_fair_demand(name):
    """The oracle itself, every input float moved by one ulp, stays within a quarter of the per-block bound on the
    discriminator output in every block of every case (the kernel's summation differs from the oracle's in the dot
    product and in the fused update: four times the oracle's own movement).  Measured 1.4e-7 ... 4.8e-7: the project's
    2e-6 is the larger of the two in every case, the cases far from convergence included."""
    c = ec.case(name)
    for s in range(c.n_streams):
        per_block, audio = ec.conditioning(name, s)
        print(f"{name}[{s}]: the oracle's own discriminator output moves by {max(per_block):.2e} in its worst block, its audio by {audio:.2e} RMS")
        assert 4 * max(per_block) < TAP_TOL
        assert 4 * audio < 1e-5


def test_tails_cover_every_remainder():
    for name in ("tails_E2_by1", "tails_E2_by4", "tails_E8_by1", "tails_E8_by4"):
        c = ec.case(name)
        active = c.lens[ec.WARM:]
        assert active == ec.TAIL_LENS and ec.reference(name).active_from == ec.WARM
        assert {n % 2048 % 4 for n in active} == {0, 1, 2, 3}
        assert {n % 2048 for n in active if n > 2048} >= {1, 2, 3, 2047}
        assert any(n < c.order for n in active) and any(n < 4 for n in active)
        assert all(len(k) == int(name[-1]) for k in c.calls[5:])


@pytest.mark.parametrize("stages", ec.LENGTH_STAGES)
def test_lengths(stages):
    c = ec.case("length_E%d" % stages)
    assert c.order == 4 * stages + 1 and set(c.lens[ec.WARM:]) == {2518, 2519} and len(c.lens) - ec.WARM == 30
    assert ec.reference(c.name).resets == 0
    assert {4 * s + 1 <= 320 for s in (79, 80)} == {True, False} and {4 * s + 1 <= 640 for s in (159, 160)} == {True, False}


def test_turn_on_inside_a_call():
    c = ec.case("turn_on_384k")
    af = ec.reference(c.name).active_from
    assert af == ec.WARM and af % len(c.calls[0]) not in (0,) and len(c.calls[af // 7]) == 7


def test_tiny_blocks_at_10_msps():
    """Some input blocks of 1 to 20 samples give no IF sample; they are not decoder blocks and do not count towards the
    warm-up, so the equaliser starts later than at input block 100 -- on a block that is not its call's first."""
    c = ec.case("turn_on_10m")
    r = ec.reference(c.name)
    af = r.active_from
    assert c.rate == 10e6
    empty = [b for b in range(af) if r.if_len[b] == 0]
    assert len(empty) >= 20 and all(1 <= c.lens[b] <= 20 for b in empty)
    assert any(r.if_len[b] == 1 for b in range(af))                         # ... and some give one
    assert af == ec.WARM + len(empty) and af % 9 != 0
    assert any(r.if_len[b] == 0 for b in range(af, len(c.lens))) and max(r.if_len) >= 2516


@pytest.mark.parametrize("name", ec.WALKS)
def test_walk(name):
    """The reference resets 4 stages + 1 times, in consecutive blocks; the next block succeeds; all audio is finite from
    there on; the walk crosses call boundaries."""
    c = ec.case(name)
    r, u = ec.reference(name), ec.unequalised(name)
    (where,) = np.flatnonzero(np.isnan(c.x[0].real))
    starts = np.cumsum([0] + c.lens)
    b0 = int(np.searchsorted(starts, where, side="right") - 1)
    pos = int(where - starts[b0])
    assert b0 == 104 and b0 > r.active_from
    assert {"walk_odd": pos % 4 != 0 and pos < 2048, "walk_mult4": pos % 4 == 0 and 0 < pos < 2048,
            "walk_chunk2": pos % 4 != 0 and pos >= 2048}[name]
    assert r.resets == 4 * c.stages + 1
    assert failed_blocks(r) == list(range(b0, b0 + c.order))
    after = b0 + c.order
    assert not np.array_equal(r.disc[after], u.disc[after])                 # equalised again
    assert all(np.all(np.isfinite(a)) for a in r.audio[after:])
    assert len(c.lens) - 1 - b0 >= 4 * c.stages + 4
    assert all(len(k) == 3 for k in c.calls[5:-1]) and len({(b - ec.WARM) // 3 for b in failed_blocks(r)}) >= 3


def test_overflow_fails_on_the_error_with_every_output_finite():
    """The stage-level MultipathFilter behind the stage-level AGC on the same input: the failing block stops at the large
    sample with a non-finite error, and every output it wrote, that sample's included, is finite."""
    c = ec.case("overflow")
    r = ec.reference(c.name)
    b0, pos = ec.OVERFLOW_AT
    assert pos % 4 == 0 and b0 > r.active_from and np.all(np.isfinite(c.x[0].view(np.float32)))
    agc, mpf = ora.IfSimpleAgc(1.0, 100000.0, 0.0001), ora.MultipathFilter(c.stages)
    failed, o = [], 0
    for b, n in enumerate(c.lens):
        y = agc.process(c.x[0, o:o + n])
        o += n
        if b < ec.WARM:
            continue
        good, out = mpf.process(y)
        if not good:
            failed.append(b)
            if b == b0:
                assert np.isfinite(y[pos].real) and np.isfinite(y[pos].imag) and abs(y[pos]) > 1e25
                written = out[:pos + 1].view(np.float32)
                assert np.all(np.isfinite(written)) and abs(out[pos]) > 1.9e19        # |y|^2 > FLT_MAX
                assert not np.isfinite(mpf.error())
            mpf.initialize_coefficients()
    assert failed and failed[0] == b0 and failed == failed_blocks(r) and r.resets == len(failed)
    assert np.array_equal(mpf.coeff(), r.coeff) and mpf.error() == r.error
    assert len(c.lens) - 1 - b0 >= 4 * c.stages + 4
    assert all(np.all(np.isfinite(a)) for a in r.audio[failed[-1] + 1:])


def test_level_step_stays_in_the_ordinary_agc_regime():
    """|g x| < 100 throughout, above 10 behind the rise; both steps inside a block the equaliser runs on.  The constant-
    modulus update diverges on the rise: the reference fails in that block and the next, and carries on."""
    c = ec.case("level_step")
    r = ec.reference(c.name)
    y = np.abs(ora.IfSimpleAgc(1.0, 100000.0, 0.0001).process(c.x[0]))
    a = np.abs(c.x[0])
    (steps,) = np.nonzero(np.abs(np.diff((a > 0.3).astype(int))))
    starts = np.cumsum([0] + c.lens)
    assert len(steps) == 2
    blocks = [int(np.searchsorted(starts, i + 1, side="right") - 1) for i in steps]
    assert blocks[0] > r.active_from and blocks[1] - blocks[0] == 20 and all((i + 1) not in starts for i in steps)
    print(f"level_step: max |g x| {y.max():.1f}, the reference fails in blocks {failed_blocks(r)}")
    assert 10 < y.max() < 100
    assert failed_blocks(r) == [blocks[0], blocks[0] + 1]
    assert len(c.lens) - blocks[1] >= 10


def test_three_streams():
    c = ec.case("three_streams")
    assert c.n_streams == 3 and len({c.x[s].tobytes() for s in range(3)}) == 3
    assert ec.reference(c.name, 0).resets == 0 and ec.reference(c.name, 2).resets == 0
    assert ec.reference(c.name, 1).resets == c.order == len(failed_blocks(ec.reference(c.name, 1)))
    assert not np.allclose(ec.reference(c.name, 0).coeff, ec.reference(c.name, 2).coeff, atol=1e-2)


def test_if_filter_case():
    c = ec.case("if_filter")
    assert c.fir is not None and c.stages == 8 and set(c.lens[ec.WARM:]) == {2519}
    assert len(c.fir_coeff()) > 3


def test_bump_moves_every_float_by_one_ulp():
    x = ec.case("walk_odd").x[0][ec.WARM * 256 + 4 * 2048:][:200]
    f, g = x.view(np.float32), ec.bump_ulp(x).view(np.float32)
    fin = np.isfinite(f)
    assert np.all(g[fin] != f[fin]) and np.all(np.abs(g[fin] - f[fin]) <= np.spacing(np.abs(f[fin])) * 1.0001)
    assert np.array_equal(np.isnan(f), np.isnan(g)) and 0.3 < np.mean(g[fin] > f[fin]) < 0.7

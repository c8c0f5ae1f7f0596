"""Channelizer on the GPU (fmr_create_channelizer): K rows of IQ at output_rate out of one wideband capture, against the
FM channel bank's IF (same stage A, same stage B), against plain front-end-only chains fed the capture mixed down on the
host (tests/chanbank_fixture.py), across call cuts, through the device path, and around NaN samples.  Also the batched
path fmr_resample_blocks on plain front-end-only chains."""
import importlib

import numpy as np
import pytest

import chanbank_fixture as cb
import oracle_py as ora

fmr = importlib.import_module("airspy-fmradion_amd")
pytestmark = pytest.mark.gpu

CLS = {"fast": fmr.RESAMPLER_FAST, "r8b": fmr.RESAMPLER_R8B}


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def rel(got, ref):
    return rms(got - ref) / rms(ref)


def run_rows(cz, x, calls):
    """resample_blocks call by call; returns the K rows over all calls and every block's out_len."""
    rows, lens, pos = [[] for _ in range(cz.n_streams)], [], 0
    for ll in calls:
        m = sum(ll)
        out, olen = cz.resample_blocks(x[pos:pos + m], ll)
        for s in range(cz.n_streams):
            rows[s].append(out[s])
        lens += [int(v) for v in olen]
        pos += m
    return [np.concatenate(r) for r in rows], lens


def plain_rows(F, out_rate, cls, u, calls):
    """One plain front-end-only chain per channel, fed u (the mixed-down capture) block by block through fmr_resample."""
    ch = fmr.Chain(mode=fmr.MODE_NONE, input_rate=F, enable_resampler=True, output_rate=out_rate, resampler_class=cls,
                   max_block_len=65536)
    got, pos = [], 0
    for b in (b for ll in calls for b in ll):
        got.append(ch.resample(u[pos:pos + b]))
        pos += b
    ch.close()
    return np.concatenate(got)


FM_OFFS = {10e6: [-4_100_000, -2_300_000, -700_000, -300_000, 1_234_567, 4_450_000],
           6e6: [-2_500_000, -700_000, 0, 1_234_567, 2_700_000]}
ODD_CALLS = [[65536, 30001], [4097, 65535, 777], [65536] * 3, [12345], [1, 3], [65536, 65536, 1000]]


@pytest.mark.parametrize("F", [10e6, 6e6], ids=["10M", "6M"])
@pytest.mark.parametrize("cls", ["fast", "r8b"])
def test_same_arithmetic_as_fm_bank(F, cls, monkeypatch):
    """Every channelizer row equals the FM bank's IF (debug tap 0) at the same offsets, call by call, bit for bit: the
    same k_ifr_chan and the same stage-B kernel (the R8B bank's k_ifr_poly5h carries the discriminator epilogue, whose IF
    samples are the plain k_ifr_poly5h's: the stores of the two share the accumulation)."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    offs = FM_OFFS[F]
    n = sum(map(sum, ODD_CALLS))
    x = cb.composite(n, F, offs, list(range(2, 2 + len(offs))), [0.3, 0.1, 0.2, 0.13, 0.25, 0.11][:len(offs)])
    bank = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=65536,
                     max_blocks=4, resampler_class=CLS[cls], channel_offsets_hz=offs)
    cz = fmr.Channelizer(F, offs, resampler_class=CLS[cls], max_blocks=4)
    pos = 0
    for ll in ODD_CALLS:
        m = sum(ll)
        bank.process_blocks(x[pos:pos + m], ll)
        rows, olen = cz.resample_blocks(x[pos:pos + m], ll)
        for s in range(len(offs)):
            tap = bank.debug_read(0, stream=s)
            assert len(tap) == rows.shape[1] == int(olen.sum()), (ll, s)
            assert np.array_equal(rows[s], tap), (ll, s, rel(rows[s], tap) if len(tap) else 0.0)
        pos += m
    assert cz.channel_bank_forms() == bank.channel_bank_forms() == {"modtap"}
    assert cz._L.fmr_resampler_info(cz.h, 6) == 0
    stage_b = cz.front_end_forms()
    assert stage_b == {"poly4"} if cls == "fast" else stage_b == {"poly5h"}, stage_b
    bank.close(); cz.close()


# (input rate, output rate, class): the FM IF rate, the AM rate from 2.4 MS/s, and rates that are neither
HOST_MIX = [(10e6, 384e3, "fast"), (10e6, 384e3, "r8b"), (2.4e6, 48e3, "fast"), (2.4e6, 48e3, "r8b"),
            (10e6, 250e3, "fast"), (6e6, 200e3, "r8b")]


@pytest.mark.parametrize("F, out, cls", HOST_MIX, ids=[f"{F / 1e6:g}M_{o / 1e3:g}k_{c}" for F, o, c in HOST_MIX])
def test_against_mixing_on_the_host(F, out, cls):
    """Each row against a plain front-end-only chain fed cb.mix_down(x, f, F) (float64 phasor): equal lengths, rel RMS
    below 2e-6 (the bank tests' bound)."""
    edge = int((F - out) // 2)
    offs = [-edge + 1000, -int(0.31 * F), 0, 77_777, edge - 5000]
    calls = [[65536] * 3, [40000, 1234], [65536] * 2]
    n = sum(map(sum, calls))
    x = cb.composite(n, F, offs, [3, 5, 7, 9, 11], [0.3, 0.1, 0.2, 0.15, 0.25])
    cz = fmr.Channelizer(F, offs, output_rate=out, resampler_class=CLS[cls], max_blocks=3)
    rows, lens = run_rows(cz, x, calls)
    assert cz.channel_bank_forms() == {"modtap"}
    for s, f in enumerate(offs):
        ref = plain_rows(F, out, CLS[cls], cb.mix_down(x, f, F), calls)
        assert len(rows[s]) == len(ref) == sum(lens) > 0, (s, len(rows[s]), len(ref))
        assert rel(rows[s], ref) < 2e-6, (s, f, rel(rows[s], ref))
    cz.close()


@pytest.mark.parametrize("cls", ["fast", "r8b"])
def test_call_cuts(cls):
    """One capture as uniform 65536-sample calls and as irregular ones: the same total length, rows within 1e-6 rel RMS
    (a phase slip across calls would show far above that)."""
    F = 10e6
    offs = [-3_333_333, 1_000_003, 4_000_001]
    n = 24 * 65536
    x = cb.composite(n, F, offs, [4, 6, 8], [0.3, 0.2, 0.1])
    uniform = [[65536]] * 24
    cuts, rest, i = [], n, 0
    pattern = [1, 4097, 65535, 30000, 7, 65536, 12289, 333, 50000]
    while rest > 0:
        b = min(pattern[i % len(pattern)], rest)
        cuts.append([b])
        rest -= b
        i += 1
    a, la = run_rows(fmr.Channelizer(F, offs, resampler_class=CLS[cls]), x, uniform)
    b, lb = run_rows(fmr.Channelizer(F, offs, resampler_class=CLS[cls]), x, cuts)
    assert sum(la) == sum(lb)
    for s in range(len(offs)):
        assert len(a[s]) == len(b[s]) and rel(b[s], a[s]) < 1e-6, (s, rel(b[s], a[s]))


def test_device_path_and_capacity_refusal():
    """resample_blocks_device with sync=0 into torch buffers, then synchronize(), equals the host path bit for bit; a call
    refused for want of room leaves the state unchanged, and its retry gives the uninterrupted rows."""
    import torch
    F, blk, nb, ncall = 10e6, 65536, 4, 5
    offs = [-2_000_000, 0, 3_000_000]
    x = cb.composite(blk * nb * ncall, F, offs, [2, 4, 6], [0.3, 0.2, 0.1])
    calls = [[blk] * nb] * ncall
    host, lens = run_rows(fmr.Channelizer(F, offs, max_blocks=nb), x, calls)
    dev = fmr.Channelizer(F, offs, max_blocks=nb)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    ostride = blk * nb // 20 + 64
    d_out = torch.full((ncall, len(offs), 2 * ostride), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()          # (the fill runs on torch's stream, the chain on its own)
    olens = []
    for c in range(ncall):
        olens.append(dev.resample_blocks_device(d_x.data_ptr() + 8 * c * blk * nb, [blk] * nb, d_out[c].data_ptr(), ostride))
    dev.synchronize()
    o = d_out.cpu().numpy().view(np.complex64)
    for s in range(len(offs)):
        g = np.concatenate([o[c, s, :int(olens[c].sum())] for c in range(ncall)])
        assert np.array_equal(g, host[s]), s
    for c in range(ncall):      # nothing written past a row's samples
        assert np.isnan(o[c, :, int(olens[c].sum()):]).all(), c
    assert [int(v) for ol in olens for v in ol] == lens
    # refusal and retry, through both paths
    retry = fmr.Channelizer(F, offs, max_blocks=nb)
    d_small = torch.zeros((len(offs), 2 * 100), dtype=torch.float32, device="cuda")
    got = [[] for _ in offs]
    for c in range(ncall):
        seg = x[c * blk * nb:(c + 1) * blk * nb]
        if c == 2:
            with pytest.raises(fmr.FmrError, match="out_stride"):
                retry.resample_blocks_device(d_x.data_ptr() + 8 * c * blk * nb, [blk] * nb, d_small.data_ptr(), 100)
            rc = retry._L.fmr_resample_blocks(retry.h, seg.ctypes.data, 0, (fmr.C.c_uint32 * nb)(*[blk] * nb), nb,
                                              np.zeros(len(offs) * 100, np.complex64).ctypes.data, 100, None)
            assert rc == fmr.ERR_CAPACITY
        out, _ = retry.resample_blocks(seg, [blk] * nb)
        for s in range(len(offs)):
            got[s].append(out[s])
    for s in range(len(offs)):
        assert np.array_equal(np.concatenate(got[s]), host[s]), s


@pytest.mark.parametrize("F, out, cls", [(10e6, 384e3, "fast"), (10e6, 384e3, "r8b"), (2.4e6, 48e3, "fast")])
def test_plain_chain_batched_path(F, out, cls):
    """An S = 3 front-end-only chain through fmr_resample_blocks equals three one-stream chains through fmr_resample,
    bit for bit (the same blocks).  FAST: calls of several blocks (every output of its forms is the same sum whatever the
    call's cut).  R8B: one block per call, because its fp16-split matrix-core forms scale each call-relative tile by
    the power of two of its own maximum, so a different cut may round the last bit differently."""
    calls = [[65536, 30000, 65536], [65536], [50000, 65536, 20000]]
    if cls == "r8b":
        calls = [[b] for ll in calls for b in ll]
    n = sum(map(sum, calls))
    u = [cb.composite(n, F, [f], [i], [0.3]) for f, i in [(0, 3), (250_000, 5), (-400_000, 7)]]
    multi = fmr.Chain(mode=fmr.MODE_NONE, input_rate=F, enable_resampler=True, output_rate=out, resampler_class=CLS[cls],
                      n_streams=3, max_block_len=65536, max_blocks=3)
    rows, pos = [[] for _ in u], 0
    for ll in calls:
        m = sum(ll)
        o, olen = multi.resample_blocks(np.stack([v[pos:pos + m] for v in u]), ll)
        for s in range(3):
            rows[s].append(o[s])
        pos += m
    for s in range(3):
        ref = plain_rows(F, out, CLS[cls], u[s], calls)
        g = np.concatenate(rows[s])
        assert len(g) == len(ref) > 0 and np.array_equal(g, ref), (s, len(g), len(ref))
    multi.close()


def test_nan_in_the_capture(monkeypatch):
    """NaN samples in the capture: the rows equal the FM bank's IF NaN for NaN; outside the NaN's support window (the
    oracle's tap support, widened by the two banded stage-B tiles of 3072 IF samples it may touch) they match the plain
    chains fed the host-mixed capture and hold no NaN."""
    monkeypatch.setenv("FMR_DEBUG_TAPS", "1")
    F, blk, nb = 10e6, 65536, 8
    offs = [-3_000_000, 0, 2_600_000]
    x = cb.composite(blk * nb, F, offs, [3, 6, 12], [0.3, 0.15, 0.2])
    k1 = 5 * blk + 4321
    x[k1:k1 + 3] = np.complex64(complex(np.nan, np.nan))
    bank = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=blk, max_blocks=nb,
                     channel_offsets_hz=offs)
    bank.process_blocks(x, [blk] * nb)
    cz = fmr.Channelizer(F, offs, max_blocks=nb)
    rows, _ = cz.resample_blocks(x, [blk] * nb)
    for s, f in enumerate(offs):
        tap = bank.debug_read(0, stream=s)
        assert np.array_equal(rows[s], tap, equal_nan=True), s
        u = cb.mix_down(x, f, F)
        ora_if = ora.IfResampler(F, 384e3)
        support = np.flatnonzero(~np.isfinite(np.concatenate([ora_if.process(u[i * blk:(i + 1) * blk]) for i in range(nb)])))
        assert support.size
        lo, hi = support[0] - 2 * 3072, support[-1] + 2 * 3072
        bad = np.flatnonzero(~np.isfinite(rows[s]))
        assert bad.size and bad[0] >= lo and bad[-1] <= hi, (s, bad[:3], bad[-3:], lo, hi)
        ref = plain_rows(F, 384e3, fmr.RESAMPLER_FAST, u, [[blk]] * nb)
        assert len(ref) == rows.shape[1]
        keep = np.ones(len(ref), bool)
        keep[max(lo, 0):hi + 1] = False
        assert np.isfinite(ref[keep]).all()
        assert rel(rows[s][keep], ref[keep]) < 2e-6, (s, rel(rows[s][keep], ref[keep]))
    bank.close(); cz.close()


def test_fmr_resample_on_a_channelizer():
    """fmr_resample on a one-channel channelizer equals its resample_blocks row; with more channels it is refused by
    name."""
    F, blk = 6e6, 65536
    x = cb.composite(6 * blk, F, [1_500_000], [4], [0.3])
    one = fmr.Channelizer(F, [1_500_000])
    two = fmr.Channelizer(F, [1_500_000])
    a = np.concatenate([one.resample(x[i * blk:(i + 1) * blk]) for i in range(6)])
    b, _ = run_rows(two, x, [[blk]] * 6)
    assert len(a) > 0 and np.array_equal(a, b[0])
    with pytest.raises(fmr.FmrError, match="fmr_resample_blocks"):
        fmr.Channelizer(F, [0, 1_500_000]).resample(x[:blk])

"""The reference side of tests/test_gpu_rds_front_end.py, without a GPU: the call schedules, rds_bounds.window_scatter,
rds_bounds.tracked_timing, and oracle_mpx + blind on the cheapest capture of the table (912 kS/s)."""
import numpy as np
import pytest

import rds_bounds as rb
import rds_fixture as rf
import rds_reference as rr
import test_gpu_rds_front_end as fe


def test_ragged_calls_hold_the_edges():
    for name, (F, blk, per, _) in fe.CASES.items():
        n = fe.n_input(F, rb.windows_len(fe.NWIN))
        calls = fe.ragged_calls(n, blk, per, seed=sum(map(ord, name)))
        lens = [b for ll in calls for b in ll]
        assert sum(lens) == n and all(1 <= len(ll) <= per for ll in calls) and all(1 <= b <= blk for b in lens), name
        assert calls[0] == [1] and calls[1] == [3] and 1 in calls[2] and blk in calls[2], name     # a ragged first IF count
        assert any(len(ll) >= 2 and set(ll) == {blk} for ll in calls), name                       # the tiled forms' calls
        assert any(0 < b < blk and b not in (1, 3, 5) for b in lens), name


def test_window_scatter_sees_one_window():
    """A known MPX: the scatter is the receiver's own (below 1e-4 of the level and 1e-4 rad); 1 % more subcarrier and 10 mrad
    over one window's samples show up in that window, at that size."""
    n = rb.windows_len(8)
    groups = rf.ps_groups(0x5CA7, "SCATTER", n=int(n / fe.FS / (104 * rf.TD)) + 2)
    t = np.arange(n) / fe.FS
    prog = rf.programme(t, "stereo")
    base = rf.rds_baseband(t, groups, 0.002)
    mpx = prog + 2.0 / 75 * base * np.cos(2 * np.pi * 57000.0 * t - np.pi / 2)
    b = rr.blind(mpx)
    lev, ph = rb.window_scatter(mpx, b)
    assert len(lev) == len(ph) >= 7 and np.abs(lev).max() < 1e-4 and np.abs(ph).max() < 1e-4, (lev, ph)
    tau = b["t0"] * fe.FS
    k0 = rr._symbol_range(n, tau)[0]
    w = 3
    sel = (np.arange(n) >= tau + (k0 + 64 * w + 4) * fe.SPS) & (np.arange(n) < tau + (k0 + 64 * w + 60) * fe.SPS)
    bent = prog + 2.0 / 75 * base * np.where(sel, 1.01, 1.0) * np.cos(2 * np.pi * 57000.0 * t - np.pi / 2 + np.where(sel, 0.01, 0.0))
    lev2, ph2 = rb.window_scatter(bent, b)
    assert 0.007 < lev2[w] < 0.011 and 0.007 < ph2[w] < 0.011, (lev2[w], ph2[w])
    others = np.arange(len(lev2)) != w
    assert np.abs(lev2[others]).max() < 1e-3 and np.abs(ph2[others]).max() < 1e-3


def test_oracle_mpx_carries_the_groups():
    """Case f on the CPU: the oracle's MPX has the chain's sample count, and blind finds the transmitted groups on it."""
    name = "f_912k"
    F, blk, per, _ = fe.CASES[name]
    x, _, okw, sent = fe.capture(name)
    lens = [b for ll in fe.ragged_calls(len(x), blk, per, seed=sum(map(ord, name))) for b in ll]
    m = fe.oracle_rows(x, okw, F, lens)[0]
    assert 64 * fe.NWIN + 8 < len(m) / fe.SPS < 64 * (fe.NWIN + 1)
    ref = fe.reference(m)
    words = [g[1] for g in ref["groups"]]
    first = [tuple(g) for g in sent[0]].index(words[0])
    assert len(words) >= 9 and words == [tuple(g) for g in sent[0][first:first + len(words)]]
    assert not any(g[2] for g in ref["groups"]) and ref["wdev"] < 0.2


def test_tracked_timing_halves_a_delay_step():
    """A known MPX whose first three windows arrive 40 samples early (a whole number: the carrier phase of 57 kHz aside,
    nothing else moves): on its own grid the tracked timing is that of the receiver, below 0.1 sample; against the late
    part's timing it starts 40 samples off and halves window by window behind the step; and fe.tracked_shift reads it, signed,
    at the window a sample lies in, zero without a track."""
    n = rb.windows_len(9)
    groups = rf.ps_groups(0x5CA8, "TRACKED", n=int(n / fe.FS / (104 * rf.TD)) + 2)
    t = np.arange(n) / fe.FS

    def mpx(t0):
        return rf.programme(t, "stereo") + 2.0 / 75 * rf.rds_baseband(t, groups, t0) * np.cos(2 * np.pi * 57000.0 * t - np.pi / 2)
    step, late = int(3 * 64 * fe.SPS), mpx(0.002)
    tau = 0.002 * fe.FS
    flat = rb.tracked_timing(late, tau)
    assert len(flat) == 9 and np.abs(flat).max() < 0.1, flat
    stepped = np.where(np.arange(n) < step, mpx(0.002 - 40 / fe.FS), late)
    tr = rb.tracked_timing(stepped, tau)
    assert np.abs(tr[:3] + 40).max() < 0.5, tr
    assert np.abs(tr[3:] + 40 * 0.5 ** np.arange(1, 7)).max() < 0.5, tr
    at = np.array([(64 * 4 + 10) * fe.SPS, (64 * 6 + 32) * fe.SPS])
    assert np.array_equal(fe.tracked_shift(tr, at), tr[[4, 6]]) and not fe.tracked_shift(None, at).any()      # (signed)
    with pytest.raises(AssertionError):
        fe.tracked_shift(tr, [64 * 5 * fe.SPS + 10.0])                   # within a symbol of an edge: no one window

"""RDS error correction in numpy, on the decisions of the float64 receiver tests/rds_reference.py: the numerical reference
of the library's burst trapping and soft-decision block repair ("Error correction").

Written from the rules as the design states them, not from host/fmradion_rds.hpp; the syndromes come from the parity-check
matrix printed in the standard (rds_fixture.H_ROWS).

    The error syndrome of a block is its syndrome xor the syndrome of the offset word expected at its position.
    burst   the error syndrome is looked up among all bursts of up to max_burst bits (first and last bit of the burst set).
    soft    the block's 26 bits depend on 27 symbols (bit i = e[i] xor e[i + 1]); each has a reliability |rho|, the
            receiver's soft value over its level.  The soft_symbols least reliable are flipped in every non-empty
            combination: a symbol toggles its two bits, an edge symbol the one bit it has in the block.  Of the
            combinations that give the expected syndrome the one with the smallest summed |rho| is kept, and accepted if
            that sum is at most soft_max_cost.
    C / C'  position 3 takes the offset block B's version bit names when B is good or corrected, otherwise both; the
            shorter burst / lower cost wins, a tie goes to C.
Blocks are decoded independently, at the block synchronisation rds_reference.blind found for the capture.
"""
import itertools

import numpy as np

import rds_fixture as rf
import rds_reference as rr

OFF, BURST, SOFT = 0, 1, 2
OK, CORRECTED, BAD, CPRIME = 0, 1, 2, 4
_SYN = {k: rf.syndrome(v) for k, v in rf.OFFSETS.items()}
_NAMES = (("A",), ("B",), ("C", "Cp"), ("D",))


def burst_table(max_len=5):
    """syndrome -> (length, pattern) of every burst of up to max_len bits in a 26-bit block (bit 25 = first on air)."""
    tab = {}
    for ln in range(1, max_len + 1):
        for inner in itertools.product((0, 1), repeat=max(ln - 2, 0)):
            shape = [1] if ln == 1 else [1, *inner, 1]
            for at in range(26 - ln + 1):
                pat = sum(b << (25 - at - i) for i, b in enumerate(shape))
                s = rf.syndrome(pat)
                assert s not in tab, "two bursts of up to five bits share a syndrome"
                tab[s] = (ln, pat)
    return tab


_BURSTS = burst_table()


def _burst_fix(err_syn, max_burst):
    hit = _BURSTS.get(err_syn)
    return (float(hit[0]), hit[1]) if hit is not None and hit[0] <= max_burst else None


def _soft_fix(err_syn, rel27, soft_symbols, soft_max_cost):
    """rel27: |rho| of the symbols e[0 .. 26] of the block.  Symbol j toggles the bits on air j - 1 and j that exist."""
    order = np.argsort(rel27, kind="stable")[:soft_symbols]
    pats = [((1 << (26 - j)) if j >= 1 else 0) | ((1 << (25 - j)) if j <= 25 else 0) for j in order]
    best = None
    for mask in range(1, 1 << len(order)):
        pat, cost = 0, 0.0
        for q in range(len(order)):
            if mask >> q & 1:
                pat ^= pats[q]
                cost += float(rel27[order[q]])
        if rf.syndrome(pat) == err_syn and (best is None or cost < best[0]):
            best = (cost, pat)
    return best if best is not None and best[0] <= soft_max_cost else None


def correct_blocks(bits, rel, first_bit, slot, mode, max_burst=2, soft_symbols=4, soft_max_cost=1.0):
    """bits: the data bits d[i] = e[i] xor e[i + 1]; rel: |rho| of e[i] (len(bits) + 1); first_bit / slot: index into bits
    and group position 0..3 of every block, in order.  Returns (status, info) per block."""
    status = np.zeros(len(first_bit), dtype=np.int64)
    info = np.zeros(len(first_bit), dtype=np.int64)
    b_state = None                                         # (status, version bit) of the current group's block B
    for n, (fb, sl) in enumerate(zip(first_bit, slot)):
        word = int("".join(map(str, bits[fb:fb + 26])), 2)
        syn = rf.syndrome(word)
        info[n] = word >> 10
        if sl == 0:
            b_state = None
        exact = [name for name in _NAMES[sl] if syn == _SYN[name]]
        if exact:
            status[n] = CPRIME if exact[0] == "Cp" else OK
        else:
            status[n] = BAD
            if mode != OFF:
                names = _NAMES[sl]
                if sl == 2 and b_state is not None and not b_state[0] & BAD:
                    names = ("Cp",) if b_state[1] else ("C",)
                cands = []
                for name in names:
                    es = syn ^ _SYN[name]
                    fix = _soft_fix(es, rel[fb:fb + 27], soft_symbols, soft_max_cost) if mode == SOFT \
                        else _burst_fix(es, max_burst)
                    if fix is not None:
                        cands.append((fix[0], name, fix[1]))
                if cands:
                    key, name, pat = min(cands, key=lambda c: c[0])     # (min keeps the first of equals: C before C')
                    status[n] = CORRECTED | (CPRIME if name == "Cp" else 0)
                    info[n] = (word ^ pat) >> 10
        if sl == 1:
            b_state = (int(status[n]), (int(info[n]) >> 11) & 1)
    return status, info


def blind_symbols(mpx):
    """rds_reference.blind's result, plus what it decided on: "bits" (the data bits of its symbols, differentially
    decoded), "rho" (its soft values over its level; rho[i], rho[i + 1] are the symbols of bits[i]) and "first_bit" (index
    into bits of every block of block_start / block_slot).  blind keeps its soft values to itself, so they are formed
    here again from its estimates with its own functions; its correlator output is computed once and handed to it."""
    y = rr.matched(mpx)
    keep = rr.matched
    rr.matched = lambda m, *a: y if (m is mpx and not a) else keep(m, *a)
    try:
        b = rr.blind(mpx)
    finally:
        rr.matched = keep
    tau = b["t0"] * rr.FS
    k = rr._symbol_range(len(y), tau)
    pos = tau + k * rr.SPS
    s = rr.sample(y, pos)
    t_sym = (pos + rr.SPS / 4) / rr.FS
    # blind's phase is known modulo pi only: a turn by pi flips every soft value, which changes neither |rho| nor a bit
    soft = (s * np.exp(-1j * (b["phase"] + 2 * np.pi * b["f_off"] * t_sym))).real
    e = (soft < 0).astype(np.uint8)
    bits = e[1:] ^ e[:-1]
    first_bit = np.round((b["block_start"] - pos[1]) / rr.SPS).astype(np.int64)
    words = np.array([int("".join(map(str, bits[i:i + 16])), 2) for i in first_bit], dtype=np.int64)
    assert np.array_equal(words, b["block_info"]), "the decisions formed here are not blind's"
    return dict(b, bits=bits, rho=soft / b["level"], first_bit=first_bit, symbol_pos=pos)


def counts(sym, groups, t0, lo_group, hi_group, mode, **kw):
    """Over the blocks of the groups lo_group .. hi_group - 1 (numbered from the transmitter's first, whose first bit
    starts at t0 [s]): (blocks that are bad or that the receiver did not reach, corrected blocks whose 16 bits are not the
    ones sent, corrected blocks)."""
    status, info = correct_blocks(sym["bits"], np.abs(sym["rho"]), sym["first_bit"], sym["block_slot"], mode, **kw)
    blk = np.round((sym["block_start"] - t0 * rr.FS) / (26 * rr.SPS)).astype(int)
    lo, hi = 4 * lo_group, 4 * hi_group
    inside = (blk >= lo) & (blk < hi)
    sent = np.array([g[b % 4] for b in blk[inside] for g in (groups[b // 4],)], dtype=np.int64)
    st, inf = status[inside], info[inside]
    bad = int(np.sum((st & BAD) != 0)) + (hi - lo - len(set(blk[inside].tolist())))
    corrected = (st & CORRECTED) != 0
    return bad, int(np.sum(corrected & (inf != sent))), int(corrected.sum())

"""RDS error correction without a GPU: burst trapping and soft-decision block repair of host/fmradion_rds.hpp, driven
through tests/rds_fec_check.cpp with blocks from the independent encoder of tests/rds_fixture.py; and the argument checks
of fmr_set_rds_correction that need no device."""
import ctypes as C
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rds_fixture as rf
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")

OFF, BURST, SOFT = fmr.RDS_FEC_OFF, fmr.RDS_FEC_BURST, fmr.RDS_FEC_SOFT
OK, CORR, BAD, CP = fmr.RDS_OK, fmr.RDS_CORRECTED, fmr.RDS_BAD, fmr.RDS_CPRIME
HOST = os.path.join(ROOT, "airspy-fmradion_amd", "host")


def _compile(tmp, name):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{HOST}", os.path.join(ROOT, "tests", name + ".cpp"),
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("rdsfec"), "rds_fec_check")


@pytest.fixture(scope="module")
def plain_checker(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("rdssync"), "rds_sync_check")


class St:
    def __init__(self, f):
        self.synced, self.blocks_ok, self.blocks_corrected, self.blocks_bad, self.groups_decoded, self.groups_dropped = \
            (int(v) for v in f)


def _parse_groups(text):
    rows = [ln.split()[1:] for ln in text.splitlines() if ln.startswith("G ")]
    out = np.zeros(len(rows), dtype=fmr.RDS_GROUP)
    for i, f in enumerate(rows):
        out[i]["sample_index"] = int(f[0])
        out[i]["block"] = [int(v) for v in f[1:5]]
        out[i]["status"] = [int(v) for v in f[5:9]]
    return out


def decode(exe, bits, rel=None, mode=OFF, max_burst=2, soft_symbols=4, soft_max_cost=1.0, switch=None):
    """The library's decoder on a bit vector (rel: |rho| per bit, negative = pushed without): (groups, counters)."""
    with tempfile.TemporaryDirectory() as d:
        bp = os.path.join(d, "bits")
        np.asarray(bits, dtype=np.uint8).tofile(bp)
        rp = "-"
        if rel is not None:
            rp = os.path.join(d, "rel")
            np.asarray(rel, dtype="<f4").tofile(rp)
        args = [exe, bp, rp, str(mode), str(max_burst), str(soft_symbols), repr(float(soft_max_cost))]
        if switch is not None:
            args += [str(switch[0]), str(switch[1])]
        r = subprocess.run(args, capture_output=True, text=True, check=True)
    assert "T 1" in r.stdout.splitlines()          # bursts of up to five bits have distinct syndromes
    st = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("S ")][0]
    return _parse_groups(r.stdout), St(st)


# ---- streams of 26-bit words ------------------------------------------------------------------------------------------
def words_of(g, third=None):
    """The four 26-bit words of group g (block 3 with the offset its version bit names, or `third`)."""
    a, b, c, d = (int(v) & 0xFFFF for v in g)
    third = third or ("Cp" if (b >> 11) & 1 else "C")
    return [rf.block_word(a, "A"), rf.block_word(b, "B"), rf.block_word(c, third), rf.block_word(d, "D")]


def bits_of(words):
    w = np.asarray(words, dtype=np.int64)
    return ((w[:, None] >> (25 - np.arange(26))[None, :]) & 1).astype(np.uint8).reshape(-1)


def group_a(i):
    return (0xC0DE, (2 << 12) | (10 << 5) | (i & 15), (0x4100 + 37 * i) & 0xFFFF, (0x2020 + 101 * i) & 0xFFFF)


def group_b(i):
    return (0xC0DE, (2 << 12) | (1 << 11) | (10 << 5) | (i & 15), 0xC0DE, (0x3030 + 53 * i) & 0xFFFF)


def all_bursts(max_len):
    """(length, 26-bit pattern) of every burst of up to max_len bits at every place of a block."""
    out = []
    for ln in range(1, max_len + 1):
        for mid in range(1 << max(ln - 2, 0)):
            shape = 1 if ln == 1 else (1 << (ln - 1)) | (mid << 1) | 1
            out += [(ln, shape << at) for at in range(26 - ln + 1)]
    return out


C_TO_CP = 0b11001 << 20                          # syndrome(C_TO_CP) == syndrome(C) ^ syndrome(C')
LEAD = 2                                         # clean groups in front: acquisition on the first one's A and B


@pytest.fixture(scope="module")
def burst_stream():
    """One group per (position A, B, C, D of a version-A group and C' of a version-B group) x (burst of up to 5 bits): the
    words sent, and per group (slot, version B, burst length, pattern)."""
    sent, cases = [], []
    for i in range(LEAD):
        sent.append(words_of(group_a(i)))
    for slot, ver_b in ((0, False), (1, False), (2, False), (3, False), (2, True)):
        for ln, pat in all_bursts(5):
            i = len(sent)
            sent.append(words_of(group_b(i) if ver_b else group_a(i)))
            cases.append((slot, ver_b, ln, pat))
    return np.array(sent, dtype=np.int64), cases


def _received(sent, cases, max_len):
    rx = sent.copy()
    for k, (slot, _, ln, pat) in enumerate(cases):
        if ln <= max_len:
            rx[LEAD + k, slot] ^= pat
    return rx


@pytest.mark.parametrize("max_burst", [1, 2, 3, 4, 5])
def test_every_burst_at_every_place(checker, burst_stream, max_burst):
    """Every burst of up to max_burst bits at every place of A, B, C, C' and D comes back as the information sent, with
    FMR_RDS_CORRECTED; every burst of max_burst + 1 <= 5 bits stays FMR_RDS_BAD with its bits as received.

    One pattern is outside the rule by the code's own construction: the offset words C and C' differ by a word whose
    syndrome is that of the five-bit burst 11001 on the block's first bits (C_TO_CP below).  A block 3 sent with C and hit
    by exactly that burst IS a valid block with C' (and the other way round): no decoder can tell, it is good with the other
    offset's flag and its bits as received, as it is today with correction off."""
    sent, cases = burst_stream
    assert rf.syndrome(C_TO_CP) == rf.syndrome(rf.OFFSETS["C"]) ^ rf.syndrome(rf.OFFSETS["Cp"])
    rx = _received(sent, cases, max_burst + 1)
    out, st = decode(checker, bits_of(rx.reshape(-1)), mode=BURST, max_burst=max_burst)
    assert len(out) == len(sent) and st.synced == 1
    n_corr = n_bad = 0
    for k, (slot, ver_b, ln, pat) in enumerate(cases):
        g = out[LEAD + k]
        want_status = [OK, OK, CP if ver_b else OK, OK]
        want_info = [int(w) >> 10 for w in sent[LEAD + k]]
        if slot == 2 and pat == C_TO_CP and ln <= max_burst + 1:
            want_status[slot] = OK if ver_b else CP
            want_info[slot] = int(rx[LEAD + k, slot]) >> 10
        elif ln <= max_burst:
            want_status[slot] = CORR | (CP if ver_b and slot == 2 else 0)
            n_corr += 1
        elif ln == max_burst + 1:
            want_status[slot] = BAD
            want_info[slot] = int(rx[LEAD + k, slot]) >> 10
            n_bad += 1
        assert [int(v) for v in g["status"]] == want_status, (k, slot, ver_b, ln, bin(pat))
        assert [int(v) for v in g["block"]] == want_info, (k, slot, ver_b, ln, bin(pat))
    assert st.blocks_corrected == n_corr and st.blocks_bad == n_bad and st.blocks_ok == 4 * len(sent) - n_corr - n_bad


def test_off_is_todays_decoder(checker, plain_checker, burst_stream):
    """Mode OFF, with or without reliabilities, and a decoder that was never told anything (tests/rds_sync_check.cpp) print
    the same groups: every hit block FMR_RDS_BAD with its bits as received, nothing corrected."""
    sent, cases = burst_stream
    rx = _received(sent, cases, 2)
    bits = bits_of(rx.reshape(-1))
    with tempfile.TemporaryDirectory() as d:
        bp = os.path.join(d, "bits")
        bits.tofile(bp)
        plain = _parse_groups(subprocess.run([plain_checker, bp], capture_output=True, text=True, check=True).stdout)
    n_hit = sum(ln <= 2 for _, _, ln, _ in cases)
    for rel in (None, np.full(len(bits), 0.01, dtype=np.float32)):
        out, st = decode(checker, bits, rel=rel, mode=OFF)
        assert np.array_equal(out, plain)
        assert st.blocks_corrected == 0 and st.blocks_bad == n_hit and st.synced == 1
    for k, (slot, ver_b, ln, pat) in enumerate(cases):
        want = [OK, OK, CP if ver_b else OK, OK]
        if ln <= 2:
            want[slot] = BAD
        assert [int(v) for v in plain[LEAD + k]["status"]] == want
        assert [int(v) for v in plain[LEAD + k]["block"]] == [int(w) >> 10 for w in rx[LEAD + k]]


# ---- C or C' ----------------------------------------------------------------------------------------------------------
B_KILL = 0b10001 << 8                            # a burst of five bits: beyond max_burst <= 4, block B stays bad
# Error patterns on a block 3 sent with offset C (found by search over all bursts; checked in the test itself):
#   0b101 << 20  a burst of 3 against C, and 0b111 << 22, also 3, against C': a tie
#   0b11 << 23   a burst of 2 against C, and 0b1 << 20, shorter, against C'
TIE_C, TIE_CP = 0b101 << 20, 0b111 << 22
TWO_C, ONE_CP = 0b11 << 23, 0b1 << 20
SYN_D = rf.syndrome(rf.OFFSETS["C"]) ^ rf.syndrome(rf.OFFSETS["Cp"])


def _one_group(checker, words, max_burst):
    sent = [words_of(group_a(i)) for i in range(LEAD)] + [words] + [words_of(group_a(9))]
    out, st = decode(checker, bits_of(np.array(sent).reshape(-1)), mode=BURST, max_burst=max_burst)
    assert len(out) == len(sent)
    return out[LEAD]


@pytest.mark.parametrize("b_good", [True, False])
def test_c_or_cprime(checker, b_good):
    """Block B good (or corrected): only the offset its version bit names is tried.  Block B bad: both, the shorter burst
    wins, a tie goes to C."""
    assert rf.syndrome(TIE_C) ^ SYN_D == rf.syndrome(TIE_CP) and rf.syndrome(TWO_C) ^ SYN_D == rf.syndrome(ONE_CP)
    kill = 0 if b_good else B_KILL
    ga, gb = group_a(5), group_b(5)
    # 1. sent with C, hit by a burst of two that looks like one bit against C'
    w = words_of(ga)
    rx = [w[0], w[1] ^ kill, w[2] ^ TWO_C, w[3]]
    g = _one_group(checker, rx, 2)
    assert int(g["status"][1]) == (OK if b_good else BAD)
    if b_good:
        assert int(g["status"][2]) == CORR and int(g["block"][2]) == ga[2]
    else:
        assert int(g["status"][2]) == CORR | CP and int(g["block"][2]) == (rx[2] ^ ONE_CP) >> 10
    # 2. a tie of two bursts of three: C
    rx = [w[0], w[1] ^ kill, w[2] ^ TIE_C, w[3]]
    g = _one_group(checker, rx, 3)
    assert int(g["status"][2]) == CORR and int(g["block"][2]) == ga[2]
    # ... also when C' was sent (version B): with B bad the tie goes to C, with B good only C' is tried
    w = words_of(gb)
    rx = [w[0], w[1] ^ kill, w[2] ^ TIE_CP, w[3]]
    g = _one_group(checker, rx, 3)
    if b_good:
        assert int(g["status"][2]) == CORR | CP and int(g["block"][2]) == gb[2]
    else:
        assert int(g["status"][2]) == CORR and int(g["block"][2]) == (rx[2] ^ TIE_C) >> 10
    # 3. a version-A group whose block 3 nevertheless carries C', one bit wrong (no burst of up to two against C):
    #    B good names C, so the block stays bad; B bad lets C' in.  A block B that was CORRECTED names its offset too.
    w = words_of(ga, third="Cp")
    for b_err, b_status in ((kill, OK if b_good else BAD), (0b11 << 3, CORR)):
        rx = [w[0], w[1] ^ b_err, w[2] ^ (1 << 5), w[3]]
        g = _one_group(checker, rx, 2)
        assert int(g["status"][1]) == b_status
        if b_status == BAD:
            assert int(g["status"][2]) == CORR | CP and int(g["block"][2]) == ga[2]
        else:
            assert int(g["status"][2]) == BAD and int(g["block"][2]) == rx[2] >> 10


# ---- loss of synchronisation ------------------------------------------------------------------------------------------
def test_corrected_blocks_do_not_hold_the_lock(checker):
    """Eight uncorrectable blocks with a corrected block between each two: the run of bad blocks is neither extended nor
    ended by the corrected ones, and the synchronisation drops at the eighth.  With good blocks in their place it holds."""
    for between, synced in ((0b11 << 7, 0), (0, 1)):
        words = []
        for i in range(LEAD + 4):
            words += words_of(group_a(i))
        for j in range(15):                                   # blocks 0 .. 14 behind the lead: even ones uncorrectable
            words[4 * LEAD + j] ^= B_KILL if j % 2 == 0 else between
        bits = bits_of(words)[:26 * (4 * LEAD + 15)]
        out, st = decode(checker, bits, mode=BURST, max_burst=2)
        assert st.synced == synced and st.blocks_bad == 8, (between, st.synced, st.blocks_bad)
        assert st.blocks_corrected == (7 if between else 0)


# ---- soft mode --------------------------------------------------------------------------------------------------------
def _soft_case(rels, flips, none_at=(), **kw):
    """Four clean groups; in block B of group 2 the symbols at the given places (0 = the symbol before the block's first
    bit ... 26) are flipped; rels {place: |rho|} (1.0 elsewhere); none_at: places whose bit is pushed without reliability."""
    words = []
    for i in range(4):
        words += words_of(group_a(i))
    bits = bits_of(words)
    first = 26 * (4 * 2 + 1)                                  # index of the block's first bit; symbol j belongs to bit first + j - 1
    rel = np.ones(len(bits), dtype=np.float32)
    for j in flips:
        for i in (first + j - 1, first + j):                  # a symbol's own bit and the next one
            bits[i] ^= 1
    for j, v in rels.items():
        rel[first + j - 1] = v
    for j in none_at:
        rel[first + j - 1] = -1.0
    return bits, rel, kw


def test_soft_mode(checker):
    ga = [group_a(i) for i in range(4)]

    def run(bits, rel, kw, mode=SOFT):
        out, st = decode(checker, bits, rel=rel, mode=mode, **kw)
        assert len(out) == 4 and st.synced == 1
        return out, st
    # two separate wrong symbols, the two weakest: repaired (burst mode cannot: two bursts)
    bits, rel, kw = _soft_case({5: 0.1, 15: 0.2, 9: 0.5, 20: 0.6}, flips=(5, 15))
    out, st = run(bits, rel, kw)
    assert int(out[2]["status"][1]) == CORR and tuple(int(v) for v in out[2]["block"]) == ga[2] and st.blocks_corrected == 1
    out, st = run(bits, rel, kw, mode=BURST)
    assert int(out[2]["status"][1]) == BAD and st.blocks_corrected == 0
    # the same with less reliable neighbours that need no flip: the cheapest combination is still the two wrong symbols
    bits, rel, kw = _soft_case({5: 0.3, 15: 0.35, 9: 0.05, 20: 0.01}, flips=(5, 15))
    out, st = run(bits, rel, kw)
    assert int(out[2]["status"][1]) == CORR and tuple(int(v) for v in out[2]["block"]) == ga[2]
    # the repair costs 0.6 + 0.7 > soft_max_cost = 1.0: refused; with soft_max_cost = 1.5 it is taken
    bits, rel, kw = _soft_case({5: 0.6, 15: 0.7}, flips=(5, 15))
    out, st = run(bits, rel, kw)
    assert int(out[2]["status"][1]) == BAD and st.blocks_corrected == 0
    out, st = run(bits, rel, dict(soft_max_cost=1.5))
    assert int(out[2]["status"][1]) == CORR and tuple(int(v) for v in out[2]["block"]) == ga[2]
    # the wrong symbols are not among the soft_symbols least reliable: not found with 2, found with 4
    bits, rel, kw = _soft_case({5: 0.3, 15: 0.35, 9: 0.05, 20: 0.01}, flips=(5, 15), soft_symbols=2)
    out, st = run(bits, rel, kw)
    assert int(out[2]["status"][1]) == BAD
    # a wrong symbol on the edge of two blocks (the symbol of block A's last bit): one bit in each, both repaired
    bits, rel, kw = _soft_case({0: 0.2}, flips=(0,))
    out, st = run(bits, rel, kw)
    assert [int(v) for v in out[2]["status"]] == [CORR, CORR, OK, OK] and tuple(int(v) for v in out[2]["block"]) == ga[2]
    # one wrong symbol that looks reliable while four others look weak: soft mode does not reach it ...
    weak = {4: 0.1, 8: 0.1, 17: 0.1, 23: 0.1}            # (no combination of these has symbol 12's syndrome)
    bits, rel, kw = _soft_case(weak, flips=(12,))
    out, st = run(bits, rel, kw)
    assert int(out[2]["status"][1]) == BAD
    # ... but a block with a bit pushed without reliability is treated in burst mode, which does (a burst of two)
    bits, rel, kw = _soft_case(weak, flips=(12,), none_at=(25,))
    out, st = run(bits, rel, kw)
    assert int(out[2]["status"][1]) == CORR and tuple(int(v) for v in out[2]["block"]) == ga[2]
    # no reliabilities at all: soft mode is burst mode
    out, st = decode(checker, bits, rel=None, mode=SOFT)
    assert int(out[2]["status"][1]) == CORR and st.blocks_corrected == 1


def test_switch_takes_effect_at_a_block_boundary(checker):
    """set_correction in the middle of a block applies from the next block on: a block under way when the mode is switched
    on stays bad, the next one is corrected."""
    words = []
    for i in range(4):
        words += words_of(group_a(i))
    words[9] ^= 0b11 << 4                                     # group 2, block B
    words[10] ^= 0b11 << 4                                    # group 2, block C
    bits = bits_of(words)
    out, st = decode(checker, bits, mode=OFF, switch=(26 * 9 + 13, BURST))
    assert [int(v) for v in out[2]["status"]] == [OK, BAD, CORR, OK] and len(out) == 4
    out, st = decode(checker, bits, mode=OFF, switch=(26 * 9, BURST))          # in front of the block's first bit
    assert [int(v) for v in out[2]["status"]] == [OK, CORR, CORR, OK]


# ---- the C-ABI's argument checks (no device) ---------------------------------------------------------------------------
def _set(fec, size=None, chain=None):
    L = fmr.lib()
    L.fmr_set_rds_correction.restype = C.c_int
    L.fmr_set_rds_correction.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    rc = L.fmr_set_rds_correction(chain, C.byref(fec) if fec is not None else None, C.sizeof(fec) if size is None else size)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("field, kw", [("mode", dict(mode=3)), ("mode", dict(mode=-1)), ("max_burst", dict(max_burst=6)),
                                       ("max_burst", dict(max_burst=-1)), ("soft_symbols", dict(soft_symbols=9)),
                                       ("soft_symbols", dict(soft_symbols=-2)), ("soft_max_cost", dict(soft_max_cost=-0.5)),
                                       ("soft_max_cost", dict(soft_max_cost=float("nan")))])
def test_set_rds_correction_names_the_field(field, kw):
    """The fields are checked before the chain is looked at, so a bad value is refused by name without a device."""
    fmr.build_library()
    args = dict(mode=SOFT, max_burst=0, soft_symbols=0, soft_max_cost=0.0)
    args.update(kw)
    fec = fmr.RdsFec(C.sizeof(fmr.RdsFec), args["mode"], args["max_burst"], args["soft_symbols"], args["soft_max_cost"])
    rc, msg = _set(fec)
    assert rc == fmr.ERR_BAD_ARG and "fmr_set_rds_correction" in msg and field in msg, (rc, msg)


def test_set_rds_correction_size_and_null():
    fmr.build_library()
    fec = fmr.RdsFec(C.sizeof(fmr.RdsFec), SOFT, 0, 0, 0.0)
    rc, msg = _set(fec, size=C.sizeof(fmr.RdsFec) + 8)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg and "larger" in msg, (rc, msg)
    fec.struct_size = C.sizeof(fmr.RdsFec) + 8
    rc, msg = _set(fec)
    assert rc == fmr.ERR_BAD_ARG and "struct_size" in msg, (rc, msg)
    rc, msg = _set(None, size=0)
    assert rc == fmr.ERR_BAD_ARG and "fec" in msg, (rc, msg)
    rc, msg = _set(fmr.RdsFec(C.sizeof(fmr.RdsFec), SOFT, 2, 4, 1.0))          # valid values, no chain
    assert rc == fmr.ERR_BAD_ARG and "chain" in msg, (rc, msg)


def test_declared_and_exported():
    fmr.build_library()
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    assert "int fmr_set_rds_correction(" in hdr and "fmr_set_rds_correction" in fmr.EXPORTS
    assert hasattr(fmr.lib(), "fmr_set_rds_correction")
    assert C.sizeof(fmr.RdsFec) == 24 and (fmr.RDS_FEC_OFF, fmr.RDS_FEC_BURST, fmr.RDS_FEC_SOFT) == (0, 1, 2)
    assert "reserved: burst correction" not in hdr

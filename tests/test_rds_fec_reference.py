"""The numpy reference of the RDS error correction (tests/rds_fec_reference.py) on its own: the rules on constructed
blocks, and its counts on the noisy captures of tests/rds_fec_cases.py, which are the caps the GPU chain is held to in
tests/test_gpu_rds_fec.py (DESIGN.md section 9 holds the table)."""
import numpy as np

import rds_fec_cases as cases
import rds_fec_reference as fr
import rds_fixture as rf


def _stream(gs):
    bits = rf.encode(gs)
    first = 26 * np.arange(len(bits) // 26)
    return bits, first, first // 26 % 4


def test_rules_on_constructed_blocks():
    """Bursts of up to max_burst bits are repaired and longer ones are not; two separate wrong symbols are repaired in soft
    mode when they are the weakest and their cost is within soft_max_cost; C / C' follows block B."""
    gs = rf.ps_groups(0x1234, "REFCHECK", n=6)
    sent = np.array([v for g in gs for v in g])
    bits, first, slot = _stream(gs)
    rel = np.ones(len(bits) + 1)
    hit = bits.copy()
    hit[26 * 5 + 3:26 * 5 + 5] ^= 1                       # a burst of two in block B of group 1
    hit[26 * 11 + 7] ^= 1                                 # 101 in block D of group 2
    hit[26 * 11 + 9] ^= 1
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.OFF)
    assert st[5] == fr.BAD and st[11] == fr.BAD and (st != fr.OK).sum() == 2
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.BURST, max_burst=2)
    assert st[5] == fr.CORRECTED and info[5] == sent[5] and st[11] == fr.BAD
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.BURST, max_burst=3)
    assert st[11] == fr.CORRECTED and np.array_equal(info, sent)
    # soft: symbols e[26 * 13 + 4] and e[26 * 13 + 20] wrong (bits 3, 4 and 19, 20 of block B of group 3)
    hit = bits.copy()
    for j in (4, 20):
        hit[26 * 13 + j - 1:26 * 13 + j + 1] ^= 1
        rel[26 * 13 + j] = 0.3
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.SOFT)
    assert st[13] == fr.CORRECTED and np.array_equal(info, sent)
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.SOFT, soft_max_cost=0.5)
    assert st[13] == fr.BAD
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.BURST, max_burst=2)
    assert st[13] == fr.BAD
    # a block 3 sent with C, hit by 11 on its second and third bit: one bit against C'.  B good: C; B bad: C' (shorter)
    hit = bits.copy()
    hit[26 * 18 + 1:26 * 18 + 3] ^= 1
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.BURST)
    assert st[18] == fr.CORRECTED and info[18] == sent[18]
    hit[26 * 17 + 2] ^= 1
    hit[26 * 17 + 6] ^= 1                                 # 10001 in block B
    st, info = fr.correct_blocks(hit, rel, first, slot, fr.BURST)
    assert st[17] == fr.BAD and st[18] == fr.CORRECTED | fr.CPRIME


def test_counts_on_the_noisy_captures():
    """Three seeds of 20 s at sigma = 0.10, 0.1122 and 0.126: the reference's bad blocks with correction off, bursts of up
    to 2 and soft (4 symbols, cost 1.0), and the corrected blocks with wrong bits.  The caps of tests/test_gpu_rds_fec.py
    are these counts 1 dB up; here the reference is held to them itself.

    Pooled over the seeds, of 2652 blocks (bad / corrected wrong / corrected):
      sigma 0.10    off 301          burst 16 / 1 / 285     soft 3 / 0 / 298
      sigma 0.1122  off 587          burst 57 / 5 / 530     soft 28 / 1 / 559
      sigma 0.126   off 1014         burst 188 / 20 / 826   soft 105 / 2 / 909"""
    n_blocks = 4 * (cases.N_SENT - cases.TAIL_GROUPS - cases.ACQ_GROUPS) * len(cases.SEEDS)
    tab = {}
    for sigma in cases.SIGMA:
        tab[sigma] = {m: tuple(cases.pooled(sigma, m, w) for w in range(3)) for m in cases.MODES}
        print(f"\nsigma {sigma}: of {n_blocks} blocks (bad, corrected wrong, corrected)",
              " ".join(f"{m} {tab[sigma][m]}" for m in cases.MODES))
        print("   per seed:", {seed: cases.reference(seed, sigma) for seed in cases.SEEDS})
    wrong_cap = sum(tab[cases.UP[s]]["burst"][1] for s in cases.UP)
    for sigma, up in cases.UP.items():
        for m in ("burst", "soft"):
            assert tab[sigma][m][0] <= tab[up][m][0], (sigma, m, tab[sigma][m], tab[up][m])
            # what a chain has to do: the cap lies below what detection alone leaves at sigma
            assert tab[up][m][0] < tab[sigma]["off"][0], (sigma, m, tab[up][m], tab[sigma]["off"])
            print(f"cap {m} at {sigma}: {tab[up][m][0]} = {tab[up][m][0] / max(tab[sigma]['off'][0], 1):.3f} of detection only")
    for m in ("burst", "soft"):
        wrong = sum(tab[s][m][1] for s in cases.UP)
        assert wrong <= wrong_cap, (m, wrong, wrong_cap)
    # soft is stronger than trapping, and no less safe, at every level
    for sigma in cases.SIGMA:
        assert tab[sigma]["soft"][0] <= tab[sigma]["burst"][0] <= tab[sigma]["off"][0]
        assert tab[sigma]["soft"][1] <= tab[sigma]["burst"][1]
        assert tab[sigma]["off"][1:] == (0, 0)

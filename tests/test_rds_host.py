"""RDS without a GPU: the data link layer of host/fmradion_rds.hpp (driven through tests/rds_sync_check.cpp) against the
standard's syndromes, block synchronisation at every bit offset, isolated bit errors, a false syndrome during
acquisition, a bit slip and the bounded queue; the parser helpers; and fmr_create_rds's refusals by name before the
device is opened."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import rds_fixture as rf
from conftest import ROOT

fmr = importlib.import_module("airspy-fmradion_amd")

STD_SYNDROMES = {"A": 0x3D8, "B": 0x3D4, "C": 0x25C, "Cp": 0x3CC, "D": 0x258}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rds") / "rds_sync_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}",
                    os.path.join(ROOT, "tests", "rds_sync_check.cpp"), "-o", exe], check=True)
    return exe


class St:
    def __init__(self, f):
        self.synced, self.blocks_ok, self.blocks_bad, self.groups_decoded, self.groups_dropped = (int(v) for v in f)


def decode(exe, bits, idx=None, hold=False):
    """The library's decoder on a bit vector: (groups as an RDS_GROUP array, counters)."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        bp = os.path.join(d, "bits")
        np.asarray(bits, dtype=np.uint8).tofile(bp)
        args = [exe, bp]
        if idx is not None or hold:
            ip = os.path.join(d, "idx")
            np.asarray(np.arange(len(bits)) if idx is None else idx, dtype="<u8").tofile(ip)
            args.append(ip)
        if hold:
            args.append("hold")
        r = subprocess.run(args, capture_output=True, text=True, check=True)
    rows = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("G ")]
    out = np.zeros(len(rows), dtype=fmr.RDS_GROUP)
    for i, f in enumerate(rows):
        out[i]["sample_index"] = int(f[0])
        out[i]["block"] = [int(v) for v in f[1:5]]
        out[i]["status"] = [int(v) for v in f[5:9]]
    st = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("S ")][0]
    return out, St(st)


def groups_of(out):
    return [tuple(int(v) for v in g["block"]) for g in out]


def test_encoder_syndromes_are_the_standards():
    """The encoder's parity-check matrix maps every offset word to the syndrome the standard lists, and every codeword
    (information bits + checkword) to 0."""
    for name, off in rf.OFFSETS.items():
        assert rf.syndrome(off) == STD_SYNDROMES[name], name
    rng = np.random.default_rng(1)
    for m in rng.integers(0, 1 << 16, 500):
        assert rf.syndrome((int(m) << 10) | rf.checkword(int(m))) == 0


def test_library_syndromes_are_the_standards(checker):
    """The library's decoder (its own construction of H) agrees: a group whose block 3 carries C' is reported with
    FMR_RDS_CPRIME, and groups whose blocks carry the wrong offset are not accepted as synchronised."""
    ver_b = [(0x1234, (0 << 12) | (1 << 11) | s, 0x1234, 0x4142 + s) for s in range(4)] * 6
    out, st = decode(checker, rf.encode(ver_b))
    assert len(out) >= len(ver_b) - 2 and st.blocks_bad == 0
    assert all(int(g["status"][2]) == fmr.RDS_CPRIME for g in out)
    # every block with offset A: two consecutive valid syndromes never follow each other, nothing synchronises
    only_a = np.array([(rf.block_word(0x1000 + i, "A") >> (25 - b)) & 1 for i in range(100) for b in range(26)],
                      dtype=np.uint8)
    out, st = decode(checker, only_a)
    assert len(out) == 0 and st.synced == 0


@pytest.mark.parametrize("lead", list(range(0, 104, 1)))
def test_groups_at_every_bit_offset(checker, lead):
    """Any number of leading junk bits: acquisition within two groups, then every group exactly, with the sample index of
    its first bit."""
    rng = np.random.default_rng(lead)
    groups = rf.ps_groups(0xC201, "RADIO 1", rt="HELLO FROM THE TEST ENCODER", n=40)
    bits = np.concatenate([rng.integers(0, 2, lead).astype(np.uint8), rf.encode(groups)])
    idx = (np.arange(len(bits), dtype=np.uint64) * 6144 + 77) // 19           # positions of a 1187.5 Hz symbol clock
    out, st = decode(checker, bits, idx)
    got = groups_of(out)
    assert len(got) >= len(groups) - 2, (lead, len(got))
    first = len(groups) - len(got)
    assert got == [tuple(g) for g in groups[first:]]
    assert [int(g["sample_index"]) for g in out] == [int(idx[lead + 104 * (first + i)]) for i in range(len(got))]
    assert all(int(s) == fmr.RDS_OK for g in out for s in g["status"])
    assert st.synced == 1 and st.blocks_bad == 0 and st.groups_dropped == 0


def test_isolated_bit_errors(checker):
    """An isolated wrong bit spoils exactly its block (flagged bad, the other three blocks of the group intact); the
    synchronisation holds."""
    groups = rf.ps_groups(0xD3A5, "STATION2", n=60)
    bits = rf.encode(groups)
    hit = [10 * 104 + 30, 25 * 104 + 3, 40 * 104 + 80]             # block B of group 10, A of 25, D of 40
    for h in hit:
        bits[h] ^= 1
    out, st = decode(checker, bits)
    assert len(out) == len(groups)                 # (acquired on blocks A and B of the first group: it is kept)
    assert st.blocks_bad == 3 and st.synced == 1
    for h in hit:
        g = out[h // 104]
        bad = [i for i in range(4) if int(g["status"][i]) & fmr.RDS_BAD]
        assert bad == [(h % 104) // 26], (h, bad)
    assert sum(a != tuple(b) for a, b in zip(groups_of(out), groups)) == 3


def test_bit_slip(checker):
    """One bit lost in the middle of the stream: the decoder flags the blocks behind it bad, loses the synchronisation
    after a run of eight, and re-acquires; no more than 4 groups are lost around the slip and every group it returns is
    either flagged or exact."""
    groups = rf.ps_groups(0xE0F1, "SLIPTEST", rt="SOME RADIOTEXT", n=80)
    bits = rf.encode(groups)
    slip = 30 * 104 + 50
    bits = np.delete(bits, slip)
    out, st = decode(checker, bits)
    clean = [g for g in out if all(int(s) == fmr.RDS_OK for s in g["status"])]
    tail = [tuple(int(v) for v in g["block"]) for g in clean if int(g["sample_index"]) > slip]
    want = [tuple(g) for g in groups[31:]]
    assert len(tail) >= len(want) - 4, (len(tail), len(want))
    assert tail == want[len(want) - len(tail):]
    assert st.synced == 1
    assert fmr.rds_ps(out) == "SLIPTEST" and fmr.rds_pi(out) == 0xE0F1


def test_differential_coding_cancels_polarity():
    """Differential decoding of the transmitter's coding gives the data back, and does so for the inverted symbols too
    (the pi ambiguity of a BPSK carrier)."""
    rng = np.random.default_rng(3)
    d = rng.integers(0, 2, 500).astype(np.uint8)
    e = rf.diff_encode(d)
    assert np.array_equal(rf.diff_decode(e), d)
    assert np.array_equal(rf.diff_decode(1 - e, 1)[1:], d[1:])


def test_parser_helpers(checker):
    groups = rf.ps_groups(0x2F1C, "ABCDEFGH", n=8)
    out, _ = decode(checker, rf.encode(groups * 3))
    assert fmr.rds_pi(out) == 0x2F1C
    assert fmr.rds_ps(out) == "ABCDEFGH"
    assert fmr.rds_ps(out[:2]) is None                # not all four segments yet
    assert fmr.rds_pi(out[:0]) is None


def test_queue_is_bounded(checker):
    """Nobody drains the queue: it keeps its newest 256 groups and counts the ones it dropped instead of growing."""
    groups = rf.ps_groups(0x1111, "CAPACITY", n=300)
    out, st = decode(checker, rf.encode(groups), hold=True)
    assert st.groups_decoded == 300 and st.groups_dropped == 44 and len(out) == 256
    assert groups_of(out) == [tuple(g) for g in groups[44:]]


def _false_hit_between_a_and_b():
    """Programme data whose first group has a bit window, ending between the ends of blocks A and B, that carries a valid
    offset syndrome (a false hit that a decoder remembering only its last hit would take instead of block A)."""
    syn = {rf.syndrome(v) for v in rf.OFFSETS.values()}
    for pi in range(0x1000, 0x2000):
        groups = rf.ps_groups(pi, "FALSEHIT", n=16)
        bits = rf.encode(groups)
        for e in range(27, 52):
            w = int("".join(map(str, bits[e - 26:e])), 2)
            if rf.syndrome(w) in syn:
                return groups, bits
    raise AssertionError("no data with a false syndrome found")


def test_false_syndrome_during_acquisition(checker):
    """Acquisition remembers a valid syndrome per bit phase: a false hit between the true blocks A and B does not hide
    block A, so the first group is kept."""
    groups, bits = _false_hit_between_a_and_b()
    out, st = decode(checker, bits)
    assert groups_of(out) == [tuple(g) for g in groups] and st.synced == 1


def test_acquisition_on_d_then_a_keeps_the_next_group(checker):
    """Bits that start inside block C: acquisition on D-A (or C-D) loses only the group it started in."""
    groups = rf.ps_groups(0x4242, "DAPAIR!!", n=12)
    bits = rf.encode(groups)[60:]                                  # first bits: the middle of block C of group 0
    out, st = decode(checker, bits)
    assert groups_of(out) == [tuple(g) for g in groups[1:]]


def test_header_compiles_for_cpp_callers(tmp_path):
    """host/fmradion_rds.hpp is plain C++17 (no HIP): a caller's own program runs the decoder and the parser."""
    src = tmp_path / "rds_check.cpp"
    words = []
    for g in rf.ps_groups(0x5A5A, "CPPCHECK", n=12):
        words += [int(b) for b in rf.group_bits(g)]
    src.write_text(
        '#include <cstdio>\n#include "fmradion_rds.hpp"\n'
        "static const unsigned char bits[] = {" + ",".join(map(str, words)) + "};\n"
        "int main() {\n  fmr_rds::Decoder d; fmr_rds::Station st;\n"
        "  for (size_t i = 0; i < sizeof bits; i++) d.push(bits[i], i);\n"
        "  fmr_rds_group g[32]; size_t n = d.pop(g, 32);\n  for (size_t i = 0; i < n; i++) st.add(g[i]);\n"
        '  std::printf("%04X %s %zu\\n", st.pi, st.ps.c_str(), n);\n  return st.ps_complete() ? 0 : 1;\n}\n')
    exe = str(tmp_path / "rds_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'airspy-fmradion_amd', 'host')}",
                    str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["5A5A", "CPPCHECK", "12"], r.stdout


def _cfg(**over):
    import ctypes as C
    cfg = fmr.Config()
    cfg.n_streams, cfg.mode, cfg.input_rate, cfg.enable_resampler = 1, fmr.MODE_FM, 10e6, 1
    cfg.max_block_len, cfg.max_blocks = 65536, 4
    # (a complete decoder configuration: a create refuses a missing filter before it opens the device)
    cfg.filter_coeff, cfg.n_filter_coeff = fmr.DELAY_3TAPS.ctypes.data_as(C.POINTER(C.c_float)), len(fmr.DELAY_3TAPS)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _create_rds(cfg):
    import ctypes as C
    L = fmr.lib()
    L.fmr_create_rds.restype = C.c_int
    L.fmr_create_rds.argtypes = [C.POINTER(fmr.Config), C.c_size_t, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    rc = L.fmr_create_rds(C.byref(cfg), C.sizeof(fmr.Config), C.byref(h))
    if rc == fmr.OK:
        L.fmr_destroy(h)
    return rc, L.fmr_last_error().decode()


@pytest.mark.parametrize("mode", [fmr.MODE_NBFM, fmr.MODE_AM, fmr.MODE_DSB, fmr.MODE_USB, fmr.MODE_LSB, fmr.MODE_CW,
                                  fmr.MODE_WSPR, fmr.MODE_NONE])
def test_rds_refused_for_other_modes(mode):
    """enable_rds on anything but an FM decoder chain is refused by name before the device is opened."""
    fmr.build_library()
    rc, msg = _create_rds(_cfg(mode=mode))
    assert rc == fmr.ERR_UNSUPPORTED and "enable_rds" in msg, (rc, msg)


def test_rds_refused_for_the_channelizer():
    import ctypes as C
    fmr.build_library()
    offs = (C.c_int32 * 2)(-1_000_000, 2_000_000)
    rc, msg = _create_rds(_cfg(mode=fmr.MODE_NONE, n_streams=2, channel_offset_hz=offs))
    assert rc == fmr.ERR_UNSUPPORTED and "enable_rds" in msg and "front-end-only" in msg, (rc, msg)
    with pytest.raises(fmr.FmrError, match="enable_rds"):
        fmr.Chain(mode=fmr.MODE_NONE, input_rate=10e6, enable_resampler=True, enable_rds=True)


@pytest.mark.parametrize("kw", [dict(), dict(enable_resampler=0, input_rate=384e3), dict(stereo=0), dict(in_order=1),
                                dict(resampler_class=fmr.RESAMPLER_R8B), dict(input_rate=10e6 * (1 + 20e-6))])
def test_rds_accepted_for_fm_shapes(kw):
    """FM chains of every shape pass the option's rules (without a GPU they stop where the device is opened)."""
    fmr.build_library()
    rc, msg = _create_rds(_cfg(**kw))
    assert rc == fmr.OK or (rc == fmr.ERR_NO_DEVICE and "no HIP device" in msg), (rc, msg)


def test_declared_and_exported():
    fmr.build_library()
    hdr = open(os.path.join(ROOT, "include", "fmradion_amd.h")).read()
    for name in ("fmr_create_rds", "fmr_get_rds_groups", "fmr_get_rds_status"):
        assert f"int {name}(" in hdr and name in fmr.EXPORTS and hasattr(fmr.lib(), name), name
    assert fmr.RDS_GROUP.itemsize == 24
    assert b"0.4" in fmr.lib().fmr_version()

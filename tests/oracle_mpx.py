"""The MPX the RDS stage is specified to read, from wideband IQ, by the CPU oracle (tests/oracle_py.py).

oracle_mpx runs the oracle's front end and FM decoder block by block, with the chain's own block lengths, and joins the
discriminator output of every block (FmDecoder.debug_vector(0, n)): a float64 array at 384 kHz, in the chain's own sample
count, the group delay of the resampler, the IF filter and the equaliser included.  tests/rds_reference.py on that array is
the reference of tests/test_gpu_rds_front_end.py.  The oracle's discriminator output is float32: it differs from an ideal
one by about 2.4e-7 MPX units, 1e-5 of a 2 / 75 subcarrier.  Not a test module.
"""
import numpy as np

import chanbank_fixture as cb
import oracle_py as ora
from conftest import load_filter

IF_RATE = 384000.0
DELAY_3TAPS = np.array([0.0, 1.0, 0.0], dtype=np.float32)
U8 = 2                                              # fmr.IQ_U8, ora.iq_convert's format number


def _one(x, lens, F, r8b, fourth_down, filter_coeff, multipath_stages, stereo, trace):
    f4 = ora.FourthConverterIQ(False) if fourth_down else None
    rs = ora.IfResampler(F, IF_RATE, 180.0, 0.98, True) if r8b else ora.IfResampler(F, IF_RATE)
    fm = ora.FmDecoder(filter_coeff is not None, DELAY_3TAPS if filter_coeff is None else filter_coeff, stereo, 50.0, False,
                       multipath_stages, load_filter("jj1bdx_48khz_fmaudio"))
    out, pos, n_mpx = [], 0, 0
    for bl in lens:
        b = x[pos:pos + bl]
        pos += bl
        if f4 is not None:
            b = f4.process(b)
        v = rs.process(b)
        fm.process(v)
        m = fm.debug_vector(0, len(v))
        assert len(m) == len(v)
        out.append(m.copy())
        n_mpx += len(m)
        if trace is not None and len(m):
            trace.append((n_mpx, fm.get_multipath_error()))
    return np.concatenate(out) if out else np.zeros(0)


def oracle_mpx(iq_or_rows, lens, F, r8b=False, fourth_down=False, u8=False, offsets_hz=None, filter_coeff=None,
               multipath_stages=0, stereo=True, trace=None):
    """iq_or_rows: one capture [n] (u8: [n, 2]) or rows [S, n] (u8: [S, n, 2]); lens: the block lengths, the same for every
    row; F: the rate the chain is told.  The shape: r8b (the 180 dB resampler class, else FAST), fourth_down (Fs/4 shift
    first), u8 (raw offset binary through ora.iq_convert first), offsets_hz (a channel bank: the one capture is mixed
    down by every offset with chanbank_fixture.mix_down first, one result per offset), filter_coeff (-f: the IF filter),
    multipath_stages (-E), stereo.  trace: a list that receives (MPX samples so far, the equaliser's error) after every
    block that yielded IF samples (one row only).  Returns one float64 array, or a list of them for rows / a bank."""
    x = np.asarray(iq_or_rows)
    rows = x.ndim == (3 if u8 else 2)
    xs = list(x) if rows else [x]
    if u8:
        xs = [ora.iq_convert(U8, r) for r in xs]
    if offsets_hz is not None:
        assert len(xs) == 1
        xs = [cb.mix_down(xs[0], f, F) for f in offsets_hz]
    assert trace is None or len(xs) == 1
    assert sum(lens) <= len(xs[0])
    out = [_one(r, lens, F, r8b, fourth_down, filter_coeff, multipath_stages, stereo, trace) for r in xs]
    return out if rows or offsets_hz is not None else out[0]

"""The output stage (include/fmradion_amd.h, fmr_enable_output) restated in numpy: the definitions of the header, one
block after the other, with no knowledge of calls.  Pure numpy; the GPU tests run it on the audio a chain returned and on
the if_rms its records carry, the CPU tests hold it to hand-computed cases."""
import numpy as np

PCM_S16, PCM_F32 = 0, 1
# fmr_output_block (56 bytes)
RECORD = np.dtype([("block", np.uint64), ("first_frame", np.uint64), ("n_frames", np.uint32), ("channels", np.uint32),
                   ("if_rms", np.float32), ("if_level", np.float32), ("audio_mean", np.float32),
                   ("audio_rms", np.float32), ("audio_level", np.float32), ("gate_open", np.uint32),
                   ("n_clipped", np.uint32), ("n_nonfinite", np.uint32)])


def squelch_level_from_db(db):
    """main.cpp:486"""
    return 10.0 ** (-(db / 20.0))


def to_s16(y):
    """y float64 -> (int16, n_clipped, n_nonfinite): rint(y 32767) half-even, saturated; NaN -> 0."""
    y = np.asarray(y, dtype=np.float64)
    nan = np.isnan(y)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.where(nan, 0.0, y) * 32767.0)
    clipped = (r > 32767.0) | (r < -32768.0)
    out = np.clip(r, -32768.0, 32767.0).astype(np.int16)
    return out, int(clipped.sum()), int((~np.isfinite(y)).sum())


def to_f32(y):
    """y float64 -> (float32, n_clipped, n_nonfinite): passed through; |y| > 1 counted."""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = y.astype(np.float32)
        clipped = np.abs(y) > 1.0
    return out, int(clipped.sum()), int((~np.isfinite(y)).sum())


def narrowed_sums(x, channels):
    """S1 = sum x_f, S2 = sum x_f^2 of the block's doubles (interleaved frames) narrowed to float32, in fp64, in the
    header's order: 256 partials over the frames t, t + 256, ..., a butterfly over each 64, the four results in order."""
    with np.errstate(invalid="ignore", over="ignore"):
        xf = np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1, channels)
    rows = -(-len(xf) // 256)
    v = np.zeros((rows * 256, channels))
    v[:len(xf)] = xf                     # (adding +0.0 to a partial that started at +0.0 changes no bit)
    v = v.reshape(rows, 256, channels)
    s, q = np.zeros(256), np.zeros(256)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            for c in range(channels):
                s = s + v[r, :, c]
                q = q + v[r, :, c] * v[r, :, c]
        lane = np.arange(64)
        out = []
        for p in (s, q):
            w = p.reshape(4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                w = w + w[:, lane ^ o]
            out.append(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])
    return out[0], out[1]


def run(blocks, channels, squelch_level=0.0, gain=0.5, fmt=PCM_S16):
    """blocks: one (if_rms, audio) per block handed in, in order -- if_rms None for a block without IF samples, audio the
    block's doubles (interleaved, possibly empty).  Returns (records RECORD [m], pcm [frames, channels])."""
    ifl = aul = np.float32(0.0)
    recs, pcm, frame = [], [], 0
    conv = to_s16 if fmt == PCM_S16 else to_f32
    for b, (if_rms, audio) in enumerate(blocks):
        if if_rms is None:
            assert len(audio) == 0
            continue
        r = np.float32(if_rms)
        ifl = np.float32(0.75 * float(ifl) + 0.25 * float(r))
        gate = float(r) >= squelch_level
        audio = np.asarray(audio, dtype=np.float64)
        n = len(audio)
        assert n % channels == 0
        rec = np.zeros((), dtype=RECORD)
        rec["block"], rec["first_frame"], rec["n_frames"], rec["channels"] = b, frame, n // channels, channels
        rec["if_rms"], rec["if_level"], rec["gate_open"] = r, ifl, int(gate)
        if n:
            s1, s2 = narrowed_sums(audio, channels)
            with np.errstate(invalid="ignore", over="ignore"):
                rec["audio_mean"] = np.float32(s1 / n)
                rec["audio_rms"] = np.float32(np.sqrt(s2 / n))
                aul = np.float32(0.95 * float(aul) + 0.05 * float(rec["audio_rms"]))
                y = audio * (gain if gate else 0.0)
            out, rec["n_clipped"], rec["n_nonfinite"] = conv(y)
            pcm.append(out.reshape(-1, channels))
            frame += n // channels
        rec["audio_level"] = aul
        recs.append(rec)
    dt = np.int16 if fmt == PCM_S16 else np.float32
    return (np.array(recs, dtype=RECORD) if recs else np.zeros(0, dtype=RECORD),
            np.concatenate(pcm) if pcm else np.zeros((0, channels), dtype=dt))


def ring_window(done, depth, read=0):
    """A ring of `depth` entries after `done` were produced with the reader at `read`: (first readable, newly dropped)."""
    first = max(read, done - depth)
    return first, first - read

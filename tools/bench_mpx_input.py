"""Cost of the MPX input (fmr_create_mpx_decoder): an MPX decoder's step at 384000 F32 ("384k_f32":
convert and store), 192000 S16 ("192k_s16") and 171000 S16 ("171k_s16"), for one stream and for 32 streams.

The method of tools/bench_mpx_output.py: device buffers in and out, one call per step, one synchronisation per step.  A step
is one second of composite per stream -- `rate` frames in blocks of 4096 -- whatever the rate, so every leg decodes the
same 384000 MPX samples per stream and step and the legs differ by their front end alone.  The signal is the composite of
siggen.fm_stereo_mpx resampled by the MPX output's fixture rule in float64 (numpy, once).  The legs are run in rounds
(--repeats), one after the other within a round, so that drift of the machine falls on all of them alike; a leg's figure is
the median of its rounds and its spread their range.
Prints one JSON line per shape: ms per step of every leg (median, min, max) and the medians of the front end's own kernel
times ("mpx_in_copy", "mpx_in_rate", "mpx_in_hist", "mpx_in_stats") from the chain's kernel timing in a separate pass.
Usage: python tools/bench_mpx_input.py [--steps 10] [--warmup 3] [--repeats 3] [--shapes 1 32] [--legs ...] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
fmr = importlib.import_module("airspy-fmradion_amd")
import siggen  # noqa: E402

BLK = 4096
LEGS = {"384k_f32": ("f32", 384000), "192k_s16": ("s16", 192000), "171k_s16": ("s16", 171000)}


def composite(rate):
    """One second of a stereo composite at `rate` as float64, |x| < 1 (the tones of siggen.fm_stereo_mpx lie below 53 kHz and
    the pilot at 19 kHz: every rate here holds them without a filter)."""
    t = np.arange(rate, dtype=np.float64) / rate
    return siggen.fm_stereo_mpx(t, 0)


def frames_of(fmt, rate):
    x = composite(rate)
    return np.rint(x * 0.5 * 32767.0).astype(np.int16) if fmt == "s16" else x.astype(np.float32)


def make(leg, K, nb):
    fmt, rate = LEGS[leg]
    return fmr.MpxChain(rate=rate, format=fmt, gain=2.0 if fmt == "s16" else 1.0, n_streams=K, stereo=True, max_block_len=BLK,
                        max_blocks=nb)


def timed(ch, d_x, stride, bl, d_out, astride, steps, warmup, torch):
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride, sync=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride, sync=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--legs", nargs="+", default=list(LEGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    lines = []
    for K in a.shapes:
        bufs = {}
        for leg in a.legs:
            fmt, rate = LEGS[leg]
            f = frames_of(fmt, rate)
            stride = (len(f) + 15) & ~15                 # rows 16-byte aligned in both formats
            rows = np.zeros((K, stride), dtype=f.dtype)
            rows[:, :len(f)] = f
            bl = [BLK] * (len(f) // BLK) + ([len(f) % BLK] if len(f) % BLK else [])
            bufs[leg] = (torch.from_numpy(rows).cuda(), stride, bl)
        astride = 2 * (48000 + 64 * 128)
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        runs = {leg: [] for leg in a.legs}
        for _ in range(a.repeats):
            for leg in a.legs:
                d_x, stride, bl = bufs[leg]
                ch = make(leg, K, len(bl))
                runs[leg].append(timed(ch, d_x, stride, bl, d_out, astride, a.steps, a.warmup, torch))
                ch.close()
        kt, seen = {}, {}
        for leg in a.legs:
            d_x, stride, bl = bufs[leg]
            ch = make(leg, K, len(bl))
            ch.enable_kernel_timing(1)
            k = {}
            for _ in range(4):
                ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride, sync=True)
                for name, ms in ch.kernel_times():
                    if name.startswith("mpx_in_"):
                        k.setdefault(name, []).append(ms)
            kt[leg] = {n: round(float(np.median(v)), 4) for n, v in k.items()}
            info = ch.mpx_input_info(0)
            seen[leg] = dict(frames_per_step=int(sum(bl)), blocks=len(bl), samples_out=int(info["samples_out"]),
                             taps_per_sample=int(info["taps_per_sample"]), stereo_detected=int(ch.status(0).stereo_detected))
            ch.close()
        ms = {k: [round(float(np.median(v)) * 1e3, 4), round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in runs.items()}
        rec = dict(tool="bench_mpx_input", streams=K, mpx_samples_per_step_and_stream=384000, steps=a.steps, warmup=a.warmup,
                   repeats=a.repeats, ms_per_step_median_min_max=ms, mpx_in_kernels_ms_per_call=kt, last_pass_stream0=seen)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del bufs, d_out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Cost of the MPX output (fmr_enable_mpx_output): the bench-shaped step with the stage off ("off"),
at 384000 F32 ("384k_f32": convert and store), at 192000 S16 ("192k_s16") and at 171000 S16 ("171k_s16"), alone and beside
the other optional stages ("busy_*": RDS, the modulation, audio and RF monitors and the output stage on in every leg).

The shapes and the method of tools/bench_output_rate.py: 10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample
blocks for one stream, and the 32-channel bank of tools/bench_channel_bank.py (2^23 samples per step), device buffers in
and out, asynchronous calls, one synchronisation per step in every leg; every leg with the stage drains its ring once per
step, the ring sized for a step.  The legs are run in rounds (--repeats), one after the other within a round, so that
drift of the machine falls on all of them alike; a leg's figure is the median of its rounds and its spread their range.
Prints one JSON line per shape: ms per step of every leg (median, min, max), the growth over the leg's "off", the bytes of
PCM drained per step and stream, and the medians of the stage's own kernel times ("mpx_copy", "mpx_rate", "mpx_hist") from
the chain's kernel timing in a separate pass.  The yardstick for "off" is bench.py run in a tree of the parent commit.
Usage: python tools/bench_mpx_output.py [--steps 10] [--warmup 3] [--repeats 3] [--shapes 1 32] [--legs ...] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
fmr = importlib.import_module("airspy-fmradion_amd")
import chanbank_fixture as cb  # noqa: E402
import siggen  # noqa: E402

F, BLK, BASE = 10_000_000, 65536, 1 << 23
# leg -> enable_mpx_output's format and rate (None: the stage off)
STAGE = {"off": None, "384k_f32": ("f32", 384000), "192k_s16": ("s16", 192000), "171k_s16": ("s16", 171000)}
LEGS = list(STAGE) + ["busy_" + k for k in STAGE]


def make(leg, nb, frames, mpx_frames, kw):
    busy = leg.startswith("busy_")
    spec = STAGE[leg[5:] if busy else leg]
    ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK, max_blocks=nb,
                   enable_rds=busy, **kw)
    if busy:
        ch.enable_monitor()
        ch.enable_loudness()
        ch.enable_rf_monitor()
        ch.enable_output(squelch_level=0.03, max_frames=frames, max_blocks=min(65536, 2 * nb))
    if spec:
        ch.enable_mpx_output(format=spec[0], rate=spec[1], max_frames=mpx_frames)
    return ch, spec is not None, busy


def drain(ch, K, mpx, busy):
    last = None
    for s in range(K):
        if busy:
            ch.output_read(s)
        if mpx:
            last = ch.mpx_output_read(s)
    return last


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K, mpx, busy):
    bl = [BLK] * nb
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        ch.synchronize()
        drain(ch, K, mpx, busy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        ch.synchronize()                 # every leg: the reads synchronise, the leg without them must not run ahead
        drain(ch, K, mpx, busy)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--legs", nargs="+", default=LEGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench_channel_bank as bcb
    lines = []
    for K in a.shapes:
        st = siggen.fm_stereo_iq(BASE, float(F), amplitude=0.2)
        if K == 1:
            N = 1 << 27
            x = np.tile(st, N // BASE)
            kw = {}
        else:
            N = BASE
            offs = bcb.offsets(K)
            acc = np.zeros(N, dtype=np.complex128)
            for f in dict.fromkeys(offs):
                acc += st * cb.phasor(N, f, F, +1)
            x = acc.astype(np.complex64)
            kw = dict(channel_offsets_hz=offs)
        nb = N // BLK
        d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
        del x
        frames = N * 48000 // F + 64 * nb
        mpx_frames = N * 384000 // F + 64 * nb           # a step's MPX samples at most: the ring holds a step at every rate
        astride = 2 * frames
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        runs = {leg: [] for leg in a.legs}
        for _ in range(a.repeats):
            for leg in a.legs:
                ch, mpx, busy = make(leg, nb, frames, mpx_frames, kw)
                runs[leg].append(timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K, mpx, busy))
                ch.close()
        kt, seen = {}, {}
        for leg in a.legs:
            ch, mpx, busy = make(leg, nb, frames, mpx_frames, kw)
            if mpx:
                ch.enable_kernel_timing(1)
                k = {}
                for _ in range(4):
                    ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
                    ch.synchronize()
                    for name, ms in ch.kernel_times():
                        if name.startswith("mpx_"):
                            k.setdefault(name, []).append(ms)
                    pcm, info = drain(ch, 1, True, busy)
                kt[leg] = {n: round(float(np.median(v)), 4) for n, v in k.items()}
                seen[leg] = dict(pcm_bytes_per_step_and_stream=int(pcm.nbytes), frames=int(len(pcm)), rate=int(info["rate"]),
                                 taps_per_phase=int(info["taps_per_phase"]), samples_in=int(info["samples_in"]),
                                 frames_dropped=int(info["frames_dropped"]), pcm_clipped=int(info["pcm_clipped"]))
            ch.close()
        ms = {k: [round(float(np.median(v)) * 1e3, 4), round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in runs.items()}
        rec = dict(tool="bench_mpx_output", tree=os.path.basename(ROOT), channels=K, samples_per_step=N, steps=a.steps,
                   warmup=a.warmup, repeats=a.repeats, ms_per_step_median_min_max=ms)
        rec["growth_over_off_ms"] = {k: round(v[0] - ms[("busy_off" if k.startswith("busy_") else "off")][0], 4)
                                     for k, v in ms.items()
                                     if k not in ("off", "busy_off") and ("busy_off" if k.startswith("busy_") else "off") in ms}
        rec["mpx_kernels_ms_per_call"] = kt
        rec["last_pass_ch0"] = seen
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del d_x, d_out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

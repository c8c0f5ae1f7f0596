"""Cost of the output stage's rate converter (fmr_set_output_rate): the bench-shaped step with
the stage off ("off"), on at the decoder's 48 kHz stereo S16 ("48k": the stage of section 14 as it is), at 16 kHz mono F32
("16k_mono_f32") and at 44.1 kHz stereo S16 ("44k1_s16").

The shapes and the method of tools/bench_output.py: 10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample
blocks for one stream, and the 32-channel bank of tools/bench_channel_bank.py (2^23 samples per step), device buffers in
and out, asynchronous calls, one synchronisation per step in every leg; every leg with the stage drains its frames and
records once per step, the ring sized for a step.  Prints one JSON line per shape: ms per step of every leg, the growth
over "48k", the bytes of PCM drained per step and stream, and the medians of the stage's own kernel times ("out_pcm",
"out_blocks", "out_z", "out_rate", "out_hist") from the chain's kernel timing in a separate pass.
The yardstick is the "on" leg of tools/bench_output.py run in a tree of the parent commit.
Usage: python tools/bench_output_rate.py [--steps 10] [--warmup 3] [--shapes 1 32] [--legs ...] [--out FILE]
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
# leg -> enable_output's format, rate, mono (None: the stage off)
LEGS = {"off": None, "48k": ("s16", None, False), "16k_mono_f32": ("f32", 16000, True), "44k1_s16": ("s16", 44100, False)}


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K, out):
    bl = [BLK] * nb
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        ch.synchronize()                 # every leg: output_read synchronises, the leg without it must not run ahead
        if out:
            for s in range(K):
                ch.output_read(s)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--legs", nargs="+", default=list(LEGS))
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
        astride = 2 * frames
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        res, kt, seen = {}, {}, {}
        for leg in a.legs:
            spec = LEGS[leg]
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=nb, **kw)
            if spec:
                fmt, rate, mono = spec
                ch.enable_output(format=fmt, squelch_level=0.03, max_frames=frames, max_blocks=min(65536, 2 * nb), rate=rate,
                                 mono=mono)
            res[leg] = timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K, spec is not None)
            if spec:
                ch.enable_kernel_timing(1)
                k = {}
                for _ in range(4):
                    ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
                    ch.synchronize()
                    for name, ms in ch.kernel_times():
                        if name.startswith("out_"):
                            k.setdefault(name, []).append(ms)
                    pcm, recs, info = ch.output_read(0)
                ri = ch.output_rate_info(0)
                kt[leg] = {n: round(float(np.median(v)), 4) for n, v in k.items()}
                seen[leg] = dict(pcm_bytes_per_step_and_stream=int(pcm.nbytes), frames=int(len(pcm)), channels=int(pcm.shape[1]),
                                 blocks=int(len(recs)), gate_open=int(recs["gate_open"].sum()), rate=int(ri["rate"]),
                                 taps_per_phase=int(ri["taps_per_phase"]), pcm_clipped=int(ri["pcm_clipped"]))
            ch.close()
        rec = dict(tool="bench_output_rate", tree=os.path.basename(ROOT), channels=K, samples_per_step=N, steps=a.steps,
                   warmup=a.warmup, ms_per_step={k: round(v * 1e3, 4) for k, v in res.items()})
        if "48k" in res:
            rec["growth_over_48k_ms"] = {k: round((v - res["48k"]) * 1e3, 4) for k, v in res.items() if k not in ("off", "48k")}
        rec["output_kernels_ms_per_call"] = kt
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

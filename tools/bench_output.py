"""Output stage cost (fmr_enable_output): the bench-shaped step with the stage off, on (S16,
squelch_level 0.03, the ring sized for a step) and on beside RDS and all three monitors ("all"; "others" is RDS and the
monitors without it).

10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample blocks (bench.py's step) for one stream, and the
32-channel bank of tools/bench_channel_bank.py (2^23 samples per step), device buffers in and out, asynchronous calls,
one synchronisation per step in every leg; the PCM frames, the block records (and the other stages' records and groups)
are drained once per step.  The capture is one 2^23-sample station repeated.  Prints one JSON line per shape: ms per step
of every leg, the differences, and the medians of the stage's own kernel times ("out_pcm", "out_blocks") from the chain's
kernel timing in a separate pass.  A call of more than ~400 blocks also makes the fused front end leave the partial sums
of ALL its blocks (k_stats otherwise needs the last ~400 only): that is part of the "on" leg's difference, not of the two
kernel times.
The yardstick is the "off" leg of the parent commit's build: copy this file into a checkout of that commit and run it
there; the legs that need fmr_enable_output are skipped where the library does not have it.
Usage: python tools/bench_output.py [--steps 10] [--warmup 3] [--shapes 1 32] [--legs off on others all] [--out FILE]
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


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K, out, others):
    bl = [BLK] * nb
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        ch.synchronize()                 # every leg: the getters below synchronise, the legs without them must not run ahead
        for s in range(K):
            if out:
                ch.output_read(s)
            if others:
                ch.loudness_records(s)
                ch.monitor_records(s)
                ch.rf_monitor_records(s)
                ch.rds_groups(s)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--legs", nargs="+", default=["off", "on", "others", "all"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench_channel_bank as bcb
    have = hasattr(fmr.Chain, "enable_output") and "fmr_enable_output" in fmr.EXPORTS
    legs = [leg for leg in a.legs if have or leg in ("off", "others")]
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
        res, kt, seen = {}, {}, None
        for leg in legs:
            out, others = leg in ("on", "all"), leg in ("others", "all")
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=nb, enable_rds=others, **kw)
            if others:
                ch.enable_monitor(interval_samples=384000)
                ch.enable_loudness()
                ch.enable_rf_monitor()
            if out:
                ch.enable_output(squelch_level=0.03, max_frames=frames, max_blocks=min(65536, 2 * nb))
            res[leg] = timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K, out, others)
            if leg == "on":
                ch.enable_kernel_timing(1)
                for _ in range(4):
                    ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
                    ch.synchronize()
                    for name, ms in ch.kernel_times():
                        if name.startswith("out_"):
                            kt.setdefault(name, []).append(ms)
                    pcm, recs, info = ch.output_read(0)
                seen = dict(frames=int(len(pcm)), blocks=int(len(recs)), frames_dropped=int(info["frames_dropped"]),
                            gate_open=int(recs["gate_open"].sum()), if_level=float(recs["if_level"][-1]),
                            audio_level=float(recs["audio_level"][-1]))
            ch.close()
        rec = dict(tool="bench_output", tree=os.path.basename(ROOT), channels=K, samples_per_step=N,
                   steps=a.steps, warmup=a.warmup, ms_per_step={k: round(v * 1e3, 4) for k, v in res.items()})
        if "off" in res and "on" in res:
            rec["output_cost_ms"] = round((res["on"] - res["off"]) * 1e3, 4)
        if "others" in res and "all" in res:
            rec["output_cost_beside_rds_and_monitors_ms"] = round((res["all"] - res["others"]) * 1e3, 4)
        if kt:
            rec["output_kernels_ms_per_call"] = {k: round(float(np.median(v)), 4) for k, v in kt.items()}
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

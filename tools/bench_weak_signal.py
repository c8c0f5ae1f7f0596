"""Weak-signal handling cost (fmr_enable_weak_signal): the bench-shaped step with the stage off, in
FMR_WS_MEASURE ("measure"), in FMR_WS_ACT ("act"), and in FMR_WS_ACT together with RDS, the three monitors and the output
stage ("all"; "others" is those five without it).

10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample blocks (bench.py's step) for one stream, and the
32-channel bank of tools/bench_channel_bank.py (2^23 samples per step), device buffers in and out, asynchronous calls,
one synchronisation per step in every leg; the records (groups, PCM) are drained once per step.  The capture is one
2^23-sample station repeated: the seams cost nothing and the generator stays short.  Prints one JSON line per shape: ms per
step of every leg, the differences, and from a separate pass with the chain's kernel timing the medians of the stage's
own kernel times ("ws_usn", "ws_control", "ws_nodes", "ws_pass2") and of the fused front end ("ifr_fused") per call.
The yardstick is the "off" and "others" legs of the parent commit's build: copy this file into a checkout of that commit
and run it there, before and after; the legs that need fmr_enable_weak_signal are skipped where the library does not have
it.  --tree names the build in the lines ("parent commit, first run").
Usage: python tools/bench_weak_signal.py [--steps 10] [--warmup 3] [--shapes 1 32] [--legs off measure act others all]
                                         [--tree LABEL] [--out FILE]
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


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K, ws, others):
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
            if ws:
                ch.weak_signal_records(s)
            if others:
                ch.monitor_records(s)
                ch.loudness_records(s)
                ch.rf_monitor_records(s)
                ch.rds_groups(s)
                ch.output_read(s)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def kernel_pass(ch, d_x, N, nb, d_out, astride):
    """medians over four calls of the per-call sums of the stage's kernels and of the fused front end"""
    kt = {}
    ch.enable_kernel_timing(1)
    for _ in range(4):
        ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
        ch.synchronize()
        call = {}
        for name, ms in ch.kernel_times():
            if name.startswith("ws_") or name == "ifr_fused":
                call[name] = call.get(name, 0.0) + ms
        for name, ms in call.items():
            kt.setdefault(name, []).append(ms)
    return {k: round(float(np.median(v)), 4) for k, v in kt.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--legs", nargs="+", default=["off", "measure", "act", "others", "all"])
    ap.add_argument("--tree", default=None, help="what the lines call this build (default: the directory's name)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench_channel_bank as bcb
    have = hasattr(fmr.Chain, "enable_weak_signal") and "fmr_enable_weak_signal" in fmr.EXPORTS
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
        astride = 2 * (N * 48000 // F + 64 * nb)
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        res, kt, nrec, reading = {}, {}, 0, None
        for leg in legs:
            ws, others = leg in ("measure", "act", "all"), leg in ("others", "all")
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=nb, enable_rds=others, **kw)
            if others:
                ch.enable_monitor(interval_samples=384000)
                ch.enable_loudness()
                ch.enable_rf_monitor()
                ch.enable_output()
            if ws:
                ch.enable_weak_signal(act=leg != "measure")
            res[leg] = timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K, ws, others)
            if leg in ("off", "measure", "act"):
                kt[leg] = kernel_pass(ch, d_x, N, nb, d_out, astride)
            if leg == "act":
                recs, _ = ch.weak_signal_records(0)
                nrec = len(recs)
                if nrec:
                    lv = fmr.weak_signal_levels(recs)
                    reading = {k: round(lv[k], 5) for k in ("usn_mean_db", "usn_peak_db", "blend_share", "t_blend")}
            ch.close()
        rec = dict(tool="bench_weak_signal", tree=a.tree or os.path.basename(ROOT), channels=K, samples_per_step=N,
                   steps=a.steps, warmup=a.warmup, ms_per_step={k: round(v * 1e3, 4) for k, v in res.items()})
        for leg in ("measure", "act"):
            if "off" in res and leg in res:
                rec[leg + "_cost_ms"] = round((res[leg] - res["off"]) * 1e3, 4)
        if "others" in res and "all" in res:
            rec["act_cost_beside_all_others_ms"] = round((res["all"] - res["others"]) * 1e3, 4)
        if kt:
            rec["kernels_ms_per_call"] = kt
        if nrec:
            rec["records_last_pass_ch0"] = int(nrec)
            rec["reading_ch0"] = reading
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

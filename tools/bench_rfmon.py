"""RF monitor cost (fmr_enable_rf_monitor): the bench-shaped step with the stage off, on (M = 38400,
the default records), and on beside RDS, the modulation monitor and the audio monitor ("all_on"; "all_off" is that chain
without the RF monitor).

10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample blocks (bench.py's step) for one stream, and the
32-channel bank of tools/bench_channel_bank.py (2^23 samples per step), device buffers in and out, asynchronous calls,
one synchronisation per step in every leg; records and groups are drained once per step, and the time the drain of the
RF monitor's records takes on the host is kept apart ("rf_drain_ms_per_step").  The capture is one 2^23-sample station
repeated.  Prints one JSON line per shape: ms per step of every leg, the differences, and the medians of the stage
kernels' own times ("rfm_seg", "rfm_reduce"; their sum per call) from the chain's kernel timing in a separate pass.
The yardstick is the "off" leg of the parent commit's build: copy this file into a checkout of that commit and run it there
with --legs off all_off.
Usage: python tools/bench_rfmon.py [--steps 10] [--warmup 3] [--shapes 1 32] [--legs off on all_off all_on] [--out FILE]
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


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K, rfm, rest):
    """(seconds per step, seconds per step spent draining the RF monitor's records)"""
    bl = [BLK] * nb
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    drain = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        ch.synchronize()                 # every leg: the getters below synchronise, the legs without them must not run ahead
        for s in range(K):
            if rfm:
                t1 = time.perf_counter()
                ch.rf_monitor_records(s)
                drain += time.perf_counter() - t1
            if rest:
                ch.monitor_records(s)
                ch.loudness_records(s)
                ch.rds_groups(s)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, drain / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--legs", nargs="+", default=["off", "on", "all_off", "all_on"])
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
        astride = 2 * (N * 48000 // F + 64 * nb)
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        res, drain, kt, nrec, level = {}, {}, {}, 0, None
        for leg in a.legs:
            rfm, rest = leg in ("on", "all_on"), leg in ("all_off", "all_on")
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=nb, enable_rds=rest, **kw)
            if rest:
                ch.enable_monitor(interval_samples=384000)
                ch.enable_loudness()
            if rfm:
                ch.enable_rf_monitor()
            res[leg], d = timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K, rfm, rest)
            if rfm:
                drain[leg] = d
            if leg == "on":
                ch.enable_kernel_timing(1)
                for _ in range(4):
                    ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
                    ch.synchronize()
                    call = {}
                    for name, ms in ch.kernel_times():
                        if name.startswith("rfm"):
                            call[name] = call.get(name, 0.0) + ms
                    for name, ms in call.items():
                        kt.setdefault(name, []).append(ms)
                recs, hist, psd, _ = ch.rf_monitor_records(0)
                nrec = len(recs)
                if nrec:
                    level = round(fmr.rf_levels(recs[-1:], hist[-1:], psd[-1:])["level_dbfs"], 2)
            ch.close()
        rec = dict(tool="bench_rfmon", tree=os.path.basename(ROOT), channels=K, samples_per_step=N,
                   steps=a.steps, warmup=a.warmup, ms_per_step={k: round(v * 1e3, 4) for k, v in res.items()})
        if "off" in res and "on" in res:
            rec["rf_monitor_cost_ms"] = round((res["on"] - res["off"]) * 1e3, 4)
        if "all_off" in res and "all_on" in res:
            rec["rf_monitor_cost_beside_the_others_ms"] = round((res["all_on"] - res["all_off"]) * 1e3, 4)
        if drain:
            rec["rf_drain_ms_per_step"] = {k: round(v * 1e3, 4) for k, v in drain.items()}
        if kt:
            rec["rf_monitor_kernels_ms_per_call"] = {k: round(float(np.median(v)), 4) for k, v in kt.items()}
            rec["records_last_pass_ch0"] = int(nrec)
            rec["level_dbfs_ch0"] = level
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

"""RDS cost (fmr_create_rds): the bench-shaped step with RDS off, on, and on with soft-decision error
correction (fmr_set_rds_correction, FMR_RDS_FEC_SOFT).

10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample blocks (bench.py's step) for one stream, and the
32-channel bank of tools/bench_channel_bank.py (2^23 samples per step), device buffers in and out, asynchronous calls,
one synchronisation per step; the groups are drained once per step (what a live receiver does).  Prints one JSON line per
shape: ms per step off / on / on with soft correction, the differences, and the medians of the RDS kernels' own times ("rds_mix": mix + low-pass +
matched filter + MPX history; "rds_sym": window estimates + scan + bits) from the chain's kernel timing in a separate
pass.
Usage: python tools/bench_rds.py [--steps 10] [--warmup 3] [--shapes 1 32] [--out FILE]
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
import rds_fixture as rf  # noqa: E402

F, BLK = 10_000_000, 65536


def station(n, pi, seed):
    t = np.arange(n, dtype=np.float64) / F
    g = rf.ps_groups(pi, "BENCH%03d" % (pi % 1000), n=int(n / F / (104 * rf.TD)) + 2)
    return rf.fm_iq(rf.station_mpx(t, g, t0=0.002, stereo_id=seed % 32), F, amplitude=0.2, sigma=1e-3, seed=seed)


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K):
    bl = [BLK] * nb
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        if ch.enable_rds:
            for s in range(K):
                ch.rds_groups(s)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench_channel_bank as bcb
    lines = []
    for K in a.shapes:
        if K == 1:
            N = 1 << 27
            x = station(N, 0x1001, 1).astype(np.complex64)
            kw = {}
        else:
            N = 1 << 23
            offs = bcb.offsets(K)
            acc = np.zeros(N, dtype=np.complex128)
            for j, f in enumerate(dict.fromkeys(offs)):
                acc += station(N, 0x2000 + j, j) * cb.phasor(N, f, F, +1)
            x = acc.astype(np.complex64)
            kw = dict(channel_offsets_hz=offs)
        nb = N // BLK
        d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
        del x
        astride = 2 * (N * 48000 // F + 64 * nb)
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        res = {}
        for leg in ("off", "on", "soft"):
            rds = leg != "off"
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=nb, enable_rds=rds, **kw)
            if leg == "soft":
                ch.set_rds_correction(fmr.RDS_FEC_SOFT)
            res[leg] = timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K)
            if leg == "soft":
                corrected = sum(ch.rds_status(s).blocks_corrected for s in range(K))
            if leg == "on":
                ch.enable_kernel_timing(1)
                kt = {}
                for _ in range(3):
                    ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
                    ch.synchronize()
                    for name, ms in ch.kernel_times():
                        if name.startswith("rds"):
                            kt.setdefault(name, []).append(ms)
                st = ch.rds_status(0)
                groups = sum(len(ch.rds_groups(s)) for s in range(K))
                synced = sum(ch.rds_status(s).synced for s in range(K))
            ch.close()
        rec = dict(tool="bench_rds", channels=K, samples_per_step=N, steps=a.steps, warmup=a.warmup,
                   off_ms_per_step=round(res["off"] * 1e3, 4), on_ms_per_step=round(res["on"] * 1e3, 4),
                   rds_cost_ms=round((res["on"] - res["off"]) * 1e3, 4), soft_ms_per_step=round(res["soft"] * 1e3, 4),
                   soft_cost_ms=round((res["soft"] - res["on"]) * 1e3, 4), blocks_corrected=int(corrected),
                   rds_kernels_ms={k: round(float(np.median(v)), 4) for k, v in kt.items()},
                   channels_synced=int(synced), groups_last_pass=int(groups), injection_ch0=round(st.injection, 5))
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

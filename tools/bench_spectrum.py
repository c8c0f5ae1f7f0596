"""Band spectrum (fmr_spectrum_*) against the same Welch spectrum composed from torch ops.

Each step hands 2^27 cf32 samples in device memory (split over the rows) to fmr_spectrum_process_device, asynchronously,
one synchronisation per timed region.  For each N and row count it prints one JSON line:
  ms per step and GS/s (input samples per second);
  the step time the larger of two bounds allows -- 8 B per sample over the HBM peak (8 TB/s) or 5 N log2 N / H fp32
  FLOPs per sample over the fp32 vector peak (157.3 TFLOPS, MI355X_MICROARCH.md) -- as a share of the measured time,
  and which bound that is;
  the torch composition of the same spectrum (unfold -> window -> torch.fft.fft -> abs()**2 -> sum over segments) on the
  same input, and the ratio of the two.
One more line: a K = 8 FM channel bank step (10 MS/s, 2^23 samples in 65536-sample blocks) alone, and with the N = 8192
spectrum of the same device capture behind it, to show what monitoring costs beside decoding.
Kernel times: run it under rocprofv3 --kernel-trace --stats (a separate run).
Usage: python tools/bench_spectrum.py --steps 20 --warmup 3 [--N 1024 8192 16384] [--rows 1 8] [--no-bank] [--out FILE]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
fmr = importlib.import_module("airspy-fmradion_amd")

TOTAL = 1 << 27
PEAK_HBM, PEAK_F32 = 8.0e12, 157.3e12
F = 10e6


def timed(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps


def torch_welch(x, w, N, H, torch):
    """Welch sum of |FFT|^2 over segments, rows of x (complex64 (rows, n)), composed from torch ops."""
    seg = x.unfold(-1, N, H) * w
    return (torch.fft.fft(seg, dim=-1).abs() ** 2).sum(dim=-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 8192, 16384])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-bank", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    lines = []
    g = torch.Generator(device="cuda").manual_seed(1)
    d_x = torch.randn(TOTAL, dtype=torch.complex64, device="cuda", generator=g)
    for N in a.N:
        H = N // 2
        for rows in a.rows:
            n = TOTAL // rows
            x = d_x.view(rows, n)
            sp = fmr.Spectrum(F, fft_size=N, hop=H, n_rows=rows, max_call_len=n)
            t = timed(lambda: sp.process_device(x.data_ptr(), n, stride=n, sync=False), a.steps, a.warmup, sp.synchronize)
            sp.close()
            w = torch.hann_window(N, periodic=True, dtype=torch.float32, device="cuda")
            try:
                t_torch = timed(lambda: torch_welch(x, w, N, H, torch), a.steps, a.warmup, torch.cuda.synchronize)
            except RuntimeError as e:          # (out of memory: the composition materialises every segment's spectrum)
                t_torch = float("nan")
                print(f"torch composition failed: {e}", file=sys.stderr)
            torch.cuda.empty_cache()
            t_hbm = TOTAL * 8 / PEAK_HBM
            t_alu = TOTAL * 5 * N * math.log2(N) / H / PEAK_F32
            bound = "hbm" if t_hbm >= t_alu else "fp32_valu"
            line = {"tool": "bench_spectrum", "N": N, "hop": H, "rows": rows, "samples_per_step": TOTAL,
                    "ms_per_step": round(t * 1e3, 4), "gsps": round(TOTAL / t / 1e9, 2), "bound": bound,
                    "bound_share": round(max(t_hbm, t_alu) / t, 4),
                    "torch_ms_per_step": round(t_torch * 1e3, 4), "speedup_vs_torch": round(t_torch / t, 2),
                    "steps": a.steps, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if not a.no_bank:
        import bench_channel_bank as bcb
        K, NB, BLK = 8, (1 << 23) // 65536, 65536
        offs = bcb.offsets(K)
        acc = np.zeros(bcb.N, dtype=np.complex128)
        for j, f in enumerate(offs):
            acc += bcb.periodic_station(j, 0.3 * 10 ** (-j / 16)) * bcb.cb.phasor(bcb.N, f, F, +1)
        cap = torch.from_numpy(acc.astype(np.complex64)).cuda()
        astride = 2 * (bcb.N * 48000 // int(F) + 64 * NB)
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        bank = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK,
                         max_blocks=NB, channel_offsets_hz=offs)
        sp = fmr.Spectrum(F, fft_size=8192, max_call_len=bcb.N)

        def bank_step():
            bank.process_blocks_device(cap.data_ptr(), 0, [BLK] * NB, d_out.data_ptr(), astride)

        def both_step():
            bank_step()
            sp.process_device(cap.data_ptr(), bcb.N, sync=False)

        def sync_both():
            bank.synchronize()
            sp.synchronize()

        t_bank = timed(bank_step, a.steps, a.warmup, sync_both)
        t_both = timed(both_step, a.steps, a.warmup, sync_both)
        line = {"tool": "bench_spectrum", "bank_K": K, "capture_samples_per_step": bcb.N,
                "bank_ms_per_step": round(t_bank * 1e3, 4), "bank_plus_spectrum_ms_per_step": round(t_both * 1e3, 4),
                "spectrum_N": 8192, "monitor_cost_pct": round(100 * (t_both - t_bank) / t_bank, 2),
                "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(line), flush=True)
        lines.append(line)
        bank.close()
        sp.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

"""What the waterfall costs beside the plain band spectrum (fmr_spectrum_create_waterfall).

The setup of tools/bench_spectrum.py: each step hands the same 2^27 cf32 samples in device memory (one row) to
fmr_spectrum_process_device, asynchronously, one synchronisation per timed region, hop N / 2.  For each N and each
R = segments per line in {1, 8, 64} it prints one JSON line: ms per step of the plain object, ms per step of the
waterfall object (MEAN, a ring of 64 lines: the lines are overwritten unread, as they would be under a slow reader)
and their ratio; and the bytes the ring takes per step as a share of the input bytes.
Usage: python tools/bench_waterfall.py --steps 20 --warmup 3 [--N 1024 8192 16384] [--R 1 8 64] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
fmr = importlib.import_module("airspy-fmradion_amd")
from bench_spectrum import F, TOTAL, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 8192, 16384])
    ap.add_argument("--R", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(TOTAL, dtype=torch.complex64, device="cuda", generator=g)
    lines = []
    for N in a.N:
        H = N // 2
        sp = fmr.Spectrum(F, fft_size=N, hop=H, max_call_len=TOTAL)
        t_plain = timed(lambda: sp.process_device(x.data_ptr(), TOTAL, stride=TOTAL, sync=False), a.steps, a.warmup, sp.synchronize)
        sp.close()
        for R in a.R:
            wf = fmr.Spectrum(F, fft_size=N, hop=H, max_call_len=TOTAL, waterfall_segments=R, waterfall_lines=64)
            t_wf = timed(lambda: wf.process_device(x.data_ptr(), TOTAL, stride=TOTAL, sync=False), a.steps, a.warmup, wf.synchronize)
            wf.close()
            line = {"tool": "bench_waterfall", "N": N, "hop": H, "R": R, "samples_per_step": TOTAL,
                    "plain_ms_per_step": round(t_plain * 1e3, 4), "waterfall_ms_per_step": round(t_wf * 1e3, 4),
                    "ratio": round(t_wf / t_plain, 3),
                    "ring_bytes_over_input_bytes": round((TOTAL / H / R) * N * 4 / (TOTAL * 8), 4),
                    "steps": a.steps, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

"""Channelizer against the plain K-stream front-end-only chain on K pre-mixed copies ("Channelizer").

10 MS/s capture, 2^23 samples per step in 65536-sample blocks, K rows of IQ out at 384 kHz, device buffers in and out
(fmr_resample_blocks_device), asynchronous calls, one synchronisation after the timed steps.  The channelizer reads the
capture once per group of eight channels (k_ifr_chan) and its stage B writes every row straight into the output
buffer; the plain chain is fed K copies of the capture mixed down on the host (the mixing is done once, outside the
timed region: what a user without the channelizer pays on top is not counted).  For each K and class it prints one
JSON line: ms per step and channel-samples per second (K N / t) of both, and the median per-step times of the
channelizer's stage-A ("ifr_chan") and stage-B ("ifr_poly") kernels from the chain's own kernel timing (a separate
pass after the timed one).
Usage: python tools/bench_channelizer.py --K 1 8 32 --cls fast r8b --steps 20 --warmup 3 [--chains channelizer plain]
       [--out FILE]
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
import chanbank_fixture as cb  # noqa: E402

F, N, BLK, OUT = 10_000_000, 1 << 23, 65536, 384_000


def offsets(K):
    """K offsets spread over +-4.6 MHz (inside (F - 384 kHz) / 2), whole hertz, none on a round number."""
    if K == 1:
        return [1_250_003]
    return [int(round(-4_600_000 + 9_200_000 * i / (K - 1))) + 7 * i for i in range(K)]


def run(call, steps, warmup, torch):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    return t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--cls", nargs="+", default=["fast", "r8b"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chains", nargs="+", default=["channelizer", "plain"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    nb = N // BLK
    bl = [BLK] * nb
    ostride = N * OUT // F + 64 * nb
    rng = np.random.Generator(np.random.PCG64(7))
    x = ((rng.standard_normal(N) + 1j * rng.standard_normal(N)) * 0.1).astype(np.complex64)
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    lines = []
    for K in a.K:
        offs = offsets(K)
        d_out = torch.zeros((K, 2 * ostride), dtype=torch.float32, device="cuda")
        copies = None
        if "plain" in a.chains:
            copies = torch.from_numpy(np.stack([cb.mix_down(x, f, F) for f in offs]).view(np.float32)).cuda()
        torch.cuda.synchronize()          # (the buffers are filled on torch's stream, the chains run on their own)
        for cls in a.cls:
            rc = fmr.RESAMPLER_R8B if cls == "r8b" else fmr.RESAMPLER_FAST
            rec = dict(tool="bench_channelizer", resampler_class=cls, K=K, capture_samples_per_step=N, block=BLK,
                       output_rate=OUT, steps=a.steps, warmup=a.warmup)
            if "channelizer" in a.chains:
                cz = fmr.Channelizer(float(F), offs, output_rate=OUT, resampler_class=rc, max_blocks=nb)
                call = lambda: cz.resample_blocks_device(d_x.data_ptr(), bl, d_out.data_ptr(), ostride)  # noqa: E731
                t0 = run(call, a.steps, a.warmup, torch)
                cz.synchronize()
                t = (time.perf_counter() - t0) / a.steps
                cz.enable_kernel_timing(2)
                for _ in range(4):
                    call()
                cz.synchronize()
                kt = cz.kernel_times()
                med = lambda name: float(np.median([ms for n, ms in kt if n == name]))  # noqa: E731
                info = cz.resampler_info()
                rec.update(D=info["D"], NA=info["NA"], group_G=8, channelizer_ms_per_step=round(t * 1e3, 4),
                           channelizer_channel_samples_per_s=K * N / t, ifr_chan_ms=round(med("ifr_chan"), 4),
                           ifr_poly_ms=round(med("ifr_poly"), 4), channelizer_stage_b=sorted(cz.front_end_forms()),
                           channelizer_input_bytes_per_step=8 * N * ((K + 7) // 8))
                cz.close()
            if "plain" in a.chains:
                plain = fmr.Chain(mode=fmr.MODE_NONE, input_rate=float(F), enable_resampler=True, output_rate=OUT,
                                  resampler_class=rc, n_streams=K, max_block_len=BLK, max_blocks=nb)
                call = lambda: plain.resample_blocks_device(copies.data_ptr(), N, bl, d_out.data_ptr(), ostride)  # noqa: E731
                t0 = run(call, a.steps, a.warmup, torch)
                plain.synchronize()
                t = (time.perf_counter() - t0) / a.steps
                rec.update(plain_ms_per_step=round(t * 1e3, 4), plain_channel_samples_per_s=K * N / t,
                           plain_front_end_forms=sorted(plain.front_end_forms()), plain_input_bytes_per_step=8 * N * K)
                plain.close()
            if "channelizer_ms_per_step" in rec and "plain_ms_per_step" in rec:
                rec["channelizer_over_plain"] = round(rec["channelizer_ms_per_step"] / rec["plain_ms_per_step"], 4)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del copies, d_out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

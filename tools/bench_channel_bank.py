"""Channel bank against the plain K-stream chain on K pre-mixed copies ("Channel bank").

10 MS/s FM stereo, the config-5 step shape: 2^23 capture samples per step in 65536-sample blocks, device buffers in
and out, asynchronous calls, one synchronisation per step.  The step replays one capture, so the capture is periodic in
N = 2^23 samples (as bench.py's synthesis): every tone is snapped to a whole number of cycles in N, the MPX has exact
zero mean (the FM phase closes on itself), and every offset is a multiple of F / gcd(N, F) = 78125 Hz.  The stream each
channel sees is then continuous across steps; `pll_fallback` in the line says whether a PLL still fell back to its
serial kernels anywhere (it must be 0 for the step times to be the chain's).  For each K and class it prints one JSON
line:
  ms per step and channel-samples per second (K N / t) of the bank and of the plain chain fed K mixed-down copies (the
  mixing itself is done once, outside the timed region: what a user without the bank pays on top is not counted);
  the "ifr_chan" kernel time (the chain's own kernel timing, a separate pass after the timed one) and its algorithmic
  rate: 8 NA real FLOPs per stage-A output per channel (4 NA complex MACs of the modulated-tap form), as a fraction of
  the fp16 MFMA peak (2.5 PFLOPS dense) and of the fp32 vector peak (157.3 TFLOPS) the form runs on.
Usage: python tools/bench_channel_bank.py --K 1 8 32 --cls fast r8b --steps 20 --warmup 3 [--out FILE]
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

F, N, BLK = 10_000_000, 1 << 23, 65536
PEAK_F16, PEAK_F32 = 2.5e15, 157.3e12


STEP_HZ = F // np.gcd(N, F)          # 78125 Hz: an offset that is a multiple of it has a whole number of cycles in N


def offsets(K):
    """K channel offsets, multiples of STEP_HZ.  Up to 31 distinct stations spread over +-4.7 MHz at least 312.5 kHz
    apart (closer FM neighbours leak into each other's pass band and a PLL that sees it falls back to its serial
    kernels, which then dominate both chains' step); channels beyond 31 decode stations a second time (the same work for
    the bank and for the plain chain)."""
    if K == 1:
        return [16 * STEP_HZ]
    n = min(K, 31)
    units = min(int(9_400_000 / (n - 1) / STEP_HZ), 2 * int(4_700_000 / STEP_HZ))
    st = [(i - (n - 1) / 2) * units for i in range(n)]
    st = [int(np.floor(u)) * STEP_HZ for u in st]
    return [st[i % n] for i in range(K)]


def periodic_station(stream_id, amplitude, sigma=1e-3):
    """siggen.fm_stereo_iq's station, periodic in N: tones snapped to whole cycles in N, the MPX of exact zero mean."""
    T = N / F

    def snap(f):
        return round(f * T) / T

    t = np.arange(N, dtype=np.float64) / F
    fl, fr, fp = snap(1000.0 + 10.0 * stream_id), snap(400.0 + 10.0 * stream_id), snap(19000.0)
    left, right, th = np.sin(2 * np.pi * fl * t), np.sin(2 * np.pi * fr * t), 2 * np.pi * fp * t
    mpx = 0.45 * (left + right) + 0.10 * np.sin(th) + 0.45 * (left - right) * np.sin(2 * th)
    mpx -= mpx.mean()
    ph = 2 * np.pi * 75000.0 / F * np.cumsum(mpx)
    rng = np.random.Generator(np.random.PCG64(1 + stream_id))
    return amplitude * np.exp(1j * ph) + (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * sigma


def run(ch, d_in, stride, d_out, astride, steps, warmup, torch):
    bl = [BLK] * (N // BLK)
    for _ in range(warmup):
        ch.process_blocks_device(d_in.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_in.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--cls", nargs="+", default=["fast", "r8b"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    nb = N // BLK
    astride = 2 * (N * 48000 // F + 64 * nb)
    # one station at every channel's offset (eight programmes, levels over 10 dB, reused round the band): a channel
    # without a station would run its PLL on noise
    base = [periodic_station(i, 0.3 * 10 ** (-i / 16)) for i in range(8)]
    lines = []
    for K in a.K:
        offs = offsets(K)
        acc = np.zeros(N, dtype=np.complex128)
        for j, f in enumerate(dict.fromkeys(offs)):          # one station per distinct offset
            acc += base[j % 8] * cb.phasor(N, f, F, +1)
        x = acc.astype(np.complex64)
        d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
        for cls in a.cls:
            rc = fmr.RESAMPLER_R8B if cls == "r8b" else fmr.RESAMPLER_FAST
            kw = dict(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                      max_blocks=nb, resampler_class=rc)
            d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
            bank = fmr.Chain(channel_offsets_hz=offs, **kw)
            t_bank = run(bank, d_x, 0, d_out, astride, a.steps, a.warmup, torch)
            fb_bank = max(bank.status(s).pll_fallback for s in range(K))
            stereo_bank = sum(bank.status(s).stereo_detected for s in range(K))
            info = bank.resampler_info()
            bank.enable_kernel_timing(2)
            for _ in range(4):
                bank.process_blocks_device(d_x.data_ptr(), 0, [BLK] * nb, d_out.data_ptr(), astride)
            bank.synchronize()
            kt = [ms for name, ms in bank.kernel_times() if name == "ifr_chan"]
            t_chan = float(np.median(kt)) * 1e-3 if kt else float("nan")
            bank.close()
            outs = N // info["D"]
            flops = 8.0 * info["NA"] * outs * K
            del bank
            copies = torch.from_numpy(np.stack([cb.mix_down(x, f, F) for f in offs]).view(np.float32)).cuda()
            plain = fmr.Chain(n_streams=K, **kw)
            t_plain = run(plain, copies, N, d_out, astride, a.steps, a.warmup, torch)
            fb_plain = max(plain.status(s).pll_fallback for s in range(K))
            forms = sorted(plain.front_end_forms())
            plain.close()
            del plain, copies
            torch.cuda.empty_cache()
            rec = dict(tool="bench_channel_bank", resampler_class=cls, K=K, capture_samples_per_step=N, block=BLK,
                       steps=a.steps, warmup=a.warmup, D=info["D"], NA=info["NA"], group_G=8,
                       bank_ms_per_step=round(t_bank * 1e3, 4), bank_channel_samples_per_s=K * N / t_bank,
                       plain_ms_per_step=round(t_plain * 1e3, 4), plain_channel_samples_per_s=K * N / t_plain,
                       plain_front_end_forms=forms, bank_over_plain=round(t_bank / t_plain, 4),
                       pll_fallback=dict(bank=int(fb_bank), plain=int(fb_plain)), bank_channels_stereo=int(stereo_bank),
                       ifr_chan_ms=round(t_chan * 1e3, 4), ifr_chan_flops=flops,
                       ifr_chan_frac_f16_mfma_peak=flops / t_chan / PEAK_F16,
                       ifr_chan_frac_f32_vector_peak=flops / t_chan / PEAK_F32,
                       bank_input_bytes_per_step=8 * N * ((K + 7) // 8), plain_input_bytes_per_step=8 * N * K)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

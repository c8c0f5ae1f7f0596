"""IQ correction cost (fmr_enable_iq_correction): the bench-shaped step with the stage off, in
FMR_IQC_MEASURE ("measure"), in FMR_IQC_ACT ("act"), acting beside the acting blanker ("act_blanker"), and the first three
legs beside RDS, the three monitors and the output stage ("others", "others_measure", "others_act").

10 MS/s FM stereo, 2^27 capture samples per step in 65536-sample blocks (bench.py's step) for one stream, and the 8- and
32-channel banks of tools/bench_channel_bank.py (2^23 samples per step), device buffers in and out, asynchronous calls,
one synchronisation per step in every leg; the records (groups, PCM) are drained once per step.  The capture is one
2^23-sample station repeated, through the receiver model of tests/iqcorr_fixture.py (g = 1.05, phi = 3 degrees, an offset
of 0.01 - 0.006j).  Prints one JSON line per shape: ms per step of every leg, the differences, the traffic the stage adds
(8 B read per capture sample measuring; two reads and one write, 24 B, acting) as a time at the box's plain-read rate
(fmr_probe_read_bandwidth), and from a separate pass with the chain's kernel timing the medians of the stage's kernel times
("iqc_moments", "iqc_coef", "iqc_apply", "iqc_records") and of the front end per call, with the share iqc_coef takes of the
stage's kernels on the decoder stream.
The yardstick is the "off" and "others" legs of the parent commit's build: copy this file into a checkout of that commit
and run it there, alternately; the legs that need fmr_enable_iq_correction are skipped where the library does not have it.
--tree names the build in the lines.
Usage: python tools/bench_iq_correction.py [--steps 10] [--warmup 3] [--shapes 1 8 32]
                                           [--legs off measure act act_blanker others others_measure others_act]
                                           [--tree LABEL] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
fmr = importlib.import_module("airspy-fmradion_amd")
import chanbank_fixture as cb  # noqa: E402
import siggen  # noqa: E402

F, BLK, BASE = 10_000_000, 65536, 1 << 23
LEGS = ["off", "measure", "act", "act_blanker", "others", "others_measure", "others_act"]
G, PHI, DC = 1.05, math.radians(3.0), 0.01 - 0.006j


def impair(s):
    """I exact, Q' = g (Q cos phi + I sin phi), then the offset (tests/iqcorr_fixture.py's impair)"""
    s = s.astype(np.complex128)
    return (s.real + 1j * (G * (s.imag * math.cos(PHI) + s.real * math.sin(PHI))) + DC).astype(np.complex64)


def timed(ch, d_x, stride, nb, d_out, astride, steps, warmup, torch, K, iqc_on, nb_on, others):
    bl = [BLK] * nb
    for _ in range(warmup):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
    ch.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ch.process_blocks_device(d_x.data_ptr(), stride, bl, d_out.data_ptr(), astride)
        ch.synchronize()                 # every leg: the getters below synchronise, the legs without them must not run ahead
        if iqc_on:
            ch.iq_correction_records(0)
        if nb_on:
            ch.blanker_records(0)
        for s in range(K):
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
    """medians over four calls of the per-call sums of the stage's kernels, the blanker's and the front end's"""
    kt = {}
    ch.enable_kernel_timing(1)
    for _ in range(4):
        ch.process_blocks_device(d_x.data_ptr(), N, [BLK] * nb, d_out.data_ptr(), astride)
        ch.synchronize()
        call = {}
        for name, ms in ch.kernel_times():
            if name.startswith(("iqc_", "nb_", "ifr_")):
                call[name] = call.get(name, 0.0) + ms
        for name, ms in call.items():
            kt.setdefault(name, []).append(ms)
    out = {k: round(float(np.median(v)), 4) for k, v in kt.items()}
    on_stream = sum(out.get(k, 0.0) for k in ("iqc_moments", "iqc_coef", "iqc_apply"))
    if on_stream > 0:
        out["iqc_coef_share"] = round(out.get("iqc_coef", 0.0) / on_stream, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--legs", nargs="+", default=LEGS)
    ap.add_argument("--tree", default=None, help="what the lines call this build (default: the directory's name)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench_channel_bank as bcb
    have = hasattr(fmr.Chain, "enable_iq_correction") and "fmr_enable_iq_correction" in fmr.EXPORTS
    legs = [leg for leg in a.legs if have or leg in ("off", "others")]
    lines = []
    for K in a.shapes:
        st = siggen.fm_stereo_iq(BASE, float(F), amplitude=0.2)
        if K == 1:
            N = 1 << 27
            x = np.tile(impair(st), N // BASE)
            kw = {}
        else:
            N = BASE
            offs = bcb.offsets(K)
            acc = np.zeros(N, dtype=np.complex128)
            for f in dict.fromkeys(offs):
                acc += st * cb.phasor(N, f, F, +1)
            x = impair(acc)
            kw = dict(channel_offsets_hz=offs)
        nb = N // BLK
        d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
        del x
        read_gbs = fmr.probe_read_bandwidth(0, d_x.data_ptr(), 8 * N)
        astride = 2 * (N * 48000 // F + 64 * nb)
        d_out = torch.zeros((K, astride), dtype=torch.float64, device="cuda")
        res, kt, reading = {}, {}, None
        for leg in legs:
            others = leg.startswith("others")
            iqc_on = leg != "off" and leg != "others"
            act = "act" in leg
            nb_on = leg == "act_blanker"
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=float(F), enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=nb, enable_rds=others, **kw)
            if others:
                ch.enable_monitor(interval_samples=384000)
                ch.enable_loudness()
                ch.enable_rf_monitor()
                ch.enable_output()
            if iqc_on:
                ch.enable_iq_correction(act=act)
            if nb_on:
                ch.enable_blanker(act=True)
            res[leg] = timed(ch, d_x, N, nb, d_out, astride, a.steps, a.warmup, torch, K, iqc_on, nb_on, others)
            if leg in ("off", "measure", "act", "act_blanker"):
                kt[leg] = kernel_pass(ch, d_x, N, nb, d_out, astride)
            if leg == "act":
                recs, _ = ch.iq_correction_records(0)
                if len(recs):
                    lv = fmr.iq_correction_levels(recs)
                    reading = {k: round(lv[k], 5) for k in ("dc_dbfs", "image_rejection_db", "gain_imbalance_db",
                                                            "phase_error_deg", "usable_share")}
            ch.close()
        rec = dict(tool="bench_iq_correction", tree=a.tree or os.path.basename(ROOT), channels=K, samples_per_step=N,
                   steps=a.steps, warmup=a.warmup, ms_per_step={k: round(v * 1e3, 4) for k, v in res.items()},
                   plain_read_gb_s=round(read_gbs, 1),
                   traffic_ms={"measure": round(8 * N / read_gbs * 1e-6, 4), "act": round(24 * N / read_gbs * 1e-6, 4)})
        for base, pre in (("off", ""), ("others", "others_")):
            for leg in ("measure", "act", "act_blanker"):
                if base in res and pre + leg in res:
                    rec[pre + leg + "_cost_ms"] = round((res[pre + leg] - res[base]) * 1e3, 4)
        if kt:
            rec["kernels_ms_per_call"] = kt
        if reading:
            rec["reading_row0"] = reading
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del d_x, d_out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

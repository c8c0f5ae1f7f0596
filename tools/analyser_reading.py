"""The audio analyser's reading of the bench.py station (last table): siggen.fm_stereo_iq at
10 MS/s, 3 s in 65536-sample blocks, with multipath_stages = 0 and 64, clean and through siggen.two_ray (a second ray of
0.35 at 30 samples).  The last two records pooled, the channel's tone given as a hint.  Prints one JSON line per input,
setting and channel: THD and THD+N in per cent, noise and SINAD in dB (0 dB = a full-scale sine).
Usage: python tools/analyser_reading.py [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
fmr = importlib.import_module("airspy-fmradion_amd")
import siggen  # noqa: E402

F, BLK, NBLK, BATCH = 10e6, 65536, 458, 62          # 458 blocks = 3.0 s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = NBLK * BLK
    clean = siggen.fm_stereo_iq(n, F)
    lines = []
    for name, x in (("clean", clean), ("two_ray", siggen.two_ray(clean, 30))):
        x = np.asarray(x, dtype=np.complex64)
        for stages in (0, 64):
            ch = fmr.Chain(mode=fmr.MODE_FM, input_rate=F, enable_resampler=True, stereo=True, max_block_len=BLK,
                           max_blocks=BATCH, multipath_stages=stages)
            ch.enable_analyser(max_records=256)
            for i in range(0, NBLK, BATCH):
                nb = min(BATCH, NBLK - i)
                ch.process_blocks(x[None, i * BLK:(i + nb) * BLK], [BLK] * nb)
            recs, sp, _ = ch.analyser_records(0)
            ch.close()
            for view, tone in (("L", 1000.0), ("R", 400.0)):
                lv = fmr.analyser_levels(recs[-2:], sp[-2:], view=view, tone_hz=tone)
                lines.append(json.dumps(dict(tool="analyser_reading", input=name, multipath_stages=stages, view=view,
                                             records=len(recs), tone_hz=round(lv["tone_hz"], 4),
                                             tone_dbfs=round(lv["tone_dbfs"], 3), thd_pct=round(100 * lv["thd"], 5),
                                             thd_n_pct=round(100 * lv["thd_n"], 5), noise_dbfs=round(lv["noise_dbfs"], 2),
                                             sinad_db=round(lv["sinad_db"], 2))))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

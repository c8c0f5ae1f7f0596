"""bench.py --dump-outputs on the GPU: the dump is the last timed step's audio, every stream of it, and two runs whose
time-bound spin-ups differ (so that different numbers of steps come before the timed ones) dump the same step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, spinup_ms, warmup, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", "64", "--steps", str(steps),
           "--warmup", str(warmup), "--streams", "2", "--spinup-ms", str(spinup_ms), "--no-cpu-baseline", "--no-r8b-leg",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_is_the_last_timed_step_and_repeatable(tmp_path):
    a = _bench(tmp_path / "a", 0, 1, 3)
    b = _bench(tmp_path / "b", 30, 2, 2)
    for out, steps in ((a, 3), (b, 2)):
        assert out["steps"] == steps and out["ms_per_step"] > 0
        assert out["dump_outputs"]["arrays"]["audio"] == {"shape": [2, out["dump_outputs"]["arrays"]["audio"]["shape"][1]]}
    assert b["clock"]["spinup_steps"] % 625 == 0 and b["clock"]["spinup_steps"] > 0 and a["clock"]["spinup_steps"] == 0
    # run a dumps stream blocks [256, 320): the cold call, one warm-up step and two timed steps of 64 blocks come first; in
    # run b the cold call, 625 k spin-up steps, two warm-up steps and one timed step: the same resampler phase, 625 k x 64
    # blocks later
    for d in ("a", "b"):
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64 * 10 ** 6
    la, lb = np.load(tmp_path / "a" / "audio_block_len.npy"), np.load(tmp_path / "b" / "audio_block_len.npy")
    np.testing.assert_array_equal(la, lb)
    xa, xb = np.load(tmp_path / "a" / "audio.npy"), np.load(tmp_path / "b" / "audio.npy")
    assert xa.dtype == np.float64 and xa.shape == (2, int(la.sum())) and xa.shape == xb.shape
    assert np.sqrt(np.mean(xa ** 2)) > 0.1            # stereo audio of the synthetic station, not silence
    # the GPU path is not bit-reproducible from run to run (two runs of the same step: up to 3e-9 here, 3e-8 at 2048 blocks);
    # a step at another resampler phase samples the audio at other instants and differs by 1e-3 and more
    np.testing.assert_allclose(xa, xb, rtol=0, atol=1e-6)
    # the two streams are different stations (tones 10 Hz apart)
    assert np.sqrt(np.mean((xa[0] - xa[1]) ** 2)) > 0.01

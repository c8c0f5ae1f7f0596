"""bench.py --dump-outputs: the budget, the seeded sample of an array that does not fit it, the phase period that makes the
dumped step repeatable, and the argument checks.  CPU only (the GPU run: tests/test_gpu_bench_dump.py)."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_arrays_are_written_whole_in_float64(tmp_path):
    audio = np.random.default_rng(1).standard_normal((2, 1000))
    alen = np.array([300, 200, 500], dtype=np.uint32)
    info = bench.dump_outputs(str(tmp_path), {"audio": audio, "audio_block_len": alen})
    assert sorted(os.listdir(tmp_path)) == ["audio.npy", "audio_block_len.npy"]
    a, b = np.load(tmp_path / "audio.npy"), np.load(tmp_path / "audio_block_len.npy")
    assert a.dtype == np.float64 and b.dtype == np.float64
    np.testing.assert_array_equal(a, audio)
    np.testing.assert_array_equal(b, alen)
    assert info["arrays"]["audio"] == {"shape": [2, 1000]}


def test_array_over_budget_is_a_seeded_sample_within_budget(tmp_path):
    budget = 64 << 10
    big = np.arange(50000, dtype=np.float64).reshape(5, 10000) * 0.5
    small = np.arange(10, dtype=np.uint32)
    runs = []
    for sub in ("a", "b"):
        d = tmp_path / sub
        info = bench.dump_outputs(str(d), {"audio": big, "audio_block_len": small}, budget=budget)
        assert _total_bytes(d) <= budget
        np.testing.assert_array_equal(np.load(d / "audio_block_len.npy"), small)
        idx = np.load(d / "audio_index.npy")
        val = np.load(d / "audio.npy")
        assert len(idx) == len(val) == info["arrays"]["audio"]["sampled_elements"] > budget // 32
        assert np.all(np.diff(idx) > 0)
        np.testing.assert_array_equal(val, big.reshape(-1)[idx.astype(np.int64)])
        runs.append(idx)
    np.testing.assert_array_equal(runs[0], runs[1])


def test_rank_suffix(tmp_path):
    bench.dump_outputs(str(tmp_path), {"audio": np.zeros(4)}, suffix="_rank1")
    assert os.listdir(tmp_path) == ["audio_rank1.npy"]


def test_phase_period():
    # FM: 65536-sample blocks at 10 MS/s -> 384 kHz / 48 kHz: the phase repeats every 625 blocks
    assert bench.phase_period_steps(65536, 10e6, 2048, False) == 625
    assert bench.phase_period_steps(65536, 10e6, 1250, False) == 1
    assert bench.phase_period_steps(65536, 10e6, 125, False) == 5
    # AM: 2048-sample blocks at 384 kS/s -> 48 kHz: 256 audio samples per block, every block starts at phase 0
    assert bench.phase_period_steps(2048, 384e3, 8192, True) == 1


def test_argument_checks():
    for extra in (["--steps", "0"], ["--cpu-dry-run", "--dump-outputs", "unused"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
        assert r.returncode == 2 and "error:" in r.stderr, (extra, r.returncode, r.stderr[-400:])

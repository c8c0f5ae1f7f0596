"""bench.py: a plain run does only what its headline figure needs, and --full adds what else the benchmark measures or
checks.  CPU only, through the --cpu-dry-run hook (the GPU path's plain line: tests/test_gpu_bench_dump.py)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dry_run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--blocks", "1",
           "--cpu-dry-run"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_leaves_the_cpu_baseline_to_full():
    plain, full = _dry_run(), _dry_run("--full")
    assert plain["cpu_baseline"] is None
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["all_cores"]["cores"] >= 1
    assert _dry_run("--full", "--no-cpu-baseline")["cpu_baseline"] is None
    for out in (plain, full):
        assert out["steps"] == 1 and out["warmup"] == 0 and out["ms_per_step"] > 0 and out["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k]

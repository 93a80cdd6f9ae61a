"""bench.py's multi-rank launch path on the CPU (--dry-run: gloo process groups, no HIP).

`bench.py --gpus N` outside a launcher must start N ranks itself (torch.distributed.run as a
child process) and report n_gpus = N; under a launcher whose WORLD_SIZE differs from --gpus it
must refuse (exit 2) instead of printing a line with the wrong n_gpus.  At N = 1 the per-step
collective runs too (world-1 process group), so 1 -> N efficiency compares equal work.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def _run(args, env, timeout=240):
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True,
                          timeout=timeout, cwd="/tmp")


def _line(out):
    lines = [ln for ln in out.strip().splitlines() if ln.strip()]
    # stdout is exactly one JSON line (rank 0's); library banners (RCCL's version lines at
    # communicator creation) and logs go to stderr
    assert len(lines) == 1 and lines[0].startswith("{"), out
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2])
def test_dry_run_reports_the_ranks_it_ran(n):
    r = _run(["--gpus", str(n), "--dry-run", "--steps", "3", "--warmup", "1", "--prewarm-ms", "20"],
             _env())
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == n and d["dry_run"] is True
    assert d["config"]["parallelism"] == f"dp{n}"
    assert d["config"]["global_batch"] == n * d["config"]["batch_per_gpu"]
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None and d["scaling"] == "weak"


def test_dump_outputs_repeat_and_full_only_adds(tmp_path):
    """--dump-outputs writes the last timed step's output as float32, the same from run to run
    with the same arguments; --full changes neither it nor what the plain fields mean, and what
    only --full computes is null in a plain run."""
    import numpy as np
    lines, outs = [], []
    for k, extra in enumerate(([], ["--full"])):
        d = tmp_path / f"run{k}"
        r = _run(["--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "1", "--prewarm-ms", "5",
                  "--dump-outputs", str(d)] + extra, _env())
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(_line(r.stdout))
        assert sorted(p.name for p in d.iterdir()) == ["output.npy", "output_rows.npy"]
        outs.append((np.load(d / "output.npy"), np.load(d / "output_rows.npy")))
    (y0, rows0), (y1, rows1) = outs
    assert y0.dtype == np.float32 and rows0.dtype == np.float64
    assert y0.nbytes + rows0.nbytes <= 64 << 20
    cfg = lines[0]["config"]
    assert y0.shape == (cfg["batch_per_gpu"], cfg["channels"], cfg["height"], cfg["width"])
    assert rows0.size == y0.size // y0.shape[-1]
    assert np.array_equal(y0, y1) and np.array_equal(rows0, rows1)
    assert np.isfinite(y0).all() and y0.std() > 0
    plain, full = lines
    assert plain["full"] is False and full["full"] is True
    assert plain["checksum"] is None and isinstance(full["checksum"], float)
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[key] == full[key]
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and full["ms_per_step"] > 0


def test_dump_outputs_samples_whole_rows_of_a_large_output(tmp_path):
    """Above the size cap the dump is whole rows, first and last included, picked from the shape
    alone with a fixed seed."""
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    w = 4096
    rows = 2 * bench.DUMP_SAMPLE_BYTES // (4 * w) + 3
    y = torch.arange(rows * w, dtype=torch.float32).reshape(1, rows, w).to(torch.bfloat16)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, y, "output")
    bench.dump_outputs(b, y.clone(), "output")
    ya, ra = np.load(os.path.join(a, "output.npy")), np.load(os.path.join(a, "output_rows.npy"))
    yb, rb = np.load(os.path.join(b, "output.npy")), np.load(os.path.join(b, "output_rows.npy"))
    assert ya.dtype == np.float32 and ya.nbytes <= bench.DUMP_SAMPLE_BYTES
    assert ya.shape == (bench.DUMP_SAMPLE_BYTES // (4 * w), w)
    assert ra[0] == 0 and ra[-1] == rows - 1 and (np.diff(ra) > 0).all()
    assert np.array_equal(ya, yb) and np.array_equal(ra, rb)
    assert np.array_equal(ya, y.reshape(rows, w)[ra.astype(np.int64)].float().numpy())


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "1", "--dry-run", "--steps", "1"],
             _env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=120)
    assert r.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 1" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_gpus_must_be_positive():
    r = _run(["--gpus", "0", "--dry-run"], _env(), timeout=120)
    assert r.returncode == 2


def test_prewarm_runs_the_same_collectives_on_every_rank():
    """The pre-warm runs for a wall-clock budget with the per-step collective inside: ranks of
    different speed must still run the same number of steps (round 6: a per-rank time loop ran
    different numbers of all-gathers: a hang at N = 2 was seen once under gloo, and RCCL
    hangs on it).  Rank 1 starts its budget 40 ms later; the line reports every rank's count."""
    r = _run(["--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1", "--prewarm-ms", "60"],
             _env(BENCH_DRY_SKEW_MS="40"), timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _line(r.stdout)
    assert d["n_gpus"] == 2
    assert len(d["prewarm_steps"]) == 2 and d["prewarm_steps"][0] == d["prewarm_steps"][1] > 0

"""bench.py command line: --steps, ms_per_step, --full and --dump-outputs
(CPU engine, tiny problem)."""

import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "1",
           "--steps", "50", "--warmup", "2", "--records-per-gpu", "300",
           "--partitions-per-gpu", "2", "--dump-outputs", str(out_dir)] + extra
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_identical_outputs(tmp_path):
    plain = _run([], tmp_path / "plain")
    full = _run(["--full"], tmp_path / "full")

    for out in (plain, full):
        assert out["steps"] == 50
        assert out["ms_per_step"] > 0
        assert abs(out["value"] * out["ms_per_step"] / 1000.0 - 1.0) < 1e-9
        for key in ("metric", "unit", "higher_is_better", "dtype"):
            assert key in out
    # the secondary figures are reported only with --full
    assert plain["ess_per_sec"] is None
    assert plain["ess"] == {"logLikelihood": None, "numObservedEntities": None}
    assert full["ess_per_sec"] is not None and full["ess_per_sec"] > 0

    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "plain" / "*.npy")))
    assert files == sorted(os.path.basename(f)
                           for f in glob.glob(str(tmp_path / "full" / "*.npy")))
    assert {"rec_cluster.npy", "rec_entity_values.npy", "rec_distortions.npy",
            "dist_probs.npy", "loglik_series.npy", "summary_scalars.npy"} <= set(files)
    total = 0
    for f in files:
        a = np.load(tmp_path / "plain" / f)
        b = np.load(tmp_path / "full" / f)
        assert a.dtype == np.float64
        assert np.array_equal(a, b), f  # same arguments -> same inputs and chain
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "plain" / "loglik_series.npy").shape == (50,)
    assert np.load(tmp_path / "plain" / "rec_cluster.npy").shape == (300,)
    scalars = np.load(tmp_path / "plain" / "summary_scalars.npy")
    assert scalars[0] == 52  # iteration counter after warm-up + timed sweeps
    assert np.load(tmp_path / "plain" / "loglik_series.npy")[-1] == scalars[1]

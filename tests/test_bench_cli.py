"""bench.py command line: a plain run prints the headline line only and
`--dump-outputs` writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_bench_plain_run_dumps_last_step(tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup",
         "1", "--workload", "si1k", "--dump-outputs", str(out_dir)],
        cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "atom_steps_per_s"
    assert line["steps"] == 2 and line["warmup"] == 1
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    n = line["config"]["n_atoms"]
    assert n == 1000
    # value and ms_per_step describe the same timed interval
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3),
                                          rel=1e-9)
    # what only --full measures stays out of a plain run
    assert line["roofline"] is None and line["cpu_baseline"] is None

    files = sorted(os.listdir(out_dir))
    assert files == ["energy.npy", "forces_owned.npy", "site_props_owned.npy"]
    arrays = {f: np.load(out_dir / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert arrays["energy.npy"].shape == (1,)
    assert arrays["forces_owned.npy"].shape == (n, 3)
    assert arrays["site_props_owned.npy"].shape[0] == n
    assert np.abs(arrays["forces_owned.npy"]).max() > 0
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20

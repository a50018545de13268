"""bench.py --dump-outputs: what the timed path computed in its last step, as float64 .npy
files within 64 MiB, sampled the same way on every run; and --steps is the timed step count."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, gpu_available

import bench


def bench_fields():
    from neutral_amd import interface
    return interface.F64_FIELDS + interface.I32_FIELDS


def test_dump_sample_is_fixed_and_one_per_stratum():
    assert bench.dump_sample(1000, 1000, 1) is None
    a = bench.dump_sample(10_000_003, 4096, 7)
    assert np.array_equal(a, bench.dump_sample(10_000_003, 4096, 7))
    assert len(a) == 4096 and a[0] >= 0 and a[-1] < 10_000_003
    edges = np.arange(4097, dtype=np.int64) * 10_000_003 // 4096
    assert np.all((a >= edges[:-1]) & (a < edges[1:]))


def test_worst_case_dump_fits_the_budget():
    particles = (len(bench_fields()) + 1) * bench.DUMP_MAX_PARTICLES
    meshes = 3 * bench.DUMP_MAX_CELLS            # tally, flux, cell_index
    assert 8 * (particles + meshes + 4) <= bench.DUMP_BUDGET_BYTES


@pytest.mark.parametrize("steps", ["0", "-1"])
def test_steps_below_one_are_refused(steps):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", steps],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not bench.parse_args().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a GPU")
def test_dump_outputs_are_what_the_line_reports(tmp_path):
    n, steps = 3000001, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "1", "--nparticles", str(n), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    # a plain run (no --full) runs nothing but the headline's steps
    assert line["lazy_export"] is None
    assert not {"cpu_baseline", "gpu_over_cpu", "parity_vs_cpu"} & set(line)
    assert "hbm_copy_measured_gbs" not in line["roofline"]["hbm"]
    files = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype == np.float64 for a in files.values())
    want = {"tally", "last_step_events", "particle_index"} | {"particle_" + f for f in bench_fields()}
    assert set(files) == want
    nx = line["config"]["nx"]
    assert files["tally"].shape == (nx * nx,)
    total = line["global_tally"]
    assert abs(files["tally"].sum() - total) <= 1e-12 * abs(total)
    idx = files["particle_index"]
    assert len(idx) == bench.DUMP_MAX_PARTICLES and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(idx, bench.dump_sample(n, bench.DUMP_MAX_PARTICLES, bench.DUMP_SEED + 1))
    for f in bench_fields():
        assert files["particle_" + f].shape == idx.shape, f
    assert set(np.unique(files["particle_dead"])) <= {0.0, 1.0}
    assert files["particle_cellx"].min() >= 0 and files["particle_cellx"].max() < nx
    ev = files["last_step_events"]
    assert ev[0] > 0 and np.all(ev == np.round(ev))

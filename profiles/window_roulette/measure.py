"""What the in-step weight window costs and what it buys (profiles/window_roulette/README.md).

    python profiles/window_roulette/measure.py cost [NPARTICLES]   # the lookup's cost, csp 400^2
    python profiles/window_roulette/measure.py fom                 # BatchedRun, auto_window with and without in_step

One JSON line per figure on stdout."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from neutral_amd import cs_table, decks, host  # noqa: E402
from neutral_amd import interface as iface  # noqa: E402


def problem(tmp, n, steps, nx=400):
    path = decks.write_deck("csp", os.path.join(tmp, "csp.params"), nx=nx, ny=nx, nparticles=n, iterations=steps)
    return host.setup_problem(path, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)


def timed_steps(sim, steps, warmup=1):
    """re-inject, `warmup` steps, re-inject, `steps` timed steps -> (wall ms per step, kernel ms per
    step, collisions per step, killed, survived)"""
    sim.inject()
    for tt in range(1, warmup + 1):
        sim.step(tt)
    sim.inject()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results = [sim.step(tt) for tt in range(1, steps + 1)]
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / steps
    return (wall, sum(r.stats.kernel_ms for r in results) / steps, sum(r.collisions for r in results) / steps,
            sum(r.stats.roulette_killed for r in results), sum(r.stats.roulette_survived for r in results))


def cost(n, steps=10, rounds=3):
    """alternating: set_roulette(0.25, 0.5) against the uniform mesh 0.25 with ratio 2 in its forms"""
    keys, values = cs_table.load()
    iface.set_quiet(True)
    with tempfile.TemporaryDirectory() as tmp:
        prob = problem(tmp, n, steps)
        nx, ny = prob.nx, prob.ny
        e0 = prob.initial_energy
        ten = np.concatenate([[1e-300], e0 * np.geomspace(1e-5, 0.9, 9), [1e300]])   # 10 groups, every energy inside
        forms = {
            "set_roulette(0.25, 0.5)": None,
            "mesh": dict(lower=0.25, survival_ratio=2.0),
            "mesh, block (1, 1)": dict(lower=0.25, survival_ratio=2.0, block=(1, 1)),
            "mesh, block (8, 8)": dict(lower=0.25, survival_ratio=2.0, block=(8, 8)),
            "mesh, 10 groups": dict(lower=0.25, survival_ratio=2.0, groups=ten),
        }
        sim = iface.Simulation(prob, keys, values, variant=2)
        for rnd in range(rounds):
            for name, window in forms.items():
                sim.roulette = (0.25, 0.5) if window is None else None
                sim.window_in_step(None)
                if window is not None:
                    sim.window_in_step(**window)
                wall, kernel, colls, killed, survived = timed_steps(sim, steps)
                print(json.dumps({"measure": "cost", "round": rnd, "form": name, "nparticles": n, "steps": steps,
                                  "wall_ms_per_step": round(wall, 3), "kernel_ms_per_step": round(kernel, 3),
                                  "collisions_per_step": colls, "killed": killed, "survived": survived}), flush=True)
        sim.close()


def fom(n=16_000_000, batches=16, steps=10):
    """BatchedRun on csp 400^2, auto_window after every step but the last: as it is, and in_step"""
    keys, values = cs_table.load()
    iface.set_quiet(True)
    iface.set_lazy_export(True)
    with tempfile.TemporaryDirectory() as tmp:
        prob = problem(tmp, n, steps)
        for in_step in (False, True, False, True):
            run = iface.BatchedRun(prob, keys, values, batches=batches, variant=2)
            collisions = []

            def between(sim, tt):
                collisions.append(iface.last_step().collisions)
                return sim.auto_window(in_step=in_step) if tt < steps else None
            result = run.run(steps, between, each_batch=lambda sim, b: sim.window_in_step(None))
            st = result["energy"].stats
            print(json.dumps({"measure": "fom", "in_step": in_step, "nparticles": n, "batches": batches,
                              "steps": steps, "wall_seconds": round(result.wall_seconds, 4),
                              "ms_per_step": round(1e3 * result.wall_seconds / (batches * steps), 3),
                              "collisions_per_step": sum(collisions) / len(collisions),
                              "mean_relerr": st.mean_relerr, "max_relerr": st.max_relerr, "fom": result.fom}),
                  flush=True)
            run.close()


if __name__ == "__main__":
    if sys.argv[1] == "cost":
        cost(int(float(sys.argv[2])) if len(sys.argv) > 2 else 100_000_000)
    else:
        fom()

"""One rank of a two-rank roulette run on a shared GPU (started by tests/test_roulette.py with
RANK / WORLD_SIZE / MASTER_PORT set): steps a deck with Russian roulette on, the particles
sharded over the ranks (mode "shard") or the mesh decomposed 2x1 (mode "domain"), and leaves
its particles in <out>/rank<r>.npz and the step statistics it reads as one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

from neutral_amd import cs_table, host  # noqa: E402
from neutral_amd import interface as iface  # noqa: E402


def main():
    deck, out, steps, mode = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    cutoff, survival = float(sys.argv[5]), float(sys.argv[6])
    iface.set_quiet(True)
    iface.set_lazy_export(False)
    iface.set_device(0)
    iface.comm_start()
    rank = iface.library().neutral_hip_comm_rank()
    prob = host.setup_problem(deck)
    keys, values = cs_table.load()
    sim = iface.Simulation(prob, keys, values, variant=2,
                           domain=(2, 1) if mode == "domain" else None,
                           roulette=(cutoff, survival))
    sim.inject()
    log = {"rank": rank, "killed": [], "survived": [], "lost": [], "gained": [], "collectives": []}
    for tt in range(1, steps + 1):
        s = sim.step(tt).stats
        log["killed"].append(s.roulette_killed)
        log["survived"].append(s.roulette_survived)
        log["lost"].append(s.roulette_weight_lost)
        log["gained"].append(s.roulette_weight_gained)
        log["collectives"].append(s.host_collectives)
    arrays = sim.particle_arrays()
    ids = sim.particle_keys() if mode == "domain" else \
        (np.arange(sim.n, dtype=np.uint32) + np.uint32(sim.pid_base))
    np.savez(os.path.join(out, f"rank{rank}.npz"), ids=ids, **arrays)
    sim.close()
    iface.library().neutral_hip_comm_barrier()
    iface.library().neutral_hip_comm_stop()
    print(json.dumps(log))


if __name__ == "__main__":
    main()

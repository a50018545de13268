"""One rank of a multi-rank run on a shared GPU (started by tests/ranks.py: launch_ranks with RANK /
WORLD_SIZE / MASTER_PORT set) that takes a blocks census and applies a blocks window:

    gpu_blocks_worker.py <deck> <out> <spec as JSON>

steps the deck `steps` times on the tiled variant with the particles sharded over the ranks, then
calls Simulation.census and Simulation.window with the spec's block and edges (null: no groups),
the window with `lower` (a .npy file), `ratios` and `seed`.  Global particle i starts at
spec["energies"][i % len].  spec["roulette"] and
spec["capture_scale"] are the Simulation's, as tests/gpu_ranks_worker.py takes them.  Leaves in
<out>/rank<r>.npz: pid_base (the shard's first particle id), before_<field> and after_<field> (its
arrays before the census and after the window), census (the 2 * B values, which went in as -1), and
said: JSON of the two calls' stats by field."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from neutral_amd import cs_table, host  # noqa: E402
from neutral_amd import interface as iface  # noqa: E402


def struct_dict(stats):
    """a stats struct by field, nested structs included"""
    return {name: struct_dict(getattr(stats, name)) if hasattr(getattr(stats, name), "_fields_") else getattr(stats, name)
            for name, *_ in stats._fields_}


def main():
    deck, out, spec = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    iface.set_quiet(True)
    iface.set_lazy_export(False)
    iface.set_device(0)
    iface.comm_start()
    rank = iface.library().neutral_hip_comm_rank()
    prob = host.setup_problem(deck)
    keys, values = cs_table.load()
    absorb = (np.array(keys), spec["capture_scale"] * np.array(values))
    sim = iface.Simulation(prob, keys, values, variant=2, roulette=tuple(spec["roulette"]), cs_absorb=absorb)
    sim.inject()
    # (the deck gives every history one energy and its collisions keep it: global particle i goes at
    # energies[i % len], as tests/test_group_window.py's scenario has it)
    energy = np.array(spec["energies"])[(sim.pid_base + np.arange(sim.n)) % len(spec["energies"])]
    iface.library().neutral_hip_memcpy_h2d(C.c_void_p(sim.particles.contents.energy), energy.ctypes.data, energy.nbytes)
    for tt in range(1, spec["steps"] + 1):
        sim.step(tt)
    before = sim.particle_arrays()
    block, edges = tuple(spec["block"]), spec["edges"]
    cnx, cny, ngroups = iface.block_bins(sim.p.nx, sim.p.ny, block, edges)
    both = torch.full((2 * max(ngroups, 1) * cnx * cny,), -1.0, dtype=torch.float64, device=sim.device)
    census = sim.census(out=both, groups=edges, block=block)[2]
    window = sim.window(np.load(spec["lower"]), seed=spec["seed"], groups=edges, block=block, **spec["ratios"])
    after = sim.particle_arrays()
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, f"rank{rank}.npz"), pid_base=np.array(sim.pid_base), census=both.cpu().numpy(),
             said=np.array(json.dumps(dict(census=struct_dict(census), window=struct_dict(window)))),
             **{f"before_{f}": a for f, a in before.items()}, **{f"after_{f}": a for f, a in after.items()})
    sim.close()
    iface.library().neutral_hip_comm_barrier()
    iface.library().neutral_hip_comm_stop()


if __name__ == "__main__":
    main()

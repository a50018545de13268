"""One rank of a multi-rank run on a shared GPU (started by tests/ranks.py: launch_gpu_ranks with
RANK / WORLD_SIZE / MASTER_PORT set):

    gpu_ranks_worker.py <deck> <out> <steps> <mode> <Simulation keywords as JSON> [--validate]

steps the deck on the tiled variant with the particles sharded over the ranks (mode "shard") or
the mesh decomposed (mode "domain PXxPY") and with whatever the keywords turn on (scalar_flux,
current, outflow, collision_tallies, roulette); leaves what it holds in <out>/rank<r>.npz --
particle ids and state, its block of the energy tally and of every optional mesh it keeps, where
the block lies in the global mesh, its event counts -- and prints the step statistics it read as
one JSON line.  --validate also runs the library's validate() (it prints)."""
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

# the log's lists, one value per step, and the field of NeutralHipStepStats each is read from
STATS = dict(host_syncs="host_syncs", collectives="host_collectives", exchange_ranks="exchange_ranks",
             killed="roulette_killed", survived="roulette_survived", lost="roulette_weight_lost",
             gained="roulette_weight_gained")


def main():
    deck, out, steps, mode, kw = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], json.loads(sys.argv[5])
    domain = tuple(int(v) for v in mode.split()[1].split("x")) if mode.startswith("domain") else None
    iface.set_quiet(True)
    iface.set_lazy_export(False)
    iface.set_device(0)
    transport = iface.comm_start()
    rank = iface.library().neutral_hip_comm_rank()
    prob = host.setup_problem(deck)
    keys, values = cs_table.load()
    sim = iface.Simulation(prob, keys, values, variant=2, domain=domain, **kw)
    sim.inject()
    log = {"rank": rank, "counts": [sim.n], "facets": [], **{name: [] for name in STATS}}
    events = []
    for tt in range(1, steps + 1):
        r = sim.step(tt)
        events.append((r.nprocessed, r.facets, r.collisions, r.census))  # (summed over the ranks)
        log["counts"].append(sim.n)
        log["facets"].append(int(r.facets))
        for name, field in STATS.items():
            log[name].append(getattr(r.stats, field))
    ids = sim.particle_keys() if domain is not None else \
        (np.arange(sim.n, dtype=np.uint32) + np.uint32(sim.pid_base))
    meshes = {name: t.cpu().numpy().reshape(sim.lny, sim.lnx)
              for name in ("flux", "collisions", "absorbed", "jx", "jy")
              for t in [getattr(sim, name)] if t is not None}
    if sim.outflow is not None:
        meshes["out"] = sim.outflow_host()
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, f"rank{rank}.npz"), ids=ids, tally=sim.tally_host(),
             origin=np.array([sim.x_off, sim.y_off]),
             block=np.array([sim.x_off, sim.y_off, sim.lnx, sim.lny]),
             events=np.array(events, dtype=np.int64), counts=np.array(log["counts"]),
             transport=np.array([transport]), **meshes, **sim.particle_arrays())
    if "--validate" in sys.argv[6:]:
        sim.validate()
    sim.close()
    iface.library().neutral_hip_comm_barrier()
    iface.library().neutral_hip_comm_stop()
    print(json.dumps(log))


if __name__ == "__main__":
    main()

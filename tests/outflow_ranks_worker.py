"""One rank of a two-rank run with the outflow tally on a shared GPU (started by
tests/test_outflow.py with RANK / WORLD_SIZE / MASTER_PORT set): steps a deck with the scalar flux
and the outflow kept (argument 5: "1"; "0" keeps the flux alone), the particles sharded over the
ranks (mode "shard") or the mesh decomposed 2x1 (mode "domain"), and leaves its meshes and where
they lie in the global mesh in <out>/rank<r>.npz, and the step statistics it reads as one JSON
line."""
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
    outflow = sys.argv[5] == "1"  # (0: the flux alone, for the steps' wait and collective counts)
    iface.set_quiet(True)
    iface.set_lazy_export(False)
    iface.set_device(0)
    iface.comm_start()
    rank = iface.library().neutral_hip_comm_rank()
    prob = host.setup_problem(deck)
    keys, values = cs_table.load()
    sim = iface.Simulation(prob, keys, values, variant=2,
                           domain=(2, 1) if mode == "domain" else None,
                           scalar_flux=True, outflow=outflow)
    sim.inject()
    log = {"rank": rank, "collectives": [], "host_syncs": [], "facets": []}
    for tt in range(1, steps + 1):
        r = sim.step(tt)
        log["collectives"].append(r.stats.host_collectives)
        log["host_syncs"].append(r.stats.host_syncs)
        log["facets"].append(int(r.facets))  # (summed over the ranks)
    if outflow:
        np.savez(os.path.join(out, f"rank{rank}.npz"), out=sim.outflow_host(),
                 flux=sim.flux.cpu().numpy().reshape(sim.lny, sim.lnx),
                 origin=np.array([sim.x_off, sim.y_off]))
    sim.close()
    iface.library().neutral_hip_comm_barrier()
    iface.library().neutral_hip_comm_stop()
    print(json.dumps(log))


if __name__ == "__main__":
    main()

"""One rank of a multi-rank run on a shared GPU (started by tests/ranks.py: launch_gpu_ranks with
RANK / WORLD_SIZE / MASTER_PORT set):

    gpu_ranks_worker.py <deck> <out> <steps> <mode> <Simulation keywords as JSON> [--validate]
                        [--schedule <file>]

steps the deck on the tiled variant with the particles sharded over the ranks (mode "shard") or
the mesh decomposed (mode "domain PXxPY") and with whatever the keywords turn on (scalar_flux,
current, outflow, collision_tallies, roulette; "capture_scale": s is the worker's own and makes the
capture table s times the scatter table); leaves what it holds in <out>/rank<r>.npz --
particle ids and state, its block of the energy tally and of every optional mesh it keeps, where
the block lies in the global mesh, its event counts -- and prints the step statistics it read as
one JSON line.  --validate also runs the library's validate() (it prints).

--schedule <file> (mode "shard" only) names a JSON list of census operations to run between the
steps, each {"after": the step it follows, "op": ..., its arguments}, in the list's order:

    comb         seed                                        Simulation.comb
    emit         count, weight: the rank emits its share of   Simulation.emit (default seed)
                 count, cut by comms_shard_range as the driver cuts --source
    window       lower (a .npy file, (ny, nx)), upper_ratio,  Simulation.window (default seed)
                 survival_ratio, max_split
    census                                                    Simulation.census, into a buffer of -1
    auto_window  target, upper_ratio, survival_ratio,         Simulation.auto_window (default seed)
                 max_split
    poke         rank, field, slot, value: that rank writes   neutral_hip_memcpy_h2d
                 one value of its arrays; the others do nothing
    keep                                                      nothing: the arrays are kept as they stand

An entry with "named_count": n makes the call name n particles instead of the shard's count (the
library takes the shard's own, whatever count the caller names).

After operation k (0, 1, ...) the rank keeps its particle_arrays() as op<k>_<field>; a census also
op<k>_census_count and op<k>_census_weight (the buffer, whatever the call made of it), an auto
window the two meshes its bounds were made from and op<k>_lower.  "ops" in rank<r>.npz is the JSON
list of what each operation returned: {"after", "op", "code" (0, or the refusal's), "stats": the
stats struct by field; for an auto window "census", "bounds" and "stats"}.  With a schedule the
file also holds "tallies", the energy tally after every step.  Without --schedule nothing of this happens."""
import ctypes as C
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


def struct_dict(stats):
    return {name: getattr(stats, name) for name, *_ in stats._fields_}


def run_operation(sim, rank, world, entry, k, kept):
    """one entry of the schedule on this rank's shard; what it left goes into `kept` (arrays, by
    name); -> what it returned, an entry of the file's ops"""
    lib, op = iface.library(), entry["op"]
    nx, ny = sim.p.nx, sim.p.ny
    said = {"after": entry["after"], "op": op, "code": 0}
    count, sim.n = sim.n, entry.get("named_count", sim.n)
    ratios = {name: entry[name] for name in ("upper_ratio", "survival_ratio", "max_split") if name in entry}
    try:
        if op == "comb":
            said["stats"] = struct_dict(sim.comb(seed=entry["seed"]))
        elif op == "emit":
            first, share = C.c_longlong(), C.c_longlong()
            host.lib().comms_shard_range(C.c_longlong(entry["count"]), rank, world, C.byref(first), C.byref(share))
            said["share"] = share.value
            said["stats"] = struct_dict(sim.emit(share.value, weight=entry["weight"]))
        elif op == "window":
            said["stats"] = struct_dict(sim.window(np.load(entry["lower"]), **ratios))
        elif op == "census":
            both = torch.full((2 * nx * ny,), -1.0, dtype=torch.float64, device=sim.device)
            try:
                said["stats"] = struct_dict(sim.census(out=both)[2])
            finally:
                kept[f"op{k}_census_count"] = both[:nx * ny].cpu().numpy()
                kept[f"op{k}_census_weight"] = both[nx * ny:].cpu().numpy()
        elif op == "auto_window":
            census, bounds, window = sim.auto_window(target_population=entry["target"], **ratios)
            said.update(census=struct_dict(census), bounds=struct_dict(bounds), stats=struct_dict(window))
            both = sim.last_census.cpu().numpy()
            kept[f"op{k}_census_count"], kept[f"op{k}_census_weight"] = both[:nx * ny], both[nx * ny:]
            kept[f"op{k}_lower"] = sim.last_lower.cpu().numpy()
        elif op == "keep":
            pass
        elif op == "poke":
            if rank == entry["rank"]:
                lib.neutral_hip_sync_particles(sim.particles)
                field = entry["field"]
                value = np.array([entry["value"]], dtype=np.float64 if field in iface.F64_FIELDS else np.int32)
                address = getattr(sim.particles.contents, field) + entry["slot"] * value.itemsize
                lib.neutral_hip_memcpy_h2d(C.c_void_p(address), value.ctypes.data, value.nbytes)
        else:
            raise SystemExit(f"no such operation: {op}")
    except ValueError as refused:  # (CombRefused, SourceRefused, WindowRefused, CensusRefused, BoundsRefused)
        if not hasattr(refused, "code"):
            raise
        said.update(code=refused.code, refused=type(refused).__name__, stats=struct_dict(refused.stats))
    finally:
        sim.n = count
    for f, a in sim.particle_arrays().items():
        kept[f"op{k}_{f}"] = a
    return said


def main():
    deck, out, steps, mode, kw = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], json.loads(sys.argv[5])
    schedule = None
    if "--schedule" in sys.argv[6:]:
        if mode != "shard":
            raise SystemExit("a schedule of census operations goes with mode \"shard\"")
        with open(sys.argv[sys.argv.index("--schedule") + 1]) as f:
            schedule = json.load(f)
    domain = tuple(int(v) for v in mode.split()[1].split("x")) if mode.startswith("domain") else None
    iface.set_quiet(True)
    iface.set_lazy_export(False)
    iface.set_device(0)
    transport = iface.comm_start()
    rank = iface.library().neutral_hip_comm_rank()
    prob = host.setup_problem(deck)
    keys, values = cs_table.load()
    if "capture_scale" in kw:
        kw["cs_absorb"] = (np.array(keys), kw.pop("capture_scale") * np.array(values))
    sim = iface.Simulation(prob, keys, values, variant=2, domain=domain, **kw)
    sim.inject()
    log = {"rank": rank, "counts": [sim.n], "facets": [], **{name: [] for name in STATS}}
    events, kept, said, tallies = [], {}, [], []
    world = iface.library().neutral_hip_comm_nranks()
    for tt in range(1, steps + 1):
        r = sim.step(tt)
        events.append((r.nprocessed, r.facets, r.collisions, r.census))  # (summed over the ranks)
        log["counts"].append(sim.n)
        log["facets"].append(int(r.facets))
        for name, field in STATS.items():
            log[name].append(getattr(r.stats, field))
        if schedule is not None:
            tallies.append(sim.tally_host())
            for entry in schedule:
                if entry["after"] == tt:
                    said.append(run_operation(sim, rank, world, entry, len(said), kept))
    if schedule is not None:
        kept.update(ops=np.array(json.dumps(said)), tallies=np.array(tallies))
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
             transport=np.array([transport]), **meshes, **sim.particle_arrays(), **kept)
    if "--validate" in sys.argv[6:]:
        sim.validate()
    sim.close()
    iface.library().neutral_hip_comm_barrier()
    iface.library().neutral_hip_comm_stop()
    print(json.dumps(log))


if __name__ == "__main__":
    main()

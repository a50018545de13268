"""The fixed source, restated in numpy (include/neutral_hip.h: neutral_hip_source_particles).

    d_0 < d_1 < ...   the indices j with dead[j] != 0
    refilled          d_0 .. d_{m-1}, m = min(count, number of dead); nothing else changes
    slot j            injection's particle of the stream (pkey = pid_base + j, master_key = seed):
                      x, y from counter 0 in the box, the cell by the edges, the direction from
                      counter 1, the given energy, weight and dt, mfp_to_collision 0, dead 0

The samples of the streams are an input (`rn`): on the GPU they come from the library's own Threefry
(probe_rows and interface.probe_threefry), on the CPU from the oracle's (cpu_samples).  The
arithmetic on them is numpy's, without fused multiply-adds: positions agree with the device's to a
rounding, not to the bit.
"""
from collections import namedtuple

import numpy as np

F64_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "dt_to_census", "mfp_to_collision")
I32_FIELDS = ("cellx", "celly", "dead")
FIELDS = F64_FIELDS + I32_FIELDS

# the box, the block's offsets in the mesh, dt, the block's edge arrays (pad removed), the energy
SourceArgs = namedtuple("SourceArgs", "left bottom width height x_off y_off dt edgex edgey energy")


def args_of(problem, energy=None, box=None) -> SourceArgs:
    """the source of a neutral_amd.host.Problem on one rank"""
    p = problem
    left, bottom, width, height = box if box is not None else (
        p.local_particle_left_off, p.local_particle_bottom_off, p.local_particle_width,
        p.local_particle_height)
    return SourceArgs(left, bottom, width, height, p.x_off, p.y_off, p.dt,
                      np.asarray(p.edgex, dtype=np.float64)[p.pad:p.pad + p.nx + 1],
                      np.asarray(p.edgey, dtype=np.float64)[p.pad:p.pad + p.ny + 1],
                      p.initial_energy if energy is None else energy)


def ranks(dead, count: int) -> np.ndarray:
    """the indices refilled: the first `count` dead slots, ascending"""
    return np.flatnonzero(np.asarray(dead) != 0)[:max(int(count), 0)]


def probe_rows(slots, pid_base: int, seed: int) -> np.ndarray:
    """rows {counter, pkey, master_key} for interface.probe_threefry: counters 0 and 1 of every slot;
    its samples reshaped (-1, 2, 2) are `rn`"""
    slots = np.asarray(slots, dtype=np.uint64)
    rows = np.empty((len(slots), 2, 3), dtype=np.uint64)
    rows[:, 0, 0], rows[:, 1, 0] = 0, 1
    rows[:, :, 1] = (np.uint64(pid_base) + slots)[:, None]
    rows[:, :, 2] = np.uint64(seed)
    return rows.reshape(-1, 3)


def cpu_samples(slots, pid_base: int, seed: int) -> np.ndarray:
    """rn[i, counter] = the two samples of slot i's stream at that counter, from the oracle's Threefry"""
    import oracle_binding as ob
    rn = np.empty((len(slots), 2, 2), dtype=np.float64)
    for i, j in enumerate(slots):
        for counter in (0, 1):
            rn[i, counter] = ob.generate_random_numbers(int(pid_base) + int(j), int(seed), counter)
    return rn


def find_cell(edge: np.ndarray, c: np.ndarray) -> np.ndarray:
    """the ii with edge[ii] <= c < edge[ii + 1], 0 where there is none"""
    ii = np.searchsorted(edge, c, side="right") - 1
    return np.where((c >= edge[0]) & (c < edge[-1]), ii, 0).astype(np.int32)


def expected(before: dict, dead, count: int, weight: float, seed: int, pid_base: int,
             args: SourceArgs, rn=None) -> dict:
    """the arrays after the call (new arrays); rn: see the module's text (None: the oracle's)"""
    slots = ranks(dead, count)
    if rn is None:
        rn = cpu_samples(slots, pid_base, seed)
    rn = np.asarray(rn, dtype=np.float64).reshape(len(slots), 2, 2)
    out = {f: np.array(before[f]) for f in FIELDS}
    x = args.left + rn[:, 0, 0] * args.width
    y = args.bottom + rn[:, 0, 1] * args.height
    theta = 2.0 * np.pi * rn[:, 1, 0]
    out["x"][slots], out["y"][slots] = x, y
    out["cellx"][slots] = args.x_off + find_cell(args.edgex, x)
    out["celly"][slots] = args.y_off + find_cell(args.edgey, y)
    out["omega_x"][slots], out["omega_y"][slots] = np.cos(theta), np.sin(theta)
    out["energy"][slots] = args.energy
    out["weight"][slots] = weight
    out["dt_to_census"][slots] = args.dt
    out["mfp_to_collision"][slots] = 0.0
    out["dead"][slots] = 0
    return out

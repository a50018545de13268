"""The arithmetic of the outflow tally (include/neutral_hip.h: neutral_hip_set_outflow_tally) and
of the conservation identities it closes.  The CPU oracle does not score the outflow: what the
kernels are held to, per cell and per side, is the replay of tests/replay.py, which scores it
beside everything else.

Sides: 0 west (-x), 1 east (+x), 2 south (-y), 3 north (+y)."""
import math

import numpy as np

from replay import EAST, NORTH, SOUTH, WEST


# ---- what the definition implies --------------------------------------------------------------

def net_outflow(out):
    """per cell: the outflow through the cell's interior sides minus the inflow, which is the
    neighbours' outflow through the shared sides.  Sides on the mesh's outer boundary do not enter
    (what they hold came back).  out: (4, ny, nx)."""
    out = np.asarray(out)
    net = np.zeros(out.shape[1:])
    net[:, 1:] += out[WEST][:, 1:]
    net[:, :-1] += out[EAST][:, :-1]
    net[1:, :] += out[SOUTH][1:, :]
    net[:-1, :] += out[NORTH][:-1, :]
    net[:, 1:] -= out[EAST][:, :-1]     # from the western neighbour, through its east side
    net[:, :-1] -= out[WEST][:, 1:]     # from the eastern neighbour, through its west side
    net[1:, :] -= out[NORTH][:-1, :]    # from the southern neighbour
    net[:-1, :] -= out[SOUTH][1:, :]    # from the northern neighbour
    return net


def wall_hits(out):
    """the weight (times 1/N) that struck the mesh's outer boundary: the boundary sides alone"""
    out = np.asarray(out)
    return math.fsum(np.concatenate([out[WEST][:, 0], out[EAST][:, -1], out[SOUTH][0, :], out[NORTH][-1, :]]))


def weight_by_cell(parts, nx, ny, select):
    """sum of the stored weight of the selected particles per cell, (ny, nx)"""
    cell = parts["celly"][select].astype(np.int64) * nx + parts["cellx"][select].astype(np.int64)
    return np.bincount(cell, weights=parts["weight"][select], minlength=nx * ny).reshape(ny, nx)


def balance_sides(before, after, absorbed_step, out_step, n, nx, ny):
    """The two sides of the per-cell balance of one step, (ny, nx) each:
        W_before - W_after - D - N * absorbed   and   N * (outflow - inflow through interior sides)
    W: stored weight of the live particles per cell; D: stored weight of the particles whose dead
    flag rose in this step, by their final cell; absorbed_step, out_step: what the step added to
    the meshes.  Also returns D."""
    alive_before = before["dead"] == 0
    alive_after = after["dead"] == 0
    died = alive_before & ~alive_after
    d = weight_by_cell(after, nx, ny, died)
    lhs = (weight_by_cell(before, nx, ny, alive_before) - weight_by_cell(after, nx, ny, alive_after) - d
           - n * np.asarray(absorbed_step).reshape(ny, nx))
    rhs = n * net_outflow(np.asarray(out_step).reshape(4, ny, nx))
    return lhs, rhs, d

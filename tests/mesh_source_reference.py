"""The mesh source, restated in numpy (include/neutral_hip.h: neutral_hip_source_mesh).

    refilled          the fixed source's slots (source_reference.ranks): the first count dead ones
    C_c, S            the inclusive prefix sums of the strengths in cell order, c = j * nx + i, S the
                      last (comb_reference.prefix_sums: extended precision, rounded once)
    slot              counter 2 of its stream chooses: t = u0 * S, the first cell with t < C_c among the
                      cells with s_c > 0 (searchsorted over those), else the last of them; the bin
                      from u1 as the described source chooses a component's.  Counter 0 places it in
                      the cell's box, left = edgex[i], width = edgex[i + 1] - edgex[i], likewise in y;
                      cellx, celly are the drawn cell.  Counter 1, weight, dt, mfp_to_collision and
                      dead come through described_source_reference, from one component with the
                      source's bins and angle interval.

The library's cumulative sums come out of its blocked f64 scan, allowed 64 eps S: a draw whose t lies
within GUARD * S (comb_reference.GUARD, the project's allowance for this scan) of a boundary C_c may
fall to either side there.  The restatement reports those draws as `guarded`; the tests choose their
seeds so that there is none, and then demand the exact cell of every slot.
"""
import numpy as np

import comb_reference as cr
import described_source_reference as dr
import source_reference as sr

FIELDS = sr.FIELDS
ISOTROPIC = dr.ISOTROPIC
MeshArgs = dr.MeshArgs
GUARD = cr.GUARD


def spectrum(energies):
    """(e, share) lines and (e_lo, e_hi, share) bins -> [(e_lo, e_hi, share), ...]"""
    return dr.component(1.0, (0.0, 0.0, 0.0, 0.0), energies).bins


class Table:
    """the cumulative mesh of `strength`, (ny, nx): K, S, the non-zero cells and their C_c"""

    def __init__(self, strength):
        s = np.asarray(strength, dtype=np.float64)
        self.ny, self.nx = s.shape
        flat = s.ravel()
        assert np.all(np.isfinite(flat)) and np.all(flat >= 0.0) and np.any(flat > 0.0)
        self.cumulative = cr.prefix_sums(flat)
        self.S = float(self.cumulative[-1])
        self.cells = np.flatnonzero(flat > 0.0)
        self.K = len(self.cells)
        self.at_cells = self.cumulative[self.cells]  # ascending: the strengths are not negative

    def choose(self, u0):
        """-> (the cell of every draw, which draws are guarded)"""
        t = np.asarray(u0, dtype=np.float64) * self.S
        r = np.minimum(np.searchsorted(self.at_cells, t, side="right"), self.K - 1)  # the first with t < C
        lower = np.where(r > 0, self.at_cells[np.maximum(r - 1, 0)], 0.0)
        upper = self.at_cells[r]
        guarded = ((t - lower <= GUARD * self.S) & (r > 0)) | ((upper - t <= GUARD * self.S) & (r < self.K - 1))
        return self.cells[r], guarded


def cpu_u(slots, pid_base: int, seed: int) -> np.ndarray:
    """counter 2's two samples of every slot's stream, from the oracle's Threefry"""
    import oracle_binding as ob
    return np.array([ob.generate_random_numbers(int(pid_base) + int(j), int(seed), 2) for j in slots],
                    dtype=np.float64).reshape(-1, 2)


def expected(before: dict, dead, count: int, weight: float, seed: int, pid_base: int, table: Table, bins,
             theta, mesh: MeshArgs, rn=None):
    """-> (the arrays after the call (new arrays), the flat cell c = j * nx + i of every refilled slot,
    its bin, which of the draws are guarded); bins as spectrum() makes them; mesh: the block's offsets,
    dt and edge arrays; rn: the samples, (slots, 3, 2) (None: the oracle's)"""
    slots = sr.ranks(dead, count)
    if rn is None:
        rn = dr.cpu_samples(slots, pid_base, seed)
    rn = np.asarray(rn, dtype=np.float64).reshape(len(slots), 3, 2)
    one = [dr.Component(1.0, (0.0, 0.0, 0.0, 0.0), list(bins), tuple(theta))]
    out, _, b = dr.expected(before, dead, count, weight, seed, pid_base, one, mesh, rn)
    cell, guarded = table.choose(rn[:, 2, 0])
    i, j = cell % table.nx, cell // table.nx
    left, bottom = mesh.edgex[i], mesh.edgey[j]
    out["x"][slots] = left + rn[:, 0, 0] * (mesh.edgex[i + 1] - left)
    out["y"][slots] = bottom + rn[:, 0, 1] * (mesh.edgey[j + 1] - bottom)
    out["cellx"][slots] = mesh.x_off + i
    out["celly"][slots] = mesh.y_off + j
    return out, cell, b, guarded

"""The in-step weight window (include/neutral_hip.h: neutral_hip_set_window_roulette) restated in
Python: the bin of a collision in plain integer arithmetic, and a replay of single histories that
looks its cutoff up per absorption.

The CPU oracle is frozen and knows only the global cutoff, so WindowReplay is the reference of a
non-uniform mesh.  It is replay.Replay with `history` restated -- Replay.history reads its cutoff
once per history -- and is pinned against Replay itself, which the oracle test pins, before
anything on the GPU is compared with it (tests/test_window_roulette.py)."""
import math

import numpy as np

import oracle_binding as ob
from replay import FIELDS, MIN_ENERGY_OF_INTEREST, EAST, NORTH, SOUTH, WEST, Replay, fma, speed_of
from closed_form import MASS_NO


def group_of(energy, edges):
    """the group g with edges[g] <= energy < edges[g + 1], by comparisons only: on an edge the group
    above; None below edges[0], at or above edges[-1], or for a NaN"""
    if edges is None or len(edges) < 2:
        return None
    count = 0
    for e in edges:          # (ascending: the count of edges at or below the energy)
        if e <= energy:
            count += 1
    return count - 1 if 1 <= count <= len(edges) - 1 else None


def _block_of(cell, block):
    """cell div block by counting whole blocks (no division: the tests compare it with //)"""
    q = 0
    while (q + 1) * block <= cell:
        q += 1
    return q


def bin_of(cellx, celly, energy, nx, ny, edges=None, block=None):
    """The bin of a collision in cell (cellx, celly) of the global mesh of nx by ny at `energy`:
    g * cnx * cny + (celly div block_y) * cnx + (cellx div block_x), in plain integers.  edges:
    the G + 1 group edges (None: no groups, g = 0); block: (block_x, block_y) (None: 1 x 1).
    None where there is no bin: a cell outside the mesh, an energy in no group."""
    bx, by = (1, 1) if block is None else (int(block[0]), int(block[1]))
    cellx, celly, nx, ny = int(cellx), int(celly), int(nx), int(ny)
    if not (0 <= cellx < nx and 0 <= celly < ny):
        return None
    cnx, cny = -(-nx // bx), -(-ny // by)
    g = 0
    if edges is not None:
        g = group_of(energy, [float(e) for e in edges])
        if g is None:
            return None
    return g * cnx * cny + _block_of(celly, by) * cnx + _block_of(cellx, bx)


class WindowReplay(Replay):
    """Replay with the roulette of the in-step window: `lower` is the flat mesh of bounds
    (max(G, 1) * cny * cnx values), `ratio` the survival ratio, `edges` / `block` say what the bins
    are.  Besides Replay's numbers it keeps, per bin, how many absorptions happened there
    (absorptions), how many histories roulette killed (killed_in) and kept (survived_in), and per
    step call what roulette did (the caller reads killed / survived / lost / gained between steps).
    (Replay's own `edges` and `box` are the spectrum's: not used here.)"""

    def __init__(self, prob, cs_scatter, cs_absorb, lower, ratio, edges=None, block=None, fused=False):
        super().__init__(prob, cs_scatter, cs_absorb, (0.0, 0.0), fused=fused)
        self.lower = np.asarray(lower, dtype=np.float64).ravel()
        self.ratio = float(ratio)
        self.w_edges = None if edges is None else [float(e) for e in edges]
        self.w_block = block
        self.absorptions = np.zeros(self.lower.size, dtype=np.int64)
        self.killed_in = np.zeros(self.lower.size, dtype=np.int64)
        self.survived_in = np.zeros(self.lower.size, dtype=np.int64)
        self.played = set()   # pids that played at least once

    def bound(self, cx, cy, energy):
        """(bin, w_lo): None and 0.0 where the collision has no bin"""
        b = bin_of(cx, cy, energy, self.p.nx, self.p.ny, self.w_edges, self.w_block)
        return (None, 0.0) if b is None else (b, float(self.lower[b]))

    def history(self, pid, master_key, s):
        """Replay.history with one change: inside an absorption the cutoff is lower[bin] of the cell
        and the energy the history collides with, and the survival weight fl(ratio * cutoff)"""
        if s["dead"]:
            return
        p = self.p
        x, y, ox, oy, e, w, cx, cy = (s[k] for k in FIELDS[:-1])
        rho = float(p.density[cy * p.nx + cx])
        micro_s, micro_a = self.cs_s.lookup(e)[0], self.cs_a.lookup(e)[0]
        sig_s, sig_a = self._sigmas(rho, micro_s, micro_a)
        speed = speed_of(e)
        left = self.dt
        counter = 0
        rn0, _ = ob.generate_random_numbers(pid, master_key, counter)
        counter += 1
        mfp = -math.log(rn0) / sig_s
        while left > 0.0:
            cell_mfp = 1.0 / (sig_s + sig_a)
            d_facet, x_facet = self._facet(x, y, ox, oy, speed, cx, cy)
            d_coll = mfp * cell_mfp
            d_census = speed * left
            if d_coll < d_facet and d_coll < d_census:
                self.ncollisions += 1
                self._segment(w, d_coll, ox, oy, e, cx, cy)
                self.collisions[cy, cx] += 1
                x, y = self._move(x, y, d_coll, ox, oy)
                p_absorb = sig_a / (sig_s + sig_a)
                rc0, rc1 = ob.generate_random_numbers(pid, master_key, counter)
                counter += 1
                if rc0 < p_absorb:
                    self.absorbed[cy, cx] += w * p_absorb * self.inv_n
                    w = w * (1.0 - p_absorb)
                    if e < MIN_ENERGY_OF_INTEREST:
                        s["dead"] = 1
                        break
                    b, wc = self.bound(cx, cy, e)
                    if b is not None:
                        self.absorptions[b] += 1
                    if w < wc:
                        ws = self.ratio * wc
                        self.played.add(pid)
                        if rc1 * ws < w:
                            self.survived += 1
                            self.survived_in[b] += 1
                            self.gained += ws - w
                            w = ws
                        else:
                            self.killed += 1
                            self.killed_in[b] += 1
                            self.lost += w
                            w = 0.0
                            s["dead"] = 1
                            break
                else:
                    mu = 1.0 - 2.0 * rc1
                    if self.fused:
                        e_new = e * (fma(mu, 2.0 * MASS_NO, MASS_NO * MASS_NO) + 1.0) / ((MASS_NO + 1.0) * (MASS_NO + 1.0))
                        cos_t = 0.5 * fma(-(MASS_NO - 1.0), math.sqrt(e / e_new), (MASS_NO + 1.0) * math.sqrt(e_new / e))
                        sin_t = math.sqrt(fma(-cos_t, cos_t, 1.0))
                        ox, oy = fma(ox, cos_t, -(oy * sin_t)), fma(ox, sin_t, oy * cos_t)
                    else:
                        e_new = e * (MASS_NO * MASS_NO + 2.0 * MASS_NO * mu + 1.0) / ((MASS_NO + 1.0) * (MASS_NO + 1.0))
                        cos_t = 0.5 * ((MASS_NO + 1.0) * math.sqrt(e_new / e) - (MASS_NO - 1.0) * math.sqrt(e / e_new))
                        sin_t = math.sqrt(1.0 - cos_t * cos_t)
                        ox, oy = ox * cos_t - oy * sin_t, ox * sin_t + oy * cos_t
                    e = e_new
                micro_s, micro_a = self.cs_s.lookup(e)[0], self.cs_a.lookup(e)[0]
                sig_s, sig_a = self._sigmas(rho, micro_s, micro_a)
                rn0, _ = ob.generate_random_numbers(pid, master_key, counter)
                counter += 1
                mfp = -math.log(rn0) / sig_s
                left -= d_coll / speed
                speed = speed_of(e)
            elif d_facet < d_census:
                self.nfacets += 1
                mfp -= d_facet / cell_mfp
                left -= d_facet / speed
                self._segment(w, d_facet, ox, oy, e, cx, cy)
                x, y = self._move(x, y, d_facet, ox, oy)
                if x_facet:
                    if ox > 0.0:
                        self.out[EAST, cy, cx] += w * self.inv_n
                        if cx >= p.nx - 1:
                            ox = -ox
                            self.wall_hits += 1
                        else:
                            cx += 1
                    elif ox < 0.0:
                        self.out[WEST, cy, cx] += w * self.inv_n
                        if cx <= 0:
                            ox = -ox
                            self.wall_hits += 1
                        else:
                            cx -= 1
                else:
                    if oy > 0.0:
                        self.out[NORTH, cy, cx] += w * self.inv_n
                        if cy >= p.ny - 1:
                            oy = -oy
                            self.wall_hits += 1
                        else:
                            cy += 1
                    elif oy < 0.0:
                        self.out[SOUTH, cy, cx] += w * self.inv_n
                        if cy <= 0:
                            oy = -oy
                            self.wall_hits += 1
                        else:
                            cy -= 1
                rho = float(p.density[cy * p.nx + cx])
                sig_s, sig_a = self._sigmas(rho, micro_s, micro_a)
            else:
                self._segment(w, d_census, ox, oy, e, cx, cy)
                x, y = self._move(x, y, d_census, ox, oy)
                left = 0.0
        s.update(x=x, y=y, omega_x=ox, omega_y=oy, energy=e, weight=w, cellx=cx, celly=cy)

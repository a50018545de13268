"""The event loop of tests/replay.py restated with vacuum sides (include/neutral_hip.h:
neutral_hip_set_vacuum_sides).  tests/replay.py is the pinned restatement and stays as it is; its
reflection sits in the middle of Replay.history() and cannot be hooked, so the loop is written
out once more here, line for line, with the one rule added: a facet event that would reflect
through a side whose bit is set in `vacuum` leaves the history dead on the wall, with the
direction it came with, and ends its time.  With vacuum = 0 this gives Replay's bits -- every
field, every mesh, every count (tests/test_vacuum.py pins that before anything else leans on it).

Beyond Replay it counts the census events, the reflections by side, the escapes by side with the
sum of their weights, and how many escaped with a weight other than 1.

Sides, as the outflow numbers them: 0 west (-x), 1 east (+x), 2 south (-y), 3 north (+y)."""
import math

import numpy as np

import oracle_binding as ob
import replay
from replay import EAST, FIELDS, MASS_NO, MIN_ENERGY_OF_INTEREST, NORTH, SOUTH, WEST, fma, speed_of


class EscapeReplay(replay.Replay):
    """replay.Replay with `vacuum`, a mask over the four sides (1 << side)."""

    def __init__(self, prob, cs_scatter, cs_absorb=None, roulette=(0.0, 0.0), dt=None, edges=(), box=None,
                 fused=False, vacuum=0):
        super().__init__(prob, cs_scatter, cs_absorb, roulette, dt, edges, box, fused)
        self.vacuum = int(vacuum)
        assert 0 <= self.vacuum <= 15
        self.ncensus = 0
        self.reflections = [0, 0, 0, 0]
        self.escaped = [0, 0, 0, 0]
        self.escape_weight = [0.0, 0.0, 0.0, 0.0]
        self.escaped_not_unit = 0   # escapes with a weight other than 1

    def _wall(self, side, w):
        """a facet event at the mesh's wall through `side`: True where the history escapes"""
        if (self.vacuum >> side) & 1:
            self.escaped[side] += 1
            self.escape_weight[side] += w
            self.escaped_not_unit += 1 if w != 1.0 else 0
            return True
        self.reflections[side] += 1
        self.wall_hits += 1
        return False

    def history(self, pid, master_key, s):
        """advances the state dict `s` of particle `pid` by one timestep (omp3/neutral.c:103-197)"""
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
        wc, ws = self.roulette
        while left > 0.0:
            cell_mfp = 1.0 / (sig_s + sig_a)
            d_facet, x_facet = self._facet(x, y, ox, oy, speed, cx, cy)
            d_coll = mfp * cell_mfp
            d_census = speed * left
            if d_coll < d_facet and d_coll < d_census:      # collision_event :209-300
                self.ncollisions += 1
                self._segment(w, d_coll, ox, oy, e, cx, cy)
                self.collisions[cy, cx] += 1
                g = self._group(e, cx, cy)
                if g is not None:
                    self.coll[g] += w * cell_mfp * self.inv_n
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
                    if w < wc:
                        if rc1 * ws < w:
                            self.survived += 1
                            self.gained += ws - w
                            w = ws
                        else:
                            self.killed += 1
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
            elif d_facet < d_census:                        # facet_event :303-380
                self.nfacets += 1
                mfp -= d_facet / cell_mfp
                left -= d_facet / speed
                self._segment(w, d_facet, ox, oy, e, cx, cy)
                x, y = self._move(x, y, d_facet, ox, oy)
                # the outflow as Replay scores it; at the wall the history turns round -- or, where
                # the side is vacuum, escapes: dead where it is, direction unturned, its time over
                escaped = False
                if x_facet:
                    if ox > 0.0:
                        self.out[EAST, cy, cx] += w * self.inv_n
                        if cx >= p.nx - 1:
                            escaped = self._wall(EAST, w)
                            ox = ox if escaped else -ox
                        else:
                            cx += 1
                    elif ox < 0.0:
                        self.out[WEST, cy, cx] += w * self.inv_n
                        if cx <= 0:
                            escaped = self._wall(WEST, w)
                            ox = ox if escaped else -ox
                        else:
                            cx -= 1
                else:
                    if oy > 0.0:
                        self.out[NORTH, cy, cx] += w * self.inv_n
                        if cy >= p.ny - 1:
                            escaped = self._wall(NORTH, w)
                            oy = oy if escaped else -oy
                        else:
                            cy += 1
                    elif oy < 0.0:
                        self.out[SOUTH, cy, cx] += w * self.inv_n
                        if cy <= 0:
                            escaped = self._wall(SOUTH, w)
                            oy = oy if escaped else -oy
                        else:
                            cy -= 1
                if escaped:
                    s["dead"] = 1
                    break
                rho = float(p.density[cy * p.nx + cx])
                sig_s, sig_a = self._sigmas(rho, micro_s, micro_a)
            else:                                           # census_event :383-405
                self.ncensus += 1
                self._segment(w, d_census, ox, oy, e, cx, cy)
                x, y = self._move(x, y, d_census, ox, oy)
                left = 0.0
        s.update(x=x, y=y, omega_x=ox, omega_y=oy, energy=e, weight=w, cellx=cx, celly=cy)


def run_steps(rep, injected, steps, first_key=1, between=None):
    """`steps` timesteps (master keys first_key ...) of every history of `injected` (arrays by field)
    through `rep`; between(tt, states), where given, runs after step tt but the last.
    -> dict(states, snaps: the arrays before the first and after every step, per_step: what each step
    added to rep's counts)"""
    states = replay.states_of(injected)
    snaps, per_step = [replay.arrays_of(states)], []
    for tt in range(first_key, first_key + steps):
        before = (rep.nfacets, rep.ncollisions, rep.ncensus, list(rep.escaped), list(rep.escape_weight))
        alive = sum(1 for s in states if not s["dead"])
        for pid, s in enumerate(states):
            rep.history(pid, tt, s)
        per_step.append(dict(nprocessed=alive, facets=rep.nfacets - before[0], collisions=rep.ncollisions - before[1],
                             census=rep.ncensus - before[2],
                             escaped=[a - b for a, b in zip(rep.escaped, before[3])],
                             weight=[a - b for a, b in zip(rep.escape_weight, before[4])]))
        snaps.append(replay.arrays_of(states))
        if between is not None and tt < first_key + steps - 1:
            between(tt, states)
    return dict(states=states, snaps=snaps, per_step=per_step)


def exits_by_geometry(x, y, ox, oy, width, height):
    """Where the straight line from (x, y) along (ox, oy) leaves the box [0, width] x [0, height], by
    nothing but the four wall distances: -> (side, exit x, exit y, distance of the line from the
    nearest corner of the box), arrays.  No event loop, no cells."""
    x, y, ox, oy = (np.asarray(a, dtype=np.float64) for a in (x, y, ox, oy))
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(ox > 0.0, (width - x) / ox, np.where(ox < 0.0, (0.0 - x) / ox, np.inf))
        ty = np.where(oy > 0.0, (height - y) / oy, np.where(oy < 0.0, (0.0 - y) / oy, np.inf))
    by_x = tx < ty
    t = np.where(by_x, tx, ty)
    side = np.where(by_x, np.where(ox > 0.0, EAST, WEST), np.where(oy > 0.0, NORTH, SOUTH))
    ex, ey = x + t * ox, y + t * oy
    ex = np.where(by_x, np.where(ox > 0.0, width, 0.0), ex)
    ey = np.where(by_x, ey, np.where(oy > 0.0, height, 0.0))
    corner = np.full(x.shape, np.inf)
    for px in (0.0, width):
        for py in (0.0, height):
            corner = np.minimum(corner, np.abs((px - x) * oy - (py - y) * ox))   # (|omega| = 1)
    return side, ex, ey, corner

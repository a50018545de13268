"""The one Python restatement of the event loop: a deliberately naive replay of one history at a
time in Python floats, written from the text of include/neutral_hip.h and the event loop of
omp3/neutral.c:134-197.  The CPU oracle is frozen, so this replay is the reference of every tally
the oracle does not score (the outflow: tests/test_outflow.py) and the second opinion on those it
does (tests/test_oracle_tallies.py); it is pinned itself by hand-computed flights and by walking
the oracle's histories event for event.  A new tally is scored HERE, not in a copy of the loop.

Borrowed from the oracle are only the three pieces pinned on their own (tests/test_oracle_pins.py):
the random numbers, the table lookup and the distance to the facet.

Outflow sides: 0 west (-x), 1 east (+x), 2 south (-y), 3 north (+y)."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob
from closed_form import AVOGADROS, BARNS, EV_TO_J, MASS_NO, MOLAR_MASS, PARTICLE_MASS

MIN_ENERGY_OF_INTEREST = 1.0   # neutral_data.h:23
WEST, EAST, SOUTH, NORTH = 0, 1, 2, 3
FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "cellx", "celly", "dead")


def speed_of(energy_ev):
    return math.sqrt((2.0 * energy_ev * EV_TO_J) / PARTICLE_MASS)   # omp3/neutral.c:117


class Replay:
    """Scores, of the histories it is asked to advance, into (ny, nx) arrays: the collisions, the
    absorbed weight, the scalar flux, the current Jx and Jy and the four outflow meshes `out`;
    by group, where `edges` are given: the spectrum's track-length and collision estimators over
    `box` = (x0, y0, x1, y1) in cells, half-open (None: every cell); and roulette's four numbers,
    the facet and collision events and the wall hits.  cs_absorb may differ from cs_scatter;
    roulette = (cutoff, survival), (0, 0) off.  `dt` overrides the deck's timestep (hand-computed
    flights)."""

    def __init__(self, prob, cs_scatter, cs_absorb=None, roulette=(0.0, 0.0), dt=None, edges=(), box=None):
        self.p = prob
        self.cs_s = ob.CsTable(*cs_scatter)
        self.cs_a = ob.CsTable(*(cs_absorb if cs_absorb is not None else cs_scatter))
        self.roulette = tuple(float(v) for v in roulette)
        self.dt = float(prob.dt if dt is None else dt)
        self.edges, self.box = [float(e) for e in edges], box
        self.inv_n = 1.0 / prob.nparticles
        self.collisions, self.absorbed, self.flux, self.jx, self.jy = (np.zeros((prob.ny, prob.nx))
                                                                       for _ in range(5))
        self.out = np.zeros((4, prob.ny, prob.nx))
        self.track = [0.0] * max(len(self.edges) - 1, 0)
        self.coll = [0.0] * max(len(self.edges) - 1, 0)
        self.killed = self.survived = 0
        self.lost = self.gained = 0.0
        self.ncollisions = self.nfacets = self.wall_hits = 0
        self.edgex = np.ascontiguousarray(prob.edgex, dtype=np.float64)
        self.edgey = np.ascontiguousarray(prob.edgey, dtype=np.float64)

    def _group(self, energy, cx, cy):
        """the spectrum's group of a flight at `energy` in cell (cx, cy); None: not scored"""
        if self.box is not None:
            x0, y0, x1, y1 = self.box
            if not (x0 <= cx < x1 and y0 <= cy < y1):
                return None
        for g in range(len(self.edges) - 1):
            if self.edges[g] <= energy < self.edges[g + 1]:
                return g
        return None

    def _segment(self, weight, length, ox, oy, energy, cx, cy):
        self.flux[cy, cx] += weight * length * self.inv_n
        self.jx[cy, cx] += weight * length * ox * self.inv_n
        self.jy[cy, cx] += weight * length * oy * self.inv_n
        g = self._group(energy, cx, cy)
        if g is not None:
            self.track[g] += weight * length * self.inv_n

    def _facet(self, x, y, ox, oy, speed, cx, cy):
        d, xf = C.c_double(), C.c_int()
        ob.lib().orc_calc_distance_to_facet(x, y, 0, 0, 0, ox, oy, speed, cx, cy, C.byref(d), C.byref(xf),
                                            self.edgex.ctypes.data_as(C.POINTER(C.c_double)),
                                            self.edgey.ctypes.data_as(C.POINTER(C.c_double)))
        return d.value, xf.value

    def _sigmas(self, rho, micro_s, micro_a):
        per_density = AVOGADROS / MOLAR_MASS
        return (rho * per_density) * micro_s * BARNS, (rho * per_density) * micro_a * BARNS

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
                x += d_coll * ox
                y += d_coll * oy
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
                x += d_facet * ox
                y += d_facet * oy
                # the outflow: the cell held, the weight flown with, the side by the direction
                # BEFORE any reflection; a zero cosine on the moving axis scores nothing
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
            else:                                           # census_event :383-405
                self._segment(w, d_census, ox, oy, e, cx, cy)
                x += d_census * ox
                y += d_census * oy
                left = 0.0
        s.update(x=x, y=y, omega_x=ox, omega_y=oy, energy=e, weight=w, cellx=cx, celly=cy)


def states_of(arrays, n=None):
    """a list of per-particle state dicts (Python scalars) from arrays by field"""
    n = len(arrays["x"]) if n is None else n
    return [{f: arrays[f][i].item() for f in FIELDS} for i in range(n)]


def arrays_of(states):
    return {f: np.array([s[f] for s in states]) for f in FIELDS}

"""The reference of the outflow tally (include/neutral_hip.h: neutral_hip_set_outflow_tally): a
replay of one history at a time in Python floats, written from the header's text and the event
loop of omp3/neutral.c:134-197, and the arithmetic of the conservation identities the tally
closes.  The CPU oracle does not score the outflow, so this replay is what the kernels are held
to, per cell and per side; it is pinned itself by hand-computed flights and by walking the
oracle's histories event for event (tests/test_outflow.py).

Borrowed from the oracle are only the three pieces pinned on their own (tests/test_oracle_pins.py):
the random numbers, the table lookup and the distance to the facet -- as `_Replay` of
tests/test_oracle_tallies.py does.

Sides: 0 west (-x), 1 east (+x), 2 south (-y), 3 north (+y)."""
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
    """Scores the four outflow meshes, the scalar flux and the absorbed weight of the histories
    it is asked to advance.  cs_absorb may differ from cs_scatter; roulette = (cutoff, survival),
    (0, 0) off.  `dt` overrides the deck's timestep (hand-computed flights)."""

    def __init__(self, prob, cs_scatter, cs_absorb=None, roulette=(0.0, 0.0), dt=None):
        self.p = prob
        self.cs_s = ob.CsTable(*cs_scatter)
        self.cs_a = ob.CsTable(*(cs_absorb if cs_absorb is not None else cs_scatter))
        self.roulette = tuple(float(v) for v in roulette)
        self.dt = float(prob.dt if dt is None else dt)
        self.inv_n = 1.0 / prob.nparticles
        self.out = np.zeros((4, prob.ny, prob.nx))
        self.flux = np.zeros((prob.ny, prob.nx))
        self.absorbed = np.zeros((prob.ny, prob.nx))
        self.killed = self.survived = 0
        self.lost = self.gained = 0.0
        self.ncollisions = self.nfacets = self.wall_hits = 0
        self.edgex = np.ascontiguousarray(prob.edgex, dtype=np.float64)
        self.edgey = np.ascontiguousarray(prob.edgey, dtype=np.float64)

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
                self.flux[cy, cx] += w * d_coll * self.inv_n
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
                self.flux[cy, cx] += w * d_facet * self.inv_n
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
                self.flux[cy, cx] += w * d_census * self.inv_n
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

"""The one Python restatement of the event loop: a deliberately naive replay of one history at a
time in Python floats, written from the text of include/neutral_hip.h and the event loop of
omp3/neutral.c:134-197.  The CPU oracle is frozen, so this replay is the reference of every tally
the oracle does not score (the outflow: tests/test_outflow.py) and the second opinion on those it
does (tests/test_oracle_tallies.py); it is pinned itself by hand-computed flights and by walking
the oracle's histories event for event.  A new tally is scored HERE, not in a copy of the loop;
and a rule that differs by configuration is one of the loop's two hooks, not a second loop: which
cutoff an absorption plays roulette against (Replay._cutoff: the global pair, or the in-step
window's bound of the bin) and what the mesh's wall does (Replay._wall: turn the history round,
or, through a vacuum side, let it escape).

Borrowed from the oracle are only the three pieces pinned on their own (tests/test_oracle_pins.py):
the random numbers, the table lookup and the distance to the facet.

Outflow sides: 0 west (-x), 1 east (+x), 2 south (-y), 3 north (+y)."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob
from window_roulette_reference import bin_of
from closed_form import AVOGADROS, BARNS, EV_TO_J, MASS_NO, MOLAR_MASS, PARTICLE_MASS

MIN_ENERGY_OF_INTEREST = 1.0   # neutral_data.h:23
WEST, EAST, SOUTH, NORTH = 0, 1, 2, 3
FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "cellx", "celly", "dead")


def _scaled_integer(v):
    """(m, e) with v == m * 2^e, m an integer"""
    m, e = math.frexp(v)
    return int(math.ldexp(m, 53)), e - 53


def fma(a, b, c):
    """a * b + c rounded once, as a fused multiply-add rounds it: the exact sum as an integer times
    a power of two, which float() rounds to nearest-even.  (Results in the normal range, which is
    where a history's coordinates, energies and cosines are.)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)) or a == 0.0 or b == 0.0 or c == 0.0:
        return a * b + c   # (nothing to fuse: one rounding at most as it stands)
    (ma, ea), (mb, eb), (mc, ec) = _scaled_integer(a), _scaled_integer(b), _scaled_integer(c)
    e = min(ea + eb, ec)
    total = ((ma * mb) << (ea + eb - e)) + (mc << (ec - e))
    if total == 0:
        return a * b + c   # (an exact zero: the product is -c itself, and the sum has the sign IEEE gives it)
    excess = total.bit_length() - 64
    if excess > 0:         # 64 bits and a sticky one round like the whole integer
        sign, mag = (-1 if total < 0 else 1), abs(total)
        total = sign * ((mag >> excess) | (1 if mag & ((1 << excess) - 1) else 0))
        e += excess
    return math.ldexp(float(total), e)


def speed_of(energy_ev):
    return math.sqrt((2.0 * energy_ev * EV_TO_J) / PARTICLE_MASS)   # omp3/neutral.c:117


class Window:
    """The in-step weight window (include/neutral_hip.h: neutral_hip_set_window_roulette): `lower`,
    the flat mesh of bounds (max(G, 1) * cny * cnx values), `ratio`, the survival ratio, and what
    the bins are: `edges`, the window's own G + 1 group edges (None: no groups), and `block` =
    (block_x, block_y) cells per bin (None: 1 x 1)."""

    def __init__(self, lower, ratio, edges=None, block=None):
        self.lower = np.asarray(lower, dtype=np.float64).ravel()
        self.ratio = float(ratio)
        self.edges = None if edges is None else [float(e) for e in edges]
        self.block = block


class Replay:
    """Scores, of the histories it is asked to advance, into (ny, nx) arrays: the collisions, the
    absorbed weight, the scalar flux, the current Jx and Jy and the four outflow meshes `out`;
    by group, where `edges` are given: the spectrum's track-length and collision estimators over
    `box` = (x0, y0, x1, y1) in cells, half-open (None: every cell); and roulette's four numbers,
    the facet and collision events and the wall hits.  cs_absorb may differ from cs_scatter;
    roulette = (cutoff, survival), (0, 0) off; or `window`, a Window: the cutoff of an absorption
    is the bound of its bin and the survival weight fl(ratio * cutoff).  `vacuum` is a mask over the
    four sides (1 << side): a facet event that would reflect through such a side leaves the history
    dead on the wall, with the direction it came with, and ends its time.  `dt` overrides the
    deck's timestep (hand-computed flights).

    Counted besides: the census events, the reflections and the escapes by side with the sum of
    the escapes' weights and how many escaped with a weight other than 1; the ids that played
    roulette at least once; and per bin of the window the absorptions, the kills and the survivals
    (the caller reads killed / survived / lost / gained between steps, or run_steps does).

    fused: the sums of products that the oracle's build (oracle/Makefile: -O3 on an ISA with fused
    multiply-add) rounds once are rounded once here too -- every move x += d * omega, and in a
    scatter the energy factor, the cosine, 1 - cos^2 and the rotation, operand for operand as
    `objdump -d oracle/liboracle.so` shows them -- so that the fields of a history are the
    oracle's bits, not only its decisions (tests/test_degenerate_geometry.py)."""

    def __init__(self, prob, cs_scatter, cs_absorb=None, roulette=(0.0, 0.0), dt=None, edges=(), box=None,
                 fused=False, vacuum=0, window=None):
        self.p = prob
        self.fused = bool(fused)
        self.cs_s = ob.CsTable(*cs_scatter)
        self.cs_a = ob.CsTable(*(cs_absorb if cs_absorb is not None else cs_scatter))
        self.roulette = tuple(float(v) for v in roulette)
        self.window, self.vacuum = window, int(vacuum)
        assert 0 <= self.vacuum <= 15
        assert window is None or self.roulette == (0.0, 0.0)   # (the library lets one exclude the other)
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
        self.ncollisions = self.nfacets = self.wall_hits = self.ncensus = 0
        self.reflections, self.escaped, self.escape_weight = [0, 0, 0, 0], [0, 0, 0, 0], [0.0, 0.0, 0.0, 0.0]
        self.escaped_not_unit = 0   # escapes with a weight other than 1
        self.played = set()         # ids that played roulette at least once
        nbins = 0 if window is None else window.lower.size
        self.absorptions, self.killed_in, self.survived_in = (np.zeros(nbins, dtype=np.int64) for _ in range(3))
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

    def _move(self, x, y, d, ox, oy):
        if self.fused:
            return fma(d, ox, x), fma(d, oy, y)
        return x + d * ox, y + d * oy

    def _facet(self, x, y, ox, oy, speed, cx, cy):
        d, xf = C.c_double(), C.c_int()
        ob.lib().orc_calc_distance_to_facet(x, y, 0, 0, 0, ox, oy, speed, cx, cy, C.byref(d), C.byref(xf),
                                            self.edgex.ctypes.data_as(C.POINTER(C.c_double)),
                                            self.edgey.ctypes.data_as(C.POINTER(C.c_double)))
        return d.value, xf.value

    def _sigmas(self, rho, micro_s, micro_a):
        per_density = AVOGADROS / MOLAR_MASS
        return (rho * per_density) * micro_s * BARNS, (rho * per_density) * micro_a * BARNS

    def _cutoff(self, w, cx, cy, e):
        """An absorption in cell (cx, cy) at energy `e` that left the weight `w`: -> (bin, cutoff,
        survival weight).  The global pair and no bin; under a window the bound of the bin (no bin:
        0, nothing plays) and, once w is under it, fl(ratio * bound)."""
        if self.window is None:
            return (None,) + self.roulette
        b = bin_of(cx, cy, e, self.p.nx, self.p.ny, self.window.edges, self.window.block)
        if b is None:
            return None, 0.0, None
        self.absorptions[b] += 1
        wc = float(self.window.lower[b])
        return b, wc, (self.window.ratio * wc if w < wc else None)

    def _wall(self, side, w):
        """a facet event at the mesh's wall through `side` with weight `w`: True where the history
        escapes, False where it turns round"""
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
                    b, wc, ws = self._cutoff(w, cx, cy, e)
                    if w < wc:
                        self.played.add(pid)
                        if rc1 * ws < w:
                            self.survived += 1
                            if b is not None:
                                self.survived_in[b] += 1
                            self.gained += ws - w
                            w = ws
                        else:
                            self.killed += 1
                            if b is not None:
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
            elif d_facet < d_census:                        # facet_event :303-380
                self.nfacets += 1
                mfp -= d_facet / cell_mfp
                left -= d_facet / speed
                self._segment(w, d_facet, ox, oy, e, cx, cy)
                x, y = self._move(x, y, d_facet, ox, oy)
                # the outflow: the cell held, the weight flown with, the side by the direction
                # BEFORE any reflection; a zero cosine on the moving axis scores nothing.  At the
                # mesh's wall the history turns round or escapes: dead where it is, direction
                # unturned, its time over without a census
                cosine = ox if x_facet else oy
                if cosine != 0.0:
                    side = (EAST if ox > 0.0 else WEST) if x_facet else (NORTH if oy > 0.0 else SOUTH)
                    self.out[side, cy, cx] += w * self.inv_n
                    to = (cx if x_facet else cy) + (1 if cosine > 0.0 else -1)
                    if 0 <= to < (p.nx if x_facet else p.ny):
                        cx, cy = (to, cy) if x_facet else (cx, to)
                    elif self._wall(side, w):
                        s["dead"] = 1
                        break
                    else:
                        ox, oy = (-ox, oy) if x_facet else (ox, -oy)
                rho = float(p.density[cy * p.nx + cx])
                sig_s, sig_a = self._sigmas(rho, micro_s, micro_a)
            else:                                           # census_event :383-405
                self.ncensus += 1
                self._segment(w, d_census, ox, oy, e, cx, cy)
                x, y = self._move(x, y, d_census, ox, oy)
                left = 0.0
        s.update(x=x, y=y, omega_x=ox, omega_y=oy, energy=e, weight=w, cellx=cx, celly=cy)


def states_of(arrays, n=None):
    """a list of per-particle state dicts (Python scalars) from arrays by field"""
    n = len(arrays["x"]) if n is None else n
    return [{f: arrays[f][i].item() for f in FIELDS} for i in range(n)]


def arrays_of(states):
    return {f: np.array([s[f] for s in states]) for f in FIELDS}


MESHES = ("collisions", "absorbed", "flux", "jx", "jy", "out")
_COUNTS = dict(facets="nfacets", collisions="ncollisions", census="ncensus", wall_hits="wall_hits", killed="killed",
               survived="survived", lost="lost", gained="gained")
_BY_SIDE = dict(escaped="escaped", weight="escape_weight", reflections="reflections")


def run_steps(rep, injected, steps, first_key=1, keys=None, between=None):
    """The one step loop: every history of `injected` (arrays by field; an "id" array beside them
    names the histories' ids, which are 0, 1, ... without it) through `rep` for `steps` timesteps
    with the master keys first_key, first_key + 1, ... or those of `keys`; between(key, states),
    where given, runs after every step but the last.
    -> dict(states; snaps: the arrays before the first and after every step; meshes: rep's MESHES,
    copied when each snap was taken; per_step: the histories alive at the step's start as
    nprocessed, and what the step added to rep's counts -- the keys of _COUNTS, and lists by side
    for those of _BY_SIDE)"""
    keys = list(range(first_key, first_key + steps)) if keys is None else list(keys)
    states = states_of(injected)
    ids = [int(i) for i in injected["id"]] if "id" in injected else range(len(states))

    def meshes_now():
        return {m: getattr(rep, m).copy() for m in MESHES}
    snaps, meshes, per_step = [arrays_of(states)], [meshes_now()], []
    for n, key in enumerate(keys):
        before = {k: getattr(rep, a) for k, a in _COUNTS.items()}
        before_by_side = {k: list(getattr(rep, a)) for k, a in _BY_SIDE.items()}
        grew = dict(nprocessed=sum(1 for s in states if not s["dead"]))
        for pid, s in zip(ids, states):
            rep.history(pid, key, s)
        grew.update({k: getattr(rep, a) - before[k] for k, a in _COUNTS.items()})
        grew.update({k: [now - was for now, was in zip(getattr(rep, a), before_by_side[k])] for k, a in _BY_SIDE.items()})
        per_step.append(grew)
        snaps.append(arrays_of(states))
        meshes.append(meshes_now())
        if between is not None and n < len(keys) - 1:
            between(key, states)
    return dict(states=states, snaps=snaps, meshes=meshes, per_step=per_step)

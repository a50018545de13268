"""The references of periodic axes (include/neutral_hip.h: neutral_hip_set_periodic_axes).  No second
event loop: tests/replay.py's, used two ways that share nothing but its history().

A. chained(): the collision-free reference, bit for bit.  escape_bank_reference.BankReplay with the
   periodic sides vacuum advances a history until it leaves; its record holds the bits on the wall
   and the time left.  The header's rule is applied by hand -- ONE addition of the shift, the
   opposite outermost cell, dead = 0 -- and history() is called again with the same id and key for
   the time left, until the history no longer leaves through a periodic side.  The restart redraws
   mfp_to_collision, so this is the periodic run only where nothing collides.

B. Lattice: a periodic mesh is one cell of an infinite lattice.  replay.Replay with no wall rule at
   all on KX x KY copies of the problem -- edges edge[i] + k * W, density tiled, histories started
   in the middle copy -- whose states and meshes are folded back: cells mod n, positions minus
   k * W, meshes summed over the copies.  Valid while no history reaches the lattice's own wall
   (rep.wall_hits == 0 and sum(rep.escaped) == 0: the caller asserts it).  A reflecting axis is
   one copy along it.

Sides: 0 west, 1 east, 2 south, 3 north; a wrap is counted by the side LEFT through."""
import types

import numpy as np

import replay
from escape_bank_reference import BankReplay

W, E, S, N = replay.WEST, replay.EAST, replay.SOUTH, replay.NORTH


def sides_of(axes):
    """the outer sides of the axes in a periodic mask, as a vacuum mask"""
    return (3 if axes & 1 else 0) | (12 if axes & 2 else 0)


def extent(prob):
    """(W, H): fl(edge[n] - edge[0]) of the two axes, what a wrap adds or takes off"""
    ex = np.asarray(prob.edgex, dtype=np.float64)[prob.pad:]
    ey = np.asarray(prob.edgey, dtype=np.float64)[prob.pad:]
    return float(ex[prob.nx] - ex[0]), float(ey[prob.ny] - ey[0])


# ---- A. chained flights ---------------------------------------------------------------------------

def chained(prob, cs, injected, steps, axes, vacuum=0, dt=None, fused=False):
    """Every history of `injected` through `steps` timesteps (keys 1, 2, ...) with the axes of the mask
    `axes` periodic and the sides of `vacuum` (none of a periodic axis) vacuum.
    -> dict(rep, snaps: arrays before the first and after every step, per_step: dicts of nprocessed,
    facets, collisions, census, wrapped[4], escaped[4], reflections[4]; bank: the true escapes)"""
    assert sides_of(axes) & vacuum == 0
    periodic = sides_of(axes)
    width, height = extent(prob)
    rep = BankReplay(prob, cs, vacuum=periodic | vacuum, dt=dt, fused=fused)
    full = rep.dt
    states = replay.states_of(injected)
    snaps, per_step, escapes = [replay.arrays_of(states)], [], []
    for key in range(1, steps + 1):
        before = (rep.nfacets, rep.ncollisions, rep.ncensus, list(rep.reflections))
        grew = dict(nprocessed=sum(1 for s in states if not s["dead"]), wrapped=[0, 0, 0, 0], escaped=[0, 0, 0, 0])
        for pid, s in enumerate(states):
            rep.dt = full
            while True:
                held = len(rep.bank)
                rep.history(pid, key, s)
                if len(rep.bank) == held:
                    break                       # it no longer leaves
                record = rep.bank[-1]
                side = record["side"]
                if not (periodic >> side) & 1:
                    grew["escaped"][side] += 1  # a true escape: it stays dead, its record stays banked
                    escapes.append(record)
                    break
                rep.bank.pop()
                grew["wrapped"][side] += 1
                if side == W:
                    s["x"], s["cellx"] = s["x"] + width, prob.nx - 1
                elif side == E:
                    s["x"], s["cellx"] = s["x"] - width, 0
                elif side == S:
                    s["y"], s["celly"] = s["y"] + height, prob.ny - 1
                else:
                    s["y"], s["celly"] = s["y"] - height, 0
                s["dead"] = 0
                rep.dt = record["time_left"]
        rep.dt = full
        grew.update(facets=rep.nfacets - before[0], collisions=rep.ncollisions - before[1],
                    census=rep.ncensus - before[2],
                    reflections=[now - was for now, was in zip(rep.reflections, before[3])])
        per_step.append(grew)
        snaps.append(replay.arrays_of(states))
    return dict(rep=rep, snaps=snaps, per_step=per_step, bank=escapes)


# ---- B. the unfolded lattice ----------------------------------------------------------------------

class _SeamCounting(np.ndarray):
    """the outflow meshes of the lattice, counting the scores on a seam: replay's loop adds to
    out[side, cy, cx] once per facet event with a cosine that is not zero, and the event is a wrap of
    the folded mesh where the cell is an outermost one of its copy on that side"""

    def __setitem__(self, index, value):
        seams = getattr(self, "seams", None)
        if seams is not None and isinstance(index, tuple) and len(index) == 3:
            side, cy, cx = index
            nx, ny, wrapped, periodic = seams
            at = (cx % nx == 0, cx % nx == nx - 1, cy % ny == 0, cy % ny == ny - 1)[side]
            if at and (periodic >> side) & 1:
                wrapped[side] += 1
        super().__setitem__(index, value)


class Lattice:
    """KX x KY copies of `prob` (a reflecting axis: one copy) and the replay on them"""

    def __init__(self, prob, kx=1, ky=1):
        assert prob.pad == 0
        self.p, self.kx, self.ky = prob, int(kx), int(ky)
        self.width, self.height = extent(prob)
        nx, ny = prob.nx, prob.ny
        ex = np.asarray(prob.edgex, dtype=np.float64)
        ey = np.asarray(prob.edgey, dtype=np.float64)
        edgex = np.array([ex[i] + k * self.width for k in range(self.kx) for i in range(nx)] +
                         [ex[nx] + (self.kx - 1) * self.width])
        edgey = np.array([ey[i] + k * self.height for k in range(self.ky) for i in range(ny)] +
                         [ey[ny] + (self.ky - 1) * self.height])
        density = np.tile(np.asarray(prob.density, dtype=np.float64).reshape(ny, nx), (self.ky, self.kx)).ravel()
        self.unfolded = types.SimpleNamespace(nx=nx * self.kx, ny=ny * self.ky, pad=0, dt=prob.dt, edgex=edgex,
                                              edgey=edgey, density=density, nparticles=prob.nparticles)

    def lift(self, arrays, copy=None):
        """the arrays by field, moved into copy (cx, cy) of the lattice (default: the middle one)"""
        cx, cy = (self.kx // 2, self.ky // 2) if copy is None else copy
        out = {f: np.array(a, copy=True) for f, a in arrays.items()}
        out["x"] = out["x"] + cx * self.width
        out["y"] = out["y"] + cy * self.height
        out["cellx"] = out["cellx"] + cx * self.p.nx
        out["celly"] = out["celly"] + cy * self.p.ny
        return out

    def fold(self, arrays):
        """the arrays by field, folded back: cells mod n, positions minus k * W"""
        out = {f: np.array(a, copy=True) for f, a in arrays.items()}
        kx, ky = out["cellx"] // self.p.nx, out["celly"] // self.p.ny
        out["x"] = out["x"] - kx * self.width
        out["y"] = out["y"] - ky * self.height
        out["cellx"] = out["cellx"] - kx * self.p.nx
        out["celly"] = out["celly"] - ky * self.p.ny
        return out

    def fold_mesh(self, mesh):
        """(..., KY * ny, KX * nx) -> (..., ny, nx): the copies summed"""
        mesh = np.asarray(mesh)
        nx, ny = self.p.nx, self.p.ny
        parts = mesh.reshape(mesh.shape[:-2] + (self.ky, ny, self.kx, nx))
        return parts.sum(axis=(-4, -2))

    def lift_mesh(self, mesh):
        """(ny, nx) -> the lattice's mesh with every copy holding `mesh` (a window's bounds)"""
        return np.tile(np.asarray(mesh).reshape(self.p.ny, self.p.nx), (self.ky, self.kx))

    def run(self, cs, injected, steps, copy=None, between=None, keys=None, **replay_kw):
        """replay.run_steps on the lattice from `injected` (arrays on the folded mesh) with the master
        keys 1, 2, ... or those of `keys`; between(key, states, lattice), where given, sees the
        lattice's own state dicts.
        -> dict(rep; snaps: folded arrays per step; meshes: folded MESHES per step; per_step: replay's,
        each with `wrapped`, the step's seam crossings by the side left through; reach: the copies
        reached along x and y, [min, max] relative to the start's)"""
        rep = replay.Replay(self.unfolded, cs, **replay_kw)
        wrapped = [0, 0, 0, 0]
        out = rep.out.view(_SeamCounting)
        # (an axis of one copy is no seam: its outer sides are the mesh's own walls)
        out.seams = (self.p.nx, self.p.ny, wrapped, (3 if self.kx > 1 else 0) | (12 if self.ky > 1 else 0))
        rep.out = out
        start = (self.kx // 2, self.ky // 2) if copy is None else copy
        marks = [[0, 0, 0, 0]]

        def after_step(key, states):
            marks.append(list(wrapped))
            if between is not None:
                between(key, states, self)
        run = replay.run_steps(rep, self.lift(injected, copy), steps, keys=keys, between=after_step)
        marks.append(list(wrapped))   # (run_steps calls nothing after the last step)
        for grew, was, now in zip(run["per_step"], marks, marks[1:]):
            grew["wrapped"] = [b - a for a, b in zip(was, now)]
        reach = dict(x=[0, 0], y=[0, 0])
        for s in run["snaps"]:
            kx, ky = s["cellx"] // self.p.nx - start[0], s["celly"] // self.p.ny - start[1]
            reach["x"] = [min(reach["x"][0], int(kx.min())), max(reach["x"][1], int(kx.max()))]
            reach["y"] = [min(reach["y"][0], int(ky.min())), max(reach["y"][1], int(ky.max()))]
        meshes = [{m: self.fold_mesh(np.asarray(v)) for m, v in step.items()} for step in run["meshes"]]
        return dict(rep=rep, snaps=[self.fold(s) for s in run["snaps"]], meshes=meshes, per_step=run["per_step"],
                    wrapped=list(wrapped), reach=reach)


def seam_density(prob):
    """the density mesh of the runs that collide, in place: 0.3, the three west columns 0.05, the four
    south rows 1.0 -- both seams join different materials"""
    mesh = prob.density.reshape(prob.ny, prob.nx)
    mesh[:] = 0.3
    mesh[:, :3] = 0.05
    mesh[:4, :] = 1.0
    return prob


def outer(out):
    """the outflow's entries on the mesh's four outer sides"""
    return (out[W][:, 0], out[E][:, -1], out[S][0, :], out[N][-1, :])

"""The net current of collision-free flights, restated in numpy from the definition alone.

A particle of weight 1 that never collides flies straight, turns round at the mesh's outer
edges (every boundary reflects) and lays down `length` of path per timestep.  The current
tally's definition (include/neutral_hip.h) then says what every cell receives:

    jx[cell] += segment length * omega_x,   jy[cell] += segment length * omega_y

for every piece of the flight between two cell edges (or its start, or its end), scored in
the cell the piece lies in with the direction it was flown with -- a piece that ends on a
wall is scored before the wall flips the sign.  No 1/N here: the caller divides.

`march()` walks all particles at once, one cell edge per trip.  The mesh is uniform: nx x ny
cells over [0, width] x [0, height], edge i of an axis at i * (extent / n).  Nothing of the
library is used -- the inputs are positions, directions and cells.
"""
import numpy as np


def cells_of(x, y, nx, ny, width=1.0, height=1.0):
    """The cell each position lies in (a position on an edge belongs to the cell above it)."""
    cx = np.clip(np.floor(np.asarray(x) / (width / nx)).astype(np.int64), 0, nx - 1)
    cy = np.clip(np.floor(np.asarray(y) / (height / ny)).astype(np.int64), 0, ny - 1)
    return cx, cy


def march(x, y, omega_x, omega_y, length, nx, ny, width=1.0, height=1.0, cellx=None, celly=None):
    """Flies every particle `length` (a scalar or one value per particle) through the mesh.

    Returns (jx, jy, state): the two (ny, nx) meshes of sum(segment * omega), and the
    particles' end state as a dict (x, y, omega_x, omega_y, cellx, celly, reflections) --
    which a further call takes up again for the next timestep."""
    x = np.array(x, dtype=np.float64)
    y = np.array(y, dtype=np.float64)
    ox = np.array(omega_x, dtype=np.float64)
    oy = np.array(omega_y, dtype=np.float64)
    n = x.size
    if cellx is None or celly is None:
        cellx, celly = cells_of(x, y, nx, ny, width, height)
    cx = np.array(cellx, dtype=np.int64)
    cy = np.array(celly, dtype=np.int64)
    left = np.broadcast_to(np.asarray(length, dtype=np.float64), (n,)).copy()
    dx, dy = width / nx, height / ny
    jx = np.zeros(ny * nx)
    jy = np.zeros(ny * nx)
    reflections = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    trips = 0
    while live.size:
        trips += 1
        assert trips < 64 * (nx + ny) * 16, "the march does not end"
        lx, ly, lox, loy, lcx, lcy, ll = x[live], y[live], ox[live], oy[live], cx[live], cy[live], left[live]
        # the edge ahead on each axis, and how far it is along the flight
        tx = np.where(lox > 0.0, (lcx + 1) * dx, lcx * dx)
        ty = np.where(loy > 0.0, (lcy + 1) * dy, lcy * dy)
        with np.errstate(divide="ignore", invalid="ignore"):
            dist_x = np.where(lox != 0.0, np.maximum((tx - lx) / lox, 0.0), np.inf)
            dist_y = np.where(loy != 0.0, np.maximum((ty - ly) / loy, 0.0), np.inf)
        to_edge = np.minimum(dist_x, dist_y)
        ends = ll <= to_edge                      # the timestep ends inside this cell
        seg = np.where(ends, ll, to_edge)
        cell = lcy * nx + lcx
        np.add.at(jx, cell, seg * lox)            # (the direction BEFORE a reflection)
        np.add.at(jy, cell, seg * loy)
        lx = lx + seg * lox
        ly = ly + seg * loy
        ll = np.where(ends, 0.0, ll - seg)
        crosses_x = ~ends & (dist_x <= dist_y)
        crosses_y = ~ends & ~crosses_x
        lx = np.where(crosses_x, tx, lx)          # (on the edge, exactly)
        ly = np.where(crosses_y, ty, ly)
        step_x = np.where(lox > 0.0, 1, -1)
        step_y = np.where(loy > 0.0, 1, -1)
        wall_x = crosses_x & (((lox > 0.0) & (lcx == nx - 1)) | ((lox < 0.0) & (lcx == 0)))
        wall_y = crosses_y & (((loy > 0.0) & (lcy == ny - 1)) | ((loy < 0.0) & (lcy == 0)))
        lcx = np.where(crosses_x & ~wall_x, lcx + step_x, lcx)
        lcy = np.where(crosses_y & ~wall_y, lcy + step_y, lcy)
        lox = np.where(wall_x, -lox, lox)
        loy = np.where(wall_y, -loy, loy)
        x[live], y[live], ox[live], oy[live], cx[live], cy[live], left[live] = lx, ly, lox, loy, lcx, lcy, ll
        reflections[live] += (wall_x | wall_y).astype(np.int64)
        live = live[~ends]
    state = dict(x=x, y=y, omega_x=ox, omega_y=oy, cellx=cx, celly=cy, reflections=reflections)
    return jx.reshape(ny, nx), jy.reshape(ny, nx), state

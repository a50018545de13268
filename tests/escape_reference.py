"""Where a history leaves a collision-free box, by nothing but straight-line geometry: the second
opinion on vacuum sides (include/neutral_hip.h: neutral_hip_set_vacuum_sides) in
tests/test_vacuum.py.  The event loop with the vacuum rule is tests/replay.py's own, through its
wall hook (Replay(vacuum=...)).

Sides, as the outflow numbers them: 0 west (-x), 1 east (+x), 2 south (-y), 3 north (+y)."""
import numpy as np

from replay import EAST, NORTH, SOUTH, WEST


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

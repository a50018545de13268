"""Degenerate starting states: the inputs where the event loop stops being straight-line
arithmetic, and which injection's random positions and angles hit with probability zero.  One
builder, shared by the CPU and GPU tests of tests/test_degenerate_geometry.py.

  * a direction cosine that is exactly zero (an infinite reciprocal; a wave whose vote sends it
    through the wrapped divisions), and one that is tiny and not zero;
  * a start exactly on a cell's edge or corner (a distance of zero; with a zero cosine, 0 * inf);
  * omega = (s, s) from a cell's centre or corner: on square cells with power-of-two edges the two
    facet times are equal to the bit, and the flight goes through the cell's corner.

NO NEGATIVE ZERO ANYWHERE.  With a cosine of -0.0 the reference's own C gives u_inv = 1 / -0.0 =
-inf and from it a distance of -inf to the facet: there is nothing defined to compare with.  Both
builders assert that no -0.0 occurs in what they return.
"""
import math

import numpy as np

S = math.sqrt(0.5)   # one double: (S, S) has dt_x == dt_y wherever the two differences are equal

# direction i % 8
DIRECTIONS = (
    (1.0, 0.0),
    (0.0, 1.0),
    (-1.0, 0.0),
    (0.0, -1.0),
    (S, S),
    (-S, S),
    (math.cos(math.pi / 2), math.sin(math.pi / 2)),   # (6.1e-17, 1.0): a tiny non-zero cosine
    (S, -S),
)
AXIS_DIRECTIONS = DIRECTIONS[:4]

# placement (i // 8) % 4
CENTRE, CENTRE_AGAIN, CORNER, LEFT_EDGE = range(4)


def _no_negative_zero(*arrays):
    for a in arrays:
        a = np.asarray(a)
        if a.dtype.kind == "f":
            assert not np.any((a == 0.0) & np.signbit(a)), "a -0.0: the reference itself is undefined there"


def direction_of(i):
    return np.asarray(i) % 8


def placement_of(i):
    return (np.asarray(i) // 8) % 4


def place(edgex, edgey, cellx, celly, placement, pad=0):
    """(x, y) of `placement` in the cells (cellx, celly): 0 and 1 the centre, 2 the lower-left
    corner, 3 the middle of the left edge"""
    cellx, celly, placement = (np.asarray(a) for a in (cellx, celly, placement))
    x_lo, x_hi = edgex[cellx + pad], edgex[cellx + pad + 1]
    y_lo, y_hi = edgey[celly + pad], edgey[celly + pad + 1]
    x = np.where(placement >= CORNER, x_lo, 0.5 * (x_lo + x_hi))
    y = np.where(placement == CORNER, y_lo, 0.5 * (y_lo + y_hi))
    return x, y


def corpus(prob, n):
    """-> dict of x, y, omega_x, omega_y (float64), cellx, celly (int32) for particles 0 .. n-1:
    direction i % 8 of DIRECTIONS, cell (7 i mod nx, 13 i mod ny) -- every column and row, the four
    walls included -- and placement (i // 8) % 4.  No -0.0 (asserted)."""
    assert prob.x_off == 0 and prob.y_off == 0
    i = np.arange(n)
    d = np.array(DIRECTIONS, dtype=np.float64)[direction_of(i)]
    cellx = ((7 * i) % prob.nx).astype(np.int32)
    celly = ((13 * i) % prob.ny).astype(np.int32)
    edgex, edgey = (np.asarray(e, dtype=np.float64) for e in (prob.edgex, prob.edgey))
    x, y = place(edgex, edgey, cellx, celly, placement_of(i), prob.pad)
    out = dict(x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), omega_x=np.ascontiguousarray(d[:, 0]),
               omega_y=np.ascontiguousarray(d[:, 1]), cellx=cellx, celly=celly)
    _no_negative_zero(*out.values())
    return out


def beams(prob, cell, n):
    """-> the same dict for 4 n particles: n identical histories in each of the four axis
    directions (particle i flies along AXIS_DIRECTIONS[i // n]) from the centre of `cell` =
    (cellx, celly).  No -0.0 (asserted)."""
    assert prob.x_off == 0 and prob.y_off == 0
    cx, cy = cell
    d = np.repeat(np.array(AXIS_DIRECTIONS, dtype=np.float64), n, axis=0)
    cellx = np.full(4 * n, cx, dtype=np.int32)
    celly = np.full(4 * n, cy, dtype=np.int32)
    edgex, edgey = (np.asarray(e, dtype=np.float64) for e in (prob.edgex, prob.edgey))
    x, y = place(edgex, edgey, cellx, celly, np.zeros(4 * n, dtype=int), prob.pad)
    out = dict(x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), omega_x=np.ascontiguousarray(d[:, 0]),
               omega_y=np.ascontiguousarray(d[:, 1]), cellx=cellx, celly=celly)
    _no_negative_zero(*out.values())
    return out


def into_oracle(ref, states):
    """the states into an OracleRun's particle arrays (energy, weight, dt_to_census and
    mfp_to_collision stay as injection left them)"""
    arrays = ref.particles.as_dict()
    for f, a in states.items():
        assert len(a) == len(arrays[f])
        arrays[f][:] = a

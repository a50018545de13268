"""The bins of the in-step weight window (include/neutral_hip.h: neutral_hip_set_window_roulette)
restated in Python, in plain integer arithmetic: the group of an energy, the block of a cell, the
bin of a collision.

The CPU oracle is frozen and knows only the global cutoff, so the reference of a non-uniform mesh
is tests/replay.py's own loop, whose cutoff hook looks the bound up by bin_of (Replay(window=...));
that path is pinned against the global cutoff, which the oracle test pins, before anything on the
GPU is compared with it (tests/test_window_roulette.py)."""


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

"""The grouped census and the grouped window by their definition (include/neutral_hip.h: energy
groups for the census tally and the weight window): the plain restatements, as they are, on the
virtual store.

    group         g(E) = #{ i in 0 .. G : edges[i] <= E } - 1 where that lies in 0 .. G - 1, else G
                  ("outside": below edges[0], at or above edges[G], -0.0, negative, inf, NaN)
    virtual store slot j in row g_j * ny + celly[j] of a mesh of nx by (G + 1) * ny; block G of
                  lower is zeros
    window        window_reference.window on it; celly put back (a copy takes its source's)
    census        census_reference.census on it; block G sliced away, the stats taken from the rest

Nothing of the two operations is restated here.  `guarded` gains every live slot whose energy is
within GUARD (relative) of an edge: two implementations of the transport that agree to 1e-9 may put
such a slot into different groups.
"""
import math
from collections import namedtuple

import numpy as np

import census_reference as cr
import window_reference as wr

GROUPS_MAX = 64
GUARD = wr.GUARD
# the edges of one group that holds every positive finite energy but the largest
ALL_EMBRACING = (float(np.nextafter(0.0, 1.0)), float(np.finfo(np.float64).max))

# window_reference.Result and `outside`: the live slots in no group
GroupResult = namedtuple("GroupResult", wr.Result._fields + ("outside",))
# count, weight: (G * ny * nx,) float64; stats: the integer ones of NeutralHipGroupCensusStats by
# name, and weight (math.fsum over the bins' sums), max_bin_weight
GroupCensus = namedtuple("GroupCensus", "count weight stats")


def valid_edges(edges) -> bool:
    """1 .. 64 groups; every edge finite and > 0, strictly ascending"""
    e = np.asarray(edges, dtype=np.float64)
    return bool(e.ndim == 1 and 2 <= e.size <= GROUPS_MAX + 1 and np.all(np.isfinite(e)) and np.all(e > 0.0)
                and np.all(e[1:] > e[:-1]))


def groups_of(energy, edges):
    """-> g per slot, G for a slot outside"""
    e = np.asarray(edges, dtype=np.float64)
    ngroups = e.size - 1
    energy = np.asarray(energy, dtype=np.float64)
    count = np.zeros(energy.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for edge in e:
            count += edge <= energy
    g = count - 1
    return np.where((g >= 0) & (g < ngroups), g, ngroups)


def near_an_edge(energy, edges):
    """energies within GUARD (relative) of an edge"""
    energy = np.asarray(energy, dtype=np.float64)
    near = np.zeros(energy.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for edge in np.asarray(edges, dtype=np.float64):
            near |= np.abs(energy - edge) <= GUARD * edge
    return near


def virtual_store(arrays: dict, edges, ny: int):
    """-> (the store with slot j in row g_j * ny + celly[j], g).  None where a live slot's celly lies
    off the mesh: the virtual row would hide it from the plain restatement's check"""
    g = groups_of(arrays["energy"], edges)
    live = arrays["dead"] == 0
    cy = arrays["celly"].astype(np.int64)
    if np.any(live & ((cy < 0) | (cy >= ny))):
        return None
    out = {f: np.array(arrays[f]) for f in wr.FIELDS}
    out["celly"] = (g * ny + cy).astype(np.int32)
    return out, g


def window(arrays: dict, edges, lower, nx: int, ny: int, upper_ratio: float, survival_ratio: float,
           max_split: int, rn0_of):
    """-> GroupResult, or None where the call refuses (code 1) and changes nothing"""
    if not valid_edges(edges) or nx < 1 or ny < 1 or len(arrays["dead"]) <= 0:
        return None
    ngroups = len(edges) - 1
    lower = np.ascontiguousarray(lower, dtype=np.float64).ravel()
    if len(lower) != ngroups * ny * nx:
        return None
    made = virtual_store(arrays, edges, ny)
    if made is None:
        return None
    virtual, g = made
    r = wr.window(virtual, np.concatenate([lower, np.zeros(ny * nx)]), nx, (ngroups + 1) * ny, upper_ratio,
                  survival_ratio, max_split, rn0_of)
    if r is None:
        return None
    out = dict(r.arrays)
    out["celly"] = np.array(arrays["celly"])
    out["celly"][r.destinations] = arrays["celly"][r.sources]
    live = arrays["dead"] == 0
    guarded = r.guarded | (live & near_an_edge(arrays["energy"], edges))
    return GroupResult(*r._replace(arrays=out, guarded=guarded), outside=int((live & (g == ngroups)).sum()))


def census(arrays: dict, edges, nx: int, ny: int):
    """-> GroupCensus, or None where the call refuses (code 1) and the meshes hold zeros"""
    if not valid_edges(edges) or nx < 1 or ny < 1 or len(arrays["dead"]) <= 0:
        return None
    ngroups = len(edges) - 1
    made = virtual_store(arrays, edges, ny)
    if made is None:
        return None
    virtual, _ = made
    c = cr.census(virtual, nx, (ngroups + 1) * ny)
    if c is None:
        return None
    bins = ngroups * ny * nx
    count, weight = c.count[:bins], c.weight[:bins]
    stats = dict(live=c.stats["live"], dead=c.stats["dead"], outside=int(c.count[bins:].sum()),
                 occupied_bins=int((count > 0).sum()), max_count=int(count.max()), weight=math.fsum(weight),
                 max_bin_weight=float(weight.max()))
    return GroupCensus(count, weight, stats)

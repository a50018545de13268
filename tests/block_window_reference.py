"""The blocks census and the blocks window by their definition (include/neutral_hip.h: a coarse
window mesh): the plain or the grouped restatements, as they are, on the virtual store.

    check         every live slot on the REAL store: a cell off the mesh of nx by ny refuses (the
                  virtual cell might lie inside the coarse mesh: nx = 10, block_x = 4, cellx = 11 is
                  block 2 of 3); bad weights are the restatements' to refuse
    coarse mesh   cnx = ceil(nx / block_x), cny = ceil(ny / block_y)
    virtual store cellx' = cellx div block_x, celly' = celly div block_y
    window        window_reference.window (edges None) or group_window_reference.window on it, on
                  the mesh of cnx by cny; cellx and celly put back (a copy takes its source's)
    census        census_reference.census or group_window_reference.census on it

Nothing of the operations is restated here.
"""
import numpy as np

import census_reference as cr
import group_window_reference as gr
import window_reference as wr


def coarse(nx: int, ny: int, block):
    """-> (cnx, cny)"""
    bx, by = block
    return -(-nx // bx), -(-ny // by)


def valid_block(block) -> bool:
    return len(block) == 2 and all(isinstance(b, (int, np.integer)) and b >= 1 for b in block)


def virtual_store(arrays: dict, block, nx: int, ny: int):
    """-> the store with every slot in its block's cell of the coarse mesh (a dead slot's cells are
    divided like the others: nobody looks at them).  None where a live slot's cell lies off the
    mesh of nx by ny: the division would hide it from the restatements' check"""
    bx, by = block
    live = arrays["dead"] == 0
    cx, cy = arrays["cellx"].astype(np.int64), arrays["celly"].astype(np.int64)
    if np.any(live & ((cx < 0) | (cx >= nx) | (cy < 0) | (cy >= ny))):
        return None
    out = {f: np.array(arrays[f]) for f in wr.FIELDS}
    out["cellx"] = (cx // bx).astype(np.int32)
    out["celly"] = (cy // by).astype(np.int32)
    return out


def window(arrays: dict, block, edges, lower, nx: int, ny: int, upper_ratio: float, survival_ratio: float,
           max_split: int, rn0_of):
    """-> group_window_reference.GroupResult (outside 0 without groups), or None where the call
    refuses (code 1) and changes nothing.  edges None: no groups"""
    if not valid_block(block) or nx < 1 or ny < 1 or len(arrays["dead"]) <= 0:
        return None
    virtual = virtual_store(arrays, block, nx, ny)
    if virtual is None:
        return None
    cnx, cny = coarse(nx, ny, block)
    if edges is None:
        lower = np.ascontiguousarray(lower, dtype=np.float64).ravel()
        if len(lower) != cny * cnx:
            return None
        r = wr.window(virtual, lower, cnx, cny, upper_ratio, survival_ratio, max_split, rn0_of)
        r = None if r is None else gr.GroupResult(*r, outside=0)
    else:
        r = gr.window(virtual, edges, lower, cnx, cny, upper_ratio, survival_ratio, max_split, rn0_of)
    if r is None:
        return None
    out = dict(r.arrays)
    for f in ("cellx", "celly"):
        out[f] = np.array(arrays[f])
        out[f][r.destinations] = arrays[f][r.sources]
    return r._replace(arrays=out)


def census(arrays: dict, block, edges, nx: int, ny: int):
    """-> group_window_reference.GroupCensus over the B bins (outside 0 without groups), or None
    where the call refuses (code 1) and the meshes hold zeros"""
    if not valid_block(block) or nx < 1 or ny < 1 or len(arrays["dead"]) <= 0:
        return None
    virtual = virtual_store(arrays, block, nx, ny)
    if virtual is None:
        return None
    cnx, cny = coarse(nx, ny, block)
    if edges is not None:
        return gr.census(virtual, edges, cnx, cny)
    c = cr.census(virtual, cnx, cny)
    if c is None:
        return None
    stats = dict(live=c.stats["live"], dead=c.stats["dead"], outside=0, occupied_bins=c.stats["occupied_cells"],
                 max_count=c.stats["max_count"], weight=c.stats["weight"], max_bin_weight=c.stats["max_cell_weight"])
    return gr.GroupCensus(c.count, c.weight, stats)

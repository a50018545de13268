"""The census tally and the window bounds, restated in numpy (include/neutral_hip.h:
neutral_hip_census_tally, neutral_hip_window_bounds).

    census   a slot with dead != 0 is skipped; a live slot j scores 1 and weight[j] in the cell
             c = celly[j] * nx + cellx[j].  Counts by np.bincount; a cell's weight by math.fsum, the
             correctly rounded exact sum, which a sum of m non-negative terms in any order stays
             within (m - 1) * 2^-53 of (relative; first order)
    bounds   eligible(c): count_c >= min_count and W_c > 0; K of them, M = the largest W_c among them
             a = fl(2.0 * K), b = fl(a * M), d = fl(fl(1.0 + upper_ratio) * target_population),
             peak = fl(b / d); eligible: r = fl(W_c / M), lower_c = fl(fmax(r, floor_ratio) * peak);
             other cells 0.0

Every step of `bounds` is one numpy f64 operation per element, hence one IEEE operation: given the
same census mesh the device's result is these bits.
"""
import math
from collections import namedtuple

import numpy as np

F64_MAX = np.finfo(np.float64).max

# count, weight: (ny * nx,) float64; stats: the integer ones of NeutralHipCensusStats by name, and
# weight (math.fsum over the cells' sums), max_cell_weight
Census = namedtuple("Census", "count weight stats")
# lower: (ny * nx,) float64; eligible: the mask; ratio: fl(W_c / M) where eligible; stats:
# NeutralHipBoundsStats by name (peak is lower_at_peak)
Bounds = namedtuple("Bounds", "lower eligible ratio peak stats")


def census(arrays: dict, nx: int, ny: int):
    """-> Census, or None where the call refuses (code 1) and the meshes hold zeros"""
    n = len(arrays["dead"])
    if n <= 0 or nx < 1 or ny < 1:
        return None
    live = np.flatnonzero(arrays["dead"] == 0)
    cx, cy = arrays["cellx"][live].astype(np.int64), arrays["celly"][live].astype(np.int64)
    w = arrays["weight"][live]
    with np.errstate(invalid="ignore"):
        inside = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        if np.any(~inside | ~(w >= 0.0) | ~(w <= F64_MAX)):
            return None
    cell = cy * nx + cx
    count = np.bincount(cell, minlength=nx * ny).astype(np.float64)
    order = np.argsort(cell, kind="stable")
    ends = np.cumsum(count.astype(np.int64))
    sorted_w = w[order]
    weight = np.array([math.fsum(sorted_w[e - int(c):e]) for c, e in zip(count, ends)], dtype=np.float64)
    stats = dict(live=len(live), dead=n - len(live), occupied_cells=int((count > 0).sum()),
                 max_count=int(count.max()), weight=math.fsum(weight), max_cell_weight=float(weight.max()))
    return Census(count, weight, stats)


def valid_bounds_settings(target_population, upper_ratio, floor_ratio, min_count) -> bool:
    """what the call accepts before it looks at the census"""
    return bool(np.isfinite(target_population) and np.isfinite(upper_ratio) and target_population > 0.0
                and upper_ratio >= 2.0 and 0.0 <= floor_ratio <= 1.0 and min_count >= 1)


def bounds(count, weight, target_population: float, upper_ratio: float, floor_ratio: float, min_count: int):
    """-> Bounds, or None where the call refuses (code 1) and leaves lower_out as it was"""
    count = np.ascontiguousarray(count, dtype=np.float64).ravel()
    weight = np.ascontiguousarray(weight, dtype=np.float64).ravel()
    if len(count) < 1 or len(count) != len(weight) or \
            not valid_bounds_settings(target_population, upper_ratio, floor_ratio, min_count):
        return None
    with np.errstate(invalid="ignore"):
        both = np.concatenate([count, weight])
        if np.any(~(both >= 0.0) | ~(both <= F64_MAX)):
            return None
    eligible = (count >= np.float64(min_count)) & (weight > 0.0)
    k = int(eligible.sum())
    if k == 0:
        return None
    m = np.float64(weight[eligible].max())
    a = np.float64(2.0) * np.float64(k)
    b = a * m
    d = (np.float64(1.0) + np.float64(upper_ratio)) * np.float64(target_population)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        peak = b / d
        ratio = np.where(eligible, weight / m, 0.0)
        lower = np.where(eligible, np.fmax(ratio, np.float64(floor_ratio)) * peak, 0.0)
    stats = dict(windowed_cells=k, floored_cells=int((eligible & (ratio < floor_ratio)).sum()),
                 max_cell_weight=float(m), lower_at_peak=float(peak))
    return Bounds(lower, eligible, ratio, float(peak), stats)

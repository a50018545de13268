"""The census weight window, restated in numpy (include/neutral_hip.h: neutral_hip_window_particles).

    slot j        c = celly[j] * nx + cellx[j], w_lo = lower[c], w_hi = fl(upper_ratio * w_lo),
                  w_s = fl(survival_ratio * w_lo), w = weight[j]
    no window     dead[j] != 0, or w_lo == 0: left alone
    roulette      w < w_lo: survives iff fl(rn0 * w_s) < w, at w_s; otherwise dead = 1, weight = 0.0
    split demand  w > w_hi: q = fl(w / w_hi), m = min(max_split, ceil(q)), e_j = m - 1
    supply        f_0 < f_1 < ...: dead going in, or killed just now
    matching      D_j = e_0 + .. + e_{j-1}; g_j = clamp(F - D_j, 0, e_j); request D_j + i - 1 -> f_r
    result        j and its g_j copies at fl(w / (1 + g_j)); a copy is j's other nine fields, dead = 0

Every step is one numpy f64 operation per element, hence one IEEE operation: the device's result is
these bits.  The first sample of a slot's stream is an input (`rn0_of`: slots -> rn0): on the GPU it
comes from the library's own Threefry (probe_rn0), on the CPU from the oracle's (cpu_rn0).

`guarded`: the slots where a comparison is within GUARD (relative) of flipping -- w against w_lo or
w_hi, q against an integer, rn0 * w_s against w.  Arrays that come from two implementations of the
transport (the library's, the oracle's) agree to 1e-9, the project's bar, not to the bit: where no
slot is guarded the window decides the same on both.
"""
import math
from collections import namedtuple

import numpy as np

F64_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "dt_to_census", "mfp_to_collision")
I32_FIELDS = ("cellx", "celly", "dead")
FIELDS = F64_FIELDS + I32_FIELDS
COPIED = tuple(f for f in FIELDS if f not in ("weight", "dead"))  # a copy's nine fields

GUARD = 1e-9
F64_MAX = np.finfo(np.float64).max
WINDOW_SEED_BASE = 2 ** 63 + 2 ** 62

STAT_NAMES = ("live_before", "dead_before", "below", "roulette_killed", "roulette_survived", "above",
              "split", "copies_made", "copies_refused")

# arrays: the store after the call (new arrays); stats: the integer ones of NeutralHipWindowStats by
# name, and the two weight sums; demand, grants: e_j and g_j; free: f_0 < f_1 < ...; sources,
# destinations: request by request (source of request r, slot it went to)
Result = namedtuple("Result", "arrays stats lost gained guarded demand grants free sources destinations")


def valid_settings(upper_ratio, survival_ratio, max_split) -> bool:
    """what the call accepts before it looks at the store"""
    return bool(np.isfinite(upper_ratio) and np.isfinite(survival_ratio) and upper_ratio >= 2.0
                and 1.0 <= survival_ratio <= upper_ratio and 2 <= max_split <= 64)


def cpu_rn0(pid_base: int, seed: int):
    """slots -> the first sample of (pkey = pid_base + slot, master_key = seed, counter 0), from the
    oracle's Threefry"""
    import oracle_binding as ob

    def rn0_of(slots):
        return np.array([ob.generate_random_numbers(int(pid_base) + int(j), int(seed), 0)[0] for j in slots],
                        dtype=np.float64)
    return rn0_of


def probe_rn0(iface, pid_base: int, seed: int):
    """the same from the library's own Threefry (interface.probe_threefry: rows {counter, pkey, key})"""
    def rn0_of(slots):
        rows = np.zeros((len(slots), 3), dtype=np.uint64)
        rows[:, 1] = np.uint64(pid_base) + np.asarray(slots, dtype=np.uint64)
        rows[:, 2] = np.uint64(seed)
        if len(slots) == 0:
            return np.zeros(0)
        _, rn = iface.probe_threefry(rows)
        return np.asarray(rn, dtype=np.float64).reshape(-1, 2)[:, 0].copy()
    return rn0_of


def window(arrays: dict, lower, nx: int, ny: int, upper_ratio: float, survival_ratio: float,
           max_split: int, rn0_of):
    """-> Result, or None where the call refuses (code 1) and changes nothing"""
    lower = np.ascontiguousarray(lower, dtype=np.float64).ravel()
    n = len(arrays["dead"])
    if n <= 0 or nx < 1 or ny < 1 or len(lower) != nx * ny or \
            not valid_settings(upper_ratio, survival_ratio, max_split):
        return None
    upper_ratio, survival_ratio = np.float64(upper_ratio), np.float64(survival_ratio)
    live = arrays["dead"] == 0
    cx, cy = arrays["cellx"].astype(np.int64), arrays["celly"].astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.where(live, arrays["weight"], 0.0)
        inside = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        if np.any(live & (~inside | ~(w >= 0.0) | ~(w <= F64_MAX))):
            return None
        w_lo = np.where(live, lower[np.where(live & inside, cy * nx + cx, 0)], 0.0)
        if np.any(live & (~(w_lo >= 0.0) | ~(w_lo <= F64_MAX))):
            return None
        windowed = live & (w_lo != 0.0)
        w_hi = upper_ratio * w_lo
        w_s = survival_ratio * w_lo
        guarded = windowed & ((np.abs(w - w_lo) <= GUARD * w_lo) | (np.abs(w - w_hi) <= GUARD * w_hi))

        # roulette
        below = windowed & (w < w_lo)
        players = np.flatnonzero(below)
        scaled = np.asarray(rn0_of(players), dtype=np.float64) * w_s[players]
        survives = scaled < w[players]
        guarded[players] |= np.abs(scaled - w[players]) <= GUARD * w[players]
        survivors, killed = players[survives], players[~survives]

        # split demand
        over = np.flatnonzero(windowed & (w > w_hi))
        q = w[over] / w_hi[over]
        ceiling = np.ceil(q)
        m = np.where(ceiling >= float(max_split), float(max_split), ceiling).astype(np.int64)
        # (q beside the integer k flips m between k and k + 1: no flip where max_split caps both)
        guarded[over] |= (np.abs(q - np.rint(q)) <= GUARD * q) & (np.rint(q) < float(max_split))
    demand = np.zeros(n, dtype=np.int64)
    demand[over] = m - 1

    # supply and matching
    is_free = ~live
    is_free[killed] = True
    free = np.flatnonzero(is_free)
    before = np.cumsum(demand) - demand
    grants = np.clip(len(free) - before, 0, demand)
    split = np.flatnonzero(grants > 0)
    sources = np.repeat(split, grants[split])
    destinations = free[:len(sources)]

    out = {f: np.array(arrays[f]) for f in FIELDS}
    out["dead"][killed] = 1
    out["weight"][killed] = 0.0
    out["weight"][survivors] = w_s[survivors]
    new_weight = w[split] / (1 + grants[split]).astype(np.float64)
    for f in COPIED:
        out[f][destinations] = arrays[f][sources]
    out["weight"][destinations] = np.repeat(new_weight, grants[split])
    out["dead"][destinations] = 0
    out["weight"][split] = new_weight

    total = int(demand.sum())
    stats = dict(live_before=int(live.sum()), dead_before=int(n - live.sum()), below=len(players),
                 roulette_killed=len(killed), roulette_survived=len(survivors),
                 above=int((demand > 0).sum()), split=len(split), copies_made=len(sources),
                 copies_refused=max(0, total - len(free)))
    lost = math.fsum(w[killed])
    gained = math.fsum(w_s[survivors] - w[survivors])
    return Result(out, stats, lost, gained, guarded, demand, grants, free, sources, destinations)

"""The census weight comb, restated in numpy (include/neutral_hip.h: neutral_hip_comb_particles).

    lw_j = weight[j] if dead[j] == 0 else 0         S_j = lw_0 + ... + lw_j, W = S_{n-1}
    delta = W / n                                   v = 1 - rn0 of key UINT64_MAX - pid_base
    tooth k at t_k = (k + v) * delta selects the live j with S_{j-1} <= t_k < S_j

The prefix sums are taken in extended precision, blocked (a block's running sum and the running
sum of the blocks' totals: a few thousand additions deep at 2^-64 each, far below an f64 ulp of W)
and rounded to f64 once.  A tooth within GUARD * W of a boundary S_j is `guarded`: the library's
blocked f64 scan is allowed 64 eps W, and may give such a tooth to either neighbour.
"""
import numpy as np

import oracle_binding as ob

GUARD = 1e-12  # of W; more than 100 times the 64 eps W the library's scan is allowed
COPIED_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "dt_to_census", "mfp_to_collision",
                 "cellx", "celly")
_BLOCK = 4096


def comb_offset(pid_base: int, seed: int) -> float:
    rn0, _ = ob.generate_random_numbers(2 ** 64 - 1 - int(pid_base), int(seed), 0)
    return 1.0 - rn0


def prefix_sums(lw: np.ndarray) -> np.ndarray:
    n = len(lw)
    blocks = -(-n // _BLOCK)
    wide = np.zeros(blocks * _BLOCK, dtype=np.longdouble)
    wide[:n] = lw
    inside = np.cumsum(wide.reshape(blocks, _BLOCK), axis=1)
    below = np.concatenate(([np.longdouble(0)], np.cumsum(inside[:, -1])[:-1]))
    return (inside + below[:, None]).reshape(-1)[:n].astype(np.float64)


class Comb:
    """src[], the weight every slot gets, the stats' fields, and which teeth are guarded"""

    def __init__(self, weight, dead, v):
        weight = np.asarray(weight, dtype=np.float64)
        live = np.asarray(dead) == 0
        n = len(weight)
        self.n, self.v = n, float(v)
        self.S = prefix_sums(np.where(live, weight, 0.0))
        self.W = float(self.S[-1])
        self.delta = self.W / n
        self.teeth = (np.arange(n, dtype=np.float64) + self.v) * self.delta
        live_idx = np.flatnonzero(live)
        src = np.searchsorted(self.S, self.teeth, side="right")  # first j with S_j > t_k: live
        self.src = np.minimum(src, live_idx[-1])
        assert np.all(live[self.src]) and np.all(np.diff(self.src) >= 0)
        self.live_before = int(live.sum())
        copies = np.bincount(self.src, minlength=n)
        self.copies = copies
        self.sources_kept = int((copies > 0).sum())
        self.max_copies = int(copies.max())
        # distance of every tooth to the boundaries of the particle it selects
        lower = np.where(self.src > 0, self.S[np.maximum(self.src - 1, 0)], 0.0)
        upper = self.S[self.src]
        near_lower = (self.teeth - lower <= GUARD * self.W) & (lower > 0.0)
        near_upper = (upper - self.teeth <= GUARD * self.W) & (self.src < live_idx[-1])
        self.guarded = near_lower | near_upper
        # the live neighbours a guarded tooth may go to instead
        rank = np.searchsorted(live_idx, self.src)
        self.src_below = live_idx[np.maximum(rank - 1, 0)]
        self.src_above = live_idx[np.minimum(rank + 1, len(live_idx) - 1)]

    def apply(self, arrays: dict) -> dict:
        """the store after the comb (new arrays)"""
        out = {f: np.ascontiguousarray(arrays[f][self.src]) for f in COPIED_FIELDS}
        out["weight"] = np.full(self.n, self.delta, dtype=np.float64)
        out["dead"] = np.zeros(self.n, dtype=np.int32)
        return out


def comb(weight, dead, pid_base=0, seed=0, v=None) -> Comb:
    return Comb(weight, dead, comb_offset(pid_base, seed) if v is None else v)


def prototype_weights(n: int, rng_seed: int = 1234):
    """uniform random weights, half of them scaled by 1e-3, 30 % dead"""
    rng = np.random.default_rng(rng_seed)
    w = rng.random(n)
    w = np.where(w > 0.0, w, 0.5)
    w[rng.random(n) < 0.5] *= 1e-3
    dead = (rng.random(n) < 0.3).astype(np.int32)
    if dead.all():
        dead[n // 2] = 0
    return w, dead

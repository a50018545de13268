"""The reference of the leakage tally (include/neutral_hip.h: neutral_hip_set_leakage_tally): the
escapes through the vacuum sides by side, energy group and exit cosine.  No copy of the event loop:
tests/replay.py's, whose wall hook says through which side a history escapes and whose history()
writes the state an escaped history left with back into its slot; the binning is a restatement of
the header's text in Python floats and comparisons.

    weight[s, g, m]   sum of w / N over the escapes through side s in row g and cosine bin m
    count[s, g, m]    how many they were

Row G ("no group") takes the energies below edges[0], at or above edges[G] and NaN; with no edges
every escape is in row 0."""
import math

import numpy as np

import replay


def group_of(edges, energy):
    """the row of `energy`: the group g with edges[g] <= energy < edges[g + 1], or G = len(edges) - 1
    where there is none; without edges row 0"""
    ngroups = max(len(edges) - 1, 0)
    for g in range(ngroups):
        if edges[g] <= energy < edges[g + 1]:
            return g
    return ngroups


def cosine_bin(mu, ncosines):
    """min(M - 1, (int)(mu * M)): one multiply of doubles, a truncation, a clamp"""
    return min(ncosines - 1, int(float(mu) * float(ncosines)))


def bin_of(edges, ncosines, side, energy, omega_x, omega_y):
    """(side, row, cosine bin) of an escape"""
    mu = abs(omega_x) if side in (replay.WEST, replay.EAST) else abs(omega_y)
    return side, group_of(edges, energy), cosine_bin(mu, ncosines)


class LeakageReplay(replay.Replay):
    """replay.Replay that also keeps the leakage tally with the group `leak_edges` (empty: no groups)
    and `ncosines` cosine bins, and every escape as it was scored: `escapes`, a list of
    dict(pid, key, side, energy, mu, weight, bin)."""

    def __init__(self, *args, leak_edges=(), ncosines=1, **kw):
        super().__init__(*args, **kw)
        self.leak_edges = [float(e) for e in leak_edges]
        self.ncosines = int(ncosines)
        shape = (4, max(len(self.leak_edges) - 1, 0) + 1, self.ncosines)
        self.leak_weight, self.leak_count = np.zeros(shape), np.zeros(shape)
        self.escapes = []
        self._left_through = None

    def _wall(self, side, w):
        escaped = super()._wall(side, w)
        if escaped:
            self._left_through = side
        return escaped

    def history(self, pid, master_key, s):
        self._left_through = None
        super().history(pid, master_key, s)
        side = self._left_through
        if side is None:
            return
        # (the parent has written the state the history left with into its slot)
        assert s["dead"] == 1
        mu = abs(s["omega_x"]) if side in (replay.WEST, replay.EAST) else abs(s["omega_y"])
        assert mu > 0.0
        b = bin_of(self.leak_edges, self.ncosines, side, s["energy"], s["omega_x"], s["omega_y"])
        self.leak_weight[b] += s["weight"] * self.inv_n
        self.leak_count[b] += 1.0
        self.escapes.append(dict(pid=pid, key=master_key, side=side, energy=s["energy"], mu=mu, weight=s["weight"],
                                 bin=b))

    def tally_of(self, master_key):
        """(weight, count) of the escapes of the step with `master_key` alone, summed in the order scored"""
        weight, count = np.zeros_like(self.leak_weight), np.zeros_like(self.leak_count)
        for e in self.escapes:
            if e["key"] == master_key:
                weight[e["bin"]] += e["weight"] * self.inv_n
                count[e["bin"]] += 1.0
        return weight, count


def rebinned(escapes, inv_n, edges, ncosines, key=None):
    """(weight, count) of `escapes` (LeakageReplay.escapes) binned anew with the group `edges` and
    `ncosines` cosine bins, in the order they were scored; key: those of one step alone"""
    edges = [float(e) for e in edges]
    shape = (4, max(len(edges) - 1, 0) + 1, int(ncosines))
    weight, count = np.zeros(shape), np.zeros(shape)
    for e in escapes:
        if key is None or e["key"] == key:
            b = (e["side"], group_of(edges, e["energy"]), cosine_bin(e["mu"], ncosines))
            weight[b] += e["weight"] * inv_n
            count[b] += 1.0
    return weight, count


def run_steps(rep, injected, steps, **kw):
    """replay.run_steps, and beside what it returns `added`: the (weight, count) pair that each step
    added to the tally (master keys 1, 2, ... as replay.run_steps numbers them)"""
    run = replay.run_steps(rep, injected, steps, **kw)
    run["added"] = [rep.tally_of(key) for key in range(1, steps + 1)]
    return run


def nearest_edge(escapes, edges, skip_exact_top=True):
    """the smallest relative distance of an escape's energy from an edge; an energy that IS the top
    edge (an unscattered history) is not near it but on it, by construction, and is left out"""
    best = math.inf
    for e in escapes:
        for k, edge in enumerate(edges):
            if skip_exact_top and k == len(edges) - 1 and e["energy"] == edge:
                continue
            best = min(best, abs(e["energy"] - edge) / edge)
    return best


def nearest_cosine_boundary(escapes, ncosines):
    """the smallest distance of an escape's mu * M from an interior bin boundary 1 .. M - 1"""
    best = math.inf
    for e in escapes:
        v = e["mu"] * ncosines
        for k in range(1, ncosines):
            best = min(best, abs(v - k))
    return best

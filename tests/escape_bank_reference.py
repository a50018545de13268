"""The reference of the escape bank and of the bank source (include/neutral_hip.h:
neutral_hip_set_escape_bank, neutral_hip_source_bank).  No copy of the event loop: tests/replay.py's,
whose wall hook notes the side a history escapes through and whose segment hook repeats the loop's
own clock -- left = dt, then left -= length / speed_of(energy) for every segment, the loop's own
terms in its own order, so the result is the bits of its local `left` -- and whose history() writes
the state an escaped history left with into its slot, from which the record is made.  The bank
source is a numpy restatement of the header's text: one IEEE operation per line.

A record is a dict(slot, key, side, x, y, omega_x, omega_y, energy, weight, time_left); `records_of`
turns a list of them into the structured array the library's bank is read as."""
import math

import numpy as np

import replay

RECORD = np.dtype([("x", "<f8"), ("y", "<f8"), ("omega_x", "<f8"), ("omega_y", "<f8"), ("energy", "<f8"),
                   ("weight", "<f8"), ("time_left", "<f8"), ("slot", "<u4"), ("side", "<u4")])
FLOATS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "time_left")
NO_BAD = 2 ** 64 - 1


class BankReplay(replay.Replay):
    """replay.Replay that also keeps every escape as the bank would: `bank`, in the order the
    histories were advanced.  `slot_of` maps a history's id to its slot (default: the id itself)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.bank = []
        self.slot_of = None
        self._left_through = None
        self._left = self.dt

    def _wall(self, side, w):
        escaped = super()._wall(side, w)
        if escaped:
            self._left_through = side
        return escaped

    def _segment(self, weight, length, ox, oy, energy, cx, cy):
        super()._segment(weight, length, ox, oy, energy, cx, cy)
        self._left -= length / replay.speed_of(energy)

    def history(self, pid, master_key, s):
        self._left_through = None
        self._left = self.dt
        super().history(pid, master_key, s)
        side = self._left_through
        if side is None:
            return
        assert s["dead"] == 1   # (the parent has written the state the history left with into its slot)
        slot = pid if self.slot_of is None else self.slot_of[pid]
        self.bank.append(dict(slot=slot, key=master_key, side=side, time_left=self._left,
                              **{f: s[f] for f in FLOATS[:-1]}))

    def bank_of(self, master_key):
        """the step's records, by slot"""
        return sorted((r for r in self.bank if r["key"] == master_key), key=lambda r: r["slot"])


def records_of(bank):
    """a list of record dicts (or a structured array) as the structured array RECORD"""
    if isinstance(bank, np.ndarray):
        return bank.astype(RECORD)
    out = np.zeros(len(bank), dtype=RECORD)
    for k, r in enumerate(bank):
        for f in RECORD.names:
            out[f][k] = r[f]
    return out


def periodic_shift(width, height):
    """west re-enters at the east wall, east at the west, south at the north, north at the south"""
    return (width, 0.0, -width, 0.0, 0.0, height, 0.0, -height)


def _snap(p, lo, hi, snap):
    """-> (p, moved, bad): one subtraction and two comparisons per wall"""
    under, over = lo - p, p - hi
    if under > 0.0:
        return (lo, 1, False) if under <= snap else (p, 0, True)
    if over > 0.0:
        return (hi, 1, False) if over <= snap else (p, 0, True)
    return (p, 0, False) if lo <= p <= hi else (p, 0, True)


def _cell(edge, n, p, omega):
    """the largest c in [0, n - 1] with edge[c] <= p; on an edge and moving down, the cell below"""
    c = max(k for k in range(n) if edge[k] <= p)
    return c - 1 if (p == edge[c] and omega < 0.0 and c > 0) else c


def bank_source(parts, records, first, count, weight_scale, shift, snap, edgex, edgey, dt, pad=0, x_off=0, y_off=0):
    """The header's definition, slot by slot.  parts: arrays by field (the eleven of the store;
    replay.FIELDS and dt_to_census, mfp_to_collision), NOT modified.  records: structured array.
    edgex / edgey: the local edges, pad + n + 1 + pad values.
    -> (code, new parts or the same, dict(dead_before, emitted, snapped, first_bad))"""
    shift = (0.0,) * 8 if shift is None else tuple(float(v) for v in shift)
    ex = [float(v) for v in np.asarray(edgex)[pad:len(edgex) - pad]]
    ey = [float(v) for v in np.asarray(edgey)[pad:len(edgey) - pad]]
    nx, ny = len(ex) - 1, len(ey) - 1
    dead = [int(j) for j in np.flatnonzero(np.asarray(parts["dead"]) != 0)]
    m = min(int(count), len(dead))
    stats = dict(dead_before=len(dead), emitted=0, snapped=0, first_bad=NO_BAD)
    filled = []
    for k in range(m):
        r = records[first + k]
        fields = [float(r[f]) for f in FLOATS]
        bad = int(r["side"]) > 3 or not all(math.isfinite(v) for v in fields) or not float(r["weight"]) > 0.0 or \
            not float(r["energy"]) > 0.0 or (float(r["omega_x"]) == 0.0 and float(r["omega_y"]) == 0.0)
        if not bad:
            side = int(r["side"])
            x, mx, bad_x = _snap(float(r["x"]) + shift[2 * side], ex[0], ex[nx], snap)
            y, my, bad_y = _snap(float(r["y"]) + shift[2 * side + 1], ey[0], ey[ny], snap)
            bad = bad_x or bad_y
        if bad:
            stats["first_bad"] = first + k
            return 3, parts, stats
        ox, oy = float(r["omega_x"]), float(r["omega_y"])
        filled.append(dict(x=x, y=y, omega_x=ox, omega_y=oy, energy=float(r["energy"]),
                           weight=float(r["weight"]) * weight_scale, dt_to_census=float(dt), mfp_to_collision=0.0,
                           cellx=x_off + _cell(ex, nx, x, ox), celly=y_off + _cell(ey, ny, y, oy), dead=0))
        stats["snapped"] += mx + my
    out = {f: np.array(a, copy=True) for f, a in parts.items()}
    for slot, state in zip(dead, filled):
        for f, v in state.items():
            if f in out:
                out[f][slot] = v
    stats["emitted"] = m
    return 0, out, stats


def emit_into(states, records, first, count, weight_scale, shift, snap, prob):
    """bank_source on the replay's list of state dicts, in place (between= of replay.run_steps);
    -> the stats.  The records must all be good."""
    parts = replay.arrays_of(states)
    code, out, stats = bank_source(parts, records, first, count, weight_scale, shift, snap, prob.edgex, prob.edgey,
                                   prob.dt, pad=prob.pad)
    assert code == 0, stats
    for j, s in enumerate(states):
        for f in replay.FIELDS:
            s[f] = out[f][j].item()
    return stats

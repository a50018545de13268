"""The escape bank and the bank source (include/neutral_hip.h: neutral_hip_set_escape_bank,
neutral_hip_source_bank): every history that leaves through a vacuum side is appended to a list on
the device, and a list of such records refills dead slots in place of a sampled source.

The reference is tests/escape_bank_reference.py -- tests/replay.py's loop with its wall hook noting
the side and its segment hook repeating the loop's clock, and a numpy restatement of the source's
definition --, pinned here on geometry, a hand-computed flight, the leakage tally's reference and
hand-picked records, then held against every kernel variant record by record.

The decks are tests/test_vacuum.py's, and so are the tolerances: counts, slots, sides and cells
exact; STATE_TOL of the mesh's width for a position, of the value for energy and weight, absolute
for a cosine, and of dt, absolute, for time_left (a difference of quantities of size dt); two runs of
the same histories 1e-13.  A record's x, y, omega_x, omega_y, energy and weight are compared BIT FOR
BIT with what the same run's arrays hold at its slot after the step."""
import ctypes as C
import json
import os
import re
import struct
import sys

import numpy as np
import pytest

import escape_bank_reference as br
import escape_reference as er
import leakage_reference as lr
import oracle_binding as ob
import replay
import test_vacuum as tv
from gpu_support import OWN_DRIVER, gpu, iface, l2, needs_gpu, run_driver, third_absorb  # noqa: F401
from ranks import launch_ranks

STATE_TOL = tv.STATE_TOL
SAME_HISTORIES_TOL = tv.SAME_HISTORIES_TOL
W, E, S, N = replay.WEST, replay.EAST, replay.SOUTH, replay.NORTH
BANK_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_bank_worker.py")
SYMBOLS = ("neutral_hip_set_escape_bank", "neutral_hip_reset_escape_bank", "neutral_hip_escape_bank_stats",
           "neutral_hip_source_bank")
CAPACITY = 1024
SNAP = 1e-12
BITWISE = ("x", "y", "omega_x", "omega_y", "energy", "weight")


def _extent(prob):
    """(x0, y0, width, height) of the mesh"""
    ex = np.asarray(prob.edgex, dtype=np.float64)[prob.pad:len(prob.edgex) - prob.pad]
    ey = np.asarray(prob.edgey, dtype=np.float64)[prob.pad:len(prob.edgey) - prob.pad]
    return float(ex[0]), float(ey[0]), float(ex[-1] - ex[0]), float(ey[-1] - ey[0])


# ---- CPU: the ABI ------------------------------------------------------------------------------

def test_library_exports_the_four_symbols_at_the_same_abi_version():
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in iface.ABI_SYMBOLS, name
    assert lib.neutral_hip_abi_version() == 12
    assert C.sizeof(iface.EscapeRecord) == 64 and iface.ESCAPE_RECORD.itemsize == 64 == br.RECORD.itemsize
    assert [(n, iface.ESCAPE_RECORD.fields[n][1]) for n in iface.ESCAPE_RECORD.names] == \
        [(n, getattr(iface.EscapeRecord, n).offset) for n, _ in iface.EscapeRecord._fields_]
    assert C.sizeof(iface.EscapeBankStats) == 40 and C.sizeof(iface.BankSourceStats) == 48


def test_the_setter_refuses_by_its_arguments_alone_and_null_is_always_accepted():
    """No device is touched: the address is only kept, and no step runs."""
    from neutral_amd import interface as iface
    lib = iface.library()
    set_ = lib.neutral_hip_set_escape_bank
    stats = iface.EscapeBankStats()
    try:
        assert set_(C.c_void_p(0x1000), 5) == 0
        lib.neutral_hip_escape_bank_stats(C.byref(stats))
        assert (stats.capacity, stats.claimed, stats.recorded, stats.step_claimed, stats.step_recorded) == (5, 0, 0, 0, 0)
        for address, capacity in ((0x1000, 0), (0x1008, 4), (0x1001, 4), (0x100c, 1)):
            assert set_(C.c_void_p(address), capacity) == 1, (address, capacity)
            lib.neutral_hip_escape_bank_stats(C.byref(stats))
            assert stats.capacity == 5                      # (refused: the setting stays as it was)
        assert lib.neutral_hip_reset_escape_bank() == 0
        for capacity in (0, 7, 2 ** 63):
            assert set_(None, capacity) == 0                # NULL turns it off beside anything
            assert lib.neutral_hip_reset_escape_bank() == 1
        assert set_(C.c_void_p(0x1008), 4) == 1 and set_(C.c_void_p(0x1010), 2 ** 40) == 0   # ... and still refuses
        with pytest.raises(ValueError):
            iface.set_escape_bank(0x1000, 0)
        with pytest.raises(ValueError):
            iface.set_escape_bank(0x1004, 8)
        iface.set_escape_bank(0x2000, 8)
        assert iface.escape_bank_stats().capacity == 8
        iface.set_escape_bank(None)
        assert iface.escape_bank_stats().capacity == 0
    finally:
        set_(None, 0)
        iface.set_escape_bank(None)


def test_the_source_call_refuses_with_code_1_before_any_device_call():
    from neutral_amd import interface as iface
    lib = iface.library()
    store = iface.Particle()
    for name, *_ in iface.Particle._fields_:
        setattr(store, name, 0x4000)       # (addresses the call never reads: it is refused first)
    parts, records, edges = C.byref(store), C.c_void_p(0x1000), C.c_void_p(0x2000)
    stats = iface.BankSourceStats()
    nan, inf = float("nan"), float("inf")
    shift_nan = (C.c_double * 8)(0, 0, 0, nan, 0, 0, 0, 0)
    good = dict(particles=parts, n=10, records=records, first=0, count=4, scale=1.0, shift=None, snap=0.0, nx=4, ny=4,
                pad=0, dt=1e-7, edgex=edges, edgey=edges)
    bad = [dict(particles=None), dict(n=0), dict(n=-3), dict(records=None), dict(count=-1), dict(scale=0.0),
           dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(snap=-1e-13), dict(snap=nan), dict(snap=inf),
           dict(nx=0), dict(ny=0), dict(pad=-1), dict(dt=0.0), dict(dt=nan), dict(edgex=None), dict(edgey=None),
           dict(shift=shift_nan)]
    for change in bad:
        a = dict(good, **change)
        stats.emitted = 99
        code = lib.neutral_hip_source_bank(a["particles"], a["n"], a["records"], a["first"], a["count"], a["scale"],
                                           a["shift"], a["snap"], a["nx"], a["ny"], a["pad"], 0, 0, a["dt"], a["edgex"],
                                           a["edgey"], C.byref(stats))
        assert code == 1, change
        assert stats.emitted == 0 and stats.first_bad == br.NO_BAD, change
    with pytest.raises(iface.BankSourceRefused) as refused:
        iface.source_bank(parts, 10, 0x1000, 0, 4, 0.0, None, 0.0, 4, 4, 0, 0, 0, 1e-7, edges, edges)
    assert refused.value.code == 1 and refused.value.first_bad is None and isinstance(refused.value, iface.Refused)
    with pytest.raises(ValueError):
        iface.source_bank(parts, 10, 0x1000, 0, 4, 1.0, (0.0,) * 7, 0.0, 4, 4, 0, 0, 0, 1e-7, edges, edges)


# ---- CPU: the reference -------------------------------------------------------------------------

_REFERENCES = {}


def _reference(prob, cs, injected, steps, vacuum, cs_absorb=None, roulette=(0.0, 0.0), window=None):
    """BankReplay over every history of `injected`, once per configuration: -> run with "rep" and
    "banks", the records of every step by slot"""
    key = (prob.nx, prob.ny, prob.dt, steps, vacuum, cs_absorb is not None, tuple(roulette),
           None if window is None else (window.lower.tobytes(), window.ratio),
           prob.density.tobytes(), tuple(injected[f].tobytes() for f in replay.FIELDS))
    if key not in _REFERENCES:
        rep = br.BankReplay(prob, cs, cs_absorb, roulette, vacuum=vacuum, window=window)
        run = replay.run_steps(rep, injected, steps)
        run["rep"] = rep
        run["banks"] = [rep.bank_of(k) for k in range(1, steps + 1)]
        _REFERENCES[key] = run
    return _REFERENCES[key]


def _wrap_reference(prob, cs, injected, steps, vacuum, cs_absorb, orders=None, check=None):
    """... with every step's escapes re-emitted before the next one through the periodic shift (snap
    SNAP): in the order of slots orders[step - 1] where given (the order a GPU's bank has), by slot
    otherwise; check(step, records by slot) runs before a step's records are used"""
    _, _, width, height = _extent(prob)
    rep = br.BankReplay(prob, cs, cs_absorb, vacuum=vacuum)
    emitted = []

    def between(key, states):
        records = rep.bank_of(key)
        if check is not None:
            check(key, records)
        if orders is not None:
            by_slot = {r["slot"]: r for r in records}
            records = [by_slot[int(slot)] for slot in orders[key - 1]]
        stats = br.emit_into(states, br.records_of(records), 0, len(records), 1.0, br.periodic_shift(width, height),
                             SNAP, prob)
        emitted.append(stats)
    run = replay.run_steps(rep, injected, steps, between=between)
    run["rep"], run["emitted"] = rep, emitted
    run["banks"] = [rep.bank_of(k) for k in range(1, steps + 1)]
    return run


def test_bank_replay_times_the_stream_deck_as_geometry_does(make_problem, cs):
    """dt - time_left is distance / speed, the distance from nothing but the four wall distances"""
    prob = tv._stream_problem(make_problem)
    injected = tv._oracle_injected(prob, cs)
    run = _reference(prob, cs, injected, 3, 15)
    bank = run["banks"][0]
    assert len(bank) == prob.nparticles and [r["slot"] for r in bank] == list(range(prob.nparticles))
    x0, y0, width, height = _extent(prob)
    side, ex, ey, corner = er.exits_by_geometry(injected["x"] - x0, injected["y"] - y0, injected["omega_x"],
                                                injected["omega_y"], width, height)
    assert np.all(corner > 1e-9 * width)
    distance = np.hypot(ex - (injected["x"] - x0), ey - (injected["y"] - y0))
    flight = distance / replay.speed_of(prob.initial_energy)
    got = np.array([prob.dt - r["time_left"] for r in bank])
    assert np.max(np.abs(got - flight)) <= 1e-12 * prob.dt
    assert [r["side"] for r in bank] == side.tolist()
    assert np.max(np.abs(np.array([r["x"] for r in bank]) - x0 - ex)) <= 1e-12
    assert np.max(np.abs(np.array([r["y"] for r in bank]) - y0 - ey)) <= 1e-12


def test_bank_replay_on_one_hand_computed_oblique_flight(make_problem, cs):
    """(0.6, 0.8) from (0.95, 0.55) on a 10 x 10 mesh of 1 m, dt = 0.2 m of flight: it crosses y = 0.6
    after 0.0625 m and reaches the east wall after 0.05 / 0.6 = 0.08333 m at y = 0.55 + 0.8 / 12 =
    0.61667, with (0.2 - 0.08333) m of its time left and the weight 0.75 it came with."""
    prob = make_problem("stream", nx=10, nparticles=4, iterations=1)
    speed = replay.speed_of(prob.initial_energy)
    dt = 0.2 / speed
    rep = br.BankReplay(prob, cs, dt=dt, vacuum=15)
    s = dict(x=0.95, y=0.55, omega_x=0.6, omega_y=0.8, energy=prob.initial_energy, weight=0.75, dead=0, cellx=9, celly=5)
    rep.history(3, 1, s)
    assert s["dead"] == 1 and rep.nfacets == 2 and rep.ncollisions == 0 and len(rep.bank) == 1
    r = rep.bank[0]
    assert (r["slot"], r["key"], r["side"], r["weight"], r["energy"]) == (3, 1, E, 0.75, prob.initial_energy)
    assert (r["omega_x"], r["omega_y"]) == (0.6, 0.8)
    assert abs(r["x"] - 1.0) <= 1e-12 and abs(r["y"] - (0.55 + 0.8 / 12.0)) <= 1e-12
    assert abs(r["time_left"] - (0.2 - 0.05 / 0.6) / speed) <= 1e-12 * dt
    assert (r["x"], r["y"]) == (s["x"], s["y"])
    # a history that does not leave banks nothing
    quiet = dict(x=0.5, y=0.5, omega_x=0.6, omega_y=0.8, energy=prob.initial_energy, weight=1.0, dead=0, cellx=5, celly=5)
    rep.history(2, 1, quiet)
    assert quiet["dead"] == 0 and len(rep.bank) == 1


def test_bank_replay_escapes_are_the_leakage_replays(make_problem, cs):
    prob = tv._case_problem(make_problem, "a")
    injected = tv._oracle_injected(prob, cs)
    vacuum = tv.CASES["a"]["vacuum"]
    run = _reference(prob, cs, injected, 3, vacuum, third_absorb(cs))
    leak = lr.LeakageReplay(prob, cs, third_absorb(cs), vacuum=vacuum)
    replay.run_steps(leak, injected, 3)
    bank = run["rep"].bank
    assert len(bank) == len(leak.escapes) > 300
    for r, e in zip(bank, leak.escapes):
        mu = abs(r["omega_x"]) if r["side"] in (W, E) else abs(r["omega_y"])
        assert (r["slot"], r["key"], r["side"], r["energy"], mu, r["weight"]) == \
            (e["pid"], e["key"], e["side"], e["energy"], e["mu"], e["weight"])
    for tt, step_bank in enumerate(run["banks"], 1):
        assert len(step_bank) == sum(run["per_step"][tt - 1]["escaped"])
        slots = [r["slot"] for r in step_bank]
        assert slots == sorted(set(slots))                   # a history escapes once per step at most
        assert all(0.0 < r["time_left"] < prob.dt for r in step_bank)


def _store(n, dead):
    parts = dict(x=np.full(n, 0.5), y=np.full(n, 0.5), omega_x=np.full(n, 1.0), omega_y=np.zeros(n),
                 energy=np.full(n, 7.0), weight=np.full(n, 1.0), dt_to_census=np.zeros(n), mfp_to_collision=np.full(n, 3.0),
                 cellx=np.full(n, 2, dtype=np.int32), celly=np.full(n, 2, dtype=np.int32), dead=np.zeros(n, dtype=np.int32))
    parts["dead"][list(dead)] = 1
    return parts


def _record(x, y, ox=0.6, oy=0.8, energy=1.0e6, weight=0.5, time_left=1e-8, slot=0, side=0):
    return dict(x=x, y=y, omega_x=ox, omega_y=oy, energy=energy, weight=weight, time_left=time_left, slot=slot, side=side)


def test_the_numpy_restatement_on_hand_picked_records():
    """a 4 x 2 mesh of cells 0.25 x 0.5 on [0, 1] x [0, 1]"""
    ex, ey = np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 3)
    parts = _store(8, dead=(1, 2, 4, 5, 6, 7))
    records = br.records_of([
        _record(0.3, 0.7),                                   # interior: cell (1, 1)
        _record(0.5, 0.25, ox=0.6),                          # on an interior edge, moving up: the cell above it, 2
        _record(0.5, 0.25, ox=-0.6),                         # ... moving down: the cell below it, 1
        _record(0.3, 1.0, oy=-0.8),                          # on the top wall: the last cell, not 0
        _record(-1e-13, 0.5, ox=0.6),                        # 1e-13 outside the west wall
        _record(0.0, 0.5, ox=-0.6),                          # on the bottom wall moving out: cell 0 all the same
    ])
    code, out, stats = br.bank_source(parts, records, 0, 6, 0.25, None, 1e-12, ex, ey, 2e-7)
    assert code == 0 and stats == dict(dead_before=6, emitted=6, snapped=1, first_bad=br.NO_BAD)
    assert out["cellx"][[1, 2, 4, 5, 6, 7]].tolist() == [1, 2, 1, 1, 0, 0]
    assert out["celly"][[1, 2, 4, 5, 6, 7]].tolist() == [1, 0, 0, 1, 1, 1]
    assert out["x"][6] == 0.0 and out["x"][1] == 0.3 and out["y"][5] == 1.0
    assert np.all(out["weight"][[1, 2, 4, 5, 6, 7]] == 0.125) and np.all(out["dead"] == 0)
    assert np.all(out["dt_to_census"][[1, 2, 4, 5, 6, 7]] == 2e-7) and np.all(out["mfp_to_collision"][[1, 2]] == 0.0)
    for f in parts:                                          # the live slots: untouched in every field
        assert np.array_equal(out[f][[0, 3]], parts[f][[0, 3]]), f
    assert parts["dead"].sum() == 6                          # (the input is not modified)
    # snap 0: the record outside is bad, nothing is written, and it is the first bad one
    code, same, stats = br.bank_source(parts, records, 0, 6, 0.25, None, 0.0, ex, ey, 2e-7)
    assert code == 3 and same is parts and stats["first_bad"] == 4 and stats["emitted"] == 0
    # ... but not when it is not among the m records that would be used
    code, _, stats = br.bank_source(parts, records, 0, 4, 1.0, None, 0.0, ex, ey, 2e-7)
    assert code == 0 and stats["emitted"] == 4 and stats["snapped"] == 0
    # side 4, NaN energy, no direction, no weight
    for change, where in ((dict(side=4), 1), (dict(energy=float("nan")), 0), (dict(ox=0.0, oy=0.0), 2),
                          (dict(weight=0.0), 0), (dict(energy=-1.0), 0), (dict(time_left=float("inf")), 1)):
        rows = [_record(0.3, 0.7) for _ in range(3)]
        rows[where] = _record(0.3, 0.7, **change)
        code, _, stats = br.bank_source(parts, br.records_of(rows), 0, 3, 1.0, None, 1e-12, ex, ey, 2e-7)
        assert code == 3 and stats["first_bad"] == where, change
    # fewer dead slots than count; first > 0: slot d_k takes record first + k
    few = _store(8, dead=(6, 3))
    code, out, stats = br.bank_source(few, records, 2, 4, 1.0, None, 1e-12, ex, ey, 2e-7)
    assert code == 0 and stats["emitted"] == 2 and stats["dead_before"] == 2 and stats["snapped"] == 0
    assert (out["cellx"][3], out["celly"][3], out["omega_x"][3]) == (1, 0, -0.6)       # record 2
    assert (out["cellx"][6], out["celly"][6], out["y"][6]) == (1, 1, 1.0)              # record 3
    # a shift by side: west + 1 lands on the east wall, in the last cell
    code, out, stats = br.bank_source(_store(2, dead=(0,)), br.records_of([_record(0.0, 0.3, ox=-0.6, side=W)]), 0, 1, 1.0,
                                      br.periodic_shift(1.0, 1.0), 0.0, ex, ey, 2e-7)
    assert code == 0 and (out["x"][0], out["cellx"][0], out["celly"][0]) == (1.0, 3, 0)


_WRAP = {}


def _wrap_on_the_oracles_injection(make_problem, cs, case):
    if case not in _WRAP:
        prob = tv._case_problem(make_problem, case)
        injected = tv._oracle_injected(prob, cs)
        _WRAP[case] = (prob, _wrap_reference(prob, cs, injected, 3, tv.CASES[case]["vacuum"], third_absorb(cs)))
    return _WRAP[case]


@pytest.mark.parametrize("case", ["a", "b", "stream"])
def test_the_decks_meet_their_conditions(make_problem, cs, case):
    """... on the CPU oracle's injection, before anything is compared with a deck"""
    if case == "stream":
        prob = tv._stream_problem(make_problem)
        run = _reference(prob, cs, tv._oracle_injected(prob, cs), 3, 15)
        first = run["banks"][0]
        by_side = [sum(1 for r in first if r["side"] == s) for s in range(4)]
        left = [r["time_left"] for r in first]
        print(f"stream: {by_side} by side, time_left {min(left):.3e} .. {max(left):.3e} of dt {prob.dt:.1e}")
        assert len(first) == 512 and not run["banks"][1] and not run["banks"][2]
        assert min(by_side) >= 121 and prob.dt == 1e-7
        # (the two figures as they are quoted, to two digits: 4.597e-8 and 6.742e-8 on this deck)
        assert float(f"{min(left):.1e}") == 4.6e-8 and float(f"{max(left):.1e}") == 6.7e-8
        return
    prob, run = _wrap_on_the_oracles_injection(make_problem, cs, case)
    per_step = [s["escaped"] for s in run["per_step"]]
    print(f"case {case} with wrap re-entry: escaped by step and side {per_step}, emitted {run['emitted']}")
    if case == "a":
        assert [sum(s) for s in per_step] == [402, 213, 275]
        assert [s[W] for s in per_step] == [358, 135, 194] and [s[N] for s in per_step] == [44, 78, 81]
    else:
        assert [sum(s) for s in per_step] == [524, 434, 369]
    for stats, escaped in zip(run["emitted"], per_step):       # every escape finds a dead slot
        assert stats["emitted"] == sum(escaped) and stats["first_bad"] == br.NO_BAD


# ---- the GPU runs -----------------------------------------------------------------------------------

def _run(iface, prob, cs, steps, variant, capacity=CAPACITY, states=None, window=None, between=None, spare=0,
         sentinel=None, **kw):
    """inject (and overwrite with `states`), step; after every step the bank's stats, the step's range
    of records [claimed before, claimed after) clipped to the capacity, and the arrays; between(tt,
    sim, lo, hi) after step tt but the last.  spare: the tensor is that many records longer than the
    capacity; sentinel: every byte of it is filled with that value first."""
    sim = iface.Simulation(prob, *cs, variant=variant, escape_bank=None if capacity is None else capacity + spare, **kw)
    try:
        if capacity is not None:
            sim.escape_bank_capacity = capacity
            if sentinel is not None:
                sim.escape_bank.fill_(sentinel)
        sim.inject()
        if states is not None:
            tv._upload(iface, sim, states)
        if window is not None:
            sim.window_in_step(**window)
        injected = sim.particle_arrays()
        results, snaps, banks, stats, said = [], [injected], [], [], []
        for tt in range(1, steps + 1):
            results.append(sim.step(tt))
            assert results[-1].stats.aborted == 0
            snaps.append(sim.particle_arrays())
            lo, hi = 0, 0
            if capacity is not None:
                st = sim.escape_bank_stats()
                stats.append({name: int(getattr(st, name)) for name, _ in st._fields_})
                # (from the stats alone: a `between` may have reset the bank)
                lo, hi = min(int(st.claimed - st.step_claimed), capacity), min(int(st.claimed), capacity)
                banks.append(sim.escape_bank_host(lo, hi))
            if between is not None and tt < steps:
                said.append(between(tt, sim, lo, hi))
        return dict(steps=results, injected=injected, snaps=snaps, parts=snaps[-1], banks=banks, stats=stats, said=said,
                    tally=sim.tally_host().copy(), flux=tv._host(sim.flux), absorbed=tv._host(sim.absorbed),
                    collisions=tv._host(sim.collisions),
                    out=sim.outflow_host().copy() if sim.outflow is not None else None,
                    tail=None if capacity is None else sim.escape_bank[64 * capacity:].cpu().numpy().copy())
    finally:
        sim.close()
        assert iface.escape_bank_stats().capacity == 0          # (close() turned the bank off)


def _assert_records(got, want, after, prob, what=""):
    """a step's range of the bank against the reference's escapes of that step, and against the same
    run's arrays after the step"""
    x0, y0, width, height = _extent(prob)
    got = np.sort(got, order="slot")
    assert len(got) == len(want), (what, len(got), len(want))
    assert got["slot"].tolist() == [r["slot"] for r in want], what
    assert len(set(got["slot"].tolist())) == len(got), what
    assert got["side"].tolist() == [r["side"] for r in want], what
    ref = br.records_of(want)
    if len(got):
        assert np.max(np.abs(got["x"] - ref["x"])) <= STATE_TOL * width, what
        assert np.max(np.abs(got["y"] - ref["y"])) <= STATE_TOL * width, what
        for f in ("omega_x", "omega_y"):
            assert np.max(np.abs(got[f] - ref[f])) <= STATE_TOL, (what, f)
        for f in ("energy", "weight"):
            assert np.max(np.abs(got[f] - ref[f]) / np.abs(ref[f])) <= STATE_TOL, (what, f)
        assert np.max(np.abs(got["time_left"] - ref["time_left"])) <= STATE_TOL * prob.dt, what
    slots = got["slot"].astype(np.int64)
    for f in BITWISE:
        assert np.array_equal(got[f], after[f][slots]), (what, f)
    assert np.all(after["dead"][slots] == 1), what


def _assert_stats(got, capacity=CAPACITY):
    """claimed is the cursor: the steps' escapes summed; recorded = min(claimed, capacity); the step_*
    fields the last step's increments; step_claimed == sum(escape.counts()), exactly"""
    claimed = 0
    for tt, (r, st) in enumerate(zip(got["steps"], got["stats"]), 1):
        k = sum(r.escape.counts())
        before, claimed = claimed, claimed + k
        assert st == dict(capacity=capacity, claimed=claimed, recorded=min(claimed, capacity), step_claimed=k,
                          step_recorded=min(claimed, capacity) - min(before, capacity)), tt
        assert (r.step_claimed, r.step_recorded) == (st["step_claimed"], st["step_recorded"]), tt


def _assert_against(got, want, prob, steps=(1, 2, 3), accumulated=True):
    for tt in steps:
        _assert_records(got["banks"][tt - 1], want["banks"][tt - 1], got["snaps"][tt], prob, f"step {tt}")
    tv._assert_events(got, want)
    if accumulated:
        _assert_stats(got)
    else:   # (the bank was reset between the steps: every step's range starts at 0)
        for r, st in zip(got["steps"], got["stats"]):
            k = sum(r.escape.counts())
            assert (st["claimed"], st["recorded"], st["step_claimed"], st["step_recorded"]) == (k, k, k, k)
    for tt in steps:
        tv._assert_state(got["snaps"][tt], want["snaps"][tt])


def _leakage(prob):
    return (prob.initial_energy * np.array([0.5, 0.9, 0.97, 1.0]), 4)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("arith", ["auto", "checked"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_against_the_reference(iface, make_problem, cs, monkeypatch, variant, arith, case):
    """1. every optional tally and the leakage tally on: after each step the step's range, sorted by
    slot, is the reference's escapes of that step; the stats' identities hold"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, case)
    iface.set_arithmetic(iface.ARITH_CHECKED if arith == "checked" else iface.ARITH_AUTO)
    vacuum = tv.CASES[case]["vacuum"]
    got = _run(iface, prob, cs, 3, variant, cs_absorb=third_absorb(cs), outflow=True, vacuum=vacuum,
               leakage=_leakage(prob), **tv._everything(prob))
    want = _reference(prob, cs, got["injected"], 3, vacuum, third_absorb(cs))
    assert len(want["banks"][0]) >= 300 and all(len(b) >= 10 for b in want["banks"]) and want["rep"].escaped_not_unit >= 50
    _assert_against(got, want, prob)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_the_collision_free_deck(iface, make_problem, cs, monkeypatch, variant):
    """2. 512 records in step 1, every weight 1.0; sides and positions by straight-line geometry within
    1e-12, time_left by geometry within STATE_TOL * dt; steps 2 and 3 claim nothing"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._stream_problem(make_problem)
    got = _run(iface, prob, cs, 3, variant, outflow=True, vacuum="all")
    want = _reference(prob, cs, got["injected"], 3, 15)
    _assert_against(got, want, prob)
    first = np.sort(got["banks"][0], order="slot")
    assert len(first) == 512 and np.all(first["weight"] == 1.0) and np.all(first["energy"] == prob.initial_energy)
    assert [s["step_claimed"] for s in got["stats"]] == [512, 0, 0] and not len(got["banks"][1]) and not len(got["banks"][2])
    inj = got["injected"]
    x0, y0, width, height = _extent(prob)
    side, ex, ey, corner = er.exits_by_geometry(inj["x"] - x0, inj["y"] - y0, inj["omega_x"], inj["omega_y"], width, height)
    assert np.all(corner > 1e-9 * width)
    assert np.array_equal(first["side"], side)
    assert np.max(np.abs(first["x"] - x0 - ex)) <= 1e-12 and np.max(np.abs(first["y"] - y0 - ey)) <= 1e-12
    flight = np.hypot(ex - (inj["x"] - x0), ey - (inj["y"] - y0)) / replay.speed_of(prob.initial_energy)
    assert np.max(np.abs((prob.dt - first["time_left"]) - flight)) <= STATE_TOL * prob.dt
    assert np.array_equal(first["omega_x"], inj["omega_x"]) and np.array_equal(first["omega_y"], inj["omega_y"])


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_the_bank_changes_nothing_else(iface, make_problem, cs, monkeypatch, variant):
    """3. deck a with the bank against the run without it: every slot's eleven fields, every event
    count and the escape counts exact; the atomically summed meshes within 1e-13"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    opts = dict(cs_absorb=third_absorb(cs), outflow=True, vacuum="wn", scalar_flux=True, collision_tallies=True)
    banked = _run(iface, prob, cs, 3, variant, **opts)
    plain = _run(iface, prob, cs, 3, variant, capacity=None, **opts)
    assert sum(s["step_claimed"] for s in banked["stats"]) > 300
    for tt in (1, 2, 3):
        for f in tv.ALL_FIELDS:
            assert np.array_equal(banked["snaps"][tt][f], plain["snaps"][tt][f]), (tt, f)
    for a, b in zip(banked["steps"], plain["steps"]):
        assert (a.nprocessed, a.facets, a.collisions, a.census) == (b.nprocessed, b.facets, b.collisions, b.census)
        assert a.escape.counts() == b.escape.counts()
        assert (b.step_claimed, b.step_recorded) == (0, 0)
        for side in range(4):
            assert abs(a.escape.weights()[side] - b.escape.weights()[side]) <= SAME_HISTORIES_TOL * b.escape.weights()[side]
    for name in ("tally", "flux", "absorbed", "out"):
        assert plain[name].any() and l2(banked[name], plain[name]) <= SAME_HISTORIES_TOL, name
    assert np.array_equal(banked["collisions"], plain["collisions"])


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("capacity", [37, 1])
def test_overflow(iface, make_problem, cs, monkeypatch, variant, capacity):
    """4. the stream deck into a bank of 37 and of 1, in a buffer 64 records longer filled with 0xA5:
    all 512 claim, `capacity` are recorded, each one of the reference's escapes and no slot twice;
    every byte from `capacity` on is untouched.  After reset the next step appends from index 0."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._stream_problem(make_problem)
    got = _run(iface, prob, cs, 1, variant, capacity=capacity, spare=64, sentinel=0xA5, outflow=True, vacuum="all")
    want = _reference(prob, cs, got["injected"], 3, 15)
    st = got["stats"][0]
    assert st == dict(capacity=capacity, claimed=512, recorded=capacity, step_claimed=512, step_recorded=capacity)
    assert sum(got["steps"][0].escape.counts()) == 512
    kept = got["banks"][0]
    assert len(kept) == capacity and len(set(kept["slot"].tolist())) == capacity
    by_slot = {r["slot"]: r for r in want["banks"][0]}
    _assert_records(kept, [by_slot[s] for s in sorted(kept["slot"].tolist())], got["snaps"][1], prob)
    assert got["tail"].size == 64 * 64 and np.all(got["tail"] == 0xA5)
    # reset: a second store's step appends from index 0 again
    sim = iface.Simulation(prob, *cs, variant=variant, outflow=True, vacuum="all", escape_bank=capacity + 64)
    try:
        sim.escape_bank_capacity = capacity
        sim.inject()
        sim.step(1)
        before = sim.escape_bank.cpu().numpy().copy()
        assert sim.escape_bank_stats().claimed == 512
        sim.reset_escape_bank()
        st = sim.escape_bank_stats()
        assert (st.claimed, st.recorded) == (0, 0)
        assert np.array_equal(sim.escape_bank.cpu().numpy(), before)     # reset leaves the records as they are
        sim.inject()
        sim.escape_bank.fill_(0xA5)
        r = sim.step(1)
        st = sim.escape_bank_stats()
        assert (st.claimed, st.recorded, r.step_claimed, r.step_recorded) == (512, capacity, 512, capacity)
        again = sim.escape_bank_host(0, capacity)
        assert set(again["slot"].tolist()) <= set(by_slot) and len(set(again["slot"].tolist())) == capacity
        assert np.all(sim.escape_bank[64 * capacity:].cpu().numpy() == 0xA5)
    finally:
        sim.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 2])
def test_accumulate_reset_and_off(iface, make_problem, cs, monkeypatch, variant):
    """5. two steps of deck b without a reset give contiguous ranges; reset leaves the bytes; with the
    bank off a further step writes nothing (sentinel bytes) and claims nothing"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "b")
    sim = iface.Simulation(prob, *cs, variant=variant, cs_absorb=third_absorb(cs), outflow=True, vacuum="ws",
                           escape_bank=CAPACITY)
    try:
        sim.inject()
        injected = sim.particle_arrays()
        want = _reference(prob, cs, injected, 3, tv.CASES["b"]["vacuum"], third_absorb(cs))
        r1 = sim.step(1)
        after1 = sim.particle_arrays()
        r2 = sim.step(2)
        after2 = sim.particle_arrays()
        st = sim.escape_bank_stats()
        k1, k2 = len(want["banks"][0]), len(want["banks"][1])
        assert (r1.step_claimed, r2.step_claimed, st.claimed, st.recorded) == (k1, k2, k1 + k2, k1 + k2) and k1 + k2 <= CAPACITY
        _assert_records(sim.escape_bank_host(0, k1), want["banks"][0], after1, prob, "step 1")
        _assert_records(sim.escape_bank_host(k1, k1 + k2), want["banks"][1], after2, prob, "step 2")
        assert len(sim.escape_bank_host()) == k1 + k2
        # sorted by slot on the device: the same records, in order
        unsorted = sim.escape_bank_host(k1, k1 + k2)
        sim.sort_escape_bank(k1, k1 + k2)
        assert np.array_equal(sim.escape_bank_host(k1, k1 + k2), np.sort(unsorted, order="slot"))
        assert np.array_equal(np.sort(sim.escape_bank_host(0, k1), order="slot"),
                              np.sort(br.records_of(sim.escape_bank_host(0, k1)), order="slot"))
        before = sim.escape_bank.cpu().numpy().copy()
        sim.reset_escape_bank()
        assert np.array_equal(sim.escape_bank.cpu().numpy(), before) and sim.escape_bank_stats().claimed == 0
        sim.escape_bank_on = False
        sim.escape_bank.fill_(0x5A)
        r3 = sim.step(3)
        assert sum(r3.escape.counts()) == len(want["banks"][2]) > 0
        assert (r3.step_claimed, r3.step_recorded) == (0, 0)
        assert np.all(sim.escape_bank.cpu().numpy() == 0x5A)
        assert iface.escape_bank_stats().capacity == 0
    finally:
        sim.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["no outflow tally", "lazy export", "stream queues"])
def test_tiled_modes(iface, make_problem, cs, monkeypatch, mode):
    """6. the tiled variant without an outflow tally, with lazy export, with stream queues: deck a"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    if mode == "lazy export":
        iface.set_lazy_export(True)
    if mode == "stream queues":
        iface.set_stream_queues(True)
    got = _run(iface, prob, cs, 3, 2, cs_absorb=third_absorb(cs), outflow=(mode != "no outflow tally"), vacuum="wn")
    want = _reference(prob, cs, got["injected"], 3, tv.CASES["a"]["vacuum"], third_absorb(cs))
    _assert_against(got, want, prob)


@gpu
@needs_gpu
@pytest.mark.parametrize("how,variant", [("roulette", 1), ("roulette", 2), ("in-step window", 2), ("in-step window", 0)])
def test_with_roulette_and_the_in_step_window(iface, make_problem, cs, monkeypatch, how, variant):
    """7. weights other than 1 -- roulette's survivors among them -- are recorded as the slot holds them"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    wc, ws = tv.ROULETTE
    kw = dict(cs_absorb=third_absorb(cs), outflow=True, vacuum="wn", scalar_flux=True, collision_tallies=True)
    if how == "roulette":
        got = _run(iface, prob, cs, 3, variant, roulette=tv.ROULETTE, **kw)
    else:
        got = _run(iface, prob, cs, 3, variant, window=dict(lower=wc, survival_ratio=ws / wc), **kw)
    want = _reference(prob, cs, got["injected"], 3, tv.CASES["a"]["vacuum"], third_absorb(cs), tv.ROULETTE)
    rep = want["rep"]
    assert rep.killed >= 20 and rep.survived >= 20
    weights = np.concatenate([b["weight"] for b in got["banks"]])
    assert np.sum(weights != 1.0) >= 50 and np.sum(weights == ws) >= 1
    _assert_against(got, want, prob)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_degenerate_geometry(iface, make_problem, cs, monkeypatch, variant):
    """8. the beams of tests/degenerate_states.py, every side vacuum: zero cosines along a wall, equal
    facet times into a corner; each history is banked once, through the side the reference names"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("stream", nx=16, nparticles=96, iterations=3)
    probe = ob.OracleRun(prob, *cs)
    probe.inject()
    states = tv._degenerate_states(prob, probe.particles.as_dict())
    got = _run(iface, prob, cs, 3, variant, states=states, outflow=True, vacuum="all")
    want = _reference(prob, cs, got["injected"], 3, 15)
    assert sum(len(b) for b in want["banks"]) == int(np.sum(want["snaps"][-1]["dead"])) >= 64
    _assert_against(got, want, prob)


def _put_back(iface, sim, parts):
    tv._upload(iface, sim, parts)
    iface.library().neutral_hip_invalidate_particles(sim.particles)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_the_bank_source_slot_for_slot(iface, make_problem, cs, monkeypatch, variant):
    """9. the bank of deck a's step 1 into the same store through the periodic shift, snap 1e-12: bit
    for bit the numpy restatement, every slot not refilled untouched; then 100 of them from record 50
    at a quarter of their weight.

    What the periodic shift cannot show is the snap: a west escape sits at x = -1.0e-13 (replayed on
    CPU: -1.00010e-13 .. -0.99996e-13) and lands at width - 1e-13, inside; a north escape sits at
    y == height exactly and lands on 0.0, on the wall.  Restatement and library agree on snapped == 0
    there, for every variant and on the CPU replay's own records, and with snap 0 no record is bad.
    So the snap is shown by the same records WITHOUT a shift -- the translation by nothing onto a mesh
    with the same origin, the driver's --source-bank --: every west record lies 1e-13 outside the
    west wall.  With snap 1e-12 they are moved onto it and counted (snapped == the west records,
    > 0), bit for bit the restatement; with snap 0 the call returns 3, first_bad is the
    restatement's -- the first west record in bank order -- and the store is untouched."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    _, _, width, height = _extent(prob)
    shift = iface.periodic_shift(width, height)
    assert shift == br.periodic_shift(width, height)
    sim = iface.Simulation(prob, *cs, variant=variant, cs_absorb=third_absorb(cs), outflow=True, vacuum="wn",
                           escape_bank=CAPACITY)
    try:
        sim.inject()
        r = sim.step(1)
        k = r.step_claimed
        assert k == sum(r.escape.counts()) >= 300
        parts = sim.particle_arrays()
        records = sim.escape_bank_host(0, k)
        assert set(parts) == set(tv.ALL_FIELDS)

        def emitted_as_restated(first, count, scale, snap):
            code, want, said = br.bank_source(parts, records, first, count, scale, shift, snap, prob.edgex, prob.edgey,
                                              prob.dt, pad=prob.pad)
            try:
                stats = sim.emit(count, source=iface.BankSource(sim.escape_bank[:64 * k], first=first, shift=shift,
                                                                weight_scale=scale, snap=snap))
                got_code = 0
            except iface.BankSourceRefused as refused:
                stats, got_code = refused.stats, refused.code
                assert refused.first_bad == said["first_bad"]
            assert got_code == code
            got = sim.particle_arrays()
            for f in tv.ALL_FIELDS:
                assert np.array_equal(got[f], want[f]), (f, first, count, scale, snap)
            assert (stats.dead_before, stats.emitted, stats.first_bad) == (said["dead_before"], said["emitted"], said["first_bad"])
            if code == 0:
                assert stats.snapped == said["snapped"]
                filled = np.flatnonzero(parts["dead"] != 0)[:said["emitted"]]
                total = float(np.sum(want["weight"][filled]))
                assert abs(stats.weight_emitted - total) <= 1e-12 * total
            return said

        said = emitted_as_restated(0, k, 1.0, SNAP)
        assert said["emitted"] == k and said["snapped"] == 0
        _put_back(iface, sim, parts)
        said = emitted_as_restated(50, 100, 0.25, SNAP)
        assert said["emitted"] == 100
        # ... and the snap, on the records where they lie: no shift
        west = np.flatnonzero(records["side"] == W)
        assert len(west) >= 300 and np.all(records["x"][west] < 0.0) and np.all(records["x"][west] >= -1.001e-13)
        shift = None
        _put_back(iface, sim, parts)
        said = emitted_as_restated(0, k, 1.0, SNAP)
        assert said["emitted"] == k and said["snapped"] == len(west) > 0
        _put_back(iface, sim, parts)
        said = emitted_as_restated(0, k, 1.0, 0.0)
        assert said["first_bad"] == int(west[0]) and said["emitted"] == 0
        _put_back(iface, sim, parts)
        said = emitted_as_restated(int(west[0]) + 1, k - int(west[0]) - 1, 1.0, 0.0)   # (first_bad counts from records[0], not from first)
        assert said["first_bad"] == int(west[west > west[0]][0])
        shift = iface.periodic_shift(width, height)
        # a numpy bank, uploaded by the source: the same slots
        _put_back(iface, sim, parts)
        code, want, _ = br.bank_source(parts, records, 0, 7, 1.0, shift, SNAP, prob.edgex, prob.edgey, prob.dt, pad=prob.pad)
        stats = sim.emit(7, source=iface.BankSource(records[:7], shift=shift, snap=SNAP))
        got = sim.particle_arrays()
        assert code == 0 and stats.emitted == 7 and all(np.array_equal(got[f], want[f]) for f in tv.ALL_FIELDS)
    finally:
        sim.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", ["a", "b"])
def test_inside_a_run(iface, make_problem, cs, monkeypatch, variant, case):
    """10. a periodic boundary out of two vacuum sides: after steps 1 and 2 the step's range is
    re-emitted with the periodic shift.  The replay does the same with ITS records in the order of
    slots the GPU's bank has, after the step's set of records has been found equal; steps 2 and 3
    are then the replay's, events, states and tallies.  The bank is reset after each re-emission --
    case b's three steps claim 1327 indexes, more than the 1024 the bank holds."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, case)
    _, _, width, height = _extent(prob)
    shift = iface.periodic_shift(width, height)
    vacuum = tv.CASES[case]["vacuum"]

    def between(tt, sim, lo, hi):
        stats = sim.emit(hi - lo, source=iface.BankSource(sim.escape_bank, first=lo, shift=shift, snap=SNAP))
        sim.reset_escape_bank()
        return dict(emitted=int(stats.emitted), snapped=int(stats.snapped), after=sim.particle_arrays())
    got = _run(iface, prob, cs, 3, variant, between=between, cs_absorb=third_absorb(cs), outflow=True, vacuum=vacuum,
               scalar_flux=True, collision_tallies=True)
    orders = [b["slot"].tolist() for b in got["banks"]]

    def check(step, records):
        _assert_records(got["banks"][step - 1], records, got["snaps"][step], prob, f"step {step}")
    want = _wrap_reference(prob, cs, got["injected"], 3, vacuum, third_absorb(cs), orders=orders, check=check)
    print(f"case {case} variant {variant}: escaped {[s['escaped'] for s in want['per_step']]}, emitted {want['emitted']}")
    assert [s["emitted"] for s in got["said"]] == [s["emitted"] for s in want["emitted"]] == [len(o) for o in orders[:2]]
    assert [s["snapped"] for s in got["said"]] == [s["snapped"] for s in want["emitted"]]
    _assert_against(got, want, prob, accumulated=False)
    rep = want["rep"]
    for side in range(4):
        tv._assert_mesh(got["out"][side], rep.out[side], tv.SIDE_NAMES[side])
    tv._assert_mesh(got["flux"], rep.flux, "flux")
    tv._assert_mesh(got["absorbed"], rep.absorbed, "absorbed")
    assert np.array_equal(got["collisions"].ravel(), rep.collisions.ravel())


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["shard", "domain 2x1"])
def test_two_ranks(iface, make_problem, cs, tmp_path, monkeypatch, mode):
    """11. shards: each rank's bank is the reference's escapes of its slots, and the ranks'
    step_claimed sum to the escape statistics.  A decomposed mesh: the step runs as without the bank
    -- by id the one-rank run's dead flags and cells, its events -- and claims nothing."""
    from neutral_amd import decks, host
    steps = 3
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), nx=24, ny=24, nparticles=600, iterations=steps, dt=1.0e-6)
    prob = host.setup_problem(deck)   # (as the worker reads it)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    one = _run(iface, prob, cs, steps, 2, capacity=None, cs_absorb=third_absorb(cs), outflow=True, vacuum="wn")
    counts = [list(r.escape.counts()) for r in one["steps"]]
    assert sum(sum(c) for c in counts) >= 40
    sim_kw = dict(capture_scale=0.5, outflow=True, vacuum="wn", escape_bank=CAPACITY)
    launch_ranks([sys.executable, BANK_WORKER, deck, str(tmp_path), str(steps), mode, json.dumps(sim_kw)], 2)
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(2)]
    said = []
    for r in range(2):
        with open(os.path.join(str(tmp_path), f"bank{r}.json")) as f:
            said.append(json.load(f))
    ids = np.concatenate([z["ids"] for z in ranks]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(prob.nparticles))
    for f in ("dead", "cellx", "celly"):
        by_id = np.empty(prob.nparticles, dtype=np.int32)
        by_id[ids] = np.concatenate([z[f] for z in ranks])
        assert np.array_equal(by_id, one["parts"][f]), f
    for r in range(2):
        assert [s["escaped"] for s in said[r]] == counts, r
        assert ranks[r]["events"].tolist() == [[s.nprocessed, s.facets, s.collisions, s.census] for s in one["steps"]]
    banks = [np.load(os.path.join(str(tmp_path), f"bank{r}.npy")).view(br.RECORD) for r in range(2)]
    if mode != "shard":
        for r in range(2):
            assert all((s["step_claimed"], s["step_recorded"]) == (0, 0) for s in said[r]) and len(banks[r]) == 0
        return
    want = _reference(prob, cs, one["injected"], steps, tv._bit(W, N), third_absorb(cs))
    for tt in range(steps):
        assert sum(said[r][tt]["step_claimed"] for r in range(2)) == sum(counts[tt])
    for r in range(2):
        first, n = int(ranks[r]["ids"][0]), len(ranks[r]["ids"])
        after = {f: ranks[r][f] for f in BITWISE + ("dead",)}
        lo = 0
        for tt in range(steps):
            mine = [dict(rec, slot=rec["slot"] - first) for rec in want["banks"][tt] if first <= rec["slot"] < first + n]
            hi = lo + said[r][tt]["step_claimed"]
            got = np.sort(banks[r][lo:hi], order="slot")
            assert len(mine) == hi - lo and got["slot"].tolist() == [m["slot"] for m in mine], (r, tt)
            assert got["side"].tolist() == [m["side"] for m in mine], (r, tt)
            ref = br.records_of(mine)
            if len(mine):
                assert np.max(np.abs(got["time_left"] - ref["time_left"])) <= STATE_TOL * prob.dt
                assert np.max(np.abs(got["weight"] - ref["weight"]) / ref["weight"]) <= STATE_TOL
            if tt == steps - 1 and len(mine):     # (the arrays the worker kept are those after the last step)
                for f in BITWISE:
                    assert np.array_equal(got[f], after[f][got["slot"].astype(np.int64)]), (r, f)
            lo = hi
        assert lo == len(banks[r])


def _read_bank_file(path):
    with open(path, "rb") as f:
        blob = f.read()
    assert blob[:8] == b"NHBANK01"
    (count,) = struct.unpack("<Q", blob[8:16])
    assert len(blob) == 16 + 64 * count
    return np.frombuffer(blob[16:], dtype=br.RECORD).copy()


@gpu
@needs_gpu
def test_driver(iface, cs, tmp_path):
    """12. --escape-bank 1024,PATH on deck b's mesh and sides: a `Banked` line per step, and the file's
    records are, as a set, the Python run's; then --source-bank PATH,1e-12: the per-step event counts
    of a Simulation emitting the same records"""
    assert os.path.exists(OWN_DRIVER), "neutral.hip not built"
    from neutral_amd import cs_table, decks, host
    run = tmp_path / "arch" / "neutral"
    (run / "problems").mkdir(parents=True)
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    size = dict(nx=24, ny=17, nparticles=600, iterations=3, dt=2.0e-6)
    sets = []
    for k, v in size.items():
        sets += ["--set", f"{k}={v}"]
    path = str(tmp_path / "escapes.bank")
    said = run_driver(str(run), rel, sets + ["--vacuum", "ws", "--escape-bank", f"{CAPACITY},{path}"])
    lines = [ln for ln in said.splitlines() if ln.startswith("Banked: ")]
    assert len(lines) == size["iterations"]
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), **size)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    py = _run(iface, prob, cs, size["iterations"], 2, vacuum="ws")
    assert [ln.split()[1:] for ln in lines] == [[str(s["claimed"]), str(s["recorded"])] for s in py["stats"]]
    records = _read_bank_file(path)
    mine = np.concatenate(py["banks"])
    assert len(records) == len(mine) >= 100
    lo = 0
    for bank in py["banks"]:                                  # step by step: the same set of records, bit for bit
        hi = lo + len(bank)
        assert np.array_equal(np.sort(records[lo:hi], order="slot"), np.sort(bank, order="slot"))
        lo = hi
    # the second run: up to 1024 records before every step from the second, continuing in the file
    again = run_driver(str(run), rel, sets + ["--vacuum", "ws", "--source", "1024", "--source-bank", f"{path},1e-12"])
    events = list(zip((int(ln.split()[1]) for ln in again.splitlines() if ln.startswith("Facets ")),
                      (int(ln.split()[1]) for ln in again.splitlines() if ln.startswith("Collisions "))))
    sim = iface.Simulation(prob, *cs, variant=2, vacuum="ws")
    try:
        sim.inject()
        source_next, emitted, want = 0, 0, []
        for tt in range(1, size["iterations"] + 1):
            if tt >= 2:
                stats = sim.emit(1024, source=iface.BankSource(records, first=source_next, snap=1e-12))
                source_next += int(stats.emitted)
                emitted += int(stats.emitted)
            r = sim.step(tt)
            want.append((r.facets, r.collisions))
    finally:
        sim.close()
    assert events == want and emitted > 0
    m = re.search(r"^Source emitted (\d+)$", again, re.M)
    assert m and int(m.group(1)) == emitted

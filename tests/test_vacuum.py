"""Vacuum sides (include/neutral_hip.h: neutral_hip_set_vacuum_sides): a history that would reflect
through a chosen outer side escapes instead -- dead on the wall, direction unturned, its time over.
The CPU oracle reflects everywhere and is frozen, so the reference is tests/replay.py, whose loop
asks its wall hook for the one rule (Replay(vacuum=...)): pinned here to the bits of the loop with
no side vacuum and to hand-computed flights, then held against every kernel variant per history,
per cell and per side; and, for the collision-free deck, against nothing but straight-line
geometry (tests/escape_reference.py).

Tolerances are tests/test_outflow.py's: a mesh against its reference TALLY_L2_TOL, a sum
TALLY_SUM_TOL, two runs of the same histories 1e-13; cells, `dead` and counts exact.  The floating
state of a slot is held to tests/test_decomposition.py's 1e-9 -- of the mesh's width for a position
(one on the west or south wall is 1e-13 by the open bound's correction: a relative measure of it
would compare rounding noise), of the value for energy and weight, absolute for a cosine."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import degenerate_states as dg
import escape_reference as er
import oracle_binding as ob
import replay
from gpu_support import OWN_DRIVER, gpu, iface, l2, needs_gpu, run_driver, third_absorb  # noqa: F401
from ranks import launch_ranks
from test_window_roulette import two_valued

TALLY_L2_TOL = 1e-9
TALLY_SUM_TOL = 1e-10
SAME_HISTORIES_TOL = 1e-13
STATE_TOL = 1e-9
ROULETTE = (0.25, 0.5)
W, E, S, N = replay.WEST, replay.EAST, replay.SOUTH, replay.NORTH
SIDE_NAMES = ("west", "east", "south", "north")
ESCAPE_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_escape_worker.py")
ALL_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "dt_to_census", "mfp_to_collision",
              "cellx", "celly", "dead")


def _bit(*sides):
    return sum(1 << s for s in sides)


# ---- CPU: the ABI and the mask -----------------------------------------------------------------

def test_library_exports_the_setter_at_the_same_abi_version():
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in ("neutral_hip_set_vacuum_sides", "neutral_hip_get_vacuum_sides", "neutral_hip_last_escape"):
        assert hasattr(lib, name), name
        assert name in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert C.sizeof(iface.EscapeStats) == 64


def test_vacuum_mask_and_the_setters_refusal():
    """letters in any case and order, "all", an int; anything else is a ValueError; the library
    refuses a bit above 8 and keeps what it had (no device is touched)"""
    from neutral_amd import interface as iface
    assert iface.vacuum_mask("wn") == 9 and iface.vacuum_mask("NW") == 9
    assert [iface.vacuum_mask(c) for c in "wesn"] == [1, 2, 4, 8]
    assert iface.vacuum_mask("all") == 15 and iface.vacuum_mask("wesn") == 15 and iface.vacuum_mask("ALL") == 15
    assert iface.vacuum_mask(None) == 0 and iface.vacuum_mask("") == 0 and iface.vacuum_mask(0) == 0
    assert iface.vacuum_mask(6) == 6 and iface.vacuum_mask(np.int32(12)) == 12
    for bad in ("x", "west", "w,n", 16, -1, 1.0, True, ["w"]):
        with pytest.raises(ValueError):
            iface.vacuum_mask(bad)
    lib = iface.library()
    try:
        assert lib.neutral_hip_get_vacuum_sides() == 0     # the default
        iface.set_vacuum_sides("es")
        assert iface.get_vacuum_sides() == 6
        for bad in (16, 17, 1 << 8, 0xFFFFFFFF):
            assert lib.neutral_hip_set_vacuum_sides(bad) == 1
            assert lib.neutral_hip_get_vacuum_sides() == 6  # nothing changed
            with pytest.raises(ValueError):
                iface.set_vacuum_sides(bad)
        assert lib.neutral_hip_set_vacuum_sides(15) == 0 and iface.get_vacuum_sides() == 15
    finally:
        iface.set_vacuum_sides(0)
    assert iface.get_vacuum_sides() == 0
    stats = iface.last_escape()
    assert len(stats.counts()) == 4 and len(stats.weights()) == 4


# ---- CPU: the restated loop --------------------------------------------------------------------

def _spectrum_of(prob):
    return (prob.initial_energy * np.geomspace(0.5, 1.02, 9), (3, 4, prob.nx - 2, prob.ny - 1))


def _oracle_injected(prob, cs):
    ref = ob.OracleRun(prob, *cs)
    ref.inject()
    return {f: a.copy() for f, a in ref.particles.as_dict().items()}


def _replayed(prob, cs, injected, steps, **kw):
    rep = replay.Replay(prob, cs, **kw)
    return rep, replay.run_steps(rep, injected, steps)


def _same_replays_bits(a, b):
    """(rep, run) twice: every field of every slot after every step, every mesh and the spectrum,
    every count and what every step added to it"""
    (rep_a, run_a), (rep_b, run_b) = a, b
    for tt, (xa, xb) in enumerate(zip(run_a["snaps"], run_b["snaps"])):
        for f in replay.FIELDS:
            assert np.array_equal(xa[f], xb[f]), (tt, f)
    for name in replay.MESHES:
        assert np.array_equal(getattr(rep_a, name), getattr(rep_b, name)), name
    assert rep_a.track == rep_b.track and rep_a.coll == rep_b.coll
    for name in ("nfacets", "ncollisions", "ncensus", "wall_hits", "killed", "survived", "lost", "gained",
                 "reflections", "escaped", "escape_weight"):
        assert getattr(rep_a, name) == getattr(rep_b, name), name
    assert run_a["per_step"] == run_b["per_step"]


def test_no_vacuum_side_gives_the_replays_bits(make_problem, cs):
    """The deck of test_replay_walks_the_oracles_histories (csp 24^2, 600, 3 steps, p_absorb 1/3,
    roulette), bit for bit.  Mask 0 against the keyword left out is one path taken twice and says
    little; so also a mask that is not 0: in one step of 5e-7 s the histories turn round on the west
    and the south wall some hundred times each and none reaches the east or the north wall
    (asserted from the reflections by side), and with those two sides vacuum no bit may change."""
    prob = make_problem("csp", nx=24, nparticles=600, iterations=3, dt=1.0e-6)
    injected = _oracle_injected(prob, cs)
    edges, box = _spectrum_of(prob)
    kw = dict(cs_absorb=third_absorb(cs), roulette=ROULETTE, edges=edges, box=box)
    left_out, zero = _replayed(prob, cs, injected, 3, **kw), _replayed(prob, cs, injected, 3, vacuum=0, **kw)
    _same_replays_bits(left_out, zero)
    rep = zero[0]
    assert rep.ncollisions > 500 and rep.wall_hits > 0 and rep.killed > 0 and any(rep.track) and any(rep.coll)
    assert sum(rep.reflections) == rep.wall_hits and sum(rep.escaped) == 0 and rep.ncensus > 0
    short = _replayed(prob, cs, injected, 1, dt=5.0e-7, **kw)
    rep = short[0]
    assert rep.reflections[E] == 0 and rep.reflections[N] == 0
    assert rep.reflections[W] >= 100 and rep.reflections[S] >= 100 and any(rep.track)
    unreached = _replayed(prob, cs, injected, 1, dt=5.0e-7, vacuum=_bit(E, N), **kw)
    _same_replays_bits(short, unreached)
    assert sum(unreached[0].escaped) == 0


def _flights(make_problem, cs, vacuum, starts, length=0.05, nx=10):
    """collision-free flights of `length` metres on an nx x nx mesh of 1 m, one history per
    (x, y, ox, oy) of `starts`, all through one Replay"""
    prob = make_problem("stream", nx=nx, nparticles=4, iterations=1)
    e0 = prob.initial_energy
    rep = replay.Replay(prob, cs, dt=length / replay.speed_of(e0), vacuum=vacuum)
    states = []
    for pid, (x, y, ox, oy) in enumerate(starts):
        s = dict(x=x, y=y, omega_x=ox, omega_y=oy, energy=e0, weight=1.0, dead=0,
                 cellx=min(int(x * nx), nx - 1), celly=min(int(y * nx), nx - 1))
        rep.history(pid, 1, s)
        states.append(s)
    assert rep.ncollisions == 0
    return rep, states


@pytest.mark.parametrize("start,omega,side,cell,back", [
    ((0.97, 0.55), (1.0, 0.0), E, (9, 5), ((0.03, 0.35), (-1.0, 0.0), W, (0, 3))),
    ((0.03, 0.55), (-1.0, 0.0), W, (0, 5), ((0.97, 0.35), (1.0, 0.0), E, (9, 3))),
    ((0.55, 0.97), (0.0, 1.0), N, (5, 9), ((0.35, 0.03), (0.0, -1.0), S, (3, 0))),
    ((0.55, 0.03), (0.0, -1.0), S, (5, 0), ((0.35, 0.97), (0.0, 1.0), N, (3, 9))),
])
def test_a_flight_at_a_vacuum_wall_escapes_and_one_at_another_wall_turns(make_problem, cs, start, omega, side, cell, back):
    """0.05 m towards a wall 0.03 m away that is vacuum: one facet event, scored as outflow through
    that side of the wall cell with the weight flown with; the history is dead ON the wall, in that
    cell, its direction unturned; nothing is scored behind the wall -- the flux holds 0.03 m, not
    0.05, and no census happened.  The second history of the same run flies at the opposite wall,
    which reflects: it turns as it always did and flies its 0.05 m."""
    (bx, by), bo, bside, bcell = back
    rep, (s, t) = _flights(make_problem, cs, 1 << side, [start + omega, (bx, by) + bo])
    assert rep.nfacets == 2 and rep.ncensus == 1
    assert rep.escaped == [1 if k == side else 0 for k in range(4)]
    assert rep.escape_weight == [1.0 if k == side else 0.0 for k in range(4)]
    assert rep.reflections == [1 if k == bside else 0 for k in range(4)] and rep.wall_hits == 1
    want = np.zeros((4, 10, 10))
    want[side, cell[1], cell[0]] = 0.25
    want[bside, bcell[1], bcell[0]] = 0.25
    assert np.array_equal(rep.out, want)
    # the one that escaped
    assert s["dead"] == 1 and (s["cellx"], s["celly"]) == cell
    assert (s["omega_x"], s["omega_y"]) == omega and s["weight"] == 1.0
    moved, kept = (s["x"], s["y"]) if omega[0] else (s["y"], s["x"])
    assert moved == pytest.approx(1.0 if sum(omega) > 0 else 0.0, abs=1e-12) and kept == 0.55
    assert rep.flux[cell[1], cell[0]] == pytest.approx(0.03 / 4, rel=1e-12)
    # the one that turned
    assert t["dead"] == 0 and (t["cellx"], t["celly"]) == bcell
    assert (t["omega_x"], t["omega_y"]) == (-bo[0] + 0.0, -bo[1] + 0.0)
    moved = t["x"] if bo[0] else t["y"]
    assert moved == pytest.approx(0.98 if sum(bo) > 0 else 0.02)
    assert rep.flux[bcell[1], bcell[0]] == pytest.approx(0.05 / 4, rel=1e-12)
    assert rep.flux.sum() == pytest.approx(0.08 / 4, rel=1e-12)


def test_a_zero_cosine_toward_a_vacuum_wall_does_not_escape(make_problem, cs):
    """along the south row with omega_y == 0, every side vacuum but the ones it can reach: it reflects
    east, never leaves through the south wall it runs along"""
    rep, (s,) = _flights(make_problem, cs, _bit(S, N), [(0.97, 0.05, 1.0, 0.0)])
    assert rep.escaped == [0, 0, 0, 0] and rep.reflections[E] == 1 and s["dead"] == 0


def test_a_window_and_vacuum_sides_in_one_replay(make_problem, cs):
    """Case (a) under the two-valued window mesh, ratio 2: the two hooks in one loop.  Mask 0 is the
    window alone and a mesh of zeros the vacuum sides alone, bit for bit; and with both, all the
    weight that the slots of live histories no longer hold is with the absorbed mesh, with
    roulette's lost and gained sums and with the escapes by side (1e-12 of N: the margin of
    tests/test_window_roulette.py::test_weight_balance)."""
    prob = _case_problem(make_problem, "a")
    n, vacuum, absorb = prob.nparticles, CASES["a"]["vacuum"], third_absorb(cs)
    injected = _oracle_injected(prob, cs)
    assert np.all(injected["weight"] == 1.0)
    mesh = two_valued(prob.nx, prob.ny)

    def replayed(**kw):
        return _replayed(prob, cs, injected, 3, cs_absorb=absorb, **kw)
    window_only = replayed(window=replay.Window(mesh, 2.0))
    _same_replays_bits(replayed(window=replay.Window(mesh, 2.0), vacuum=0), window_only)
    vacuum_only = replayed(vacuum=vacuum)
    _same_replays_bits(replayed(window=replay.Window(np.zeros_like(mesh), 2.0), vacuum=vacuum), vacuum_only)
    rep, run = replayed(window=replay.Window(mesh, 2.0), vacuum=vacuum)
    end = run["snaps"][-1]
    print(f"killed {rep.killed} survived {rep.survived} escaped {rep.escaped} lost {rep.lost} gained {rep.gained}")
    assert rep.killed >= 20 and rep.survived >= 20 and min(rep.escaped[W], rep.escaped[N]) >= 50
    dead =end["dead"] != 0
    killed = dead & (end["weight"] == 0.0)
    too_slow = dead & ~killed & (end["energy"] < replay.MIN_ENERGY_OF_INTEREST)
    escaped = dead & ~killed & ~too_slow
    assert (int(killed.sum()), int(escaped.sum())) == (rep.killed, sum(rep.escaped))
    assert abs(end["weight"][escaped].sum() - sum(rep.escape_weight)) <= 1e-12 * n
    missing = n - end["weight"][~dead].sum()
    accounted = n * rep.absorbed.sum() + rep.lost - rep.gained + sum(rep.escape_weight) + end["weight"][too_slow].sum()
    print("missing from the live slots", missing, "accounted for", accounted)
    assert abs(missing - accounted) <= 1e-12 * n


# ---- the GPU runs and their references ----------------------------------------------------------

def _host(t):
    return None if t is None else t.cpu().numpy().copy()


def _upload(iface, sim, states):
    p = sim.particles.contents
    for f, a in states.items():
        a = np.ascontiguousarray(a)
        assert a.dtype == (np.int32 if f in ("cellx", "celly", "dead") else np.float64) and len(a) == sim.n
        iface.library().neutral_hip_memcpy_h2d(C.c_void_p(getattr(p, f)), a.ctypes.data, a.nbytes)


def _run(iface, prob, cs, steps, variant, states=None, between=None, window=None, **kw):
    """inject (and overwrite with `states`), step; the arrays after every step; between(tt, sim) after
    step tt but the last; window = dict(lower=, survival_ratio=) puts the in-step window in force"""
    sim = iface.Simulation(prob, *cs, variant=variant, **kw)
    try:
        sim.inject()
        if states is not None:
            _upload(iface, sim, states)
        if window is not None:
            sim.window_in_step(**window)
        injected = sim.particle_arrays()
        results, snaps, said = [], [injected], []
        for tt in range(1, steps + 1):
            results.append(sim.step(tt))
            assert results[-1].stats.aborted == 0
            snaps.append(sim.particle_arrays())
            if between is not None and tt < steps:
                said.append(between(tt, sim))
        return dict(steps=results, injected=injected, snaps=snaps, parts=snaps[-1], said=said,
                    tally=sim.tally_host().copy(), flux=_host(sim.flux), absorbed=_host(sim.absorbed),
                    collisions=_host(sim.collisions),
                    out=sim.outflow_host().copy() if sim.outflow is not None else None)
    finally:
        sim.close()


def _everything(prob, roulette=None):
    return dict(scalar_flux=True, collision_tallies=True, current=True, spectrum=_spectrum_of(prob), roulette=roulette)


_REFERENCES = {}


def _reference(prob, cs, injected, steps, vacuum, cs_absorb=None, roulette=(0.0, 0.0), window=None):
    """the restated replay of every history of `injected`, once per configuration"""
    key = (prob.nx, prob.ny, prob.dt, steps, vacuum, cs_absorb is not None, tuple(roulette),
           None if window is None else (window.lower.tobytes(), window.ratio),
           prob.density.tobytes(), tuple(injected[f].tobytes() for f in replay.FIELDS))
    if key not in _REFERENCES:
        rep = replay.Replay(prob, cs, cs_absorb, roulette, vacuum=vacuum, window=window)
        run = replay.run_steps(rep, injected, steps)
        run["rep"] = rep
        _REFERENCES[key] = run
    return _REFERENCES[key]


def _assert_events(got, want):
    """per step: histories processed, facets, collisions, census, escapes by side -- exact; the
    escapes' weights within TALLY_SUM_TOL"""
    for tt, (r, w) in enumerate(zip(got["steps"], want["per_step"]), 1):
        assert (r.nprocessed, r.facets, r.collisions, r.census) == \
            (w["nprocessed"], w["facets"], w["collisions"], w["census"]), tt
        assert list(r.escape.counts()) == w["escaped"], tt
        for side in range(4):
            assert abs(r.escape.weights()[side] - w["weight"][side]) <= TALLY_SUM_TOL * w["weight"][side], (tt, side)


def _assert_state(got, want, width=1.0):
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("x", "y"):
        assert np.max(np.abs(got[f] - want[f])) <= STATE_TOL * width, f
    for f in ("omega_x", "omega_y"):
        assert np.max(np.abs(got[f] - want[f])) <= STATE_TOL, f
    for f in ("energy", "weight"):
        assert np.max(np.abs(got[f] - want[f]) / np.maximum(np.abs(want[f]), 1e-300)) <= STATE_TOL, f


def _assert_mesh(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert want.any(), what
    assert not got[want == 0.0].any(), what
    assert l2(got, want) <= TALLY_L2_TOL, (what, l2(got, want))


CASES = {
    "a": dict(vacuum=_bit(W, N), dt=1.0e-6, reflecting=(E, S)),
    "b": dict(vacuum=_bit(W, S), dt=2.0e-6, reflecting=(E, N)),
}


def _case_problem(make_problem, case, nx=24, ny=17):
    """csp, 600 particles, 3 steps, the density mesh rewritten to a uniform 0.3: histories collide
    everywhere and reach every wall"""
    prob = make_problem("csp", nx=nx, ny=ny, nparticles=600, iterations=3, dt=CASES[case]["dt"])
    prob.density[:] = 0.3
    return prob


def _case_reference(prob, cs, injected, case, roulette=(0.0, 0.0)):
    """... and what the case must show before anything is compared with it"""
    c = CASES[case]
    want = _reference(prob, cs, injected, 3, c["vacuum"], third_absorb(cs), roulette)
    rep = want["rep"]
    print(f"case {case}: escaped {rep.escaped} ({rep.escaped_not_unit} with weight != 1), reflections "
          f"{rep.reflections}, {rep.ncollisions} collisions, {int(np.sum(want['snaps'][-1]['dead'] == 0))} live")
    for side in range(4):
        if (c["vacuum"] >> side) & 1:
            assert rep.escaped[side] >= 50 and rep.reflections[side] == 0, side
        else:
            assert rep.reflections[side] >= 50 and rep.escaped[side] == 0, side
    assert rep.escaped_not_unit >= 50
    if case == "a":
        assert np.sum(want["snaps"][-1]["dead"] == 0) >= 20
    return want


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("arith", ["auto", "checked"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_against_the_restated_replay(iface, make_problem, cs, monkeypatch, variant, arith, case):
    """4. A mesh that is not square, collisions everywhere, every optional tally on, two vacuum and
    two reflecting sides: every slot, every event count, the escapes by side and every mesh are the
    restated replay's."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _case_problem(make_problem, case)
    iface.set_arithmetic(iface.ARITH_CHECKED if arith == "checked" else iface.ARITH_AUTO)
    got = _run(iface, prob, cs, 3, variant, cs_absorb=third_absorb(cs), outflow=True, vacuum=CASES[case]["vacuum"],
               **_everything(prob))
    want = _case_reference(prob, cs, got["injected"], case)
    rep = want["rep"]
    _assert_events(got, want)
    for tt in (1, 2, 3):
        _assert_state(got["snaps"][tt], want["snaps"][tt])
    for side in range(4):
        _assert_mesh(got["out"][side], rep.out[side], SIDE_NAMES[side])
    _assert_mesh(got["flux"], rep.flux, "flux")
    _assert_mesh(got["absorbed"], rep.absorbed, "absorbed")
    assert np.array_equal(got["collisions"].ravel(), rep.collisions.ravel())
    # the per-side weight is N times the outflow through that outer side (an identity, not how it is made)
    n = prob.nparticles
    outer = (got["out"][W][:, 0], got["out"][E][:, -1], got["out"][S][0, :], got["out"][N][-1, :])
    total = [sum(r.escape.weights()[side] for r in got["steps"]) for side in range(4)]
    for side in range(4):
        if (CASES[case]["vacuum"] >> side) & 1:
            assert abs(n * outer[side].sum() - total[side]) <= TALLY_SUM_TOL * total[side], side


# ---- 5. exact, collision-free ---------------------------------------------------------------------

def _stream_problem(make_problem):
    return make_problem("stream", nx=20, ny=13, nparticles=512, iterations=3)


def _outer(out):
    return (out[W][:, 0], out[E][:, -1], out[S][0, :], out[N][-1, :])


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_every_history_leaves_a_collision_free_box_exactly(iface, make_problem, cs, monkeypatch, variant):
    """Every side vacuum, every weight 1, N a power of two: all 512 histories are out in step 1; the
    escapes' weight and N times the outflow through each outer side ARE the counts; steps 2 and 3
    process nothing.  And where each history left is what straight-line geometry says."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _stream_problem(make_problem)
    n = prob.nparticles
    got = _run(iface, prob, cs, 3, variant, outflow=True, vacuum="all")
    want = _reference(prob, cs, got["injected"], 3, 15)
    rep = want["rep"]
    print(f"variant {variant}: escaped {rep.escaped}")
    assert sum(rep.escaped) == n and min(rep.escaped) >= 50 and rep.ncollisions == 0
    assert want["per_step"][0]["escaped"] == rep.escaped
    _assert_events(got, want)
    first = got["steps"][0].escape
    assert list(first.counts()) == rep.escaped
    assert list(first.weights()) == [float(c) for c in rep.escaped]
    assert [n * side.sum() for side in _outer(got["out"])] == [float(c) for c in rep.escaped]
    for r in got["steps"][1:]:
        assert (r.nprocessed, r.facets, r.census) == (0, 0, 0) and sum(r.escape.counts()) == 0
    for tt in (1, 2, 3):
        _assert_state(got["snaps"][tt], want["snaps"][tt])
        assert np.all(got["snaps"][tt]["dead"] == 1)
    # the second opinion: no event loop, no cells
    x0, x1, y0, y1 = (float(v) for v in (prob.edgex[0], prob.edgex[-1], prob.edgey[0], prob.edgey[-1]))
    inj, end = got["injected"], got["parts"]
    side, ex, ey, corner = er.exits_by_geometry(inj["x"] - x0, inj["y"] - y0, inj["omega_x"], inj["omega_y"],
                                                x1 - x0, y1 - y0)
    clear = corner > 1e-9 * (x1 - x0)
    assert np.all(clear)
    on = np.stack([np.abs(end["x"] - x0), np.abs(end["x"] - x1), np.abs(end["y"] - y0), np.abs(end["y"] - y1)])
    assert np.all(np.sum(on <= 1e-12, axis=0) == 1)
    assert np.array_equal(np.argmin(on, axis=0), side)
    assert np.max(np.abs(end["x"] - x0 - ex)) <= 1e-12 and np.max(np.abs(end["y"] - y0 - ey)) <= 1e-12
    assert [int(np.sum(side == k)) for k in range(4)] == rep.escaped


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_two_vacuum_and_two_reflecting_sides_collision_free(iface, make_problem, cs, monkeypatch, variant):
    """east + south vacuum on the same deck: some histories turn on the other two walls first and
    leave a step later; exact like the above"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _stream_problem(make_problem)
    n = prob.nparticles
    got = _run(iface, prob, cs, 3, variant, outflow=True, vacuum="es")
    want = _reference(prob, cs, got["injected"], 3, _bit(E, S))
    rep = want["rep"]
    alive = [int(np.sum(s["dead"] == 0)) for s in want["snaps"]]
    print(f"variant {variant}: alive {alive}, escaped {rep.escaped}, reflections {rep.reflections}")
    assert 50 <= alive[1] < n and alive[3] == 0
    assert rep.reflections[W] >= 50 and rep.reflections[N] >= 50 and rep.escaped[W] == rep.escaped[N] == 0
    _assert_events(got, want)
    for tt in (1, 2, 3):
        _assert_state(got["snaps"][tt], want["snaps"][tt])
    total = [sum(r.escape.counts()[k] for r in got["steps"]) for k in range(4)]
    weight = [sum(r.escape.weights()[k] for r in got["steps"]) for k in range(4)]
    assert total == rep.escaped and weight == [float(c) for c in total]
    outer = [n * side.sum() for side in _outer(got["out"])]
    assert outer[E] == float(total[E]) and outer[S] == float(total[S])
    assert outer[W] == float(rep.reflections[W]) and outer[N] == float(rep.reflections[N])


# ---- 6. only the rule changed -------------------------------------------------------------------

def _same_bits(a, b, fields=ALL_FIELDS):
    for f in fields:
        assert np.array_equal(a["parts"][f], b["parts"][f]), f
    assert np.array_equal(a["out"], b["out"])


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_a_mask_that_changes_no_history_changes_no_bit(iface, make_problem, cs, monkeypatch, variant):
    """both runs keep the outflow: mask 0 set outright is never having called the setter, and a mask
    whose sides no history reaches is mask 0 -- all eleven arrays and the four meshes, bit for bit"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=24, nparticles=600, iterations=1, dt=1.0e-7)
    never = _run(iface, prob, cs, 1, variant, outflow=True)
    want = _reference(prob, cs, never["injected"], 1, 0)
    rep = want["rep"]
    assert rep.reflections[E] == 0 and rep.reflections[N] == 0 and rep.nfacets > 0
    assert never["steps"][0].facets == rep.nfacets
    iface.set_vacuum_sides(0)
    zero = _run(iface, prob, cs, 1, variant, outflow=True)
    unreached = _run(iface, prob, cs, 1, variant, outflow=True, vacuum="en")
    _same_bits(never, zero)
    _same_bits(never, unreached)
    assert sum(unreached["steps"][0].escape.counts()) == 0
    assert iface.get_vacuum_sides() == 0    # (the Simulation put it back)


# ---- 7. write-back --------------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("vacuum", ["all", "es"])
def test_write_back_of_histories_that_only_stream_and_escape(iface, make_problem, cs, monkeypatch, vacuum):
    """The tiled variant on the stream deck: a history that escaped did nothing but stream, and its
    record must say that it changed.  Eager: after step 1 `dead` and the position on the wall are in
    the caller's arrays.  Lazy: neutral_hip_sync_particles after one and after three steps gives the
    eager run's arrays -- all eleven for a live slot, all but the two clocks for a dead one."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _stream_problem(make_problem)
    eager = _run(iface, prob, cs, 3, 2, outflow=True, vacuum=vacuum)
    want = _reference(prob, cs, eager["injected"], 3, iface.vacuum_mask(vacuum))
    after1 = eager["snaps"][1]
    assert np.array_equal(after1["dead"], want["snaps"][1]["dead"]) and after1["dead"].any()
    _assert_state(after1, want["snaps"][1])
    gone = after1["dead"] == 1
    x0, x1, y0, y1 = (float(v) for v in (prob.edgex[0], prob.edgex[-1], prob.edgey[0], prob.edgey[-1]))
    on_wall = np.minimum(np.minimum(np.abs(after1["x"] - x0), np.abs(after1["x"] - x1)),
                         np.minimum(np.abs(after1["y"] - y0), np.abs(after1["y"] - y1)))
    assert np.all(on_wall[gone] <= 1e-12)
    for steps in (1, 3):
        iface.set_lazy_export(True)
        sim = iface.Simulation(prob, *cs, variant=2, outflow=True, vacuum=vacuum)
        try:
            sim.inject()
            for tt in range(1, steps + 1):
                sim.step(tt)
            lazy = sim.particle_arrays()     # (neutral_hip_sync_particles)
        finally:
            sim.close()
            iface.set_lazy_export(False)
        ref = eager["snaps"][steps]
        assert np.array_equal(lazy["dead"], ref["dead"])
        live = ref["dead"] == 0
        for f in ALL_FIELDS:
            assert np.array_equal(lazy[f][live], ref[f][live]), (steps, f)
            if f not in ("dt_to_census", "mfp_to_collision"):
                assert np.array_equal(lazy[f][~live], ref[f][~live]), (steps, f)


# ---- 8. vacuum without a caller's outflow mesh ---------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_vacuum_without_an_outflow_tally(iface, make_problem, cs, monkeypatch, variant):
    """the rule rides the outflow's kernels, whose buffer is then scored and added to nothing: the
    same slots and escapes as with the tally, the energy deposition within 1e-13"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _case_problem(make_problem, "a")
    opts = dict(cs_absorb=third_absorb(cs), vacuum="wn")
    kept = _run(iface, prob, cs, 3, variant, outflow=True, **opts)
    bare = _run(iface, prob, cs, 3, variant, **opts)
    assert bare["out"] is None
    for f in ALL_FIELDS:
        assert np.array_equal(kept["parts"][f], bare["parts"][f]), f
    for a, b in zip(kept["steps"], bare["steps"]):
        assert (a.nprocessed, a.facets, a.collisions, a.census) == (b.nprocessed, b.facets, b.collisions, b.census)
        assert a.escape.counts() == b.escape.counts() and sum(a.escape.counts()) > 0
        for side in range(4):
            assert abs(a.escape.weights()[side] - b.escape.weights()[side]) <= \
                SAME_HISTORIES_TOL * a.escape.weights()[side]
    assert kept["tally"].any() and l2(bare["tally"], kept["tally"]) <= SAME_HISTORIES_TOL


# ---- 9. degenerate geometry -------------------------------------------------------------------------

def _degenerate_states(prob, injected):
    """Beams from cell centres, eight histories each (tests/degenerate_states.py): along the south
    row and along the west column in the four axis directions -- a zero cosine toward the wall they
    run along -- and from the centres of the four corner cells along the diagonal into the corner,
    where on square cells both facet times are equal to the bit."""
    nx, ny = prob.nx, prob.ny
    rows = []
    for cell in ((nx // 2, 0), (0, ny // 2)):
        b = dg.beams(prob, cell, 8)
        rows += [(b["x"][i], b["y"][i], b["omega_x"][i], b["omega_y"][i], cell[0], cell[1]) for i in range(32)]
    s = dg.S
    for cell, d in (((nx - 1, ny - 1), (s, s)), ((0, ny - 1), (-s, s)), ((nx - 1, 0), (s, -s)), ((0, 0), (-s, -s))):
        x, y = dg.place(np.asarray(prob.edgex, dtype=np.float64), np.asarray(prob.edgey, dtype=np.float64),
                        np.full(8, cell[0]), np.full(8, cell[1]), np.zeros(8, dtype=int), prob.pad)
        rows += [(x[i], y[i], d[0], d[1], cell[0], cell[1]) for i in range(8)]
    assert len(rows) == len(injected["x"])
    cols = list(zip(*rows))
    return dict(x=np.array(cols[0], dtype=np.float64), y=np.array(cols[1], dtype=np.float64),
                omega_x=np.array(cols[2], dtype=np.float64), omega_y=np.array(cols[3], dtype=np.float64),
                cellx=np.array(cols[4], dtype=np.int32), celly=np.array(cols[5], dtype=np.int32))


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_degenerate_geometry(iface, make_problem, cs, monkeypatch, variant):
    """south + west vacuum on a square collision-free mesh.  A beam along the south row with
    omega_y == 0 never leaves through the south wall (it leaves west, or turns east and then leaves
    west), one along the west column never through the west wall; a beam into a corner escapes once,
    through the side its x_facet names.  All against the restated replay."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("stream", nx=16, nparticles=96, iterations=3)
    sim_states = None

    def states_for(injected):
        return _degenerate_states(prob, injected)
    probe = ob.OracleRun(prob, *cs)
    probe.inject()
    sim_states = states_for(probe.particles.as_dict())
    vacuum = _bit(S, W)
    got = _run(iface, prob, cs, 3, variant, states=sim_states, outflow=True, vacuum=vacuum)
    for f, a in sim_states.items():
        assert np.array_equal(got["injected"][f], a), f
    want = _reference(prob, cs, got["injected"], 3, vacuum)
    rep = want["rep"]
    end = want["snaps"][-1]
    # the reference itself: who can and who cannot leave through which wall
    row, column = slice(0, 32), slice(32, 64)
    along_x = np.abs(got["injected"]["omega_y"]) == 0.0
    along_y = np.abs(got["injected"]["omega_x"]) == 0.0
    assert np.all(end["dead"][row][along_x[row]] == 1) and np.all(np.abs(end["x"][row][along_x[row]]) <= 1e-12)
    assert np.all(end["celly"][row][along_x[row]] == 0) and np.all(end["cellx"][row][along_x[row]] == 0)
    assert np.all(end["dead"][column][along_y[column]] == 1) and np.all(np.abs(end["y"][column][along_y[column]]) <= 1e-12)
    corners = slice(64, 96)
    assert np.all(end["dead"][corners][8:] == 1) and rep.escaped[E] == rep.escaped[N] == 0
    assert sum(rep.escaped) == int(np.sum(end["dead"]))          # each history escapes once at most
    _assert_events(got, want)
    for tt in (1, 2, 3):
        _assert_state(got["snaps"][tt], want["snaps"][tt])
    for side in range(4):
        if rep.out[side].any():
            _assert_mesh(got["out"][side], rep.out[side], SIDE_NAMES[side])
        else:
            assert not got["out"][side].any(), side


# ---- 10. with the other options -------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("how", ["roulette", "in-step window"])
def test_with_roulette_the_in_step_window_and_the_census_operations(iface, make_problem, cs, monkeypatch, variant, how):
    """Case (a) with Russian roulette, and under the in-step window with one bound everywhere, which
    is the roulette of the same cutoff and survival weight: the restated replay with that roulette.
    Between steps 2 and 3 the census, the census window and the comb find the escaped slots as the
    dead slots they are."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _case_problem(make_problem, "a")
    n = prob.nparticles
    wc, ws = ROULETTE

    def between(tt, sim):
        if tt != 2:
            return None
        census = sim.census()[2]
        # (every live weight lies in [0.25, 1]: under the roulette's cutoff none stays, and a window of
        # 0.2 .. 1.0 counts and changes nothing)
        window = sim.window(0.2, upper_ratio=5.0)
        assert (window.roulette_killed, window.copies_made) == (0, 0)
        comb = sim.comb(seed=7)
        return dict(census_dead=int(census.dead), census_live=int(census.live), window_dead=int(window.dead_before),
                    comb_live=int(comb.live_before))
    sim_kw = dict(cs_absorb=third_absorb(cs), outflow=True, vacuum="wn", scalar_flux=True, collision_tallies=True)
    if how == "roulette":
        sim_kw["roulette"] = ROULETTE
    sim = iface.Simulation(prob, *cs, variant=variant, **sim_kw)
    try:
        sim.inject()
        injected = sim.particle_arrays()
        if how == "in-step window":
            sim.window_in_step(wc, survival_ratio=ws / wc)
        steps, snaps = [], []
        for tt in (1, 2):
            steps.append(sim.step(tt))
            snaps.append(sim.particle_arrays())
        said = between(2, sim)
        last = sim.step(3)
        assert last.stats.aborted == 0 and last.nprocessed == n    # (the comb filled every slot)
        out = sim.outflow_host().copy()
    finally:
        sim.close()
    want = _reference(prob, cs, injected, 3, CASES["a"]["vacuum"], third_absorb(cs), ROULETTE)
    assert want["rep"].killed >= 20 and want["rep"].survived >= 20 and min(want["rep"].escaped[W], want["rep"].escaped[N]) >= 50
    assert [r.stats.roulette_killed for r in steps] and \
        sum(r.stats.roulette_killed for r in steps) + last.stats.roulette_killed >= 20
    got = dict(steps=steps)
    _assert_events(got, dict(per_step=want["per_step"][:2]))
    for tt in (1, 2):
        _assert_state(snaps[tt - 1], want["snaps"][tt])
    dead = int(np.sum(want["snaps"][2]["dead"]))
    assert dead >= 50
    assert said == dict(census_dead=dead, census_live=n - dead, window_dead=dead, comb_live=n - dead)
    assert out.any()


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_a_two_valued_window_with_vacuum_sides(iface, make_problem, cs, monkeypatch, variant):
    """Case (a) under an in-step window that is no global roulette -- tests/test_window_roulette.py's
    two-valued mesh, ratio 2 -- with the tallies of the test above: every slot, every event count,
    roulette's kills and survivals per step, the escapes by side and every mesh are the replay's
    with the window and the vacuum sides together."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _case_problem(make_problem, "a")
    mesh = two_valued(prob.nx, prob.ny)
    got = _run(iface, prob, cs, 3, variant, window=dict(lower=mesh, survival_ratio=2.0), cs_absorb=third_absorb(cs),
               outflow=True, vacuum="wn", scalar_flux=True, collision_tallies=True)
    want = _reference(prob, cs, got["injected"], 3, CASES["a"]["vacuum"], third_absorb(cs),
                      window=replay.Window(mesh, 2.0))
    rep = want["rep"]
    print(f"variant {variant}: killed {rep.killed}, survived {rep.survived}, escaped {rep.escaped}")
    assert rep.killed >= 20 and rep.survived >= 20 and min(rep.escaped[W], rep.escaped[N]) >= 50
    _assert_events(got, want)
    assert [(r.stats.roulette_killed, r.stats.roulette_survived) for r in got["steps"]] == \
        [(s["killed"], s["survived"]) for s in want["per_step"]]
    for tt in (1, 2, 3):
        _assert_state(got["snaps"][tt], want["snaps"][tt])
    for side in range(4):
        _assert_mesh(got["out"][side], rep.out[side], SIDE_NAMES[side])
    _assert_mesh(got["flux"], rep.flux, "flux")
    _assert_mesh(got["absorbed"], rep.absorbed, "absorbed")
    assert np.array_equal(got["collisions"].ravel(), rep.collisions.ravel())


# ---- 11. ranks sharing the GPU ----------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["shard", "domain 2x1"])
def test_two_ranks(iface, make_problem, cs, tmp_path, monkeypatch, mode):
    """Two ranks on one GPU: by id, `dead` and the cells are the one-rank run's; the outflow meshes
    -- every rank's for shards, assembled for the domain -- are its meshes; the escapes, summed over
    the ranks by the library, are its counts.  (tests/gpu_escape_worker.py is the suite's rank worker
    with the escape stats written out beside what it leaves.)"""
    from neutral_amd import decks, host
    steps = 3
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), nx=24, ny=24, nparticles=600, iterations=steps,
                            dt=1.0e-6)
    prob = host.setup_problem(deck)   # (as the worker reads it)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    one = _run(iface, prob, cs, steps, 2, cs_absorb=third_absorb(cs), outflow=True, scalar_flux=True, vacuum="wn")
    counts = [list(r.escape.counts()) for r in one["steps"]]
    assert sum(c[W] for c in counts) >= 20 and sum(c[N] for c in counts) >= 20
    sim_kw = dict(capture_scale=0.5, outflow=True, scalar_flux=True, vacuum="wn")
    argv = [sys.executable, ESCAPE_WORKER, deck, str(tmp_path), str(steps), mode, json.dumps(sim_kw)]
    launch_ranks(argv, 2)
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(2)]
    ids = np.concatenate([z["ids"] for z in ranks]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(prob.nparticles))
    for f in ("dead", "cellx", "celly"):
        by_id = np.empty(prob.nparticles, dtype=np.int32)
        by_id[ids] = np.concatenate([z[f] for z in ranks])
        assert np.array_equal(by_id, one["parts"][f]), f
    if mode == "shard":
        meshes = [z["out"] for z in ranks]
    else:
        assembled = np.zeros_like(one["out"])
        for z in ranks:
            x0, y0 = (int(v) for v in z["origin"])
            block = z["out"]
            assert block.shape[2] < prob.nx
            assembled[:, y0:y0 + block.shape[1], x0:x0 + block.shape[2]] += block
        meshes = [assembled]
    for out in meshes:
        for side in range(4):
            assert l2(out[side], one["out"][side]) <= TALLY_L2_TOL, side
    for r in range(2):
        with open(os.path.join(str(tmp_path), f"escape{r}.json")) as f:
            said = json.load(f)
        assert [s["escaped"] for s in said] == counts, r
        for s, ref in zip(said, one["steps"]):
            for side in range(4):
                assert abs(s["weight"][side] - ref.escape.weights()[side]) <= TALLY_SUM_TOL * ref.escape.weights()[side]


# ---- 12. the driver ----------------------------------------------------------------------------------

@gpu
@needs_gpu
def test_driver(iface, cs, tmp_path):
    """--vacuum wn prints one `Escaped` line per step, with the counts of the library through Python
    on the same deck"""
    assert os.path.exists(OWN_DRIVER), "neutral.hip not built"
    from neutral_amd import cs_table, decks, host
    run = tmp_path / "arch" / "neutral"
    (run / "problems").mkdir(parents=True)
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    size = dict(nx=64, ny=64, nparticles=20001, iterations=3, dt=2.0e-6)
    sets = []
    for k, v in size.items():
        sets += ["--set", f"{k}={v}"]
    plain = run_driver(str(run), rel, sets)
    assert "Escaped" not in plain
    said = run_driver(str(run), rel, sets + ["--vacuum", "wn"])
    lines = [ln for ln in said.splitlines() if ln.startswith("Escaped")]
    assert len(lines) == size["iterations"]
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), **size)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    py = _run(iface, prob, cs, size["iterations"], 2, vacuum="wn")
    pattern = r"^Escaped  west (\d+) \((\S+)\) east (\d+) \((\S+)\) south (\d+) \((\S+)\) north (\d+) \((\S+)\)$"
    for line, r in zip(lines, py["steps"]):
        m = re.match(pattern, line)
        assert m, line
        assert [int(m.group(1 + 2 * k)) for k in range(4)] == list(r.escape.counts())
        for k in range(4):
            assert abs(float(m.group(2 + 2 * k)) - r.escape.weights()[k]) <= 1e-8 * max(r.escape.weights()[k], 1.0)
    assert sum(py["steps"][0].escape.counts()) > 0
    assert py["steps"][0].escape.counts()[E] == 0 and py["steps"][0].escape.counts()[S] == 0

"""Periodic axes (include/neutral_hip.h: neutral_hip_set_periodic_axes): a history that would
reflect through a side of a periodic axis goes on from the opposite side in the same step, with the
same clocks and the same random stream.  The references are tests/periodic_reference.py's two, both
built on tests/replay.py's one loop: A, chained flights, the collision-free run bit for bit; B, the
unfolded lattice, for runs that collide.  They are held against each other here on the CPU, B
against its own translation, and then every kernel variant against them.

Tolerances are tests/test_vacuum.py's: a mesh TALLY_L2_TOL, a position STATE_TOL of the width, a sum
TALLY_SUM_TOL; counts, cells and `dead` exact.  What translating the lattice by one copy costs is
printed by test_translating_the_lattice_changes_nothing and sits far under them.

The library's axes are process-global and tests/gpu_support.py's table has no line for them: every
test here that sets them outside a Simulation step puts them back to 0 in a `finally`."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import periodic_reference as pr
import replay
from conftest import ROOT
from gpu_support import OWN_DRIVER, gpu, iface, l2, needs_gpu, run_driver, third_absorb, zero_capture  # noqa: F401
from ranks import launch_ranks
from test_vacuum import (ALL_FIELDS, SAME_HISTORIES_TOL, STATE_TOL, TALLY_L2_TOL, TALLY_SUM_TOL, _assert_mesh, _assert_state, _host,
                         _oracle_injected, _spectrum_of, _upload)

W, E, S, N = pr.W, pr.E, pr.S, pr.N
SIDE_NAMES = ("west", "east", "south", "north")
ROULETTE = (0.25, 0.5)
PERIODIC_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_periodic_worker.py")
BIT_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "cellx", "celly", "dead")


# ---- CPU: the ABI, the mask, the two setters ---------------------------------------------------------

def test_library_exports_the_symbols_at_the_same_abi_version():
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in ("neutral_hip_set_periodic_axes", "neutral_hip_get_periodic_axes", "neutral_hip_last_wraps"):
        assert hasattr(lib, name), name
        assert name in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert C.sizeof(iface.WrapStats) == 64
    stats = iface.last_wraps()
    assert len(stats.counts()) == 4 and len(stats.weights()) == 4


def test_periodic_mask_and_the_setters_refusal():
    """letters in any case and order, "" or None, an int; anything else is a ValueError; the library
    refuses a bit above 2 and keeps what it had (no device is touched)"""
    from neutral_amd import interface as iface
    assert iface.periodic_mask("x") == 1 and iface.periodic_mask("y") == 2
    assert iface.periodic_mask("xy") == 3 and iface.periodic_mask("YX") == 3 and iface.periodic_mask(" Xy ") == 3
    assert iface.periodic_mask(None) == 0 and iface.periodic_mask("") == 0 and iface.periodic_mask(0) == 0
    assert iface.periodic_mask(2) == 2 and iface.periodic_mask(np.int32(3)) == 3
    for bad in ("z", "w", "x,y", "all", 4, -1, 1.0, True, ["x"]):
        with pytest.raises(ValueError):
            iface.periodic_mask(bad)
    lib = iface.library()
    try:
        assert lib.neutral_hip_get_periodic_axes() == 0     # the default
        iface.set_periodic_axes("y")
        assert iface.get_periodic_axes() == 2
        for bad in (4, 7, 0xFFFFFFFF):
            assert lib.neutral_hip_set_periodic_axes(bad) == 1
            assert lib.neutral_hip_get_periodic_axes() == 2  # nothing changed
            with pytest.raises(ValueError):
                iface.set_periodic_axes(bad)
        assert lib.neutral_hip_set_periodic_axes(3) == 0 and iface.get_periodic_axes() == 3
    finally:
        iface.set_periodic_axes(0)
    assert iface.get_periodic_axes() == 0


def test_a_side_is_never_vacuum_and_periodic():
    """in both orders the later setter is refused and nothing changes; sides of the other axis are
    accepted beside a periodic one"""
    from neutral_amd import interface as iface
    lib = iface.library()
    try:
        for sides in ("w", "e", "we", "wn"):
            iface.set_vacuum_sides(sides)
            assert lib.neutral_hip_set_periodic_axes(1) == 1 and lib.neutral_hip_set_periodic_axes(3) == 1
            assert iface.get_periodic_axes() == 0 and iface.get_vacuum_sides() == iface.vacuum_mask(sides)
            with pytest.raises(ValueError):
                iface.set_periodic_axes("x")
        iface.set_vacuum_sides("w")
        iface.set_periodic_axes("y")                        # (the other axis: accepted)
        assert iface.get_periodic_axes() == 2
        iface.set_periodic_axes(0)
        iface.set_vacuum_sides(0)
        iface.set_periodic_axes("x")
        for sides in ("w", "e", "wn", "all"):
            assert lib.neutral_hip_set_vacuum_sides(iface.vacuum_mask(sides)) == 1
            with pytest.raises(ValueError):
                iface.set_vacuum_sides(sides)
            assert iface.get_vacuum_sides() == 0 and iface.get_periodic_axes() == 1
        iface.set_vacuum_sides("sn")                        # (accepted beside x)
        assert iface.get_vacuum_sides() == 12 and iface.get_periodic_axes() == 1
    finally:
        iface.set_vacuum_sides(0)
        iface.set_periodic_axes(0)
    assert iface.get_vacuum_sides() == 0 and iface.get_periodic_axes() == 0


def test_a_simulation_refuses_the_conflict_where_it_is_named():
    """before anything touches a device"""
    from neutral_amd import interface as iface
    for vacuum, periodic in (("w", "x"), ("all", "y"), (8, 3)):
        with pytest.raises(ValueError, match="wraps or leaks"):
            iface.Simulation(None, None, None, vacuum=vacuum, periodic=periodic)
    assert iface.periodic_sides(0) == 0 and iface.periodic_sides(1) == 3 and iface.periodic_sides(2) == 12
    assert iface.get_vacuum_sides() == 0 and iface.get_periodic_axes() == 0


# ---- the decks and their references, made once --------------------------------------------------------

def _stream_problem(make_problem, dt_scale=1):
    prob = make_problem("stream", nx=20, ny=13, nparticles=512, iterations=3)
    prob.dt = prob.dt * dt_scale
    return prob


def _seam_problem(make_problem, iterations=3):
    """csp 24 x 17, 600 particles, dt 1e-6; density 0.3 with the three west columns at 0.05 and the
    four south rows at 1.0: both seams join different materials"""
    prob = make_problem("csp", nx=24, ny=17, nparticles=600, iterations=iterations, dt=1.0e-6)
    pr.seam_density(prob)
    return prob


_REFERENCES = {}


def _key(prob, injected, *more):
    return (prob.nx, prob.ny, prob.dt, prob.density.tobytes(), np.asarray(prob.edgex).tobytes(),
            tuple(np.asarray(injected[f]).tobytes() for f in replay.FIELDS)) + more


def _chained(prob, cs, injected, steps, axes, vacuum=0, fused=False):
    """reference A, once per configuration, with what it must show: at least 50 wraps through every
    periodic side, no collision.  fused: every move x += d * omega rounded once (replay.Replay), as the
    library's build and the oracle's round it -- the bits of a GPU run"""
    key = _key(prob, injected, "A", steps, axes, vacuum, fused)
    if key not in _REFERENCES:
        want = pr.chained(prob, cs, injected, steps, axes, vacuum, fused=fused)
        total = [sum(s["wrapped"][k] for s in want["per_step"]) for k in range(4)]
        print(f"A: axes {axes} vacuum {vacuum} dt {prob.dt}: wrapped {total}, reflections {want['rep'].reflections}, "
              f"escaped {[sum(s['escaped'][k] for s in want['per_step']) for k in range(4)]}")
        assert want["rep"].ncollisions == 0
        for side in range(4):
            assert total[side] >= 50 if (pr.sides_of(axes) >> side) & 1 else total[side] == 0, side
        _REFERENCES[key] = want
    return _REFERENCES[key]


def _lattice(prob, cs, injected, steps, axes, k, copy=None, valid=True, **replay_kw):
    """reference B, once per configuration: k copies along every periodic axis, one along the others;
    asserts its own validity -- no history met the lattice's wall on a periodic axis -- and at least
    50 wraps through every periodic side"""
    signature = tuple(sorted((name, repr(v) if not isinstance(v, replay.Window) else (v.lower.tobytes(), v.ratio))
                             for name, v in replay_kw.items() if name != "cs_absorb"))
    capture = replay_kw["cs_absorb"][1].tobytes() if "cs_absorb" in replay_kw else None
    key = _key(prob, injected, "B", steps, axes, k, copy, capture, signature)
    if key not in _REFERENCES:
        lattice = pr.Lattice(prob, k if axes & 1 else 1, k if axes & 2 else 1)
        want = lattice.run(cs, injected, steps, copy=copy, **replay_kw)
        want["lattice"] = lattice
        rep = want["rep"]
        met = [rep.reflections[s] + rep.escaped[s] for s in range(4)]
        print(f"B: axes {axes} k {k} copy {copy}: wrapped {want['wrapped']}, reach {want['reach']}, lattice wall {met}, "
              f"{rep.ncollisions} collisions")
        if valid:
            for side in range(4):
                if (pr.sides_of(axes) >> side) & 1:
                    assert met[side] == 0, (side, met)
                    assert want["wrapped"][side] >= 50, (side, want["wrapped"])
            if axes == 3:
                assert rep.wall_hits == 0 and sum(rep.escaped) == 0
        _REFERENCES[key] = want
    return _REFERENCES[key]


# ---- CPU: the two references against each other, and B against its own translation ----------------

@pytest.mark.parametrize("dt_scale,k", [(1, 9), (4, 61)])
def test_chained_flights_against_the_unfolded_lattice(make_problem, cs, dt_scale, k):
    """A against B on the collision-free deck: two references that share only history() agree --
    cells and `dead` exactly, positions within STATE_TOL of the width, the wraps by side and step and
    every event count exactly.  With the deck's dt every history wraps once or twice a step, with
    4 dt five to eight times."""
    prob = _stream_problem(make_problem, dt_scale)
    injected = _oracle_injected(prob, cs)
    a = _chained(prob, cs, injected, 3, 3)
    b = _lattice(prob, cs, injected, 3, 3, k)
    assert b["rep"].ncollisions == 0
    for tt in range(4):
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(a["snaps"][tt][f], b["snaps"][tt][f]), (tt, f)
        for f, width in (("x", b["lattice"].width), ("y", b["lattice"].height)):
            worst = np.max(np.abs(a["snaps"][tt][f] - b["snaps"][tt][f]))
            print(f"step {tt} {f}: A - B at most {worst:.3e}")
            assert worst <= STATE_TOL * width, (tt, f)
    for sa, sb in zip(a["per_step"], b["per_step"]):
        assert sa["wrapped"] == sb["wrapped"]
        assert (sa["nprocessed"], sa["facets"], sa["census"]) == (sb["nprocessed"], sb["facets"], sb["census"])
        assert sum(sa["reflections"]) == 0 and sum(sa["escaped"]) == 0
    first = sum(a["per_step"][0]["wrapped"])
    print(f"dt x {dt_scale}: {first} wraps in step 1, {first / prob.nparticles:.2f} per history")
    assert first >= (prob.nparticles if dt_scale == 1 else 5 * prob.nparticles)


def test_translating_the_lattice_changes_nothing(make_problem, cs):
    """B started in copy c and in copy c + 1 of 9 x 9: the event counts and the collisions mesh are
    identical, the other meshes and the positions differ by rounding alone -- printed, and held to
    the tolerances the GPU runs are held to"""
    prob = _seam_problem(make_problem)
    injected = _oracle_injected(prob, cs)
    kw = dict(cs_absorb=third_absorb(cs))
    a = _lattice(prob, cs, injected, 3, 3, 9, copy=(4, 4), **kw)
    b = _lattice(prob, cs, injected, 3, 3, 9, copy=(5, 5), valid=False, **kw)
    assert b["rep"].wall_hits == 0 and sum(b["rep"].escaped) == 0
    assert a["rep"].ncollisions > 500
    assert [(s["nprocessed"], s["facets"], s["collisions"], s["census"], s["wrapped"]) for s in a["per_step"]] == \
        [(s["nprocessed"], s["facets"], s["collisions"], s["census"], s["wrapped"]) for s in b["per_step"]]
    ma, mb = a["meshes"][-1], b["meshes"][-1]
    assert np.array_equal(ma["collisions"], mb["collisions"])
    for name in ("flux", "absorbed", "jx", "jy"):
        print(f"{name}: relative L2 of the translated run {l2(mb[name], ma[name]):.3e}")
        assert l2(mb[name], ma[name]) <= TALLY_L2_TOL, name
    for side in range(4):
        print(f"outflow {SIDE_NAMES[side]}: {l2(mb['out'][side], ma['out'][side]):.3e}")
        assert l2(mb["out"][side], ma["out"][side]) <= TALLY_L2_TOL, side
    for tt in range(4):
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(a["snaps"][tt][f], b["snaps"][tt][f]), (tt, f)
        worst = max(np.max(np.abs(a["snaps"][tt][f] - b["snaps"][tt][f])) for f in ("x", "y"))
        print(f"step {tt}: positions differ by at most {worst:.3e} of the width")
        assert worst <= STATE_TOL
        for f in ("omega_x", "omega_y", "energy", "weight"):
            assert np.max(np.abs(a["snaps"][tt][f] - b["snaps"][tt][f])) <= STATE_TOL * max(1.0, np.max(np.abs(a["snaps"][tt][f]))), f


# ---- the GPU runs ----------------------------------------------------------------------------------------

def _run(iface, prob, cs, steps, variant, states=None, window=None, between=None, **kw):
    """inject (and overwrite with `states`), step; the arrays after every step, every mesh kept"""
    sim = iface.Simulation(prob, *cs, variant=variant, **kw)
    try:
        sim.inject()
        if states is not None:
            _upload(iface, sim, states)
        if window is not None:
            sim.window_in_step(**window)
        injected = sim.particle_arrays()
        results, snaps = [], [injected]
        for tt in range(1, steps + 1):
            results.append(sim.step(tt))
            assert results[-1].stats.aborted == 0
            snaps.append(sim.particle_arrays())
            if between is not None and tt < steps:
                between(tt, sim)
        jx, jy = sim.current_host() if sim.jx is not None else (None, None)
        got = dict(steps=results, injected=injected, snaps=snaps, parts=snaps[-1], tally=sim.tally_host().copy(),
                   flux=_host(sim.flux), absorbed=_host(sim.absorbed), collisions=_host(sim.collisions),
                   jx=None if jx is None else jx.copy(), jy=None if jy is None else jy.copy(),
                   out=sim.outflow_host().copy() if sim.outflow is not None else None)
        if sim.leakage is not None:
            got["leakage"] = sim.leakage_host()
        if sim.escape_bank is not None:
            got["bank"] = sim.escape_bank_host()
        return got
    finally:
        sim.close()
        assert iface.get_periodic_axes() == 0     # (the Simulation put them back)


def _everything(prob):
    return dict(scalar_flux=True, collision_tallies=True, current=True, outflow=True, spectrum=_spectrum_of(prob))


def _assert_events(got, want, collisions=True):
    """per step: histories processed, facets, collisions, census and the wraps by side -- exact"""
    for tt, (r, w) in enumerate(zip(got["steps"], want["per_step"]), 1):
        assert (r.nprocessed, r.facets, r.census) == (w["nprocessed"], w["facets"], w["census"]), tt
        if collisions:
            assert r.collisions == w["collisions"], tt
        assert list(r.wraps.counts()) == w["wrapped"], tt


def _assert_against_the_lattice(got, want, prob, steps=3):
    """case 2's comparison: events, every slot, every mesh, and the wraps' weights against the
    run's own outflow through the outer sides"""
    lattice, meshes = want["lattice"], want["meshes"][-1]
    _assert_events(got, want)
    for tt in range(1, steps + 1):
        _assert_state(got["snaps"][tt], want["snaps"][tt], width=max(lattice.width, lattice.height))
    for side in range(4):
        _assert_mesh(got["out"][side], meshes["out"][side], SIDE_NAMES[side])
    for name in ("flux", "absorbed", "jx", "jy"):
        if got.get(name) is not None:
            _assert_mesh(got[name], meshes[name], name)
    if got.get("collisions") is not None:
        assert np.array_equal(got["collisions"].ravel(), meshes["collisions"].ravel())
    n = prob.nparticles
    total = [sum(r.wraps.weights()[side] for r in got["steps"]) for side in range(4)]
    for side, entries in enumerate(pr.outer(got["out"])):
        if sum(s["wrapped"][side] for s in want["per_step"]):
            assert abs(n * entries.sum() - total[side]) <= TALLY_SUM_TOL * total[side], side
        else:
            assert total[side] == 0.0


# ---- 1. collision-free, bit for bit against A -----------------------------------------------------------

COLLISION_FREE = {"xy": dict(axes=3, vacuum=0), "x": dict(axes=1, vacuum=0), "x, north vacuum": dict(axes=1, vacuum=8)}


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("dt_scale", [1, 4])
@pytest.mark.parametrize("config", list(COLLISION_FREE))
def test_collision_free_bit_for_bit(iface, make_problem, cs, monkeypatch, variant, dt_scale, config):
    """stream 20 x 13, 512 particles of weight 1, three steps.  After every step position, direction,
    energy, weight, cells and `dead` of every slot are reference A's bits (A with every move rounded
    once, as the library's build contracts it: against A with the product rounded by itself the
    positions are 9e-16 apart after three steps, 8e-15 with 4 dt); the wraps by side are its
    counts and their weights those counts as floats; N times the outflow through an outer side is the
    number of facet events through it -- wraps, reflections, escapes -- exactly.  With x alone south
    and north reflect; with north vacuum the leakage tally and the escape bank hold the north
    escapes and nothing else."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    c = COLLISION_FREE[config]
    prob = _stream_problem(make_problem, dt_scale)
    n = prob.nparticles
    extra = dict(leakage=(None, 1), escape_bank=2 * n) if c["vacuum"] else {}
    got = _run(iface, prob, cs, 3, variant, outflow=True, periodic=c["axes"], vacuum=c["vacuum"] or None, **extra)
    want = _chained(prob, cs, got["injected"], 3, c["axes"], c["vacuum"], fused=True)
    assert np.all(got["injected"]["weight"] == 1.0)
    for tt in range(1, 4):
        for f in BIT_FIELDS:
            same = np.array_equal(got["snaps"][tt][f], want["snaps"][tt][f])
            if not same and f in ("x", "y"):
                print(f"step {tt} {f}: off by at most {np.max(np.abs(got['snaps'][tt][f] - want['snaps'][tt][f])):.3e}")
            assert same, (tt, f)
    _assert_events(got, want, collisions=False)
    through = [0, 0, 0, 0]
    for r, w in zip(got["steps"], want["per_step"]):
        assert r.collisions == 0
        assert list(r.wraps.weights()) == [float(v) for v in w["wrapped"]]
        assert list(r.escape.counts()) == w["escaped"]
        through = [t + w["wrapped"][k] + w["reflections"][k] + w["escaped"][k] for k, t in enumerate(through)]
    assert [n * entries.sum() for entries in pr.outer(got["out"])] == [float(v) for v in through]
    if config == "xy":
        assert want["rep"].reflections == [0, 0, 0, 0] and not got["parts"]["dead"].any()
    else:
        assert want["rep"].reflections[W] == want["rep"].reflections[E] == 0
    if c["vacuum"]:
        escaped = sum(w["escaped"][N] for w in want["per_step"])
        assert escaped >= 50 and sum(sum(w["escaped"]) for w in want["per_step"]) == escaped
        weight, count = got["leakage"]
        assert count[N].sum() == escaped and not count[[W, E, S]].any() and not weight[[W, E, S]].any()
        assert len(got["bank"]) == escaped and np.all(got["bank"]["side"] == N)
        assert sorted(got["bank"]["slot"].tolist()) == sorted(int(i) for i in np.flatnonzero(got["parts"]["dead"]))


# ---- 2. collisions, against B; 4. at every tile edge ---------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("arith", ["auto", "checked"])
def test_against_the_unfolded_lattice(iface, make_problem, cs, monkeypatch, variant, arith):
    """csp 24 x 17 with both seams between different materials, p_absorb 1/3, every optional tally on,
    both axes periodic: every event count, every slot and every mesh are the folded lattice's"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _seam_problem(make_problem)
    iface.set_arithmetic(iface.ARITH_CHECKED if arith == "checked" else iface.ARITH_AUTO)
    got = _run(iface, prob, cs, 3, variant, cs_absorb=third_absorb(cs), periodic="xy", **_everything(prob))
    want = _lattice(prob, cs, got["injected"], 3, 3, 9, cs_absorb=third_absorb(cs))
    assert want["rep"].ncollisions > 500
    _assert_against_the_lattice(got, want, prob)


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", [16, 32, 64])
def test_at_every_tile_edge(iface, make_problem, cs, monkeypatch, tile):
    """the same run with tiles of every edge: a wrap changes tiles whatever their size"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    monkeypatch.setenv("NEUTRAL_TILE_CELLS", str(tile))
    prob = _seam_problem(make_problem)
    got = _run(iface, prob, cs, 3, 2, cs_absorb=third_absorb(cs), periodic="xy", **_everything(prob))
    assert got["steps"][0].stats.tile_cells == tile
    want = _lattice(prob, cs, got["injected"], 3, 3, 9, cs_absorb=third_absorb(cs))
    _assert_against_the_lattice(got, want, prob)


# ---- 3. the uniform window and the jump -----------------------------------------------------------------

def _window_edge():
    """the stream kernel's window edge with the flux's code and no staged index (window_cells() in
    neutral_history.h), from the header's own constant"""
    text = open(os.path.join(ROOT, "neutral_amd", "csrc", "neutral_history.h")).read()
    return int(re.search(r"#define NEUTRAL_FLUX_WINDOW_NO_INDEX (\d+)", text).group(1))


def _westward(prob, n, seed=5):
    """n histories in the west quarter of the mesh, flying west within 60 degrees of the axis"""
    rng = np.random.default_rng(seed)
    ex, ey = np.asarray(prob.edgex, dtype=np.float64), np.asarray(prob.edgey, dtype=np.float64)
    x = ex[0] + (ex[prob.nx] - ex[0]) * rng.uniform(0.02, 0.25, n)
    y = ey[0] + (ey[prob.ny] - ey[0]) * rng.uniform(0.05, 0.95, n)
    theta = np.pi + rng.uniform(-np.pi / 3, np.pi / 3, n)
    cellx = (np.searchsorted(ex, x, side="right") - 1).astype(np.int32)
    celly = (np.searchsorted(ey, y, side="right") - 1).astype(np.int32)
    return dict(x=x, y=y, omega_x=np.cos(theta), omega_y=np.sin(theta), cellx=cellx, celly=celly)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant,queues", [(0, False), (1, False), (2, False), (2, True)])  # (queues: the tiled variant's)
@pytest.mark.parametrize("edges", ["computed", "loaded"])
def test_a_wrap_out_of_a_uniform_window(iface, make_problem, cs, monkeypatch, variant, queues, edges):
    """A mesh two windows wide along x, one density everywhere but the two east columns: a history
    that leaves west under a window of one density enters a density its window has never seen, a
    whole mesh away from it, with most of its flight ahead.  x periodic, y reflecting, against the
    lattice of five copies along x (one step's flight is under a width, and there are two steps:
    asserted from its reach)."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    nx = 2 * _window_edge()
    prob = make_problem("csp", nx=nx, ny=13, nparticles=384, iterations=2)
    prob.density[:] = 0.1
    prob.density.reshape(prob.ny, prob.nx)[:, -2:] = 5.0   # (most reach the wall, and collide behind it)
    if edges == "loaded":
        prob.edgex[5] = np.nextafter(prob.edgex[5], 1.0e9)   # (no formula gives this mesh's edges)
    prob.dt = 0.7 * pr.extent(prob)[0] / replay.speed_of(prob.initial_energy)
    iface.set_stream_queues(queues)
    states = _westward(prob, prob.nparticles)
    got = _run(iface, prob, cs, 2, variant, states=states, cs_absorb=third_absorb(cs), periodic="x",
               scalar_flux=True, collision_tallies=True, outflow=True)
    for f, a in states.items():
        assert np.array_equal(got["injected"][f], a), f
    want = _lattice(prob, cs, got["injected"], 2, 1, 5, valid=False, cs_absorb=third_absorb(cs))
    rep = want["rep"]
    assert rep.reflections[W] + rep.reflections[E] + rep.escaped[W] + rep.escaped[E] == 0
    assert want["wrapped"][W] >= 200 and want["reach"]["x"][0] in (-1, -2) and rep.ncollisions >= 50
    if variant == 2:
        # The tiled variant built windows, and histories left them with far to go: without queues
        # they migrate to a further pass, with queues they hop.  (The step stats name no kind of
        # window; that the west half's windows are of one density follows from the mesh: every cell
        # but the two east columns holds the same bits, and a window is at most `nx / 2` cells wide.)
        passes, hops = [r.stats.stream_passes for r in got["steps"]], [r.stats.stream_hops for r in got["steps"]]
        print(f"tile {got['steps'][0].stats.tile_cells}, passes {passes}, hops {hops}")
        assert got["steps"][0].stats.tile_cells <= _window_edge()
        if queues:
            assert min(hops) >= want["per_step"][0]["wrapped"][W] // 2 and max(passes) == 1
        else:
            assert min(passes) >= 2 and max(hops) == 0
    else:
        print(f"variant {variant} builds no window: the case runs for the rule alone")
    _assert_against_the_lattice(got, want, prob, steps=2)


# ---- 5. only the rule changed ---------------------------------------------------------------------------

def _same_bits(a, b):
    """all eleven arrays, the outflow's four meshes (sums of weights that are all 1: exact in any order)
    and the collisions mesh (counts) bit for bit; the flux, the current, the absorbed weight and the
    energy deposition, whose atomic adds of unequal terms round by the order they arrive in, as two
    runs of the same histories: SAME_HISTORIES_TOL (two runs with NO axis set differ by that too)"""
    for f in ALL_FIELDS:
        assert np.array_equal(a["parts"][f], b["parts"][f]), f
    assert np.array_equal(a["out"], b["out"]) and a["out"].any()
    assert np.array_equal(a["collisions"], b["collisions"]) and a["collisions"].any()   # (counts: exact)
    assert not a["absorbed"].any() and not b["absorbed"].any()   # (nothing is captured: every weight stays 1)
    for name in ("flux", "tally", "jx", "jy"):
        assert a[name].any() and l2(b[name], a[name]) <= SAME_HISTORIES_TOL, name


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_axes_that_change_no_history_change_no_bit(iface, make_problem, cs, monkeypatch, variant):
    """axes 0 set outright is never having called the setter, and y periodic in a run whose histories
    meet only the west wall is axes 0: all eleven arrays and every mesh, bit for bit"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=24, ny=17, nparticles=600, iterations=1, dt=1.0e-7)
    prob.density[:] = 0.3    # (collisions everywhere, all of them scatters: the weights stay 1)
    states = _westward(prob, prob.nparticles)
    states["y"] = np.asarray(prob.edgey)[0] + 0.25 * pr.extent(prob)[1] + 0.5 * (states["y"] - np.asarray(prob.edgey)[0])
    states["celly"] = (np.searchsorted(np.asarray(prob.edgey, dtype=np.float64), states["y"], side="right") - 1).astype(np.int32)
    kw = dict(states=states, cs_absorb=zero_capture(cs), outflow=True, scalar_flux=True, collision_tallies=True,
              current=True)
    never = _run(iface, prob, cs, 1, variant, **kw)
    rep = replay.Replay(prob, cs, zero_capture(cs))
    replay.run_steps(rep, never["injected"], 1)
    print(f"reflections {rep.reflections}, {rep.ncollisions} collisions")
    assert rep.ncollisions >= 50 and never["steps"][0].collisions == rep.ncollisions
    assert rep.reflections[W] >= 50 and rep.reflections[S] == rep.reflections[N] == rep.reflections[E] == 0
    assert never["steps"][0].facets == rep.nfacets
    try:
        iface.set_periodic_axes(0)
        zero = _run(iface, prob, cs, 1, variant, **kw)
    finally:
        iface.set_periodic_axes(0)
    unreached = _run(iface, prob, cs, 1, variant, periodic="y", **kw)
    _same_bits(never, zero)
    _same_bits(never, unreached)
    assert sum(unreached["steps"][0].wraps.counts()) == 0 and sum(zero["steps"][0].wraps.counts()) == 0


# ---- 6. write-back ---------------------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("dt_scale", [1, 4])
def test_write_back_of_histories_that_only_stream_and_wrap(iface, make_problem, cs, monkeypatch, dt_scale):
    """The tiled variant on the stream deck: a history that wrapped did nothing but stream, and its
    position and cell must reach the caller's arrays -- with the eager export, and with the lazy one
    plus neutral_hip_sync_particles after one and after three steps: all eleven arrays, bit for bit"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _stream_problem(make_problem, dt_scale)
    eager = _run(iface, prob, cs, 3, 2, outflow=True, periodic="xy")
    want = _chained(prob, cs, eager["injected"], 3, 3, fused=True)
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(eager["snaps"][1][f], want["snaps"][1][f]), f
    for steps in (1, 3):
        iface.set_lazy_export(True)
        sim = iface.Simulation(prob, *cs, variant=2, outflow=True, periodic="xy")
        try:
            sim.inject()
            for tt in range(1, steps + 1):
                sim.step(tt)
            lazy = sim.particle_arrays()     # (neutral_hip_sync_particles)
        finally:
            sim.close()
            iface.set_lazy_export(False)
        for f in ALL_FIELDS:
            assert np.array_equal(lazy[f], eager["snaps"][steps][f]), (steps, f)


# ---- 7. with roulette and the in-step window ----------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("how", ["roulette", "in-step window"])
def test_with_roulette_and_the_in_step_window(iface, make_problem, cs, monkeypatch, variant, how):
    """case 2 with Russian roulette, and under the in-step window with one bound everywhere, which is
    the roulette of the same cutoff and survival weight: the lattice with that roulette"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _seam_problem(make_problem)
    wc, ws = ROULETTE
    kw = dict(cs_absorb=third_absorb(cs), periodic="xy", scalar_flux=True, collision_tallies=True, outflow=True)
    if how == "roulette":
        got = _run(iface, prob, cs, 3, variant, roulette=ROULETTE, **kw)
    else:
        got = _run(iface, prob, cs, 3, variant, window=dict(lower=wc, survival_ratio=ws / wc), **kw)
    want = _lattice(prob, cs, got["injected"], 3, 3, 9, cs_absorb=third_absorb(cs), roulette=ROULETTE)
    assert want["rep"].killed >= 20 and want["rep"].survived >= 20
    assert [(r.stats.roulette_killed, r.stats.roulette_survived) for r in got["steps"]] == \
        [(s["killed"], s["survived"]) for s in want["per_step"]]
    _assert_against_the_lattice(got, want, prob)


def _rows(arrays, fields=("x", "y", "omega_x", "omega_y", "energy", "cellx", "celly")):
    return set(zip(*(arrays[f].tolist() for f in fields)))


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_with_source_window_and_comb_between_the_steps(iface, make_problem, cs, monkeypatch, variant):
    """Case 2 with roulette, and between its steps the operations that meet a wrapped history's
    position, cell and record first: after step 1 the census and the fixed source (every dead slot
    refilled), after step 2 the census, a census window that plays roulette and splits, and the comb.
    The lattice takes the same hooks: every step is replayed on it from the store as the operations
    left it (a slot's id is its index), with that step's key, and holds the step's events, wraps,
    slots and what the step added to every mesh.  The operations themselves are held to what they
    promise of a store they did not make: the census per cell is the lattice's folded cells, exactly;
    the source fills the dead slots and touches no live one; the window's numbers add up; after the
    comb every slot is a copy of a slot from before it, alive, at one weight."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _seam_problem(make_problem)
    n, absorb = prob.nparticles, third_absorb(cs)
    sim = iface.Simulation(prob, *cs, variant=variant, cs_absorb=absorb, roulette=ROULETTE, periodic="xy",
                           scalar_flux=True, collision_tallies=True, outflow=True)

    def meshes_now():
        return dict(out=sim.outflow_host().copy(), flux=_host(sim.flux).reshape(prob.ny, prob.nx),
                    absorbed=_host(sim.absorbed).reshape(prob.ny, prob.nx),
                    collisions=_host(sim.collisions).reshape(prob.ny, prob.nx))

    def census_is(want_arrays):
        count, weight, stats = sim.census()
        live = want_arrays["dead"] == 0
        cells = np.zeros((prob.ny, prob.nx))
        np.add.at(cells, (want_arrays["celly"][live], want_arrays["cellx"][live]), 1.0)
        held = np.zeros((prob.ny, prob.nx))
        np.add.at(held, (want_arrays["celly"][live], want_arrays["cellx"][live]), want_arrays["weight"][live])
        assert (int(stats.live), int(stats.dead)) == (int(live.sum()), int((~live).sum()))
        assert np.array_equal(count.cpu().numpy().reshape(prob.ny, prob.nx), cells)
        assert l2(weight.cpu().numpy().reshape(prob.ny, prob.nx), held) <= TALLY_L2_TOL
    try:
        sim.inject()
        before, meshes = sim.particle_arrays(), meshes_now()
        for tt in (1, 2, 3):
            r = sim.step(tt)
            assert r.stats.aborted == 0
            after, now = sim.particle_arrays(), meshes_now()
            want = _lattice(prob, cs, before, 1, 3, 9, cs_absorb=absorb, roulette=ROULETTE, keys=[tt])
            step = want["per_step"][0]
            assert (r.nprocessed, r.facets, r.collisions, r.census) == \
                (step["nprocessed"], step["facets"], step["collisions"], step["census"]), tt
            assert list(r.wraps.counts()) == step["wrapped"], tt
            assert (r.stats.roulette_killed, r.stats.roulette_survived) == (step["killed"], step["survived"]), tt
            _assert_state(after, want["snaps"][1], width=max(pr.extent(prob)))
            added = want["meshes"][1]
            for side in range(4):
                _assert_mesh(now["out"][side] - meshes["out"][side], added["out"][side], (tt, SIDE_NAMES[side]))
            for name in ("flux", "absorbed"):
                _assert_mesh(now[name] - meshes[name], added[name], (tt, name))
            assert np.array_equal(now["collisions"] - meshes["collisions"], added["collisions"]), tt
            census_is(want["snaps"][1])
            dead = int(np.sum(after["dead"] != 0))
            if tt == 1:
                assert dead >= 20
                source = sim.emit(dead)
                assert (int(source.dead_before), int(source.emitted)) == (dead, dead)
                filled = sim.particle_arrays()
                live = after["dead"] == 0
                for f in ALL_FIELDS:
                    assert np.array_equal(filled[f][live], after[f][live]), f
                assert not filled["dead"].any() and np.all(filled["weight"][~live] == 1.0)
            elif tt == 2:
                window = sim.window(0.4, upper_ratio=2.0, survival_ratio=1.5)
                windowed = sim.particle_arrays()
                assert (int(window.live_before), int(window.dead_before)) == (n - dead, dead)
                print(f"window: {window.roulette_killed} killed, {window.roulette_survived} survived, "
                      f"{window.copies_made} copies, {window.copies_refused} refused")
                assert window.roulette_killed >= 1 and window.copies_made >= 1
                assert int(np.sum(windowed["dead"] == 0)) == n - dead - window.roulette_killed + window.copies_made
                assert _rows(dict((f, a[windowed["dead"] == 0]) for f, a in windowed.items())) <= \
                    _rows(dict((f, a[after["dead"] == 0]) for f, a in after.items()))
                comb = sim.comb(seed=7)
                assert int(comb.live_before) == int(np.sum(windowed["dead"] == 0))
                filled = sim.particle_arrays()
                assert not filled["dead"].any() and np.all(filled["weight"] == comb.weight_each)
                assert _rows(filled) <= _rows(dict((f, a[windowed["dead"] == 0]) for f, a in windowed.items()))
            before, meshes = sim.particle_arrays(), now   # (the next step starts from what the operations left)
        assert r.nprocessed == n    # (the comb filled every slot)
    finally:
        sim.close()


# ---- 8. conservation -----------------------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_nothing_is_lost_on_a_torus(iface, make_problem, cs, monkeypatch, variant):
    """Both axes periodic, no capture, weight 1: after every step all N are alive with weight exactly
    1; the step's outflow entries sum to facets / N; and for every cell the weight that entered --
    its neighbours' outflow towards it, indices mod n across the seams -- is the weight that left plus
    what stayed (the histories it holds more than at the start)."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = _seam_problem(make_problem)
    n = prob.nparticles
    sim = iface.Simulation(prob, *cs, variant=variant, cs_absorb=zero_capture(cs), outflow=True, periodic="xy")
    try:
        sim.inject()
        start = sim.particle_arrays()
        before = np.zeros((4, prob.ny, prob.nx))
        wrapped, counts = 0, []
        for tt in (1, 2, 3):
            r = sim.step(tt)
            parts, out = sim.particle_arrays(), sim.outflow_host().copy()
            assert r.nprocessed == n and not parts["dead"].any() and np.all(parts["weight"] == 1.0)
            step_out = out - before
            assert abs(n * step_out.sum() - r.facets) <= TALLY_SUM_TOL * r.facets
            before = out
            wrapped += sum(r.wraps.counts())
            counts.append(list(r.wraps.counts()))
            assert list(r.wraps.weights()) == [float(c) for c in r.wraps.counts()]
        assert wrapped >= 200
        # (the reach: at least 50 wraps through every side, asserted by the lattice of the same run)
        want = _lattice(prob, cs, start, 3, 3, 9, cs_absorb=zero_capture(cs))
        assert counts == [s["wrapped"] for s in want["per_step"]]
    finally:
        sim.close()
    inflow = np.roll(out[E], 1, axis=1) + np.roll(out[W], -1, axis=1) + np.roll(out[N], 1, axis=0) + np.roll(out[S], -1, axis=0)
    held = np.zeros((prob.ny, prob.nx))
    np.add.at(held, (parts["celly"], parts["cellx"]), 1.0)
    np.add.at(held, (start["celly"], start["cellx"]), -1.0)
    assert np.max(np.abs(n * (inflow - out.sum(axis=0)) - held)) <= 1e-9 * n


# ---- 9. two ranks on one GPU ---------------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("mode,axes", [("shard", "xy"), ("domain 2x1", "x"), ("domain 1x2", "x")])
def test_two_ranks(iface, make_problem, cs, tmp_path, monkeypatch, mode, axes):
    """Two ranks on one GPU on case 2's deck, against B: particle shards; a mesh cut along x with x
    periodic, where a wrap changes ranks between blocks that are no neighbours by index; and cut
    along y, where the wrap stays at home.  Events, the states by id, the meshes summed or assembled
    over the ranks and the wraps, summed over the ranks by the library."""
    from neutral_amd import decks, host
    steps = 3
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), nx=24, ny=17, nparticles=600, iterations=steps,
                            dt=1.0e-6)
    prob = host.setup_problem(deck)   # (as the worker reads it; it rewrites the density likewise)
    pr.seam_density(prob)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    injected = _oracle_injected(prob, cs)
    mask = iface.periodic_mask(axes)
    want = _lattice(prob, cs, injected, steps, mask, 9, valid=(mask == 3), cs_absorb=third_absorb(cs))
    if mask == 1:
        rep = want["rep"]
        assert rep.reflections[W] + rep.reflections[E] + rep.escaped[W] + rep.escaped[E] == 0
        assert min(want["wrapped"][W], want["wrapped"][E]) >= 50
    sim_kw = dict(capture_scale=0.5, outflow=True, scalar_flux=True, periodic=axes)
    argv = [sys.executable, PERIODIC_WORKER, deck, str(tmp_path), str(steps), mode, json.dumps(sim_kw)]
    launch_ranks(argv, 2)
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(2)]
    ids = np.concatenate([z["ids"] for z in ranks]).astype(np.int64)
    assert np.array_equal(np.sort(ids), np.arange(prob.nparticles))
    by_id = {}
    for f in replay.FIELDS:
        a = np.concatenate([z[f] for z in ranks])
        by_id[f] = np.empty(prob.nparticles, dtype=a.dtype)
        by_id[f][ids] = a
    _assert_state(by_id, want["snaps"][-1])
    for z in ranks:
        assert [tuple(e) for e in z["events"].tolist()] == \
            [(s["nprocessed"], s["facets"], s["collisions"], s["census"]) for s in want["per_step"]]
    meshes = want["meshes"][-1]
    if mode == "shard":
        outs, fluxes = [z["out"] for z in ranks], [z["flux"] for z in ranks]
    else:
        out, flux = np.zeros((4, prob.ny, prob.nx)), np.zeros((prob.ny, prob.nx))
        for z in ranks:
            x0, y0, lnx, lny = (int(v) for v in z["block"])
            assert lnx * lny < prob.nx * prob.ny
            out[:, y0:y0 + lny, x0:x0 + lnx] += z["out"]
            flux[y0:y0 + lny, x0:x0 + lnx] += z["flux"]
        outs, fluxes = [out], [flux]
    for out, flux in zip(outs, fluxes):
        for side in range(4):
            _assert_mesh(out[side], meshes["out"][side], SIDE_NAMES[side])
        _assert_mesh(flux, meshes["flux"], "flux")
    for r in range(2):
        with open(os.path.join(str(tmp_path), f"wraps{r}.json")) as f:
            said = json.load(f)
        assert [s["wrapped"] for s in said] == [s["wrapped"] for s in want["per_step"]], r
        total = [sum(s["weight"][side] for s in said) for side in range(4)]
        for side, entries in enumerate(pr.outer(outs[0])):
            if sum(s["wrapped"][side] for s in said):
                assert abs(prob.nparticles * entries.sum() - total[side]) <= TALLY_SUM_TOL * total[side], side


# ---- 10. the driver ----------------------------------------------------------------------------------------------

@gpu
@needs_gpu
def test_driver(iface, cs, tmp_path):
    """--periodic xy on the stream deck prints one `Wrapped` line per step, with the counts of the
    library through Python on the same deck; --periodic x --vacuum w ends with the message"""
    import subprocess
    assert os.path.exists(OWN_DRIVER), "neutral.hip not built"
    from neutral_amd import cs_table, decks, host
    run = tmp_path / "arch" / "neutral"
    (run / "problems").mkdir(parents=True)
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "stream.params")
    decks.write_deck("stream", str(run / rel))
    size = dict(nx=64, ny=48, nparticles=4096, iterations=3)
    sets = []
    for k, v in size.items():
        sets += ["--set", f"{k}={v}"]
    plain = run_driver(str(run), rel, sets)
    assert "Wrapped" not in plain
    said = run_driver(str(run), rel, sets + ["--periodic", "xy"])
    lines = [ln for ln in said.splitlines() if ln.startswith("Wrapped")]
    assert len(lines) == size["iterations"]
    deck = decks.write_deck("stream", str(tmp_path / "stream.params"), **size)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    py = _run(iface, prob, cs, size["iterations"], 2, periodic="xy")
    pattern = r"^Wrapped  west (\d+) \((\S+)\) east (\d+) \((\S+)\) south (\d+) \((\S+)\) north (\d+) \((\S+)\)$"
    for line, r in zip(lines, py["steps"]):
        m = re.match(pattern, line)
        assert m, line
        assert [int(m.group(1 + 2 * k)) for k in range(4)] == list(r.wraps.counts())
        assert [float(m.group(2 + 2 * k)) for k in range(4)] == list(r.wraps.weights())
    assert min(py["steps"][0].wraps.counts()) > 0
    for order in (["--periodic", "x", "--vacuum", "w"], ["--vacuum", "e", "--periodic", "xy"]):
        out = subprocess.run([OWN_DRIVER, rel] + sets + order, cwd=str(run), capture_output=True, text=True, timeout=600)
        assert out.returncode != 0
        assert "--vacuum and --periodic name a side of the same axis" in out.stdout + out.stderr

"""Outflow tally (include/neutral_hip.h: neutral_hip_set_outflow_tally): the weight that leaves
each cell through each of its four sides, scored at every facet event.  The CPU oracle does not
score it, so the reference is the Python replay of tests/replay.py -- pinned here by
hand-computed flights and by walking the oracle's own histories -- and, on the GPU at any size,
what the definition implies without any oracle: the entries count the facet events exactly where
every weight is 1, and in every cell the weight that went missing is what flowed out minus what
flowed in."""
import math
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
import outflow_reference as orf
import replay
from gpu_support import OWN_DRIVER, allowed_tile, gpu, iface, l2, needs_gpu, run_driver, third_absorb, untimed_lines  # noqa: F401
from ranks import launch_gpu_ranks


TALLY_L2_TOL = 1e-9       # tests/test_tallies_parity.py: a weighted mesh against its reference
TALLY_SUM_TOL = 1e-10     # ... and a sum over the mesh
ROULETTE = (0.25, 0.5)
W, E, S, N = replay.WEST, replay.EAST, replay.SOUTH, replay.NORTH


# ---- 1. CPU: the ABI ------------------------------------------------------------------------

def test_library_exports_the_setter_at_the_same_abi_version():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_set_outflow_tally")
    assert "neutral_hip_set_outflow_tally" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12


def test_wrapper_argument_handling():
    """a tensor or an address; None and a null address turn it off; a tensor that is not float64
    is a TypeError (no device is touched: the address is only kept)"""
    import torch
    from neutral_amd import interface as iface
    iface.set_outflow_tally()
    iface.set_outflow_tally(None)
    iface.set_outflow_tally(0)
    iface.set_outflow_tally(0x1000)
    iface.set_outflow_tally(torch.zeros(16, dtype=torch.float64))
    with pytest.raises(TypeError):
        iface.set_outflow_tally(torch.zeros(16, dtype=torch.float32))
    with pytest.raises(TypeError):
        iface.set_outflow_tally("mesh")
    iface.set_outflow_tally(None)


# ---- 2. CPU: hand-computed flights through the replay ----------------------------------------

def _flight(make_problem, cs, x, y, ox, oy, length, nx=10):
    """one collision-free flight of `length` metres from (x, y) on an nx x nx mesh of 1 m"""
    prob = make_problem("stream", nx=nx, nparticles=4, iterations=1)
    e0 = prob.initial_energy
    rep = replay.Replay(prob, cs, dt=length / replay.speed_of(e0))
    s = dict(x=x, y=y, omega_x=ox, omega_y=oy, energy=e0, weight=1.0, dead=0,
             cellx=min(int(x * nx), nx - 1), celly=min(int(y * nx), nx - 1))
    rep.history(0, 1, s)
    assert rep.ncollisions == 0
    return rep, s


def test_replay_one_flight_inside_a_cell(make_problem, cs):
    rep, s = _flight(make_problem, cs, 0.52, 0.53, 0.6, 0.8, 0.03)
    assert rep.nfacets == 0 and not rep.out.any()
    assert (s["cellx"], s["celly"]) == (5, 5)
    assert s["x"] == pytest.approx(0.538) and s["y"] == pytest.approx(0.554)
    assert rep.flux[5, 5] == pytest.approx(0.03 / 4)


def test_replay_one_flight_crossing_two_cells(make_problem, cs):
    """+x from the middle of cell 3 for 0.2 m: out of cell 3 and of cell 4 through their east
    sides, 1/N each, nothing else"""
    rep, s = _flight(make_problem, cs, 0.35, 0.55, 1.0, 0.0, 0.2)
    assert rep.nfacets == 2 and rep.wall_hits == 0
    want = np.zeros((4, 10, 10))
    want[E, 5, 3] = want[E, 5, 4] = 0.25
    assert np.array_equal(rep.out, want)
    assert (s["cellx"], s["celly"]) == (5, 5)
    assert s["x"] == pytest.approx(0.55)


@pytest.mark.parametrize("start,omega,side,cell", [
    ((0.97, 0.55), (1.0, 0.0), E, (9, 5)),
    ((0.03, 0.55), (-1.0, 0.0), W, (0, 5)),
    ((0.55, 0.97), (0.0, 1.0), N, (5, 9)),
    ((0.55, 0.03), (0.0, -1.0), S, (5, 0)),
])
def test_replay_scores_a_bounce_on_the_wall_side_it_struck(make_problem, cs, start, omega, side, cell):
    """0.05 m towards a wall 0.03 m away: one facet event, scored on the boundary side of the
    wall cell by the direction before the reflection; the history is still in that cell, turned
    round, 0.02 m from the wall"""
    rep, s = _flight(make_problem, cs, start[0], start[1], omega[0], omega[1], 0.05)
    assert rep.nfacets == 1 and rep.wall_hits == 1
    want = np.zeros((4, 10, 10))
    want[side, cell[1], cell[0]] = 0.25
    assert np.array_equal(rep.out, want)
    assert (s["cellx"], s["celly"]) == cell
    assert (s["omega_x"], s["omega_y"]) == (-omega[0] + 0.0, -omega[1] + 0.0)
    moved = s["x"] if omega[0] else s["y"]
    assert moved == pytest.approx(0.98 if sum(omega) > 0 else 0.02)
    assert orf.wall_hits(rep.out) == 0.25 and not orf.net_outflow(rep.out).any()


# ---- 3, 4. CPU: the replay walks the oracle's histories ---------------------------------------

STEPS = 3


def _oracle_problem(make_problem):
    """the configuration of test_oracle_equals_a_naive_replay_of_single_histories"""
    return make_problem("csp", nx=24, nparticles=600, iterations=STEPS, dt=1.0e-6)


_REPLAYS = {}


def _replayed(prob, cs, injected, roulette):
    """STEPS timesteps of every history from `injected`, with the absorb table of one third;
    keeps the states before and after every step and what every step added to the meshes"""
    key = (roulette, tuple(injected[f].tobytes() for f in replay.FIELDS))
    if key not in _REPLAYS:
        rep = replay.Replay(prob, cs, third_absorb(cs), roulette)
        _REPLAYS[key] = dict(replay.run_steps(rep, injected, STEPS), rep=rep)
    return _REPLAYS[key]


def _oracle(prob, cs, roulette):
    ref = ob.OracleRun(prob, *cs, cs_absorb=third_absorb(cs), roulette=roulette if roulette[1] > 0 else None,
                       scalar_flux=True, collision_tallies=True)
    ref.inject()
    injected = {f: a.copy() for f, a in ref.particles.as_dict().items()}
    steps = [ref.step(tt) for tt in range(1, STEPS + 1)]
    return dict(injected=injected, steps=steps, parts={f: a.copy() for f, a in ref.particles.as_dict().items()},
                flux=ref.flux.copy(), absorbed=ref.absorbed.copy())


def test_replay_walks_the_oracles_histories(make_problem, cs):
    """csp 24^2, 600 histories, three steps, p_absorb = 1/3, roulette (0.25, 0.5): where every
    history ends, what it died of and every event count are the oracle's exactly; the flux and the
    absorbed weight agree to 1e-12 of their mesh's largest value (the bar of that test for this
    pair of programs).  And the run is not vacuous."""
    prob = _oracle_problem(make_problem)
    ref = _oracle(prob, cs, ROULETTE)
    r = _replayed(prob, cs, ref["injected"], ROULETTE)
    rep, end = r["rep"], r["snaps"][-1]
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(end[f], ref["parts"][f]), f
    assert rep.nfacets == sum(s.facets for s in ref["steps"])
    assert rep.ncollisions == sum(s.collisions for s in ref["steps"])
    assert rep.killed == sum(s.roulette_killed for s in ref["steps"]) > 0
    assert rep.survived == sum(s.roulette_survived for s in ref["steps"]) > 0
    for got, want, what in ((rep.flux, ref["flux"], "flux"), (rep.absorbed, ref["absorbed"], "absorbed")):
        got, want = got.ravel(), np.asarray(want).ravel()
        assert np.array_equal(got == 0.0, want == 0.0), what
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what
    print(f"replay: {rep.ncollisions} collisions, {rep.nfacets} facets, {rep.wall_hits} wall hits, "
          f"sides {[int(np.count_nonzero(rep.out[s])) for s in range(4)]}")
    assert rep.ncollisions > 500
    assert rep.wall_hits > 0 and orf.wall_hits(rep.out) > 0.0
    assert all(rep.out[s].any() for s in range(4))


def test_replay_obeys_the_balance_per_cell(make_problem, cs):
    """Identity (B) on the replay's own output, roulette off, for every step and cell.  Both sides
    are sums of at most a few thousand terms no larger than the step's weight in the cell, each
    rounded to 2^-53 of its partial sum, so they agree to 1e-11 of the mesh's L2 norm with two
    decades to spare."""
    prob = _oracle_problem(make_problem)
    ref = _oracle(prob, cs, (0.0, 0.0))
    r = _replayed(prob, cs, ref["injected"], (0.0, 0.0))
    n, nx, ny = prob.nparticles, prob.nx, prob.ny
    for tt in range(1, STEPS + 1):
        out_step = r["meshes"][tt]["out"] - r["meshes"][tt - 1]["out"]
        absorbed_step = r["meshes"][tt]["absorbed"] - r["meshes"][tt - 1]["absorbed"]
        lhs, rhs, d = orf.balance_sides(r["snaps"][tt - 1], r["snaps"][tt], absorbed_step, out_step, n, nx, ny)
        print(f"replay step {tt}: balance L2 {l2(lhs, rhs):.3e}, {np.count_nonzero(rhs)} cells")
        assert np.count_nonzero(rhs) > 20
        assert l2(lhs, rhs) <= 1e-11
    assert r["rep"].nfacets == sum(s.facets for s in ref["steps"])
    assert r["rep"].ncollisions == sum(s.collisions for s in ref["steps"]) > 0


# ---- GPU --------------------------------------------------------------------------------------

def _host(t):
    return None if t is None else t.cpu().numpy().copy()


def _run(iface, prob, cs, steps, variant, per_step=False, **kw):
    """inject and step; with per_step the particle arrays and the meshes after every step too"""
    sim = iface.Simulation(prob, *cs, variant=variant, **kw)
    try:
        sim.inject()
        injected = sim.particle_arrays()
        results, snaps, meshes = [], [injected], []

        def meshes_now():
            return dict(out=sim.outflow_host().copy() if sim.outflow is not None else None,
                        absorbed=_host(sim.absorbed))
        if per_step:
            meshes.append(meshes_now())
        for tt in range(1, steps + 1):
            results.append(sim.step(tt))
            assert results[-1].stats.aborted == 0
            if per_step:
                snaps.append(sim.particle_arrays())
                meshes.append(meshes_now())
        out = dict(steps=results, injected=injected, snaps=snaps, meshes=meshes, tally=sim.tally_host().copy(),
                   parts=sim.particle_arrays(), flux=_host(sim.flux), collisions=_host(sim.collisions),
                   absorbed=_host(sim.absorbed), jx=_host(sim.jx), jy=_host(sim.jy),
                   spectrum=_host(sim.spectrum),
                   out=sim.outflow_host().copy() if sim.outflow is not None else None)
    finally:
        sim.close()
    return out


def _spectrum_of(prob):
    return (prob.initial_energy * np.geomspace(0.5, 1.02, 9), (3, 4, prob.nx - 2, prob.ny - 1))


def _everything(prob, cs, roulette=ROULETTE):
    return dict(scalar_flux=True, collision_tallies=True, current=True, spectrum=_spectrum_of(prob),
                roulette=roulette)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("arith", ["auto", "checked"])
def test_outflow_per_cell_and_side_against_the_replay(iface, make_problem, cs, monkeypatch, variant, arith):
    """5. The problem of the CPU test above with every other option on at once: exactly zero where
    the replay scored nothing, and each of the four meshes within TALLY_L2_TOL of the replay's."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")   # small decks under windows too
    prob = _oracle_problem(make_problem)
    iface.set_arithmetic(iface.ARITH_CHECKED if arith == "checked" else iface.ARITH_AUTO)
    got = _run(iface, prob, cs, STEPS, variant, cs_absorb=third_absorb(cs), outflow=True,
               **_everything(prob, cs))
    want = _replayed(prob, cs, got["injected"], ROULETTE)
    rep = want["rep"]
    assert sum(s.facets for s in got["steps"]) == rep.nfacets
    assert sum(s.collisions for s in got["steps"]) == rep.ncollisions > 500
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got["parts"][f], want["snaps"][-1][f]), f
    for side in range(4):
        err = l2(got["out"][side], rep.out[side])
        print(f"variant {variant} {arith} side {side}: L2 {err:.3e}, {np.count_nonzero(rep.out[side])} cells")
        assert rep.out[side].any()
        assert not got["out"][side][rep.out[side] == 0.0].any(), side
        assert err <= TALLY_L2_TOL, (side, err)
    assert l2(got["flux"], rep.flux.ravel()) <= TALLY_L2_TOL
    assert l2(got["absorbed"], rep.absorbed.ravel()) <= TALLY_L2_TOL


def _exact_count(iface, prob, cs, variant, steps):
    n = prob.nparticles
    assert n & (n - 1) == 0    # 1/N and every multiple of it below 2^53 / N are exact
    got = _run(iface, prob, cs, steps, variant, outflow=True)
    assert sum(s.collisions for s in got["steps"]) == 0
    assert np.all(got["parts"]["weight"] == 1.0)
    counts = n * got["out"]
    facets = sum(s.facets for s in got["steps"])
    print(f"variant {variant}: {facets} facets, sides {[int(counts[s].sum()) for s in range(4)]}, "
          f"wall hits {n * orf.wall_hits(got['out'])}")
    assert facets > 0
    assert np.array_equal(counts, np.round(counts))
    assert int(counts.sum()) == facets and counts.sum() == float(facets)
    assert all(counts[s].any() for s in range(4))
    return got


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_outflow_counts_the_facet_events_exactly(iface, make_problem, cs, monkeypatch, variant):
    """6. (A) collision-free, every weight 1, N a power of two: N * out is integer-valued and sums
    to the steps' facet events, exactly.  Three steps of 1.4 m on a 1 m mesh: every wall is hit."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("stream", nx=100, nparticles=1 << 14, iterations=3)
    got = _exact_count(iface, prob, cs, variant, 3)
    assert orf.wall_hits(got["out"]) > 0.0


@gpu
@needs_gpu
def test_outflow_counts_the_facet_events_exactly_at_full_size(iface, make_problem, cs):
    """6. ... and once at 400^2 with 2^23 particles, the tiled pipeline as it runs in production"""
    prob = make_problem("stream", nx=400, nparticles=1 << 23, iterations=1)
    _exact_count(iface, prob, cs, 2, 1)


def _balance(iface, prob, cs, variant, steps, roulette=None):
    kw = dict(cs_absorb=third_absorb(cs), outflow=True, collision_tallies=True)
    if roulette is not None:
        kw["roulette"] = roulette
    got = _run(iface, prob, cs, steps, variant, per_step=True, **kw)
    n, nx, ny = prob.nparticles, prob.nx, prob.ny
    sides = []
    for tt in range(1, steps + 1):
        out_step = got["meshes"][tt]["out"] - got["meshes"][tt - 1]["out"]
        absorbed_step = got["meshes"][tt]["absorbed"] - got["meshes"][tt - 1]["absorbed"]
        sides.append(orf.balance_sides(got["snaps"][tt - 1], got["snaps"][tt], absorbed_step, out_step, n, nx, ny)
                     + (out_step,))
    return got, sides


BALANCE_DECKS = [dict(nx=64, nparticles=100_000, dt=2.0e-6), dict(nx=400, nparticles=1_000_000, dt=1.0e-6)]


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", BALANCE_DECKS, ids=lambda d: f"{d['nx']}")
def test_balance_per_cell(iface, make_problem, cs, deck):
    """7. (B) csp with p_absorb = 1/3, roulette off, the collision tallies on, the tiled pipeline:
    for every step and every cell, the weight before minus the weight after minus what died minus
    what was absorbed is what flowed out through the interior sides minus what flowed in."""
    steps = 3
    prob = make_problem("csp", iterations=steps, **deck)
    got, sides = _balance(iface, prob, cs, 2, steps)
    assert sum(s.collisions for s in got["steps"]) > 0
    died_somewhere = False
    nx, ny = prob.nx, prob.ny
    dense = (slice(int(0.4 * ny), int(0.6 * ny)), slice(int(0.4 * nx), int(0.6 * nx)))   # the deck's dense box
    for tt, (lhs, rhs, d, out_step) in enumerate(sides, 1):
        err = l2(lhs, rhs)
        print(f"{nx}^2 step {tt}: balance L2 {err:.3e}, {np.count_nonzero(rhs)} cells with a net flow, "
              f"D in {np.count_nonzero(d)} cells")
        assert err <= TALLY_L2_TOL, (tt, err)
        died_somewhere |= bool(d.any())
    scored = got["out"].sum(axis=0)[dense]
    assert np.count_nonzero(scored) >= scored.size / 2
    assert died_somewhere


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_balance_over_the_mesh_with_roulette(iface, make_problem, cs, variant):
    """8. The same identity summed over the mesh with roulette on: the weight roulette took and
    gave (the step statistics) stands in for the killed, whose stored weight is 0, and the
    promoted.  Every interior outflow is somebody's inflow, so the right side is 0 up to rounding;
    both sides are held to TALLY_SUM_TOL of the weight the step began with."""
    steps = 3
    prob = make_problem("csp", nx=64, nparticles=100_000, iterations=steps, dt=2.0e-6)
    got, sides = _balance(iface, prob, cs, variant, steps, roulette=ROULETTE)
    assert sum(s.stats.roulette_killed for s in got["steps"]) > 0
    assert sum(s.stats.roulette_survived for s in got["steps"]) > 0
    for tt, (lhs, rhs, d, out_step) in enumerate(sides, 1):
        st = got["steps"][tt - 1].stats
        before = got["snaps"][tt - 1]
        scale = math.fsum(before["weight"][before["dead"] == 0])
        left = math.fsum(lhs.ravel()) - st.roulette_weight_lost + st.roulette_weight_gained
        right = math.fsum(rhs.ravel())
        print(f"variant {variant} step {tt}: left {left:.6e} right {right:.6e} of {scale:.6e}")
        assert abs(left - right) <= TALLY_SUM_TOL * scale
        assert out_step.any()


def _same(a, b, what):
    if a is None and b is None:
        return
    assert np.array_equal(a, b), what


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_keeping_the_outflow_changes_nothing_else(iface, make_problem, cs, monkeypatch, variant):
    """9. With it on and off, every other option on.  Bit for bit: the particle arrays, all event
    counts, the collision counts (integer-valued sums) -- on a csp deck of 30 000 -- and every
    mesh, the energy tally and the spectrum where the order of a cell's additions is defined at
    all: single histories of the split deck (one particle of the store at a time; floating-point
    atomics of several lanes into one cell come in whatever order the hardware serves them, so
    two runs of ONE build differ in last bits there).  On the big deck those sums are held to the
    summation order, 1e-13 relative L2, the bar of tests/test_current.py for the same question."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=100, nparticles=30000, iterations=3, dt=1.0e-6)
    kw = dict(cs_absorb=third_absorb(cs), **_everything(prob, cs))
    off = _run(iface, prob, cs, 3, variant, **kw)
    on = _run(iface, prob, cs, 3, variant, outflow=True, **kw)
    alone = _run(iface, prob, cs, 3, variant, outflow=True, cs_absorb=third_absorb(cs), roulette=ROULETTE)
    assert on["out"].any() and sum(s.collisions for s in on["steps"]) > 0
    for run in (on, alone):
        for f in off["parts"]:
            assert np.array_equal(run["parts"][f], off["parts"][f]), f
        for a, b in zip(run["steps"], off["steps"]):
            assert (a.nprocessed, a.facets, a.collisions, a.census, a.stats.roulette_killed,
                    a.stats.roulette_survived) == \
                (b.nprocessed, b.facets, b.collisions, b.census, b.stats.roulette_killed, b.stats.roulette_survived)
    _same(on["collisions"], off["collisions"], "collisions")
    for name in ("tally", "flux", "absorbed", "jx", "jy", "spectrum"):
        print(f"variant {variant} {name}: bit for bit {np.array_equal(on[name], off[name])}, "
              f"L2 {l2(on[name], off[name]):.3e}")
        assert l2(on[name], off[name]) <= 1e-13, name
    # without a flux tally of the caller's (or anything else) the outflow is the same outflow
    for side in range(4):
        assert l2(alone["out"][side], on["out"][side]) <= 1e-13
    # one history at a time
    single = make_problem("split", nx=100, nparticles=8, iterations=2)
    kw1 = dict(cs_absorb=third_absorb(cs), **_everything(single, cs))
    facets = collisions = 0
    for pid in range(4):
        off1 = _run(iface, single, cs, 2, variant, shard=(pid, 1), **kw1)
        on1 = _run(iface, single, cs, 2, variant, shard=(pid, 1), outflow=True, **kw1)
        for name in ("tally", "flux", "collisions", "absorbed", "jx", "jy", "spectrum"):
            _same(on1[name], off1[name], (pid, name))
        for f in off1["parts"]:
            assert np.array_equal(on1["parts"][f], off1["parts"][f]), (pid, f)
        assert [(s.facets, s.collisions) for s in on1["steps"]] == [(s.facets, s.collisions) for s in off1["steps"]]
        crossed = sum(s.facets for s in on1["steps"])
        facets += crossed
        collisions += sum(s.collisions for s in on1["steps"])
        assert bool(on1["out"].any()) == (crossed > 0)   # (a history born in the dense half may cross nothing)
    assert facets > 0 and collisions > 0


OUTFLOW_ON = dict(scalar_flux=True, outflow=True)


@gpu
@needs_gpu
def test_variants_agree_per_cell(iface, make_problem, cs, monkeypatch):
    """10. csp that collides: the three variants' four meshes agree within TALLY_L2_TOL"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=100, nparticles=30000, iterations=3, dt=1.0e-6)
    runs = [_run(iface, prob, cs, 3, v, **OUTFLOW_ON) for v in (0, 1, 2)]
    assert sum(r.collisions for r in runs[0]["steps"]) > 0
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for side in range(4):
            print(f"variants {i}, {j} side {side}: L2 {l2(runs[i]['out'][side], runs[j]['out'][side]):.3e}")
            assert l2(runs[i]["out"][side], runs[j]["out"][side]) <= TALLY_L2_TOL
            assert np.array_equal(runs[i]["out"][side] == 0.0, runs[j]["out"][side] == 0.0)


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", [16, 32, 64, 128])
def test_outflow_at_every_tile_edge(iface, make_problem, cs, monkeypatch, tile):
    """10. tiles of every edge, histories changing windows: the plain tiled run's meshes"""
    prob = make_problem("csp", nx=400, nparticles=30000, iterations=1, dt=1.0e-6)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    base = _run(iface, prob, cs, 1, 2, **OUTFLOW_ON)
    monkeypatch.setenv("NEUTRAL_TILE_CELLS", str(tile))
    tiled = _run(iface, prob, cs, 1, 2, **OUTFLOW_ON)
    stats = tiled["steps"][0].stats
    assert stats.tile_cells == allowed_tile(tile, prob.nx, prob.ny, prob.nparticles)
    assert stats.stream_passes > 1         # histories did change windows
    assert tiled["steps"][0].facets == base["steps"][0].facets
    for side in range(4):
        assert base["out"][side].any()
        assert l2(tiled["out"][side], base["out"][side]) <= TALLY_L2_TOL
        assert np.array_equal(tiled["out"][side] == 0.0, base["out"][side] == 0.0)


@gpu
@needs_gpu
def test_nothing_is_pending_across_the_time_sliced_collision_stage(iface, make_problem, cs, monkeypatch):
    """10. Histories set aside in the middle of their collision chains, requeued and stolen, owe
    the outflow nothing: the plain tiled run's meshes."""
    prob = make_problem("csp", nx=100, nparticles=100000, iterations=2, dt=1.0e-6)
    base = _run(iface, prob, cs, 2, 2, **OUTFLOW_ON)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    sliced = _run(iface, prob, cs, 2, 2, **OUTFLOW_ON)
    print(f"sliced: requeued {sum(r.stats.requeued for r in sliced['steps'])}, "
          f"steals {sum(r.stats.steals for r in sliced['steps'])}")
    assert sum(r.stats.requeued for r in sliced["steps"]) > 0
    for side in range(4):
        assert l2(sliced["out"][side], base["out"][side]) <= TALLY_L2_TOL
    assert l2(sliced["flux"], base["flux"]) <= TALLY_L2_TOL


@gpu
@needs_gpu
def test_nothing_is_pending_across_a_steal(iface, make_problem, cs, monkeypatch):
    """10. The knobs above requeue but leave nothing to steal (steals 0 at that size).  Here
    histories are taken over by another wave of the collision stage -- the deck and the knob of
    tests/test_tiled_pipeline.py: test_histories_taken_over_by_another_wave -- and the meshes are
    the over-particle kernel's."""
    prob = make_problem("split", nx=200, nparticles=1000000, iterations=2, dt=5.0e-7)
    base = _run(iface, prob, cs, 2, 0, **OUTFLOW_ON)
    monkeypatch.setenv("NEUTRAL_STEAL_MIN", "1")
    stolen = _run(iface, prob, cs, 2, 2, **OUTFLOW_ON)
    print(f"steals {sum(r.stats.steals for r in stolen['steps'])}")
    assert sum(r.stats.steals for r in stolen["steps"]) > 100
    assert [s.facets for s in stolen["steps"]] == [s.facets for s in base["steps"]]
    for side in range(4):
        assert base["out"][side].any()
        assert l2(stolen["out"][side], base["out"][side]) <= TALLY_L2_TOL


@gpu
@needs_gpu
def test_outflow_with_the_stream_queues_on(iface, make_problem, cs, monkeypatch):
    """10. records that change hands inside a launch: the plain tiled run's meshes"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=400, nparticles=30000, iterations=2, dt=1.0e-6)
    base = _run(iface, prob, cs, 2, 2, **OUTFLOW_ON)
    iface.set_stream_queues(True)
    try:
        queued = _run(iface, prob, cs, 2, 2, **OUTFLOW_ON)
    finally:
        iface.set_stream_queues(False)
    assert [s.facets for s in queued["steps"]] == [s.facets for s in base["steps"]]
    for side in range(4):
        assert l2(queued["out"][side], base["out"][side]) <= TALLY_L2_TOL


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["shard", "domain"])
def test_two_ranks(iface, make_problem, cs, tmp_path, monkeypatch, mode):
    """11. Two ranks on one GPU over the host transport.  Sharded particles: every rank holds the
    one-rank meshes (all-reduced on the device: no host collective in a step, and the waits of a
    step are what they are with the flux alone).  Decomposed mesh: the ranks' blocks assemble to
    them, and the assembly counts every facet event once -- the stream deck, every weight 1, N a
    power of two: (A) holds exactly, an emigrant's crossing included."""
    from neutral_amd import decks, host
    steps = 3
    name = "stream" if mode == "domain" else "csp"
    deck = decks.write_deck(name, str(tmp_path / f"{name}.params"), nx=64, ny=64, nparticles=8192,
                            iterations=steps, dt=2.0e-6 if name == "csp" else None)
    prob = host.setup_problem(deck)  # (as the worker reads it)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    one = _run(iface, prob, cs, steps, 2, **OUTFLOW_ON)
    launch = "domain 2x1" if mode == "domain" else "shard"
    ranks, logs = launch_gpu_ranks(deck, tmp_path, steps, launch, 2, **OUTFLOW_ON)
    if mode == "shard":
        for z in ranks:
            for side in range(4):
                assert l2(z["out"][side], one["out"][side]) <= TALLY_L2_TOL
        _, flux_only = launch_gpu_ranks(deck, tmp_path / "flux_only", steps, launch, 2, scalar_flux=True)
        for with_outflow, without in zip(logs, flux_only):
            assert with_outflow["collectives"] == [0] * steps
            assert with_outflow["host_syncs"] == without["host_syncs"]
    else:
        assembled = np.zeros_like(one["out"])
        for z in ranks:
            x0, y0 = (int(v) for v in z["origin"])
            block = z["out"]
            assert block.shape[1] == prob.ny and block.shape[2] < prob.nx
            assembled[:, y0:y0 + block.shape[1], x0:x0 + block.shape[2]] += block
        for side in range(4):
            assert l2(assembled[side], one["out"][side]) <= TALLY_L2_TOL
        n = prob.nparticles
        facets = sum(logs[0]["facets"])
        assert facets == sum(s.facets for s in one["steps"]) > 0
        counts = n * assembled
        assert np.array_equal(counts, np.round(counts)) and counts.sum() == float(facets)
        # histories did cross between the blocks, both ways
        x_cut = max(int(z["origin"][0]) for z in ranks)
        assert x_cut > 0 and assembled[E][:, x_cut - 1].any() and assembled[W][:, x_cut].any()


@gpu
@needs_gpu
def test_driver(iface, cs, tmp_path):
    """12. --outflow prints its two lines; the sums are the library's through Python on the same
    deck; without the flag the output is what it was"""
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
    assert "Outflow" not in plain
    kept = run_driver(str(run), rel, sets + ["--outflow"])
    lines = [ln for ln in kept.splitlines() if ln.startswith("Outflow")]
    assert len(lines) == 2
    m = re.match(r"^Outflow west (\S+) east (\S+) south (\S+) north (\S+)$", lines[0])
    assert m, lines[0]
    sums = [float(v) for v in m.groups()]
    m = re.match(r"^Outflow wall hits (\S+)$", lines[1])
    assert m, lines[1]
    hits = float(m.group(1))
    others = [ln for ln in untimed_lines(kept) if not ln.startswith(("Outflow", "Allocated"))]
    assert others == [ln for ln in untimed_lines(plain) if not ln.startswith("Allocated")]
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), **size)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    py = _run(iface, prob, cs, size["iterations"], 2, outflow=True)
    scale = math.fsum(py["out"].ravel())
    assert scale > 0.0
    for side in range(4):
        assert abs(sums[side] - math.fsum(py["out"][side].ravel())) <= TALLY_SUM_TOL * scale
    assert hits > 0.0 and abs(hits - orf.wall_hits(py["out"])) <= TALLY_SUM_TOL * scale

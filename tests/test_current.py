"""Net current tally (include/neutral_hip.h: neutral_hip_set_current_tally): Jx and Jy per cell,
the scalar flux's segments times the direction they were flown with.  The CPU oracle restates it and the
HIP path is compared with that cell by cell, decks that collide included
(tests/test_tallies_parity.py); here, without any oracle, the truth comes from what the definition implies: a numpy march of collision-free flights
(tests/current_reference.py), the displacement identity (a history's segments times its
direction sum to its displacement, whatever it scatters; reflections do not move it), |J| <=
phi per cell, agreement between the kernel variants, the ranks, and the driver -- and keeping
the current changes nothing else the library computes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import current_reference as cr
from gpu_support import OWN_DRIVER, allowed_tile, gpu, iface, l2_of_nonzero, needs_gpu, run_driver, untimed_lines, zero_capture  # noqa: F401
from ranks import launch_gpu_ranks
from replay import speed_of


# ---- CPU: the ABI ---------------------------------------------------------------------------

def test_library_exports_the_setter_at_the_same_abi_version():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_set_current_tally")
    assert "neutral_hip_set_current_tally" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12


def test_setter_refuses_one_mesh_without_the_other():
    """Both or neither: one alone returns 1 and leaves the previous setting in force (no device
    is touched: the addresses are only kept)."""
    from neutral_amd import interface as iface
    lib = iface.library()
    lib.neutral_hip_set_current_tally.restype = C.c_int
    assert lib.neutral_hip_set_current_tally(C.c_void_p(0x1000), C.c_void_p(0x2000)) == 0
    assert lib.neutral_hip_set_current_tally(C.c_void_p(0x1000), None) == 1
    assert lib.neutral_hip_set_current_tally(None, C.c_void_p(0x1000)) == 1
    assert lib.neutral_hip_set_current_tally(None, None) == 0
    assert lib.neutral_hip_set_current_tally(None, C.c_void_p(0x1000)) == 1
    assert lib.neutral_hip_set_current_tally(None, None) == 0


def test_wrapper_argument_handling():
    import torch
    from neutral_amd import interface as iface
    iface.set_current_tally()
    iface.set_current_tally(None, None)
    iface.set_current_tally(0, 0)                 # null addresses are None
    with pytest.raises(ValueError):
        iface.set_current_tally(0x1000, None)
    with pytest.raises(ValueError):
        iface.set_current_tally(None, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        iface.set_current_tally(torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.float32))
    iface.set_current_tally(None, None)


# ---- CPU: the numpy march against hand-computed flights --------------------------------------

def test_march_one_flight_inside_a_cell():
    # 4 x 4 cells of 0.25; from (0.30, 0.30) along (0.6, 0.8) for 0.1: stays in cell (1, 1)
    jx, jy, s = cr.march([0.30], [0.30], [0.6], [0.8], 0.1, 4, 4)
    want_x, want_y = np.zeros((4, 4)), np.zeros((4, 4))
    want_x[1, 1], want_y[1, 1] = 0.1 * 0.6, 0.1 * 0.8
    assert np.allclose(jx, want_x, rtol=1e-15, atol=0) and np.allclose(jy, want_y, rtol=1e-15, atol=0)
    assert s["x"][0] == pytest.approx(0.36, rel=1e-15) and s["y"][0] == pytest.approx(0.38, rel=1e-15)
    assert (s["cellx"][0], s["celly"][0], s["reflections"][0]) == (1, 1, 0)


def test_march_one_flight_crossing_two_cells():
    # along +x from (0.20, 0.10) for 0.2: 0.05 in cell (0, 0), then 0.15 in cell (1, 0)
    jx, jy, s = cr.march([0.20], [0.10], [1.0], [0.0], 0.2, 4, 4)
    want = np.zeros((4, 4))
    want[0, 0], want[0, 1] = 0.05, 0.15
    assert np.allclose(jx, want, rtol=1e-13, atol=1e-17)
    assert not jy.any()
    assert s["x"][0] == pytest.approx(0.40, rel=1e-14) and (s["cellx"][0], s["celly"][0]) == (1, 0)


@pytest.mark.parametrize("start,omega,cell,axis", [
    ((0.90, 0.60), (1.0, 0.0), (3, 2), 0),    # right wall
    ((0.10, 0.60), (-1.0, 0.0), (0, 2), 0),   # left wall
    ((0.60, 0.90), (0.0, 1.0), (2, 3), 1),    # top wall
    ((0.60, 0.10), (0.0, -1.0), (2, 0), 1),   # bottom wall
])
def test_march_reflects_off_each_wall(start, omega, cell, axis):
    # 0.1 to the wall, 0.1 back: the two pieces cancel in the wall's cell, the particle is
    # where it started and flies the other way
    jx, jy, s = cr.march([start[0]], [start[1]], [omega[0]], [omega[1]], 0.2, 4, 4)
    assert abs(jx).max() < 1e-16 and abs(jy).max() < 1e-16
    assert s["reflections"][0] == 1
    assert (s["cellx"][0], s["celly"][0]) == cell
    assert s["x"][0] == pytest.approx(start[0], abs=1e-15) and s["y"][0] == pytest.approx(start[1], abs=1e-15)
    assert (s["omega_x"][0], s["omega_y"][0]) == (-omega[0], -omega[1])
    # ... and a flight that ends BEFORE it is back: 0.1 out, 0.04 back in the same cell
    jx, jy, s = cr.march([start[0]], [start[1]], [omega[0]], [omega[1]], 0.14, 4, 4)
    got = (jx, jy)[axis][cell[1], cell[0]]
    assert got == pytest.approx(0.06 * omega[axis], rel=1e-12)
    assert abs((jx, jy)[1 - axis]).max() == 0.0


def test_march_obeys_the_displacement_identity():
    """sum(segment * omega) over a flight is its displacement when nothing reflects it."""
    rng = np.random.default_rng(5)
    n = 500
    x, y = rng.uniform(0.4, 0.6, n), rng.uniform(0.4, 0.6, n)
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    jx, jy, s = cr.march(x, y, np.cos(th), np.sin(th), 0.3, 50, 40)
    assert not s["reflections"].any()
    assert jx.sum() == pytest.approx((s["x"] - x).sum(), rel=1e-12)
    assert jy.sum() == pytest.approx((s["y"] - y).sum(), rel=1e-12)


# ---- GPU ------------------------------------------------------------------------------------


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_current_per_cell_in_a_collision_free_deck(iface, make_problem, cs, monkeypatch, variant):
    """stream deck: nobody collides, weight 1, speed of the initial energy.  Every particle's
    straight flight with reflections, marched in numpy from where inject() put it, gives Jx and
    Jy per cell: relative L2 <= 1e-9 (the project's bar for a mesh against an independent
    evaluation), the same zero pattern, after three timesteps."""
    steps = 3
    prob = make_problem("stream", nx=100, nparticles=20000, iterations=steps)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")   # small decks under windows too
    sim = iface.Simulation(prob, *cs, variant=variant, current=True)
    sim.inject()
    p = sim.particle_arrays()
    state = dict(x=p["x"], y=p["y"], omega_x=p["omega_x"], omega_y=p["omega_y"], cellx=p["cellx"],
                 celly=p["celly"])
    length = speed_of(prob.initial_energy) * prob.dt
    want_x = np.zeros((prob.ny, prob.nx))
    want_y = np.zeros((prob.ny, prob.nx))
    reflections = 0
    for tt in range(1, steps + 1):
        r = sim.step(tt)
        assert r.collisions == 0 and r.census == prob.nparticles
        jx, jy, state = cr.march(state["x"], state["y"], state["omega_x"], state["omega_y"], length,
                                 prob.nx, prob.ny, prob.width, prob.height, state["cellx"], state["celly"])
        want_x += jx
        want_y += jy
        reflections += int(state["reflections"].sum())
    want_x /= prob.nparticles
    want_y /= prob.nparticles
    got_x, got_y = sim.current_host()
    print(f"variant {variant}: L2 Jx {l2_of_nonzero(got_x, want_x):.3e} Jy {l2_of_nonzero(got_y, want_y):.3e}, "
          f"{reflections} reflections, {r.stats.stream_passes} stream passes")
    assert l2_of_nonzero(got_x, want_x) <= 1e-9
    assert l2_of_nonzero(got_y, want_y) <= 1e-9
    assert np.array_equal(got_x == 0.0, want_x == 0.0)
    assert np.array_equal(got_y == 0.0, want_y == 0.0)
    assert reflections > 0   # (three steps of 1.4 m on a 1 m mesh: everybody turns round)
    # the particles end where the march ends them
    end = sim.particle_arrays()
    assert np.allclose(end["x"], state["x"], rtol=0, atol=1e-9)
    assert np.allclose(end["y"], state["y"], rtol=0, atol=1e-9)
    sim.close()


DISPLACEMENT_DECKS = [
    # deck, nx, nparticles, dt, steps
    ("csp", 100, 20000, 1.0e-6, 2),
    # scatter: a dense medium everywhere, a mean free path of 1e-10 m.  The identity's right-hand
    # side is read from float64 POSITIONS near 0.5, which every event moves with an error of up
    # to 2^-53 -- a millionth of such a segment.  Over the step the errors add up like a random
    # walk, sqrt(events) * 2^-54, against a summed path of events * 1e-10: the comparison
    # resolves 1e-10 only from 1e8 events on, hence 65 536 histories at the deck's own dt.  And
    # one step only: with no absorption to end them the histories are down to 1e-19 eV after it
    # and then cover 1e-12 m per step, where nothing is left to compare.  (_displacement_identity
    # checks both cases for this.)
    ("scatter", 64, 65536, None, 1),
]


def _displacement_identity(iface, prob, cs, variant, steps):
    """Per step: N * sum(J) against the particles' summed displacement, in float64 with fsum.
    Returns (collisions, reflected histories, worst deviation relative to N * sum(flux))."""
    sim = iface.Simulation(prob, *cs, cs_absorb=zero_capture(cs), variant=variant, scalar_flux=True,
                           current=True)
    sim.inject()
    n = prob.nparticles
    length = speed_of(prob.initial_energy) * prob.dt
    collisions = reflected = 0
    worst = 0.0
    for tt in range(1, steps + 1):
        before = sim.particle_arrays()
        sim.zero_tally()
        sim.flux.zero_()
        r = sim.step(tt)
        after = sim.particle_arrays()
        assert np.all(after["weight"] == 1.0) and not after["dead"].any()
        collisions += r.collisions
        jx, jy = sim.current_host()
        scale = n * math.fsum(sim.flux.cpu().numpy())
        dx = math.fsum(after["x"] - before["x"])
        dy = math.fsum(after["y"] - before["y"])
        dev_x = abs(n * math.fsum(jx.ravel()) - dx) / scale
        dev_y = abs(n * math.fsum(jy.ravel()) - dy) / scale
        print(f"variant {variant} step {tt}: N sum(Jx) - sum(dx) = {dev_x:.3e}, y {dev_y:.3e} of N sum(flux); "
              f"{r.collisions} collisions")
        worst = max(worst, dev_x, dev_y)
        # the positions the right-hand side is read from are float64 numbers below 1: every event
        # moves one with an error of up to 2^-53 (2^-54 in the root mean square), and the random
        # walk of those must stay inside the tolerance for the comparison to mean anything
        events = r.facets + r.collisions + r.census
        print(f"    positions resolve {math.sqrt(events) * 2.0 ** -54 / scale:.3e} of N sum(flux) "
              f"({events} events)")
        assert math.sqrt(events) * 2.0 ** -54 <= 1e-10 * scale, (events, scale)
        # a history that never scattered keeps the source's energy and flies straight: it covered
        # less ground than its path is long only if a wall folded the path
        straight = (after["energy"] == before["energy"]) & (before["energy"] == prob.initial_energy)
        moved = np.hypot(after["x"] - before["x"], after["y"] - before["y"])
        reflected += int(np.count_nonzero(straight & (moved < length * (1.0 - 1e-6))))
    sim.close()
    return collisions, reflected, worst


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_displacement_identity_with_collisions(iface, make_problem, cs, monkeypatch, variant):
    """With the capture table all zero no weight changes, and then N * sum(Jx) is the summed
    x displacement of the step (likewise y) however the histories scatter: 1e-10 of N *
    sum(flux), the flux test's bar for a global sum.  (The zeroed table makes the steps run the
    checked arithmetic by themselves.)  The scatter deck's histories, in a dense medium far
    from the walls, collide and never reflect; csp's collide in its dense square and reflect
    off the walls: both are asked of the decks together.  Measured, all three variants alike
    (the positions are the same bits): csp 0 and 7e-17, scatter 4.2e-11 (x) and 2.6e-11 (y),
    where the positions themselves resolve 6.5e-11 (DISPLACEMENT_DECKS)."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    reflected_anywhere = 0
    for deck, nx, n, dt, steps in DISPLACEMENT_DECKS:
        kw = dict(nx=nx, nparticles=n, iterations=steps)
        if dt is not None:
            kw["dt"] = dt
        prob = make_problem(deck, **kw)
        collisions, reflected, worst = _displacement_identity(iface, prob, cs, variant, steps)
        assert collisions > 0, deck
        assert worst <= 1e-10, (deck, worst)
        reflected_anywhere += reflected
    assert reflected_anywhere > 0


def _run(iface, prob, cs, steps, variant, **kw):
    sim = iface.Simulation(prob, *cs, variant=variant, **kw)
    sim.inject()
    results = [sim.step(tt) for tt in range(1, steps + 1)]
    out = dict(steps=results, tally=sim.tally_host(), parts=sim.particle_arrays(),
               flux=sim.flux.cpu().numpy() if sim.flux is not None else None,
               current=sim.current_host() if sim.jx is not None else None)
    sim.close()
    return out


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("arith", ["auto", "checked"])
def test_current_is_bounded_by_the_flux_and_disturbs_nothing(iface, make_problem, cs, monkeypatch, variant,
                                                             arith):
    """csp with the real tables (absorptions change weights).  |J| <= phi in every cell, and J =
    0 where phi = 0; with the current on the particles are bitwise those of a plain run, the
    energy tally and the flux agree with the runs without it to 1e-13 (summation order only),
    the event counts are equal -- with a flux tally of the caller's and without one."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=100, nparticles=30000, iterations=3, dt=1.0e-6)
    iface.set_arithmetic(iface.ARITH_CHECKED if arith == "checked" else iface.ARITH_AUTO)
    try:
        plain = _run(iface, prob, cs, 3, variant)
        flux_only = _run(iface, prob, cs, 3, variant, scalar_flux=True)
        both = _run(iface, prob, cs, 3, variant, scalar_flux=True, current=True)
        alone = _run(iface, prob, cs, 3, variant, current=True)
    finally:
        iface.set_arithmetic(iface.ARITH_AUTO)
    jx, jy = (m.ravel() for m in both["current"])
    phi = both["flux"]
    assert np.all(jx * jx + jy * jy <= phi * phi * (1.0 + 1e-12))
    assert not jx[phi == 0.0].any() and not jy[phi == 0.0].any()
    assert np.count_nonzero(phi) > 0 and np.count_nonzero(jx) > 0 and np.count_nonzero(jy) > 0
    for run in (both, alone):
        for f in plain["parts"]:
            assert np.array_equal(run["parts"][f], plain["parts"][f]), f
        for a, b in zip(run["steps"], plain["steps"]):
            assert (a.nprocessed, a.facets, a.collisions, a.census) == (b.nprocessed, b.facets, b.collisions, b.census)
        assert l2_of_nonzero(run["tally"], plain["tally"]) <= 1e-13
    assert l2_of_nonzero(both["flux"], flux_only["flux"]) <= 1e-13
    # without a flux tally of the caller's the current is the same current
    for a, b in zip(alone["current"], both["current"]):
        assert l2_of_nonzero(a, b) <= 1e-13


@gpu
@needs_gpu
def test_variants_agree_per_cell(iface, make_problem, cs, monkeypatch):
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=100, nparticles=30000, iterations=3, dt=1.0e-6)
    runs = [_run(iface, prob, cs, 3, v, scalar_flux=True, current=True) for v in (0, 1, 2)]
    assert sum(r.collisions for r in runs[0]["steps"]) > 0
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for a, b in zip(runs[i]["current"], runs[j]["current"]):
            print(f"variants {i}, {j}: L2 {l2_of_nonzero(a, b):.3e}")
            assert l2_of_nonzero(a, b) <= 1e-9


@gpu
@needs_gpu
def test_pending_current_survives_the_time_sliced_collision_stage(iface, make_problem, cs, monkeypatch):
    """A history set aside in the middle of its collision chain carries its pending x and y
    sums along, as it carries its pending flux."""
    prob = make_problem("csp", nx=100, nparticles=100000, iterations=2, dt=1.0e-6)
    base = _run(iface, prob, cs, 2, 0, scalar_flux=True, current=True)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    sliced = _run(iface, prob, cs, 2, 2, scalar_flux=True, current=True)
    assert sum(r.stats.requeued for r in sliced["steps"]) > 0
    for a, b in zip(sliced["current"], base["current"]):
        assert l2_of_nonzero(a, b) <= 1e-9
    assert l2_of_nonzero(sliced["flux"], base["flux"]) <= 1e-9


@gpu
@needs_gpu
def test_pending_current_is_flushed_at_a_roulette_death(iface, make_problem, cs):
    """Roulette on, with the collision tallies and the spectrum beside it: the variants agree per
    cell, and |J| <= phi still holds (a killed history's pending sums go to its cell)."""
    prob = make_problem("csp", nx=100, nparticles=30000, iterations=3, dt=1.0e-6)
    kw = dict(scalar_flux=True, current=True, roulette=(0.25, 0.5), collision_tallies=True,
              spectrum=([1.0e-2, 1.0, 1.0e2, 2.0e4], None))
    runs = [_run(iface, prob, cs, 3, v, **kw) for v in (0, 1, 2)]
    assert sum(r.stats.roulette_killed for r in runs[2]["steps"]) > 0
    for i, j in ((0, 1), (0, 2)):
        for a, b in zip(runs[i]["current"], runs[j]["current"]):
            assert l2_of_nonzero(a, b) <= 1e-9
    jx, jy = (m.ravel() for m in runs[2]["current"])
    phi = runs[2]["flux"]
    assert np.all(jx * jx + jy * jy <= phi * phi * (1.0 + 1e-12))


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", [16, 32, 64, 128])
def test_current_windows_at_every_tile_edge(iface, make_problem, cs, monkeypatch, tile):
    prob = make_problem("csp", nx=400, nparticles=30000, iterations=1, dt=1.0e-6)
    base = _run(iface, prob, cs, 1, 0, scalar_flux=True, current=True)
    monkeypatch.setenv("NEUTRAL_TILE_CELLS", str(tile))
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    tiled = _run(iface, prob, cs, 1, 2, scalar_flux=True, current=True)
    stats = tiled["steps"][0].stats
    assert stats.tile_cells == allowed_tile(tile, prob.nx, prob.ny, prob.nparticles)
    assert stats.tile_cells <= 64          # a tile never exceeds the 64-cell window
    assert stats.stream_passes > 1         # histories did change windows
    for a, b in zip(tiled["current"], base["current"]):
        assert l2_of_nonzero(a, b) <= 1e-9
    assert l2_of_nonzero(tiled["flux"], base["flux"]) <= 1e-9


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["shard", "domain"])
def test_two_ranks(iface, make_problem, cs, tmp_path, monkeypatch, mode):
    """Two ranks on one GPU over the host transport.  Sharded particles: every rank holds the
    one-rank meshes (all-reduced on the device: no host collective in a step, and the waits of a
    step are what they are with the flux alone).  Decomposed mesh: the ranks' blocks assemble
    to them."""
    from neutral_amd import decks, host
    steps = 3
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), nx=64, ny=64, nparticles=8192,
                            iterations=steps, dt=2.0e-6)
    prob = host.setup_problem(deck)  # (as the worker reads it)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    one = _run(iface, prob, cs, steps, 2, scalar_flux=True, current=True)
    launch = "domain 2x1" if mode == "domain" else "shard"
    ranks, logs = launch_gpu_ranks(deck, tmp_path, steps, launch, 2, scalar_flux=True, current=True)
    one_jx, one_jy = one["current"]
    one_flux = one["flux"].reshape(prob.ny, prob.nx)
    if mode == "shard":
        for z in ranks:
            assert l2_of_nonzero(z["jx"], one_jx) <= 1e-9 and l2_of_nonzero(z["jy"], one_jy) <= 1e-9
            assert l2_of_nonzero(z["flux"], one_flux) <= 1e-9
        _, flux_only = launch_gpu_ranks(deck, tmp_path / "flux_only", steps, launch, 2, scalar_flux=True)
        for with_current, without in zip(logs, flux_only):
            assert with_current["collectives"] == [0] * steps
            assert with_current["host_syncs"] == without["host_syncs"]
    else:
        for name, whole in (("jx", one_jx), ("jy", one_jy), ("flux", one_flux)):
            assembled = np.zeros_like(whole)
            for z in ranks:
                x0, y0 = (int(v) for v in z["origin"])
                block = z[name]
                assembled[y0:y0 + block.shape[0], x0:x0 + block.shape[1]] += block
            assert l2_of_nonzero(assembled, whole) <= 1e-9, name


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver(iface, cs, tmp_path):
    """--current prints one line; its sums agree with the Python run of the same deck; without
    the flag the output is what it was (no such line, nothing else changed by the flag but the
    memory the three meshes take)."""
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
    assert "Current" not in plain
    kept = run_driver(str(run), rel, sets + ["--current"])
    lines = [ln for ln in kept.splitlines() if ln.startswith("Current")]
    assert len(lines) == 1
    m = re.match(r"^Current sum Jx (\S+) sum Jy (\S+) max \|J\|/phi (\S+)$", lines[0])
    assert m, lines[0]
    sum_jx, sum_jy, ratio = (float(v) for v in m.groups())
    others = [ln for ln in untimed_lines(kept) if not ln.startswith(("Current", "Allocated"))]
    assert others == [ln for ln in untimed_lines(plain) if not ln.startswith("Allocated")]
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), **size)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    py = _run(iface, prob, cs, size["iterations"], 2, scalar_flux=True, current=True)
    jx, jy = py["current"]
    scale = math.fsum(py["flux"])
    assert abs(sum_jx - math.fsum(jx.ravel())) <= 1e-10 * scale
    assert abs(sum_jy - math.fsum(jy.ravel())) <= 1e-10 * scale
    phi = py["flux"].reshape(jx.shape)
    want_ratio = (np.hypot(jx, jy)[phi > 0] / phi[phi > 0]).max()
    assert ratio == pytest.approx(want_ratio, rel=1e-9)
    assert 0.0 < ratio <= 1.0 + 1e-12


@gpu
@needs_gpu
def test_displacement_identity_at_the_stream_config_full_size(iface, make_problem, cs):
    """BASELINE config 2 (stream 400^2, 1e7 particles) with the current kept: N * sum(J) is the
    particles' summed displacement (nobody collides, every weight is 1)."""
    prob = make_problem("stream", nx=400, nparticles=10_000_000, iterations=1)
    sim = iface.Simulation(prob, *cs, variant=2, scalar_flux=True, current=True)
    sim.inject()
    before = sim.particle_arrays()
    r = sim.step(1)
    assert r.collisions == 0 and r.census == 10_000_000
    after = sim.particle_arrays()
    jx, jy = sim.current_host()
    n = prob.nparticles
    scale = n * math.fsum(sim.flux.cpu().numpy())
    dev_x = abs(n * math.fsum(jx.ravel()) - math.fsum(after["x"] - before["x"])) / scale
    dev_y = abs(n * math.fsum(jy.ravel()) - math.fsum(after["y"] - before["y"])) / scale
    print(f"full size: deviation {dev_x:.3e} (x), {dev_y:.3e} (y) of N sum(flux)")
    assert dev_x <= 1e-10 and dev_y <= 1e-10
    assert scale / n == pytest.approx(speed_of(prob.initial_energy) * prob.dt, rel=1e-10)
    sim.close()

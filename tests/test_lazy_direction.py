"""The collision stage works out the direction's reciprocals, u_x_inv and u_y_inv, where a chain
of collisions may end instead of at every collision (neutral_history.h: collide(), kLazyDirection;
history_regroup_kernel).  On a real MI355X (`-m gpu`).

The shipped csp deck hardly ever takes the deferred refresh: in its dense block a collision is ten
million times closer than the cell's edge.  Here the block is thinned until a mean free path is of
the order of a cell, so that chains of collisions keep ending at facets: every such end reads
reciprocals that the deferred refresh made.  Everything is checked against the over-particle
kernel (variant 0), which refreshes in every collision: same particle bits, same event counts,
tallies equal up to summation order.

The block's density, 3.0 (the deck's 1e4 times 3e-4), was chosen with the CPU oracle and the
Python replay (tests/replay.py), at 50 000 particles, dt = 1e-6, 3 steps:

    density   collisions   facets of a history after its first collision of the step / collisions
    10.0       5 224 698   0.03
     5.0       3 183 945   0.13
     3.0       1 716 469   0.39   <- 17 times the collisions asked for, 8 times the facets
     2.0         787 614   1.01
     1.0         101 760   9.8

(the ratio from a replay of the first 400 histories).  Measured on the GPU at 3.0: 1 716 469
collisions, 646 834 facets in the collision stage.

How many particles: 50 000 where nothing else is asked.  Time slices and steals need rings that
hold more histories than a wave has lanes, and this deck queues a tenth of its particles for the
collision stage: with the full grid of 4 096 waves, 1e6 particles gave no steal and no swap, 3e6
gave 25 steals and 4e6 gave 582 steals and 390 547 swaps in the third step -- 4e6.  With roulette
at w_c = 0.25, w_s = 0.5 a history dies after a handful of absorptions (the oracle: 45 946
collisions at 50 000 particles, 225 711 at 250 000) -- 400 000, for 3.6 times the collisions asked
for."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import gpu, iface, l2_of_nonzero, needs_gpu  # noqa: F401

pytestmark = [gpu, needs_gpu]

BLOCK_DENSITY_SCALE = 3.0e-4
STEPS = 3


def _problem(make_problem, n):
    prob = make_problem("csp", nx=100, nparticles=n, iterations=STEPS, dt=1.0e-6)
    dense = prob.density > 1.0
    assert dense.any() and not dense.all()
    prob.density[dense] *= BLOCK_DENSITY_SCALE
    return prob


def _run(iface, prob, cs, variant, between=None, **sim_kw):
    sim = iface.Simulation(prob, *cs, variant=variant, **sim_kw)
    sim.inject()
    steps = []
    for tt in range(1, STEPS + 1):
        if between is not None:
            between(sim, tt)
        steps.append(sim.step(tt))
    out = dict(steps=steps, parts=sim.particle_arrays(), tally=sim.tally_host())
    if sim.flux is not None:
        out["flux"] = sim.flux.cpu().numpy()
    if sim.collisions is not None:
        out["collisions"], out["absorbed"] = sim.collisions_host(), sim.absorbed_host()
    if sim.jx is not None:
        out["current"] = sim.current_host()
    sim.close()
    return out


def _events(run):
    return [(r.nprocessed, r.facets, r.collisions, r.census) for r in run["steps"]]


def _same(want, got):
    assert _events(want) == _events(got)
    for f in want["parts"]:
        assert np.array_equal(want["parts"][f], got["parts"][f]), f
    assert np.linalg.norm(want["tally"] - got["tally"]) / np.linalg.norm(want["tally"]) < 1e-13


def _sum(run, field):
    return sum(getattr(r.stats, field) for r in run["steps"])


def _chains_kept_leaving(run):
    """the deferred refresh ran: plenty of collisions, and plenty of facets crossed by histories
    of the collision stage -- each of them behind a chain's end"""
    collisions = sum(r.collisions for r in run["steps"])
    stage_facets = sum(r.facets for r in run["steps"]) - _sum(run, "stream_facets")
    print(f"collisions {collisions}, facets in the collision stage {stage_facets}, "
          f"requeued {_sum(run, 'requeued')}, steals {_sum(run, 'steals')}")
    assert collisions >= 100000
    assert stage_facets >= 0.05 * collisions
    assert all(r.stats.aborted == 0 for r in run["steps"])
    assert all(r.stats.checked_arithmetic == 0 for r in run["steps"])


_CACHE = {}


def _reference(iface, make_problem, cs, n):
    """(problem, variant 0's run) per store size, shared by the tests below and left as it is"""
    if n not in _CACHE:
        prob = _problem(make_problem, n)
        _CACHE[n] = (prob, _run(iface, prob, cs, 0))
    return _CACHE[n]


def test_chains_that_keep_leaving(iface, make_problem, cs):
    prob, want = _reference(iface, make_problem, cs, 50000)
    got = _run(iface, prob, cs, 2)
    _chains_kept_leaving(got)
    _same(want, got)


def test_histories_set_aside_and_taken_over_mid_chain(iface, make_problem, cs, monkeypatch):
    """A history that a time slice sets aside, or that another wave takes over, in the middle of
    a chain comes back with a direction that resume() made: its record carries no reciprocals."""
    prob, want = _reference(iface, make_problem, cs, 4000000)
    monkeypatch.setenv("NEUTRAL_STEAL_MIN", "1")
    got = _run(iface, prob, cs, 2)
    _chains_kept_leaving(got)
    assert _sum(got, "steals") > 0
    assert _sum(got, "requeued") > 0
    _same(want, got)


def test_optional_scores_beside_the_deferred_refresh(iface, make_problem, cs):
    """Flux, current, collision tallies and roulette (w_c = 0.25, w_s = 0.5) on: none of them reads
    the reciprocals.  Each against variant 0 at the tolerance of its own test file (the flux and
    the current 1e-9, the collision counts exact, the absorbed weight 1e-12, roulette's counts
    exact)."""
    prob = _problem(make_problem, 400000)
    kw = dict(scalar_flux=True, current=True, collision_tallies=True, roulette=(0.25, 0.5))
    want = _run(iface, prob, cs, 0, **kw)
    got = _run(iface, prob, cs, 2, **kw)
    _chains_kept_leaving(got)
    _same(want, got)
    assert _sum(got, "roulette_killed") > 0 and _sum(got, "roulette_survived") > 0
    for f in ("roulette_killed", "roulette_survived"):
        assert [getattr(r.stats, f) for r in got["steps"]] == [getattr(r.stats, f) for r in want["steps"]], f
    assert l2_of_nonzero(got["flux"], want["flux"]) <= 1e-9
    for a, b in zip(got["current"], want["current"]):
        assert l2_of_nonzero(a, b) <= 1e-9
    assert np.array_equal(got["collisions"], want["collisions"])
    assert got["collisions"].sum() == float(sum(r.collisions for r in got["steps"]))
    assert l2_of_nonzero(got["absorbed"], want["absorbed"]) <= 1e-12


def test_zero_cosines_at_the_deferred_refresh(iface, make_problem, cs):
    """omega = (1, 0) written into 400 particles before the first step, through the array hooks.
    The source lies beside the block, not below it, so the same particles are put level with the
    block, at the middle of a row of its cells: they fly into it along x.  An absorption leaves the
    direction alone: until its first scatter such a history has u_y_inv = 1 / 0, and its wave takes
    the wrapped divisions at the deferred refresh.  The same bits as variant 0."""
    n, aimed = 50000, 400
    prob = _problem(make_problem, n)
    rows = np.where((np.asarray(prob.density).reshape(prob.ny, prob.nx) > 1.0e-20).any(axis=1))[0]
    edgey = np.asarray(prob.edgey)
    assert prob.x_off == 0 and prob.y_off == 0
    celly = rows[np.arange(aimed) % len(rows)].astype(np.int32)
    y = 0.5 * (edgey[celly + prob.pad] + edgey[celly + prob.pad + 1])
    which = np.arange(aimed) * (n // aimed)  # spread over the waves

    def aim(sim, tt):
        if tt != 1:
            return
        p = sim.particles.contents
        for field, dtype, values in (("omega_x", np.float64, 1.0), ("omega_y", np.float64, 0.0),
                                     ("y", np.float64, y), ("celly", np.int32, celly)):
            a = iface.to_host(getattr(p, field), n, dtype).copy()
            a[which] = values
            iface.library().neutral_hip_memcpy_h2d(C.c_void_p(getattr(p, field)), a.ctypes.data, a.nbytes)

    want = _run(iface, prob, cs, 0, between=aim)
    got = _run(iface, prob, cs, 2, between=aim)
    _chains_kept_leaving(got)
    _same(want, got)
    # the case tests what it says: aimed histories reached the block and collided -- a scatter
    # has turned them off the x axis by the end -- and every second one of those was absorbed, not
    # scattered, at its first collision (p_absorb = 1/2) and went on along x from there
    collided = got["parts"]["omega_y"][which] != 0.0
    print(f"aimed histories that collided: {int(collided.sum())} of {aimed}")
    assert collided.sum() >= aimed // 4


def test_checked_policy_keeps_the_eager_refresh(iface, make_problem, cs):
    """csp with its vacuum at density 0 (tests/test_arithmetic_policy.py): the steps run checked,
    where collide() refreshes as it always did -- and the bits are variant 0's."""
    prob = _problem(make_problem, 50000)
    prob.density[prob.density < 1.0e-20] = 0.0
    assert (prob.density == 0.0).any() and (prob.density > 1.0).any()
    want = _run(iface, prob, cs, 0)
    got = _run(iface, prob, cs, 2)
    assert all(r.stats.checked_arithmetic == 1 for r in got["steps"])
    assert sum(r.collisions for r in got["steps"]) >= 100000
    assert all(r.stats.aborted == 0 for r in got["steps"])
    _same(want, got)

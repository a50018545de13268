"""The CPU oracle's restatement of the optional tallies and of Russian roulette
(oracle/neutral_oracle.c: orc_set_collision_tallies, orc_set_current_tally, orc_set_spectrum_tally,
orc_set_roulette), pinned on the CPU before the HIP path is compared with it
(tests/test_tallies_parity.py).  The oracle is the reference there, so nothing here takes a kernel's
word: what the definitions of include/neutral_hip.h imply is checked on the oracle itself, the
current against the numpy marcher of tests/current_reference.py, the stream deck against its closed
forms, and everything at once against a second, deliberately naive replay of single histories in
Python (tests/replay.py) that shares with the oracle only its random numbers, its table lookup and its distance to
the facet.  At one thread and at several.  No GPU."""
import math

import numpy as np
import pytest

import current_reference as cr
import oracle_binding as ob
from closed_form import EV_TO_J, PARTICLE_MASS
from gpu_support import third_absorb as _third_absorb, zero_capture as _zero_capture
from replay import Replay, run_steps

THREADS = (1, 4)
ROULETTE = (0.25, 0.5)


@pytest.fixture()
def threads():
    before = ob.lib().orc_num_threads()

    def _set(n):
        ob.lib().orc_set_num_threads(n)
    yield _set
    ob.lib().orc_set_num_threads(before)


def _edges(e0, n=12, lo=0.5, hi=1.02):
    return e0 * np.geomspace(lo, hi, n + 1)


def _run(prob, cs, steps, **kw):
    """inject, steps 1..steps -> dict of everything the oracle computed"""
    ref = ob.OracleRun(prob, *cs, **kw)
    ref.inject()
    injected = {f: a.copy() for f, a in ref.particles.as_dict().items()}
    results = [ref.step(tt) for tt in range(1, steps + 1)]
    out = dict(ref=ref, steps=results, injected=injected,
               parts={f: a.copy() for f, a in ref.particles.as_dict().items()}, tally=ref.tally.copy(),
               flux=ref.flux, collisions=ref.collisions, absorbed=ref.absorbed, jx=ref.jx, jy=ref.jy)
    if ref.spectrum is not None:
        out["track"], out["coll"] = ref.spectrum_host()
    return out


def _csp(make_problem, n=4000, steps=2):
    return make_problem("csp", nx=48, nparticles=n, iterations=steps, dt=1.0e-6)


ALL_ON = dict(scalar_flux=True, collision_tallies=True, current=True)


# ---- what the definitions imply ---------------------------------------------------------------

@pytest.mark.parametrize("nthreads", THREADS)
@pytest.mark.parametrize("tables", ["same", "third"])
def test_counts_balance_and_bounds(make_problem, cs, threads, nthreads, tables):
    """counts sum exactly to the steps' collisions; sum(weights) + N sum(absorbed) + lost - gained
    = N; the track-length groups sum to the flux over the box; |J| <= phi in every cell"""
    threads(nthreads)
    prob = _csp(make_problem)
    n = prob.nparticles
    box = (10, 12, 30, 31)
    # (one wide group below: the histories that no roulette ends slow down to 1 eV)
    edges = np.concatenate([[0.5], _edges(prob.initial_energy)])
    absorb = _third_absorb(cs) if tables == "third" else None
    for roulette in (None, ROULETTE):
        r = _run(prob, cs, 2, cs_absorb=absorb, roulette=roulette, spectrum=(edges, box), **ALL_ON)
        total = sum(s.collisions for s in r["steps"])
        assert total > 0 and np.count_nonzero(r["collisions"]) > 1
        assert r["collisions"].sum() == total
        assert np.array_equal(r["collisions"], np.round(r["collisions"]))
        lost = math.fsum(s.roulette_weight_lost for s in r["steps"])
        gained = math.fsum(s.roulette_weight_gained for s in r["steps"])
        killed = sum(s.roulette_killed for s in r["steps"])
        survived = sum(s.roulette_survived for s in r["steps"])
        if roulette is None:
            assert (killed, survived, lost, gained) == (0, 0, 0.0, 0.0)
        else:
            assert killed > 0 and survived > 0 and lost > 0.0 and gained > 0.0
            ended = (r["parts"]["dead"] == 1) & (r["parts"]["weight"] == 0.0)
            assert np.count_nonzero(ended) == killed
        balance = math.fsum(r["parts"]["weight"]) + n * math.fsum(r["absorbed"]) + lost - gained
        assert abs(balance - n) <= 1e-11 * n, (balance, n)
        flux = r["flux"].reshape(prob.ny, prob.nx)
        want = flux[box[1]:box[3], box[0]:box[2]].sum()
        assert want > 0.0
        assert abs(r["track"].sum() - want) <= 1e-12 * want
        assert np.count_nonzero(r["track"]) >= 3 and np.count_nonzero(r["coll"]) >= 3
        # no energy above the initial one is ever flown with
        above = np.searchsorted(edges, prob.initial_energy, side="right")
        assert not r["track"][above:].any() and not r["coll"][above:].any()
        phi = r["flux"]
        assert np.all(r["jx"] ** 2 + r["jy"] ** 2 <= phi * phi * (1.0 + 1e-12))
        assert not r["jx"][phi == 0.0].any() and not r["jy"][phi == 0.0].any()
        assert not r["absorbed"][r["collisions"] == 0.0].any()


@pytest.mark.parametrize("nthreads", THREADS)
def test_absorbed_is_the_weight_the_histories_lost(make_problem, cs, threads, nthreads):
    """Without roulette a history's weight is the product of (1 - p_absorb) over its absorptions;
    with identical tables p_absorb = 1/2 exactly, every weight is 2^-k and N * sum(absorbed) is
    sum(1 - 2^-k) with no rounding at all (a constant factor on `absorbed`, as from the weight
    after the absorption, shows here)."""
    threads(nthreads)
    prob = _csp(make_problem)
    r = _run(prob, cs, 2, collision_tallies=True)
    w = r["parts"]["weight"]
    assert np.array_equal(np.exp2(np.round(np.log2(w))), w) and (w < 1.0).any()
    got = prob.nparticles * math.fsum(r["absorbed"])
    assert abs(got - math.fsum(1.0 - w)) <= 1e-12 * got


@pytest.mark.parametrize("nthreads", THREADS)
def test_stream_deck_closed_forms(make_problem, cs, threads, nthreads):
    """collision-free, one energy, weight 1: the initial energy's group holds speed * dt per step
    and nothing else is scored; the current is the numpy marcher's, cell by cell, reflections at
    all four walls included"""
    threads(nthreads)
    steps = 3
    prob = make_problem("stream", nx=40, nparticles=3000, iterations=steps)
    e0 = prob.initial_energy
    edges = np.geomspace(0.5, 2.0e6, 9)
    r = _run(prob, cs, steps, spectrum=(edges, None), **ALL_ON)
    assert sum(s.collisions for s in r["steps"]) == 0
    assert not r["collisions"].any() and not r["absorbed"].any() and not r["coll"].any()
    g0 = int(np.searchsorted(edges, e0, side="right")) - 1
    length = math.sqrt(2.0 * e0 * EV_TO_J / PARTICLE_MASS) * prob.dt
    assert abs(r["track"][g0] - length * steps) <= 1e-12 * length * steps
    assert not np.delete(r["track"], g0).any()
    assert abs(r["flux"].sum() - length * steps) <= 1e-12 * length * steps
    state = {k: r["injected"][k] for k in ("x", "y", "omega_x", "omega_y", "cellx", "celly")}
    want_x, want_y = np.zeros((prob.ny, prob.nx)), np.zeros((prob.ny, prob.nx))
    walls = set()
    for _ in range(steps):
        before = state
        jx, jy, state = cr.march(state["x"], state["y"], state["omega_x"], state["omega_y"], length,
                                 prob.nx, prob.ny, prob.width, prob.height, state["cellx"], state["celly"])
        want_x += jx
        want_y += jy
        # a wall is met where the march ends a particle flying away from it
        for axis, o in (("x", "omega_x"), ("y", "omega_y")):
            turned = np.sign(state[o]) != np.sign(before[o])
            walls |= {(axis, s) for s in np.sign(before[o][turned])}
    assert walls == {("x", 1.0), ("x", -1.0), ("y", 1.0), ("y", -1.0)}
    want_x /= prob.nparticles
    want_y /= prob.nparticles
    got_x, got_y = r["ref"].current_host()
    for got, want in ((got_x, want_x), (got_y, want_y)):
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-9
        assert np.array_equal(got == 0.0, want == 0.0)
    assert np.allclose(r["parts"]["x"], state["x"], rtol=0, atol=1e-9)
    assert np.array_equal(r["parts"]["cellx"], state["cellx"])
    assert np.array_equal(r["parts"]["celly"], state["celly"])


@pytest.mark.parametrize("nthreads", THREADS)
def test_displacement_identity(make_problem, cs, threads, nthreads):
    """capture table zero: every weight stays 1, and N * sum(J) is the summed displacement of the
    steps however the histories scatter and reflect (1e-10 of N * sum(flux), the bar of
    tests/test_current.py)"""
    threads(nthreads)
    # (two steps: csp's histories cross the vacuum in the first and collide from the second on)
    prob = _csp(make_problem, n=6000, steps=2)
    r = _run(prob, cs, 2, cs_absorb=_zero_capture(cs), scalar_flux=True, current=True)
    assert r["steps"][1].collisions > 0 and np.all(r["parts"]["weight"] == 1.0)
    n = prob.nparticles
    scale = n * math.fsum(r["flux"])
    dx = math.fsum(r["parts"]["x"] - r["injected"]["x"])
    dy = math.fsum(r["parts"]["y"] - r["injected"]["y"])
    assert abs(n * math.fsum(r["jx"]) - dx) <= 1e-10 * scale
    assert abs(n * math.fsum(r["jy"]) - dy) <= 1e-10 * scale
    straight = r["parts"]["energy"] == prob.initial_energy
    flipped = straight & ((r["parts"]["omega_x"] == -r["injected"]["omega_x"]) |
                          (r["parts"]["omega_y"] == -r["injected"]["omega_y"]))
    assert flipped.any()   # (1.4 m a step on a 1 m mesh)


@pytest.mark.parametrize("nthreads", THREADS)
def test_roulette_leaves_every_surviving_path_bit_for_bit(make_problem, cs, threads, nthreads):
    threads(nthreads)
    prob = _csp(make_problem)
    for absorb in (None, _third_absorb(cs)):
        off = _run(prob, cs, 2, cs_absorb=absorb)
        on = _run(prob, cs, 2, cs_absorb=absorb, roulette=ROULETTE)
        ended = (on["parts"]["dead"] == 1) & (on["parts"]["weight"] == 0.0)
        assert 0 < np.count_nonzero(ended) == sum(s.roulette_killed for s in on["steps"])
        kept = ~ended
        for f in on["parts"]:
            if f != "weight":
                assert np.array_equal(on["parts"][f][kept], off["parts"][f][kept]), f
        # the weights of survivors still alive (if any: in this deck most play until they lose) are
        # w_s times the (1 - p_absorb) factors since: w_s 2^-j here
        if absorb is None:
            played = kept & (on["parts"]["weight"] != off["parts"]["weight"])
            j = np.log2(ROULETTE[1] / on["parts"]["weight"][played])
            assert np.array_equal(j, np.round(j)) and (j >= 0).all()


@pytest.mark.parametrize("nthreads", THREADS)
def test_merged_groups_are_sums_of_fine_ones(make_problem, cs, threads, nthreads):
    threads(nthreads)
    prob = _csp(make_problem)
    edges = _edges(prob.initial_energy, n=12)
    box = (19, 19, 29, 29)
    fine = _run(prob, cs, 2, spectrum=(edges, box), roulette=ROULETTE)
    coarse = _run(prob, cs, 2, spectrum=(edges[::2], box), roulette=ROULETTE)
    for est in ("track", "coll"):
        f, c = fine[est], coarse[est]
        assert c.sum() > 0.0
        assert np.abs(c - (f[0::2] + f[1::2])).max() <= 1e-12 * c.max()


def test_group_edges_are_half_open(make_problem, cs, threads):
    """an edge exactly at the initial energy: as a lower edge the flights at that energy are
    scored in its group, as the last upper edge they are not scored at all"""
    threads(1)
    prob = make_problem("stream", nx=16, nparticles=200, iterations=1)
    e0 = prob.initial_energy
    length = math.sqrt(2.0 * e0 * EV_TO_J / PARTICLE_MASS) * prob.dt
    lower = _run(prob, cs, 1, spectrum=([0.5 * e0, e0, 2.0 * e0], None))
    assert lower["track"][0] == 0.0 and abs(lower["track"][1] - length) <= 1e-12 * length
    upper = _run(prob, cs, 1, spectrum=([0.25 * e0, 0.5 * e0, e0], None))
    assert not upper["track"].any() and not upper["coll"].any()


def test_box_is_global_half_open_and_may_reach_beyond_the_mesh(make_problem, cs, threads):
    threads(1)
    prob = _csp(make_problem, n=2000)
    edges = [0.5, 2.0 * prob.initial_energy]
    whole = _run(prob, cs, 2, spectrum=(edges, None), scalar_flux=True)
    beyond = _run(prob, cs, 2, spectrum=(edges, (0, 0, 10 * prob.nx, 2 ** 31 - 1)))
    assert np.array_equal(whole["track"], beyond["track"]) and np.array_equal(whole["coll"], beyond["coll"])
    flux = whole["flux"].reshape(prob.ny, prob.nx)
    parts = [(0, 0, 20, prob.ny), (20, 0, prob.nx + 7, 25), (20, 25, prob.nx, prob.ny + 1)]
    total = sum(_run(prob, cs, 2, spectrum=(edges, b))["track"][0] for b in parts)
    assert abs(total - flux.sum()) <= 1e-12 * flux.sum()
    one = _run(prob, cs, 2, spectrum=(edges, (20, 21, 21, 22)))
    assert flux[21, 20] > 0.0 and abs(one["track"][0] - flux[21, 20]) <= 1e-12 * flux[21, 20]


@pytest.mark.parametrize("option", [dict(scalar_flux=True), dict(collision_tallies=True), dict(current=True),
                                    dict(spectrum=(np.geomspace(0.5, 2.0e4, 9), (3, 4, 40, 41)))])
def test_an_option_changes_nothing_else(make_problem, cs, threads, option):
    """particles and energy tally bitwise (one thread: one summation order), alone and beside
    roulette; and the step after a run with every option finds every setting reset"""
    threads(1)
    prob = _csp(make_problem, n=2000)
    for base in (dict(), dict(roulette=ROULETTE), dict(cs_absorb=_third_absorb(cs), roulette=(0.5, 0.5))):
        plain = _run(prob, cs, 2, **base)
        with_it = _run(prob, cs, 2, **base, **option)
        for f in plain["parts"]:
            assert np.array_equal(plain["parts"][f], with_it["parts"][f]), f
        assert np.array_equal(plain["tally"], with_it["tally"])
        assert [(s.facets, s.collisions, s.census, s.roulette_killed) for s in plain["steps"]] == \
            [(s.facets, s.collisions, s.census, s.roulette_killed) for s in with_it["steps"]]
    everything = _run(prob, cs, 2, roulette=ROULETTE, spectrum=([1.0, 2.0e4], None), **ALL_ON)
    after = _run(prob, cs, 2)
    assert sum(s.roulette_killed for s in everything["steps"]) > 0
    assert sum(s.roulette_killed for s in after["steps"]) == 0
    first = _run(prob, cs, 2)
    assert np.array_equal(after["tally"], first["tally"])


# ---- the naive replay -----------------------------------------------------------------------

@pytest.mark.parametrize("nthreads", THREADS)
def test_oracle_equals_a_naive_replay_of_single_histories(make_problem, cs, threads, nthreads):
    """csp with distinct tables (p_absorb = 1/3) and roulette on, 600 histories, three steps.  Counts,
    cells, the groups that are scored and roulette's decisions: exact.  Sums: 1e-12 of the largest
    value of their mesh or estimator -- a few hundred terms of 2^-52 each with two decades of
    margin (the operations are the same; the C side may contract a multiply-add and adds in
    another order), taken against the mesh's scale because the current's terms cancel."""
    threads(nthreads)
    steps = 3
    prob = make_problem("csp", nx=24, nparticles=600, iterations=steps, dt=1.0e-6)
    absorb = _third_absorb(cs)
    edges = np.concatenate([[0.5], _edges(prob.initial_energy, n=10, lo=0.6, hi=1.0)])
    edges[-1] = prob.initial_energy * 0.999   # (the source's own energy lies above every group)
    box = (9, 9, 13, 30)
    ref = _run(prob, cs, steps, cs_absorb=absorb, roulette=ROULETTE, spectrum=(edges, box), **ALL_ON)
    rep = Replay(prob, cs, absorb, ROULETTE, edges=edges, box=box)
    states = run_steps(rep, ref["injected"], steps)["states"]
    print(rep.ncollisions, rep.nfacets, rep.killed, rep.survived, np.count_nonzero(ref["track"]),
          np.count_nonzero(ref["coll"]), np.count_nonzero(ref["collisions"]))
    assert rep.ncollisions == sum(s.collisions for s in ref["steps"]) > 500
    assert rep.nfacets == sum(s.facets for s in ref["steps"])
    assert rep.killed == sum(s.roulette_killed for s in ref["steps"]) > 0
    assert rep.survived == sum(s.roulette_survived for s in ref["steps"]) > 0
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(np.array([s[f] for s in states]), ref["parts"][f]), f
    w = np.array([s["weight"] for s in states])
    assert np.array_equal(w == 0.0, ref["parts"]["weight"] == 0.0)
    assert np.abs(w - ref["parts"]["weight"]).max() <= 1e-12
    assert np.array_equal(rep.collisions.ravel(), ref["collisions"])
    assert np.count_nonzero(ref["collisions"]) > 1

    def close(got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        assert np.array_equal(got == 0.0, want == 0.0), what
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what

    close(rep.absorbed.ravel(), ref["absorbed"], "absorbed")
    close(rep.jx.ravel(), ref["jx"], "jx")
    close(rep.jy.ravel(), ref["jy"], "jy")
    close(rep.flux.ravel(), ref["flux"], "flux")
    close(rep.track, ref["track"], "track")
    close(rep.coll, ref["coll"], "coll")
    assert np.count_nonzero(ref["track"]) >= 3 and np.count_nonzero(ref["coll"]) >= 3
    close([rep.lost, rep.gained], [math.fsum(s.roulette_weight_lost for s in ref["steps"]),
                                   math.fsum(s.roulette_weight_gained for s in ref["steps"])], "roulette")

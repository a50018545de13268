"""The in-step weight window (include/neutral_hip.h: neutral_hip_set_window_roulette): roulette
inside the steps with the cutoff taken per bin from the census window's mesh.

The CPU oracle is frozen and knows only the global cutoff.  So the chain of references is: the
oracle pins replay.Replay with a global cutoff (tests/test_oracle_tallies.py); here, on the CPU,
that pins the window's path through the loop's cutoff hook (Replay(window=...)) on a uniform mesh
and on a mesh of zeros, and the path's own additions -- the bin per cell, group and block
(tests/window_roulette_reference.py) -- are checked by what the definition implies; then the GPU
is compared with the windowed replay on non-uniform meshes, and with itself wherever the
definition names two calls that must give the same bits."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import replay
from gpu_support import OWN_DRIVER, gpu, iface, l2, needs_gpu, run_driver, third_absorb, untimed_lines  # noqa: F401
from test_roulette import DECKS, _agree, _counts, _sum, _variants_agree
from window_roulette_reference import bin_of, group_of

ON = (0.25, 0.5)          # set_roulette's pair that a uniform mesh of 0.25 with ratio 2 restates
WEIGHT_TOL = 1e-12        # tests/test_oracle_tallies.py: weights and roulette's sums against a replay
TALLY_L2_TOL = 1e-9       # tests/test_outflow.py: a weighted mesh against its reference
SUM_ORDER_TOL = 1e-13     # tests/test_roulette.py::test_off_is_off: one tally summed in another order
FAKE = 0x1000             # an address no refused call may touch: used only where there is no device


# ---- CPU: the ABI and the setter -----------------------------------------------------------

def _setter():
    from neutral_amd import interface
    f = interface.library().neutral_hip_set_window_roulette
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int]
    return f


_VALID_MESH = []


def _address():
    """The `lower` of a call that must be refused on the host.  Where there is a device: a real
    buffer of valid bounds, large enough for every mesh named here -- a refusal that regressed
    would then read mapped memory, find nothing wrong and return 0, which the test sees, instead
    of faulting a GPU that others share.  Without a device: an address that nothing may touch."""
    from conftest import gpu_available
    if not gpu_available():
        return FAKE
    if not _VALID_MESH:
        import torch
        _VALID_MESH.append(torch.full((8192,), 0.25, dtype=torch.float64, device="cuda"))
    return _VALID_MESH[0].data_ptr()


def _edges_arg(edges):
    return None if edges is None else (C.c_double * len(edges))(*edges)


def test_library_exports_the_setter():
    from neutral_amd import interface
    lib = interface.library()
    assert hasattr(lib, "neutral_hip_set_window_roulette")
    assert "neutral_hip_set_window_roulette" in interface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert callable(interface.set_window_roulette)
    assert callable(interface.Simulation.window_in_step)


nan, inf = float("nan"), float("inf")
REFUSED = [
    # nx, ny, ratio, ngroups, edges, block_x, block_y
    (0, 4, 3.0, 0, None, 1, 1), (4, 0, 3.0, 0, None, 1, 1), (-3, 4, 3.0, 0, None, 1, 1),
    (4, 4, nan, 0, None, 1, 1), (4, 4, inf, 0, None, 1, 1), (4, 4, 0.999, 0, None, 1, 1), (4, 4, -2.0, 0, None, 1, 1),
    (4, 4, 3.0, -1, None, 1, 1), (4, 4, 3.0, 65, [float(i + 1) for i in range(66)], 1, 1),
    (4, 4, 3.0, 2, None, 1, 1),
    (4, 4, 3.0, 2, [1.0, 1.0, 2.0], 1, 1), (4, 4, 3.0, 2, [1.0, 3.0, 2.0], 1, 1),
    (4, 4, 3.0, 2, [1.0, nan, 2.0], 1, 1), (4, 4, 3.0, 2, [1.0, 2.0, inf], 1, 1),
    (4, 4, 3.0, 0, None, 0, 1), (4, 4, 3.0, 0, None, 1, 0), (4, 4, 3.0, 0, None, -2, 2),
]


@pytest.mark.parametrize("nx, ny, ratio, ngroups, edges, bx, by", REFUSED)
def test_setter_refuses_on_the_host(nx, ny, ratio, ngroups, edges, bx, by):
    """Every refusal that is decided before any device call: 1, on a machine with or without a
    device (_address: what the call is given for a mesh)."""
    try:
        assert _setter()(nx, ny, _address(), ratio, ngroups, _edges_arg(edges), bx, by) == 1
    finally:
        _setter()(0, 0, None, 0.0, 0, None, 1, 1)   # (had it been accepted: off again)


def test_null_turns_it_off_without_a_device():
    from neutral_amd import interface
    assert _setter()(0, 0, None, nan, -5, None, 0, 0) == 0   # (the other arguments are ignored)
    interface.set_window_roulette(0, 0, None)
    interface.set_window_roulette(64, 64, 0)                 # (a null address, likewise)


def test_wrapper_raises_where_the_library_refuses():
    from neutral_amd import interface
    for nx, ny, ratio, ngroups, edges, bx, by in REFUSED:
        if ngroups in (-1, 65) or (ngroups > 0 and edges is None):
            continue   # (the wrapper takes the edges alone: no way to name a count without them)
        with pytest.raises(ValueError):
            interface.set_window_roulette(nx, ny, _address(), ratio, edges, (bx, by))
    with pytest.raises(ValueError):
        interface.set_window_roulette(4, 4, _address(), 3.0, [float(i + 1) for i in range(66)])
    with pytest.raises(TypeError):
        interface.set_window_roulette(4.5, 4, _address())


def test_a_global_cutoff_excludes_the_mesh():
    """With a cutoff in force the mesh is refused before any device call; (0, 0) is accepted as
    ever.  (The other direction needs a mesh set, hence a device: the GPU part.)"""
    from neutral_amd import interface
    interface.set_roulette(*ON)
    try:
        assert _setter()(4, 4, _address(), 3.0, 0, None, 1, 1) == 1
        with pytest.raises(ValueError):
            interface.set_window_roulette(4, 4, _address(), 3.0)
        assert interface._roulette == ON   # (the previous setting stays in force)
    finally:
        interface.set_roulette(0.0, 0.0)
    assert _setter()(0, 0, None, 0.0, 0, None, 1, 1) == 0


# ---- CPU: the reference, pinned ---------------------------------------------------------------

STEPS = 3


def _oracle_problem(make_problem):
    """the configuration of test_oracle_equals_a_naive_replay_of_single_histories"""
    return make_problem("csp", nx=24, nparticles=600, iterations=STEPS, dt=1.0e-6)


def _oracle_edges(prob):
    """... and its edges: one wide group, then ten below the source energy, which lies above all"""
    edges = np.concatenate([[0.5], prob.initial_energy * np.geomspace(0.6, 1.0, 11)])
    edges[-1] = prob.initial_energy * 0.999
    return edges


def _injected(prob, cs):
    ref = ob.OracleRun(prob, *cs)
    ref.inject()
    return {f: a.copy() for f, a in ref.particles.as_dict().items()}


def two_valued(nx, ny, left=0.25, right=0.5):
    """one half of the columns one bound, the other half another, one row of zeros through both"""
    m = np.empty((ny, nx))
    m[:, :nx // 2] = left
    m[:, nx // 2:] = right
    m[ny // 2, :] = 0.0
    return m


def grouped(prob, edges):
    """a bound that differs by group, the same in every cell: (G, ny, nx)"""
    g = len(edges) - 1
    per_group = 0.15 + 0.04 * np.arange(g)
    return np.repeat(per_group, prob.ny * prob.nx).reshape(g, prob.ny, prob.nx)


def _windowed(prob, cs, absorb, lower, ratio, edges=None):
    return replay.Replay(prob, cs, absorb, window=replay.Window(lower, ratio, edges))


def _events(step):
    """of what replay.run_steps says a step added: what the GPU's step result is compared with"""
    return step["collisions"], step["facets"], step["killed"], step["survived"]


_REPLAYS = {}


def _replayed(prob, cs, injected, kind):
    """the replays the tests share, made once: off, global (Replay with ON), uniform, zeros, two, groups;
    -> (rep, the final arrays, the arrays after every step, what every step added to rep's counts)"""
    key = (kind, prob.nx, prob.nparticles, tuple(injected[f].tobytes() for f in replay.FIELDS))
    if key not in _REPLAYS:
        absorb = third_absorb(cs)
        if kind == "off":
            rep = replay.Replay(prob, cs, absorb)
        elif kind == "global":
            rep = replay.Replay(prob, cs, absorb, ON)
        elif kind == "uniform":
            rep = _windowed(prob, cs, absorb, np.full(prob.nx * prob.ny, 0.25), 2.0)
        elif kind == "zeros":
            rep = _windowed(prob, cs, absorb, np.zeros(prob.nx * prob.ny), 2.0)
        elif kind == "two":
            rep = _windowed(prob, cs, absorb, two_valued(prob.nx, prob.ny), 2.0)
        else:
            edges = _oracle_edges(prob)
            rep = _windowed(prob, cs, absorb, grouped(prob, edges), 2.0, edges=edges)
        run = replay.run_steps(rep, injected, STEPS)
        _REPLAYS[key] = (rep, run["snaps"][-1], run["snaps"], run["per_step"])
    return _REPLAYS[key]


def _same_replay(a, b):
    (rep_a, end_a, snaps_a, steps_a), (rep_b, end_b, snaps_b, steps_b) = a, b
    for sa, sb in zip(snaps_a, snaps_b):
        for f in replay.FIELDS:
            assert np.array_equal(sa[f], sb[f]), f          # state for state, bit for bit
    assert steps_a == steps_b                                # every count per step: killed / survived / lost / gained
    for mesh in ("collisions", "absorbed", "flux", "jx", "jy", "out"):
        assert np.array_equal(getattr(rep_a, mesh), getattr(rep_b, mesh)), mesh   # score for score
    assert (rep_a.killed, rep_a.survived, rep_a.lost, rep_a.gained) == \
        (rep_b.killed, rep_b.survived, rep_b.lost, rep_b.gained)


def test_uniform_mesh_is_the_replay_with_a_global_cutoff(make_problem, cs):
    """c = 0.25, ratio 2 against Replay(roulette=(0.25, 0.5)), which the oracle test pins"""
    prob = _oracle_problem(make_problem)
    injected = _injected(prob, cs)
    uniform, glob = _replayed(prob, cs, injected, "uniform"), _replayed(prob, cs, injected, "global")
    _same_replay(uniform, glob)
    assert glob[0].killed > 0 and glob[0].survived > 0 and glob[0].ncollisions > 500


def test_mesh_of_zeros_is_the_replay_with_roulette_off(make_problem, cs):
    prob = _oracle_problem(make_problem)
    injected = _injected(prob, cs)
    zeros, off = _replayed(prob, cs, injected, "zeros"), _replayed(prob, cs, injected, "off")
    _same_replay(zeros, off)
    assert zeros[0].killed == zeros[0].survived == 0 and zeros[0].absorptions.sum() > 0


def test_two_valued_mesh(make_problem, cs):
    """Paths are the roulette-off paths up to a death; histories that never absorb in a windowed
    bin keep the roulette-off weights; and the mesh does exercise both halves and the strip."""
    prob = _oracle_problem(make_problem)
    injected = _injected(prob, cs)
    rep, end, snaps, _ = _replayed(prob, cs, injected, "two")
    _, off_end, off_snaps, _ = _replayed(prob, cs, injected, "off")
    nx, ny = prob.nx, prob.ny
    cells = np.arange(nx * ny).reshape(ny, nx)
    left, right, strip = cells[:, :nx // 2].ravel(), cells[:, nx // 2:].ravel(), cells[ny // 2, :]
    left, right = np.setdiff1d(left, strip), np.setdiff1d(right, strip)
    print("killed", rep.killed_in[left].sum(), rep.killed_in[right].sum(), "survived", rep.survived_in[left].sum(),
          rep.survived_in[right].sum(), "absorptions in the strip", rep.absorptions[strip].sum())
    for half in (left, right):
        assert rep.killed_in[half].sum() > 0 and rep.survived_in[half].sum() > 0
    assert rep.absorptions[strip].sum() >= 1
    assert rep.killed_in[strip].sum() == rep.survived_in[strip].sum() == 0
    alive = end["dead"] == 0
    for f in ("x", "y", "omega_x", "omega_y", "energy", "cellx", "celly"):
        assert np.array_equal(end[f][alive], off_end[f][alive]), f
    assert np.all(end["dead"][off_end["dead"] != 0] != 0)
    # every history, killed ones too: after each step it is still alive at the end of, its path
    # fields are the roulette-off replay's (the step it dies in is the first it is not compared in)
    compared_before_a_death = 0
    for snap, off_snap in zip(snaps, off_snaps):
        still = snap["dead"] == 0
        for f in ("x", "y", "omega_x", "omega_y", "energy", "cellx", "celly"):
            assert np.array_equal(snap[f][still], off_snap[f][still]), f
        assert np.all(off_snap["dead"][still] == 0)
        compared_before_a_death += int((still & (end["dead"] != 0) & (end["weight"] == 0.0)).sum())
    assert compared_before_a_death > 0   # (histories roulette ended later were compared while they lived)
    untouched = np.array([pid not in rep.played for pid in range(prob.nparticles)])
    assert untouched.any() and not untouched.all()
    assert np.array_equal(end["weight"][untouched], off_end["weight"][untouched])
    assert np.array_equal(end["dead"][untouched], off_end["dead"][untouched])


def _absorber(cs):
    """capture = 10^3 scatter: p_absorb = 1000 / 1001, so a history that makes a few collisions
    keeps the energy it starts with (the tests assert that it did)"""
    return cs[0].copy(), cs[1] * 1.0e3


@pytest.mark.parametrize("where", ["inside", "on an edge", "below", "above", "top edge"])
def test_a_history_plays_in_the_group_of_its_energy(make_problem, cs, where):
    prob = _oracle_problem(make_problem)
    edges = _oracle_edges(prob)
    g = 4
    energy, expect = {"inside": (0.5 * (edges[g] + edges[g + 1]), g), "on an edge": (edges[g], g),
                      "below": (0.25, None), "above": (prob.initial_energy, None),
                      "top edge": (edges[-1], None)}[where]
    assert group_of(energy, list(edges)) == expect
    cx = cy = prob.nx // 2
    x, y = 0.5 * (prob.edgex[cx] + prob.edgex[cx + 1]), 0.5 * (prob.edgey[cy] + prob.edgey[cy + 1])
    others = np.ones((len(edges) - 1, prob.ny, prob.nx))      # every other group: a bound of 1 ...
    others[g] = 0.0                                           # ... and none in group g
    only_g = 1.0 - others
    for lower, plays in ((only_g, expect == g), (others, expect is not None and expect != g)):
        rep = _windowed(prob, cs, _absorber(cs), lower, 2.0, edges=edges)
        # (a timestep of eight mean flights at this energy -- a flight is -log(rn) / Sigma_s mean free
        # paths of 1 / Sigma_t, omp3/neutral.c:135,295 --: a handful of collisions)
        sig_s, sig_a = rep._sigmas(float(prob.density[cy * prob.nx + cx]), rep.cs_s.lookup(float(energy))[0],
                                   rep.cs_a.lookup(float(energy))[0])
        rep.dt = 8.0 / (replay.speed_of(float(energy)) * sig_s * (sig_s + sig_a))
        s = dict(x=float(x), y=float(y), omega_x=1.0, omega_y=0.0, energy=float(energy), weight=1.0, dead=0,
                 cellx=cx, celly=cy)
        rep.history(7, 1, s)
        print(where, "collisions", rep.ncollisions, "weight", s["weight"], "killed", rep.killed, "survived", rep.survived)
        assert rep.ncollisions > 0 and s["energy"] == energy
        assert (rep.killed + rep.survived > 0) == plays, (where, rep.killed, rep.survived)
        if plays and expect == g:
            in_g = slice(g * prob.nx * prob.ny, (g + 1) * prob.nx * prob.ny)
            assert (rep.killed_in[in_g] + rep.survived_in[in_g]).sum() == rep.killed + rep.survived
        if not plays:
            # (below every group is below 1 eV too: that history dies for its energy, and plays none)
            assert s["dead"] == (1 if energy < replay.MIN_ENERGY_OF_INTEREST else 0) and 0.0 < s["weight"] < 1.0


def test_grouped_mesh_plays_by_group(make_problem, cs):
    prob = _oracle_problem(make_problem)
    injected = _injected(prob, cs)
    rep, end, _, _ = _replayed(prob, cs, injected, "groups")
    ncells = prob.nx * prob.ny
    played = (rep.killed_in + rep.survived_in).reshape(-1, ncells).sum(axis=1)
    print("plays by group", played.tolist())
    assert rep.killed > 0 and rep.survived > 0 and np.count_nonzero(played) >= 2


@pytest.mark.parametrize("block", [(3, 2), (8, 8)])
def test_bin_of_with_blocks(block):
    nx, ny = 7, 5
    bx, by = block
    cnx, cny = -(-nx // bx), -(-ny // by)
    edges = [1.0, 2.0, 4.0]
    seen = set()
    for cy in range(ny):
        for cx in range(nx):
            assert bin_of(cx, cy, 0.0, nx, ny, None, block) == (cy // by) * cnx + cx // bx
            assert bin_of(cx, cy, 3.0, nx, ny, edges, block) == cnx * cny + (cy // by) * cnx + cx // bx
            assert bin_of(cx, cy, 2.0, nx, ny, edges, block) == cnx * cny + (cy // by) * cnx + cx // bx
            assert bin_of(cx, cy, 4.0, nx, ny, edges, block) is None
            assert bin_of(cx, cy, nan, nx, ny, edges, block) is None
            seen.add(bin_of(cx, cy, 0.0, nx, ny, None, block))
    assert seen == set(range(cnx * cny))
    assert bin_of(nx, 0, 0.0, nx, ny, None, block) is None and bin_of(0, -1, 0.0, nx, ny, None, block) is None
    if block == (8, 8):
        assert seen == {0}


# ---- GPU ----------------------------------------------------------------------------------------

def _host(t):
    return None if t is None else t.cpu().numpy().copy()


def _run(iface, prob, cs, its, variant=2, window=None, roulette=None, keys=None, per_step=False, after_step=None,
         **kw):
    """inject and step; window = dict(lower=, survival_ratio=, groups=, block=) puts the in-step
    window in force first; after_step(sim, tt) runs between the steps"""
    sim = iface.Simulation(prob, *cs, variant=variant, roulette=roulette, **kw)
    try:
        sim.inject()
        if window is not None:
            sim.window_in_step(**window)
        injected = sim.particle_arrays()
        steps, snaps = [], [injected]
        for n, k in enumerate(keys or range(1, its + 1)):
            steps.append(sim.step(k))
            assert steps[-1].stats.aborted == 0
            if per_step:
                snaps.append(sim.particle_arrays())
            if after_step is not None and n + 1 < its:
                after_step(sim, k)
                if per_step:
                    snaps.append(sim.particle_arrays())
        out = {"steps": steps, "injected": injected, "snaps": snaps, "parts": sim.particle_arrays(),
               "tally": sim.tally_host().copy()}
        for name in ("flux", "collisions", "absorbed", "jx", "jy", "spectrum"):
            if getattr(sim, name, None) is not None:
                out[name] = _host(getattr(sim, name))
        if sim.outflow is not None:
            out["out"] = sim.outflow_host().copy()
    finally:
        sim.close()
    return out


def _deck(make_problem, deck):
    nx, n, its, dt = DECKS[deck]
    kw = dict(nx=nx, nparticles=n, iterations=its)
    if dt is not None:
        kw["dt"] = dt
    return make_problem(deck, **kw), its


def _weights(run):
    return [(r.stats.roulette_weight_lost, r.stats.roulette_weight_gained) for r in run["steps"]]


def _same_weights(a, b, what=""):
    """The weight roulette lost and gained per step.  Each is a sum of f64 terms through a wave
    shuffle sum and one unordered f64 atomic per wave, and in the tiled variant which lane holds
    which history follows the queue's order; the sum keeps its bits from run to run only while
    every term is a small dyadic number (a uniform mesh of 0.25).  Under a mesh with bins of
    bound 0 a weight falls through dozens of halvings before it meets a bound, and terms like
    2^-46 land under the ulp of a running sum of several hundred: held to their bits, the blocks
    comparison failed in one run on an MI355X and passed in the next.  They are held to the margin that
    tests/test_roulette.py::test_two_ranks sets for these two numbers, 1e-12 * max(value, 1)."""
    for (la, ga), (lb, gb) in zip(_weights(a), _weights(b)):
        assert abs(la - lb) <= WEIGHT_TOL * max(lb, 1.0), (what, la, lb)
        assert abs(ga - gb) <= WEIGHT_TOL * max(gb, 1.0), (what, ga, gb)
    assert len(_weights(a)) == len(_weights(b)), what


def _bitwise(a, b, what=""):
    """Every particle array and the per-step integer counters (roulette's killed and survived
    among them), bit for bit; roulette's two weight sums as _same_weights says.
    The tally meshes are sums of unordered f64 atomics: two runs of one and the same configuration
    differ in their last bits on this hardware (measured here, roulette off, fresh Simulations: the
    energy tally of csp 64^2 differs in 1e-16 relative L2 between identical runs, in all three
    variants), so no two runs can be held to the tally's bits.  They are held to the bound that
    tests/test_roulette.py::test_off_is_off sets for the same comparison, 1e-13 of the mesh's norm
    -- the histories, their deposits and their count are the same, only the order of the adds is
    not -- and the collision counts, whose sums are exact, to their bits."""
    assert _counts(a) == _counts(b), what
    _same_weights(a, b, what)
    for f in a["parts"]:
        assert np.array_equal(a["parts"][f], b["parts"][f]), (what, f)
    for t in ("tally", "flux", "collisions", "absorbed", "jx", "jy", "out", "spectrum"):
        assert (t in a) == (t in b)
        if t == "collisions" and t in a:
            assert np.array_equal(a[t], b[t]), (what, t)
        elif t in a:
            norm = np.linalg.norm(b[t])
            print(what, t, "relative L2 between the two runs", np.linalg.norm(a[t] - b[t]) / max(norm, 1e-300))
            assert np.array_equal(a[t] == 0.0, b[t] == 0.0), (what, t)
            assert np.linalg.norm(a[t] - b[t]) <= SUM_ORDER_TOL * norm, (what, t)


def _uniform(prob, value=0.25, ratio=2.0):
    return dict(lower=np.full((prob.ny, prob.nx), value), survival_ratio=ratio)


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
@pytest.mark.parametrize("arith", ["auto", "checked"])
def test_uniform_mesh_equals_set_roulette(iface, make_problem, cs, deck, arith):
    """A uniform mesh of c with ratio r gives the bits of set_roulette(c, fl(r * c))."""
    prob, its = _deck(make_problem, deck)
    if arith == "checked":
        iface.set_arithmetic(iface.ARITH_CHECKED)
    for variant in (0, 1, 2):
        cutoff = _run(iface, prob, cs, its, variant, roulette=ON)
        mesh = _run(iface, prob, cs, its, variant, window=_uniform(prob))
        assert _sum(mesh, "roulette_killed") > 0
        _bitwise(mesh, cutoff, (deck, arith, variant))


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_mesh_of_zeros_equals_nothing_set(iface, make_problem, cs, variant):
    prob, its = _deck(make_problem, "csp")
    never = _run(iface, prob, cs, its, variant)
    zeros = _run(iface, prob, cs, its, variant, window=_uniform(prob, 0.0))
    assert _sum(zeros, "roulette_killed") == _sum(zeros, "roulette_survived") == 0
    _bitwise(zeros, never, variant)


@gpu
@needs_gpu
def test_off_is_off(iface, make_problem, cs):
    """a run after window_in_step(None) is bitwise the run that never had it"""
    prob, its = _deck(make_problem, "csp")
    never = _run(iface, prob, cs, its)
    sim = iface.Simulation(prob, *cs, variant=2)
    try:
        sim.inject()
        sim.window_in_step(0.25, 2.0)
        assert sim.step(1).stats.roulette_killed + sim.step(2).stats.roulette_survived > 0
        sim.window_in_step(None)
        sim.inject()
        steps = [sim.step(k) for k in range(1, its + 1)]
        after = {"steps": steps, "parts": sim.particle_arrays()}
    finally:
        sim.close()
    assert _counts(after) == _counts(never) and _weights(after) == [(0.0, 0.0)] * its
    for f in never["parts"]:
        assert np.array_equal(after["parts"][f], never["parts"][f]), f
    # (the tally of this Simulation holds the played steps too: the particle arrays and the
    # counters say that nothing played; a fresh Simulation says the same of the tally)
    fresh = _run(iface, prob, cs, its)
    _bitwise(fresh, never)


def _against_replay(got, rep, end, per_step):
    assert [(r.collisions, r.facets, r.stats.roulette_killed, r.stats.roulette_survived) for r in got["steps"]] == \
        [_events(s) for s in per_step]
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got["parts"][f], end[f]), f
    assert np.array_equal(got["parts"]["weight"] == 0.0, end["weight"] == 0.0)
    print("weights: max deviation", np.abs(got["parts"]["weight"] - end["weight"]).max())
    assert np.abs(got["parts"]["weight"] - end["weight"]).max() <= WEIGHT_TOL
    lost = math.fsum(r.stats.roulette_weight_lost for r in got["steps"])
    gained = math.fsum(r.stats.roulette_weight_gained for r in got["steps"])
    print("lost", lost, rep.lost, "gained", gained, rep.gained)
    scale = max(abs(rep.lost), abs(rep.gained))
    assert abs(lost - rep.lost) <= WEIGHT_TOL * scale and abs(gained - rep.gained) <= WEIGHT_TOL * scale
    assert np.array_equal(got["collisions"], rep.collisions.ravel())
    for name in ("flux", "absorbed"):
        err = l2(got[name], getattr(rep, name).ravel())
        print(name, "L2", err)
        assert err <= TALLY_L2_TOL, (name, err)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("kind", ["two", "groups"])
def test_against_the_replay(iface, make_problem, cs, monkeypatch, variant, kind):
    """csp 24 / 600 / 3 with p_absorb = 1/3: the two-valued mesh and the grouped mesh against
    the windowed replay, history by history."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")   # small decks under windows too
    prob = _oracle_problem(make_problem)
    if kind == "two":
        window = dict(lower=two_valued(prob.nx, prob.ny), survival_ratio=2.0)
    else:
        edges = _oracle_edges(prob)
        window = dict(lower=grouped(prob, edges), survival_ratio=2.0, groups=edges)
    got = _run(iface, prob, cs, STEPS, variant, window=window, cs_absorb=third_absorb(cs), scalar_flux=True,
               collision_tallies=True)
    rep, end, _, per_step = _replayed(prob, cs, got["injected"], kind)
    assert rep.killed > 0 and rep.survived > 0
    _against_replay(got, rep, end, per_step)


def _two_64(prob):
    return two_valued(prob.nx, prob.ny)


@gpu
@needs_gpu
def test_equivalent_forms(iface, make_problem, cs):
    """block (1, 1), one all-containing group, and G groups that carry the same mesh: the plain
    form's bits"""
    prob, its = _deck(make_problem, "csp")
    mesh = _two_64(prob)
    plain = _run(iface, prob, cs, its, window=dict(lower=mesh, survival_ratio=2.0))
    assert _sum(plain, "roulette_killed") > 0 and _sum(plain, "roulette_survived") > 0
    unit = _run(iface, prob, cs, its, window=dict(lower=mesh, survival_ratio=2.0, block=(1, 1)))
    _bitwise(unit, plain, "block 1 x 1")
    one = _run(iface, prob, cs, its, window=dict(lower=mesh[None], survival_ratio=2.0, groups=[1e-300, 1e300]))
    _bitwise(one, plain, "one group")
    edges = np.concatenate([[1e-300], prob.initial_energy * np.geomspace(1e-4, 0.9, 6), [1e300]])
    many = _run(iface, prob, cs, its,
                window=dict(lower=np.repeat(mesh[None], len(edges) - 1, axis=0), survival_ratio=2.0, groups=edges))
    _bitwise(many, plain, "seven groups, one mesh")
    both = _run(iface, prob, cs, its, window=dict(lower=mesh[None], survival_ratio=2.0, groups=[1e-300, 1e300],
                                                  block=(1, 1)))
    _bitwise(both, plain, "one group, block 1 x 1")


@gpu
@needs_gpu
def test_blocks_equal_the_expanded_mesh(iface, make_problem, cs):
    """blocks (3, 2) on 64^2 -- the last block of a row and of a column narrower -- against the
    plain form on the bounds expanded to cells; with groups, against groups on the expanded bounds"""
    prob, its = _deck(make_problem, "csp")
    bx, by = 3, 2
    cnx, cny = -(-prob.nx // bx), -(-prob.ny // by)
    assert cnx * bx > prob.nx                      # (the last block of a row is narrower)
    rng = np.random.default_rng(5)
    coarse = rng.choice([0.0, 0.125, 0.25, 0.5], size=(cny, cnx))
    expanded = np.kron(coarse, np.ones((by, bx)))[:prob.ny, :prob.nx]
    blocks = _run(iface, prob, cs, its, window=dict(lower=coarse, survival_ratio=2.0, block=(bx, by)))
    plain = _run(iface, prob, cs, its, window=dict(lower=expanded, survival_ratio=2.0))
    assert _sum(plain, "roulette_killed") > 0 and _sum(plain, "roulette_survived") > 0
    _bitwise(blocks, plain, "blocks")
    edges = np.concatenate([[1e-300], prob.initial_energy * np.array([1e-3, 0.1, 0.5]), [1e300]])
    g = len(edges) - 1
    coarse_g = rng.choice([0.0, 0.125, 0.25, 0.5], size=(g, cny, cnx))
    expanded_g = np.stack([np.kron(c, np.ones((by, bx)))[:prob.ny, :prob.nx] for c in coarse_g])
    blocks_g = _run(iface, prob, cs, its, window=dict(lower=coarse_g, survival_ratio=2.0, groups=edges, block=(bx, by)))
    groups = _run(iface, prob, cs, its, window=dict(lower=expanded_g, survival_ratio=2.0, groups=edges))
    assert _sum(groups, "roulette_killed") > 0
    _bitwise(blocks_g, groups, "blocks with groups")
    assert _counts(groups) != _counts(plain)


def _everything(prob):
    spectrum = (prob.initial_energy * np.geomspace(0.5, 1.02, 9), (3, 4, prob.nx - 2, prob.ny - 1))
    return dict(scalar_flux=True, collision_tallies=True, current=True, outflow=True, spectrum=spectrum)


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_variants_agree_with_every_tally(iface, make_problem, cs, lazy):
    prob, its = _deck(make_problem, "csp")
    iface.set_lazy_export(lazy)
    window = dict(lower=_two_64(prob), survival_ratio=2.0)
    runs = {v: _run(iface, prob, cs, its, v, window=window, **_everything(prob)) for v in (0, 1, 2)}
    assert _sum(runs[0], "roulette_killed") > 0
    _variants_agree(runs)
    for v, run in runs.items():
        for t in ("jx", "jy", "out", "spectrum"):
            ref = np.linalg.norm(runs[0][t])
            assert np.linalg.norm(run[t] - runs[0][t]) <= 1e-9 * max(ref, 1e-300), (v, t)


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_weight_balance(iface, make_problem, cs, deck):
    """N = sum(weights) + N * sum(absorbed) + lost - gained, with a two-valued mesh"""
    prob, its = _deck(make_problem, deck)
    run = _run(iface, prob, cs, its, window=dict(lower=_two_64(prob), survival_ratio=2.0), collision_tallies=True)
    n = prob.nparticles
    lost, gained = _sum(run, "roulette_weight_lost"), _sum(run, "roulette_weight_gained")
    balance = run["parts"]["weight"].sum() + n * run["absorbed"].sum() + lost - gained
    print(deck, "balance - N", balance - n, "killed", _sum(run, "roulette_killed"))
    assert _sum(run, "roulette_killed") > 0
    assert abs(balance - n) <= 1e-12 * n


@gpu
@needs_gpu
def test_time_sliced_collision_stage(iface, make_problem, cs, monkeypatch):
    """Requeued histories play by the mesh like the others: a bound forty absorptions down in
    half the mesh, none elsewhere."""
    prob = make_problem("csp", nx=100, nparticles=100000, iterations=2, dt=1.0e-6)
    mesh = np.zeros((prob.ny, prob.nx))
    mesh[:, :prob.nx // 2] = 2.0 ** -40
    window = dict(lower=mesh, survival_ratio=4.0)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    sliced = _run(iface, prob, cs, 2, 2, window=window)
    plain = _run(iface, prob, cs, 2, 0, window=window)
    assert _sum(sliced, "requeued") > 0 and _sum(sliced, "roulette_killed") > 0
    _variants_agree({0: plain, 2: sliced})
    assert _weights(sliced) != [(0.0, 0.0)] * 2


@gpu
@needs_gpu
def test_the_mesh_is_checked_when_it_is_set(iface, make_problem, cs):
    """A negative entry, a NaN and an infinity each refuse and leave the previous mesh in force;
    and while a mesh is set, a global cutoff is refused."""
    import torch
    prob, its = _deck(make_problem, "scatter")
    first = _run(iface, prob, cs, its, window=_uniform(prob))
    assert _sum(first, "roulette_killed") > 0
    sim = iface.Simulation(prob, *cs, variant=2)
    try:
        sim.inject()
        sim.window_in_step(**_uniform(prob))
        for bad in (-1e-300, nan, inf, -inf):
            mesh = np.full((prob.ny, prob.nx), 0.5)
            mesh[prob.ny - 1, prob.nx - 1] = bad
            with pytest.raises(ValueError):
                sim.window_in_step(mesh, 2.0)
        steps = [sim.step(k) for k in range(1, its + 1)]
        again = {"steps": steps, "parts": sim.particle_arrays()}
    finally:
        sim.close()
    assert _counts(again) == _counts(first)
    _same_weights(again, first)
    for f in first["parts"]:
        assert np.array_equal(again["parts"][f], first["parts"][f]), f
    # the library's own setting: a refused mesh leaves the previous one, and the two roulettes exclude each other
    good = torch.full((prob.nx * prob.ny,), 0.25, dtype=torch.float64, device="cuda")
    bad = good.clone()
    bad[17] = float("nan")
    try:
        iface.set_window_roulette(prob.nx, prob.ny, good, 2.0)
        with pytest.raises(ValueError):
            iface.set_window_roulette(prob.nx, prob.ny, bad, 2.0)
        with pytest.raises(ValueError):
            iface.set_roulette(*ON)
        iface.set_roulette(0.0, 0.0)   # ((0, 0) is still accepted, and still means what it did)
        sim = iface.Simulation(prob, *cs, variant=2)
        sim.inject()
        steps = [sim.step(k) for k in range(1, its + 1)]
        held = {"steps": steps, "parts": sim.particle_arrays()}
        sim.close()
    finally:
        iface.set_window_roulette(0, 0, None)
    assert _counts(held) == _counts(first)
    iface.set_roulette(*ON)            # (accepted again once the mesh is off)
    iface.set_roulette(0.0, 0.0)


@gpu
@needs_gpu
def test_a_rewritten_mesh(iface, make_problem, cs, monkeypatch):
    """Four steps with auto_window(in_step=True) after each: variants 0 and 2 agree bit for bit,
    and the step after a call plays by the new bounds -- checked against the windowed replay fed
    last_lower, step by step from the arrays the census window left."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=24, nparticles=600, iterations=4, dt=1.0e-6)
    absorb = third_absorb(cs)
    runs = {}
    for variant in (0, 2):
        lowers = []

        def rewindow(sim, tt):
            sim.auto_window(in_step=True, survival_ratio=2.0)
            lowers.append(sim.last_lower.cpu().numpy().copy())
        runs[variant] = _run(iface, prob, cs, 4, variant, per_step=True, after_step=rewindow, cs_absorb=absorb)
        runs[variant]["lowers"] = lowers
    a, b = runs[0], runs[2]
    # The bounds are made from the census's weights, per cell a sum of unordered f64 atomics: the
    # two runs' bounds are held to that sum's margin, and -- a survivor goes on at ratio * bound --
    # the weights to their bits wherever the bounds came out bit for bit equal, which is the usual
    # case; cells, deaths and every counter are held to their bits whatever the bounds' last bits.
    assert _counts(a) == _counts(b)
    for la, lb in zip(a["lowers"], b["lowers"]):
        assert np.array_equal(la == 0.0, lb == 0.0)
        assert np.linalg.norm(la - lb) <= SUM_ORDER_TOL * np.linalg.norm(lb)
    same_bounds = all(np.array_equal(la, lb) for la, lb in zip(a["lowers"], b["lowers"]))
    print("bounds bit for bit equal between the variants:", same_bounds)
    for sa, sb in zip(a["snaps"], b["snaps"]):
        for f in sa:
            if same_bounds or f in ("cellx", "celly", "dead"):
                assert np.array_equal(sa[f], sb[f]), f
            elif f == "weight":
                assert np.abs(sa[f] - sb[f]).max() <= WEIGHT_TOL, f
    assert not np.array_equal(a["lowers"][0], a["lowers"][1])     # (the mesh was rewritten)
    assert a["steps"][0].stats.roulette_killed == a["steps"][0].stats.roulette_survived == 0   # (no bounds yet)
    # snaps: injected, after step 1, after window 1, after step 2, after window 2, ...
    played = 0
    for n in range(1, 4):
        start, end = a["snaps"][2 * n], a["snaps"][2 * n + 1]
        rep = _windowed(prob, cs, absorb, a["lowers"][n - 1], 2.0)
        run = replay.run_steps(rep, start, 1, keys=[n + 1])
        want, events = run["snaps"][-1], _events(run["per_step"][0])
        got = a["steps"][n]
        print("step", n + 1, "replay", events, "gpu", got.collisions, got.facets, got.stats.roulette_killed,
              got.stats.roulette_survived)
        assert (got.collisions, got.facets, got.stats.roulette_killed, got.stats.roulette_survived) == events
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(end[f], want[f]), (n, f)
        assert np.array_equal(end["weight"] == 0.0, want["weight"] == 0.0)
        assert np.abs(end["weight"] - want["weight"]).max() <= WEIGHT_TOL
        played += rep.killed + rep.survived
    assert played > 0


@gpu
@needs_gpu
def test_a_global_cutoff_of_the_simulation_excludes_the_window(iface, make_problem, cs):
    prob, its = _deck(make_problem, "scatter")
    sim = iface.Simulation(prob, *cs, variant=2, roulette=ON)
    try:
        sim.inject()
        with pytest.raises(ValueError):
            sim.window_in_step(0.25, 2.0)
        assert sim.in_step_window is None
        assert sim.step(1).stats.roulette_killed > 0   # (the cutoff plays on)
    finally:
        sim.close()


@gpu
@needs_gpu
def test_tallies_are_unbiased(iface, make_problem, cs):
    """tests/test_roulette.py::test_tallies_are_unbiased's method and margin for the two-valued
    mesh: 16 key sets, deposition and flux totals within 5 sigma of the roulette-off runs"""
    prob, its = _deck(make_problem, "csp")

    def totals(window):
        dep, flux = [], []
        for key in range(16):
            run = _run(iface, prob, cs, its, window=window, scalar_flux=True,
                       keys=[1000 * (key + 1) + t for t in range(1, its + 1)])
            dep.append(run["tally"].sum())
            flux.append(run["flux"].sum())
        return np.array(dep), np.array(flux)
    d_off, f_off = totals(None)
    d_on, f_on = totals(dict(lower=_two_64(prob), survival_ratio=2.0))
    _agree(d_on, d_off)
    _agree(f_on, f_off)
    assert not np.array_equal(d_on, d_off)   # (roulette did play)


# ---- the driver -----------------------------------------------------------------------------------

def _driver_dir(tmp_path):
    from neutral_amd import cs_table, decks
    run = tmp_path / "arch" / "neutral"
    (run / "problems").mkdir(parents=True)
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    return run, rel


def _driver_numbers(stdout):
    facets = [int(x) for x in re.findall(r"^Facets\s+(\d+)", stdout, flags=re.M)]
    colls = [int(x) for x in re.findall(r"^Collisions\s+(\d+)", stdout, flags=re.M)]
    killed = int(re.search(r"^Roulette killed (\d+)$", stdout, flags=re.M).group(1))
    survived = int(re.search(r"^Roulette survived (\d+)$", stdout, flags=re.M).group(1))
    tally = float(re.search(r"Final global_energy_tally (\S+)", stdout).group(1))
    return facets, colls, killed, survived, tally


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_usage_error(tmp_path):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params", "--window-in-step"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert "--window-in-step needs --window" in out.stderr + out.stdout


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_and_ranks(tmp_path):
    """csp 64^2 / 8192 / 3 steps with --window 0.25 --window-in-step on one rank, on two ranks
    that share the mesh, and on a mesh decomposed 2x1: the same roulette lines and event counts."""
    run, rel = _driver_dir(tmp_path)
    sets = []
    for kv in ("nx=64", "ny=64", "nparticles=8192", "iterations=3", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), rel, sets)
    assert "Roulette" not in plain
    window_only = run_driver(str(run), rel, sets + ["--window", "0.25"])
    # without the flag the output keeps the parent's form: the plain run's lines, number for number
    # in shape, and after them the census window's five totals and nothing else
    def shapes(lines):
        return [re.sub(r"[-+]?\d[\d.]*(e[-+]?\d+)?", "N", ln) for ln in lines]
    lines = untimed_lines(window_only)
    own = [ln for ln in lines if ln.startswith("Window ")]
    assert shapes(own) == ["Window roulette killed N", "Window roulette survived N", "Window split N",
                           "Window copies made N", "Window copies refused N"]
    assert shapes([ln for ln in lines if not ln.startswith("Window ")]) == shapes(untimed_lines(plain))
    assert not any(ln.startswith("Roulette") for ln in lines)
    in_step = ["--window", "0.25", "--window-in-step"]
    one = run_driver(str(run), rel, sets + in_step)
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "20", "NEUTRAL_HIP_COMM": "host"}
    shard = run_driver(str(run), rel, sets + in_step + ["--gpus", "2"], env)
    domain = run_driver(str(run), rel, sets + in_step + ["--gpus", "2", "--decompose", "2x1"], env)
    f1, c1, k1, s1, t1 = _driver_numbers(one)
    assert k1 > 0 and s1 > 0 and len(c1) == 3
    assert sum(c1) < sum(int(x) for x in re.findall(r"^Collisions\s+(\d+)", plain, flags=re.M))
    for name, many in (("shard", shard), ("domain", domain)):
        f, c, k, s, t = _driver_numbers(many)
        print(name, f, c, k, s, t, "one rank", t1)
        assert (f, c, k, s) == (f1, c1, k1, s1), name
        assert abs(t - t1) <= 1e-12 * max(abs(t1), 1.0), name

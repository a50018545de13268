"""Collision tallies (include/neutral_hip.h: neutral_hip_set_collision_tallies): the
collision events per cell and the weight absorbed per cell (times 1/N), scored by the
kernels that collide.  The CPU oracle restates them and the HIP path is compared with that
cell by cell (tests/test_tallies_parity.py); here, without any oracle, what the definitions
imply: the counts sum exactly to the step's collision count, they agree bitwise
between the kernel variants, the absorbed weight balances the weight the particles
keep, only cells of a dense region see collisions, and keeping the tallies changes
nothing else the library computes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, run_driver  # noqa: F401


# ---- CPU: the ABI and the wrapper's argument handling ---------------------------------------

def test_library_exports_the_setter_at_abi_12():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_set_collision_tallies")
    assert "neutral_hip_set_collision_tallies" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12


def test_setter_refuses_one_mesh_without_the_other():
    """Both or neither: one alone returns 1 and changes nothing (no device is touched)."""
    from neutral_amd import interface as iface
    lib = iface.library()
    assert lib.neutral_hip_set_collision_tallies(C.c_void_p(0x1000), None) == 1
    assert lib.neutral_hip_set_collision_tallies(None, C.c_void_p(0x1000)) == 1
    assert lib.neutral_hip_set_collision_tallies(None, None) == 0


def test_wrapper_argument_handling():
    import torch
    from neutral_amd import interface as iface
    iface.set_collision_tallies()                 # both None: off
    iface.set_collision_tallies(None, None)
    iface.set_collision_tallies(0, 0)             # null addresses are None
    with pytest.raises(ValueError):
        iface.set_collision_tallies(0x1000, None)
    with pytest.raises(ValueError):
        iface.set_collision_tallies(None, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError):
        iface.set_collision_tallies(torch.zeros(4, dtype=torch.float32),
                                    torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError):
        t = torch.zeros(4, 4, dtype=torch.float64).t()
        iface.set_collision_tallies(t, t)
    with pytest.raises(TypeError):
        iface.set_collision_tallies("collisions", "absorbed")
    iface.set_collision_tallies(None, None)


# ---- GPU ---------------------------------------------------------------------------------


DECKS = {
    # deck: nx, nparticles, iterations, dt
    "csp": (64, 8192, 3, 2.0e-6),
    "scatter": (64, 4096, 2, None),
    "split": (64, 8192, 2, None),
    "stream": (64, 4096, 2, None),
}
VARIANTS = (0, 1, 2)


def _problem(make_problem, deck):
    nx, n, its, dt = DECKS[deck]
    kw = dict(nx=nx, nparticles=n, iterations=its)
    if dt is not None:
        kw["dt"] = dt
    return make_problem(deck, **kw), its


def _run(iface, prob, cs, its, variant, tallies=True):
    """steps 1..its; -> (collisions mesh, absorbed mesh, step results, particle arrays, tally)"""
    sim = iface.Simulation(prob, *cs, variant=variant, collision_tallies=tallies)
    sim.inject()
    steps = [sim.step(tt) for tt in range(1, its + 1)]
    out = (sim.collisions_host() if tallies else None, sim.absorbed_host() if tallies else None,
           steps, sim.particle_arrays(), sim.tally_host())
    sim.close()
    return out


_CACHE = {}


def _runs(iface, make_problem, cs, deck):
    """every variant once per deck, with the tallies (shared by the tests below)"""
    if deck not in _CACHE:
        prob, its = _problem(make_problem, deck)
        _CACHE[deck] = (prob, {v: _run(iface, prob, cs, its, v) for v in VARIANTS})
    return _CACHE[deck]


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_counts_sum_exactly_to_the_collisions(iface, make_problem, cs, deck):
    prob, runs = _runs(iface, make_problem, cs, deck)
    for v, (coll, _, steps, _, _) in runs.items():
        total = sum(r.collisions for r in steps)
        assert coll.sum() == float(total), (v, coll.sum(), total)
        assert np.array_equal(coll, np.floor(coll)) and coll.min() >= 0.0
        if deck == "stream":
            assert total == 0 and not coll.any()
        else:
            assert total > 0


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_variants_agree(iface, make_problem, cs, deck):
    prob, runs = _runs(iface, make_problem, cs, deck)
    c0, a0 = runs[0][0], runs[0][1]
    for v in VARIANTS[1:]:
        c, a = runs[v][0], runs[v][1]
        assert np.array_equal(c, c0), v
        if np.linalg.norm(a0) == 0.0:
            assert not a.any()
        else:
            assert np.linalg.norm(a - a0) / np.linalg.norm(a0) <= 1e-12, v


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_absorbed_weight_balances_the_particles_weight(iface, make_problem, cs, deck):
    """Every particle starts with weight 1 and loses weight only where it is absorbed (the
    mesh reflects, nobody leaves): N * sum(absorbed) + sum(weight) = N."""
    prob, runs = _runs(iface, make_problem, cs, deck)
    n = prob.nparticles
    for v, (_, absorbed, _, parts, _) in runs.items():
        balance = n * absorbed.sum() + parts["weight"].sum()
        assert abs(balance - n) <= 1e-12 * n, (v, balance, n)
        if deck != "stream":
            assert absorbed.sum() > 0.0


@gpu
@needs_gpu
def test_csp_collides_only_in_the_dense_box(iface, make_problem, cs):
    """csp: background density 1e-30 (problem_0), 1e4 in problem_1's box: a collision
    outside the box would take a path length of ~1e30 mean free paths."""
    prob, runs = _runs(iface, make_problem, cs, "csp")
    density = np.asarray(prob.density).reshape(-1)
    for v, (coll, absorbed, _, _, _) in runs.items():
        hit = coll > 0
        assert hit.any()
        assert np.all(density[hit] == 1.0e4), v
        assert not absorbed[~hit].any(), v


def _same_histories(on, off):
    coll, absorbed, s_on, p_on, t_on = on
    _, _, s_off, p_off, t_off = off
    for a, b in zip(s_on, s_off):
        assert (a.nprocessed, a.facets, a.collisions, a.census) == \
            (b.nprocessed, b.facets, b.collisions, b.census)
    for f in p_on:
        assert np.array_equal(p_on[f], p_off[f]), f
    # (the energy tally's atomics add in whatever order the waves arrive, with or without)
    if np.linalg.norm(t_off) == 0.0:
        assert not t_on.any()
    else:
        assert np.linalg.norm(t_on - t_off) / np.linalg.norm(t_off) < 1e-13
    assert np.array_equal(t_on == 0.0, t_off == 0.0)


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_tallies_disturb_nothing(iface, make_problem, cs, deck, variant):
    prob, runs = _runs(iface, make_problem, cs, deck)
    _, its = _problem(make_problem, deck)
    _same_histories(runs[variant], _run(iface, prob, cs, its, variant, tallies=False))


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_checked_arithmetic_with_a_true_vacuum(iface, make_problem, cs, variant):
    """csp with its background at density 0 (cell_mfp = 1/0 = inf): the checked kernels run,
    with the tallies as without, and the counts still sum to the collisions."""
    prob, its = _problem(make_problem, "csp")
    prob.density[prob.density < 1.0e-20] = 0.0
    on = _run(iface, prob, cs, its, variant)
    assert all(r.stats.checked_arithmetic == 1 for r in on[2])
    _same_histories(on, _run(iface, prob, cs, its, variant, tallies=False))
    assert on[0].sum() == float(sum(r.collisions for r in on[2]))
    n = prob.nparticles
    assert abs(n * on[1].sum() + on[3]["weight"].sum() - n) <= 1e-12 * n


@gpu
@needs_gpu
def test_tallies_survive_the_time_sliced_collision_stage(iface, make_problem, cs, monkeypatch):
    """A history set aside in the middle of its collision chain flushes its scores first:
    its record carries none, and none are lost or counted twice."""
    prob = make_problem("csp", nx=100, nparticles=100000, iterations=2, dt=1.0e-6)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    coll, absorbed, steps, parts, _ = _run(iface, prob, cs, 2, 2)
    assert sum(r.stats.requeued for r in steps) > 0
    assert coll.sum() == float(sum(r.collisions for r in steps))
    n = prob.nparticles
    assert abs(n * absorbed.sum() + parts["weight"].sum() - n) <= 1e-12 * n


@gpu
@needs_gpu
def test_zero_tally_zeroes_them(iface, make_problem, cs):
    prob, _ = _problem(make_problem, "scatter")   # (collides from the first step on)
    sim = iface.Simulation(prob, *cs, variant=2, collision_tallies=True)
    sim.inject()
    r = sim.step(1)
    assert sim.collisions_host().sum() == float(r.collisions) > 0
    sim.zero_tally()
    assert not sim.collisions_host().any() and not sim.absorbed_host().any()
    r = sim.step(2)
    assert sim.collisions_host().sum() == float(r.collisions)
    sim.close()
    plain = iface.Simulation(prob, *cs, variant=2)
    with pytest.raises(RuntimeError):
        plain.collisions_host()
    plain.close()


def _driver_deck(tmp_path):
    from neutral_amd import cs_table, decks
    run = tmp_path / "arch" / "neutral"
    (run / "problems").mkdir(parents=True)
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    sets = []
    for kv in ("nx=128", "ny=128", "nparticles=200001", "iterations=3", "dt=1.0e-6"):
        sets += ["--set", kv]
    return str(run), rel, sets


def _totals(stdout):
    colls = sum(int(x) for x in re.findall(r"^Collisions\s+(\d+)", stdout, flags=re.M))
    total = float(re.search(r"^Collision tally total (\S+)", stdout, flags=re.M).group(1))
    absorbed = float(re.search(r"^Absorbed weight total (\S+)", stdout, flags=re.M).group(1))
    return colls, total, absorbed


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("extra", [[], ["--decompose", "2x1"]])
def test_two_ranks_sum_to_the_global_collisions(tmp_path, extra):
    """`neutral.hip --gpus 2 --collision-tallies`, both ranks on one GPU: shards of the
    particles (the all-reduce route) or blocks of the mesh (each rank its own cells).  The
    totals equal the one-rank run's; without the flag, stdout says nothing of them."""
    run, rel, sets = _driver_deck(tmp_path)
    plain = run_driver(run, rel, sets)
    assert "Collision tally" not in plain and "Absorbed weight" not in plain
    c1, t1, a1 = _totals(run_driver(run, rel, sets + ["--collision-tallies"]))
    assert t1 == float(c1) > 0
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60",
           "NEUTRAL_HIP_COMM": "host"}
    c2, t2, a2 = _totals(run_driver(run, rel, sets + ["--gpus", "2", "--collision-tallies"] + extra,
                                 env))
    assert c2 == c1 and t2 == float(c2)
    assert abs(a2 - a1) <= 1e-12 * a1


@gpu
@needs_gpu
def test_full_size_csp(iface, make_problem, cs):
    """csp 400^2 with 1e8 particles (the benchmark's configuration): the histories reach the
    dense box after a few steps of dt = 1e-7, and then collide some 1e9 times per step -- all
    summed exactly from the per-cell flushes."""
    prob = make_problem("csp", nx=400, nparticles=100_000_000, iterations=10)
    sim = iface.Simulation(prob, *cs, variant=2, collision_tallies=True)
    sim.inject()
    total = 0
    for tt in range(1, 11):
        sim.zero_tally()
        r = sim.step(tt)
        total += r.collisions
        assert sim.collisions_host().sum() == float(r.collisions), tt
        if r.collisions > 1_000_000_000:
            break
    assert r.collisions > 1_000_000_000, total
    sim.close()

"""Weight cutoff with Russian roulette (include/neutral_hip.h: neutral_hip_set_roulette).

The CPU oracle restates it and the HIP path is compared with that decision by decision
(tests/test_tallies_parity.py); here, without any oracle, what its definition implies.  Roulette draws
nothing (it takes the second number of the absorption's own draw), so a history's path with
roulette on is bit for bit its path with roulette off up to where roulette ends it; the
weights it leaves are the roulette-off weights or w_s halved; the weight it moves balances
exactly; the game is fair; the tallies keep their expected value; and the kernel variants,
the arithmetic policies, the time-sliced collision stage and several ranks all agree."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, run_driver, untimed_lines  # noqa: F401
from ranks import launch_gpu_ranks

ON = (0.25, 0.5)


# ---- CPU: the ABI and the wrapper's argument handling ---------------------------------------

REFUSED = [
    (float("nan"), 0.5), (0.25, float("nan")), (-0.25, 0.5), (0.25, -0.5), (-0.0, -1.0),
    (0.0, 0.5), (0.25, 0.0), (0.5, 0.25), (float("inf"), float("inf")), (0.25, float("inf")),
]
ACCEPTED = [(0.0, 0.0), (0.25, 0.5), (0.5, 0.5), (1e-300, 1.0), (0.75, 1.0)]


def test_library_exports_the_setter():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_set_roulette")
    assert "neutral_hip_set_roulette" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    names = [f[0] for f in iface.StepStats._fields_]
    assert names[-4:] == ["roulette_killed", "roulette_survived", "roulette_weight_lost",
                          "roulette_weight_gained"]


@pytest.mark.parametrize("wc, ws", REFUSED)
def test_setter_refuses(wc, ws):
    from neutral_amd import interface as iface
    lib = iface.library()
    lib.neutral_hip_set_roulette.restype = C.c_int
    assert lib.neutral_hip_set_roulette(C.c_double(wc), C.c_double(ws)) == 1
    assert lib.neutral_hip_set_roulette(C.c_double(0.0), C.c_double(0.0)) == 0


@pytest.mark.parametrize("wc, ws", ACCEPTED)
def test_setter_accepts(wc, ws):
    from neutral_amd import interface as iface
    assert iface.library().neutral_hip_set_roulette(C.c_double(wc), C.c_double(ws)) == 0
    assert iface.library().neutral_hip_set_roulette(C.c_double(0.0), C.c_double(0.0)) == 0


def test_wrapper_raises_where_the_library_refuses():
    from neutral_amd import interface as iface
    iface.set_roulette(*ON)
    for wc, ws in REFUSED:
        with pytest.raises(ValueError):
            iface.set_roulette(wc, ws)
        assert iface._roulette == ON  # (the previous setting stays in force)
    for wc, ws in ACCEPTED:
        iface.set_roulette(wc, ws)
        assert iface._roulette == (wc, ws)
    iface.set_roulette()
    assert iface._roulette == (0.0, 0.0)


# ---- GPU ---------------------------------------------------------------------------------


DECKS = {
    # deck: nx, nparticles, iterations, dt (tests/test_collision_tallies.py's sizes)
    "csp": (64, 8192, 3, 2.0e-6),
    "scatter": (64, 4096, 2, None),
    "split": (64, 8192, 2, None),
}
POSITION_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "dt_to_census", "mfp_to_collision",
                   "cellx", "celly")


def _problem(make_problem, deck):
    nx, n, its, dt = DECKS[deck]
    kw = dict(nx=nx, nparticles=n, iterations=its)
    if dt is not None:
        kw["dt"] = dt
    return make_problem(deck, **kw), its


def _run(iface, prob, cs, its, variant=2, roulette=None, keys=None, **kw):
    """steps with master keys `keys` (1..its); -> dict of the run's results"""
    sim = iface.Simulation(prob, *cs, variant=variant, roulette=roulette, **kw)
    sim.inject()
    steps = [sim.step(k) for k in (keys or range(1, its + 1))]
    out = {"steps": steps, "parts": sim.particle_arrays(), "tally": sim.tally_host()}
    if sim.flux is not None:
        out["flux"] = sim.flux.cpu().numpy()
    if sim.collisions is not None:
        out["collisions"], out["absorbed"] = sim.collisions_host(), sim.absorbed_host()
    sim.close()
    return out


def _sum(run, field):
    return sum(getattr(r.stats, field) for r in run["steps"])


def _counts(run):
    return [(r.nprocessed, r.facets, r.collisions, r.census, r.stats.roulette_killed,
             r.stats.roulette_survived) for r in run["steps"]]


_CACHE = {}


def _pair(iface, make_problem, cs, deck):
    """(problem, roulette-off run, roulette-on run) per deck, shared by the tests below"""
    if deck not in _CACHE:
        prob, its = _problem(make_problem, deck)
        _CACHE[deck] = (prob, _run(iface, prob, cs, its), _run(iface, prob, cs, its, roulette=ON))
    return _CACHE[deck]


@gpu
@needs_gpu
def test_off_is_off(iface, make_problem, cs):
    """set_roulette(0, 0) after a roulette run: bitwise the run that never had it."""
    prob, its = _problem(make_problem, "csp")
    never = _run(iface, prob, cs, its)
    iface.set_roulette(*ON)
    played = _run(iface, prob, cs, its)
    assert _sum(played, "roulette_killed") > 0
    iface.set_roulette(0.0, 0.0)
    after = _run(iface, prob, cs, its)
    assert _counts(after) == _counts(never)
    assert _sum(after, "roulette_killed") == _sum(after, "roulette_survived") == 0
    assert _sum(after, "roulette_weight_lost") == _sum(after, "roulette_weight_gained") == 0.0
    for f in never["parts"]:
        assert np.array_equal(after["parts"][f], never["parts"][f]), f
    assert np.linalg.norm(after["tally"] - never["tally"]) <= 1e-13 * np.linalg.norm(never["tally"])


@gpu
@needs_gpu
def test_refused_values_leave_the_setting_in_force(iface, make_problem, cs):
    prob, its = _problem(make_problem, "scatter")
    iface.set_roulette(*ON)
    first = _run(iface, prob, cs, its)
    for wc, ws in REFUSED:
        with pytest.raises(ValueError):
            iface.set_roulette(wc, ws)
    again = _run(iface, prob, cs, its)
    assert _counts(again) == _counts(first) and _sum(first, "roulette_killed") > 0
    for f in first["parts"]:
        assert np.array_equal(again["parts"][f], first["parts"][f]), f


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_paths_are_unchanged(iface, make_problem, cs, deck):
    prob, off, on = _pair(iface, make_problem, cs, deck)
    po, pn = off["parts"], on["parts"]
    alive = pn["dead"] == 0
    for f in POSITION_FIELDS:
        assert np.array_equal(pn[f][alive], po[f][alive]), f
    assert np.all(pn["dead"][po["dead"] != 0] != 0)
    killed = _sum(on, "roulette_killed")
    assert killed > 0 and _sum(on, "roulette_survived") > 0
    # the ones roulette ended are the dead of weight 0 (an energy death keeps its weight)
    assert int(((pn["dead"] != 0) & (pn["weight"] == 0.0)).sum()) == killed
    assert not np.any((po["dead"] != 0) & (po["weight"] == 0.0))
    c_on, c_off = sum(r.collisions for r in on["steps"]), sum(r.collisions for r in off["steps"])
    assert c_on <= c_off
    if deck == "csp":
        assert c_on < c_off
    assert _sum(off, "roulette_killed") == _sum(off, "roulette_survived") == 0


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_weights(iface, make_problem, cs, deck):
    """Same-table decks (p_absorb = 1/2): every alive weight is the roulette-off weight or
    w_s 2^-j >= w_c, exactly; every history roulette ended holds weight 0."""
    prob, off, on = _pair(iface, make_problem, cs, deck)
    wc, ws = ON
    po, pn = off["parts"], on["parts"]
    alive = pn["dead"] == 0
    allowed = [ws * 2.0 ** -j for j in range(64) if ws * 2.0 ** -j >= wc]
    w = pn["weight"][alive]
    assert np.all((w == po["weight"][alive]) | np.isin(w, allowed))
    assert np.all(w >= wc)
    # (on these small decks the histories roulette ends would mostly die of their energy later
    # in the step: they are the dead of weight 0, one per kill)
    by_roulette = (pn["dead"] != 0) & (pn["weight"] == 0.0)
    assert int(by_roulette.sum()) == _sum(on, "roulette_killed") > 0
    assert np.all(pn["weight"][(pn["dead"] != 0) & (po["dead"] == 0)] == 0.0)


def _balance(run, n):
    lost, gained = _sum(run, "roulette_weight_lost"), _sum(run, "roulette_weight_gained")
    return run["parts"]["weight"].sum() + n * run["absorbed"].sum() + lost - gained


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_weight_balance(iface, make_problem, cs, deck):
    """N = sum of the record weights + N sum(absorbed) + lost - gained, to rounding."""
    prob, its = _problem(make_problem, deck)
    run = _run(iface, prob, cs, its, roulette=ON, collision_tallies=True)
    n = prob.nparticles
    assert _sum(run, "roulette_killed") > 0
    assert abs(_balance(run, n) - n) <= 1e-12 * n
    assert run["collisions"].sum() == float(sum(r.collisions for r in run["steps"]))


@gpu
@needs_gpu
def test_a_fair_game(iface, make_problem, cs):
    prob, its = _problem(make_problem, "scatter")
    run = _run(iface, prob, cs, its, roulette=ON)
    k, s = _sum(run, "roulette_killed"), _sum(run, "roulette_survived")
    lost, gained = _sum(run, "roulette_weight_lost"), _sum(run, "roulette_weight_gained")
    assert k + s > 1000
    assert abs(gained - lost) <= 5 * (ON[1] / 2) * math.sqrt(k + s)
    # w_c = 0.75, w_s = 1: every absorption (1 -> 0.5) plays, at probability exactly 1/2
    half = _run(iface, prob, cs, its, roulette=(0.75, 1.0))
    k, s = _sum(half, "roulette_killed"), _sum(half, "roulette_survived")
    assert k + s > 1000
    assert abs(k - s) <= 5 * math.sqrt(k + s)
    alive = half["parts"]["dead"] == 0
    assert np.all(half["parts"]["weight"][alive] == 1.0)


def _tally_totals(iface, prob, cs, its, roulette, nkeys=16, **kw):
    """energy deposition and scalar flux totals of runs with master keys 1000 k + (1..its)"""
    dep, flux = [], []
    for key in range(nkeys):
        run = _run(iface, prob, cs, its, roulette=roulette, scalar_flux=True,
                   keys=[1000 * (key + 1) + t for t in range(1, its + 1)], **kw)
        dep.append(run["tally"].sum())
        flux.append(run["flux"].sum())
    return np.array(dep), np.array(flux)


def _agree(a, b):
    sigma = math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    assert sigma > 0.0
    assert abs(a.mean() - b.mean()) <= 5 * sigma, (a.mean(), b.mean(), sigma)


@gpu
@needs_gpu
@pytest.mark.parametrize("tables", ["same", "different"])
def test_tallies_are_unbiased(iface, make_problem, cs, tables):
    prob, its = _problem(make_problem, "csp")
    kw = {}
    if tables == "different":
        keys, values = cs
        kw["cs_absorb"] = (np.array(keys), 0.5 * np.array(values))  # p_absorb = 1/3
    d_off, f_off = _tally_totals(iface, prob, cs, its, None, **kw)
    d_on, f_on = _tally_totals(iface, prob, cs, its, ON, **kw)
    _agree(d_on, d_off)
    _agree(f_on, f_off)
    assert not np.array_equal(d_on, d_off)  # (roulette did play)


def _variants_agree(runs):
    base = runs[0]
    for v, run in runs.items():
        assert _counts(run) == _counts(base), v
        for f in base["parts"]:
            assert np.array_equal(run["parts"][f], base["parts"][f]), (v, f)
        for t in ("tally", "flux", "collisions", "absorbed"):
            if t in base:
                ref = np.linalg.norm(base[t])
                assert np.linalg.norm(run[t] - base[t]) <= 1e-9 * max(ref, 1e-300), (v, t)


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
@pytest.mark.parametrize("arith", ["auto", "checked"])
def test_variants_and_policies_agree(iface, make_problem, cs, deck, arith):
    prob, its = _problem(make_problem, deck)
    if arith == "checked":
        iface.set_arithmetic(iface.ARITH_CHECKED)
    runs = {v: _run(iface, prob, cs, its, variant=v, roulette=ON) for v in (0, 1, 2)}
    assert _sum(runs[0], "roulette_killed") > 0
    if arith == "checked":
        assert all(r.stats.checked_arithmetic == 1 for r in runs[2]["steps"])
    _variants_agree(runs)


@gpu
@needs_gpu
def test_variants_agree_with_flux_and_collision_tallies(iface, make_problem, cs):
    prob, its = _problem(make_problem, "csp")
    runs = {v: _run(iface, prob, cs, its, variant=v, roulette=ON, scalar_flux=True,
                    collision_tallies=True) for v in (0, 1, 2)}
    _variants_agree(runs)
    for v, run in runs.items():
        assert run["collisions"].sum() == float(sum(r.collisions for r in run["steps"])), v
        n = prob.nparticles
        assert abs(_balance(run, n) - n) <= 1e-12 * n, v


@gpu
@needs_gpu
def test_time_sliced_collision_stage(iface, make_problem, cs, monkeypatch):
    """Requeued, handed-back and stolen histories carry the weight roulette gave them.  (A cutoff
    forty absorptions down: the chains stay longer than a time slice before roulette plays.)"""
    prob = make_problem("csp", nx=100, nparticles=100000, iterations=2, dt=1.0e-6)
    far = (2.0 ** -40, 2.0 ** -38)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    sliced = _run(iface, prob, cs, 2, variant=2, roulette=far, collision_tallies=True)
    plain = _run(iface, prob, cs, 2, variant=0, roulette=far, collision_tallies=True)
    assert _sum(sliced, "requeued") > 0 and _sum(sliced, "roulette_killed") > 0
    _variants_agree({0: plain, 2: sliced})
    n = prob.nparticles
    assert abs(_balance(sliced, n) - n) <= 1e-12 * n


# ---- two ranks on one GPU ---------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["shard", "domain"])
def test_two_ranks(iface, make_problem, cs, tmp_path, mode):
    """Two ranks, particles sharded or the mesh decomposed 2x1: the one-rank particle state
    and the one-rank roulette counts, summed over the ranks."""
    from neutral_amd import decks
    steps = 3
    from neutral_amd import host
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), nx=64, ny=64, nparticles=8192,
                            iterations=steps, dt=2.0e-6)
    prob = host.setup_problem(deck)  # (as the worker reads it)
    one = _run(iface, prob, cs, steps, variant=2, roulette=ON)
    ranks, logs = launch_gpu_ranks(deck, tmp_path, steps, "domain 2x1" if mode == "domain" else "shard", 2,
                                   roulette=ON)
    # every rank reports the sums over both
    for log in logs:
        assert log["killed"] == [r.stats.roulette_killed for r in one["steps"]]
        assert log["survived"] == [r.stats.roulette_survived for r in one["steps"]]
        for a, b in zip(log["lost"], (r.stats.roulette_weight_lost for r in one["steps"])):
            assert abs(a - b) <= 1e-12 * max(b, 1.0)
        for a, b in zip(log["gained"], (r.stats.roulette_weight_gained for r in one["steps"])):
            assert abs(a - b) <= 1e-12 * max(b, 1.0)
        if mode == "shard":
            assert log["collectives"] == [0] * steps
    assert sum(log["killed"]) > 0
    ids = np.concatenate([z["ids"] for z in ranks])
    assert np.array_equal(np.sort(ids), np.arange(prob.nparticles))
    for f in one["parts"]:
        merged = np.empty_like(one["parts"][f])
        for z in ranks:
            merged[z["ids"]] = z[f]
        assert np.array_equal(merged, one["parts"][f]), f


# ---- the driver ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver(tmp_path):
    from neutral_amd import cs_table, decks
    run = tmp_path / "arch" / "neutral"
    (run / "problems").mkdir(parents=True)
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    sets = []
    for kv in ("nx=64", "ny=64", "nparticles=20001", "iterations=3", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), rel, sets)
    assert "Roulette" not in plain
    off = untimed_lines(run_driver(str(run), rel, sets + ["--roulette", "0,0"]))
    assert [ln for ln in off if not ln.startswith("Roulette")] == untimed_lines(plain)
    assert "Roulette killed 0" in off and "Roulette survived 0" in off
    played = run_driver(str(run), rel, sets + ["--roulette", "0.25,0.5"])
    killed = int(re.search(r"^Roulette killed (\d+)$", played, flags=re.M).group(1))
    survived = int(re.search(r"^Roulette survived (\d+)$", played, flags=re.M).group(1))
    assert killed > 0 and survived > 0
    colls = [int(x) for x in re.findall(r"^Collisions\s+(\d+)", plain, flags=re.M)]
    colls_r = [int(x) for x in re.findall(r"^Collisions\s+(\d+)", played, flags=re.M)]
    assert sum(colls_r) < sum(colls)
    bad = subprocess.run([OWN_DRIVER, rel] + sets + ["--roulette", "0.5,0.25"], cwd=str(run),
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0

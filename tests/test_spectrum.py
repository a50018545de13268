"""Energy-group flux spectrum over a box of cells (include/neutral_hip.h:
neutral_hip_set_spectrum_tally): the track-length estimator sum(weight * segment) / N and the
collision estimator sum(weight / Sigma_t) / N by energy group, scored in every kernel variant.
The CPU oracle restates it and the HIP path is compared with that group by group
(tests/test_tallies_parity.py); here, without any oracle, what the definition implies: the track-length values
sum to the scalar-flux tally over the box, the stream deck's closed form, merged groups are sums
of fine ones, the two estimators agree within their noise, the variants agree, and keeping the
spectrum changes nothing else the library computes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, run_driver  # noqa: F401


# 8 log-spaced groups over [0.5, 2e6] eV: every energy the decks reach (1e3 ... 1e6 eV at the
# start, the histories end below 1 eV)
EDGES = np.geomspace(0.5, 2.0e6, 9)


# ---- CPU: the ABI and the wrapper's argument handling ---------------------------------------

def test_library_exports_the_setter_at_abi_12():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_set_spectrum_tally")
    assert "neutral_hip_set_spectrum_tally" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12


def _set(lib, edges, box=(0, 0, 4, 4), out=0x1000):
    e = np.ascontiguousarray(edges, dtype=np.float64)
    return lib.neutral_hip_set_spectrum_tally(max(len(e) - 1, 0), e.ctypes.data_as(C.POINTER(C.c_double)),
                                              *box, C.c_void_p(out) if out else None)


def test_setter_refusals():
    """Returns 1 for every refusal, 0 otherwise (no device is touched: nothing runs)."""
    from neutral_amd import interface as iface
    lib = iface.library()
    assert _set(lib, [1.0, 2.0]) == 0
    assert _set(lib, np.geomspace(1.0, 2.0, 65)) == 0                 # 64 groups
    assert _set(lib, np.geomspace(1.0, 2.0, 66)) == 1                 # 65 groups
    assert lib.neutral_hip_set_spectrum_tally(0, (C.c_double * 2)(1.0, 2.0), 0, 0, 4, 4,
                                              C.c_void_p(0x1000)) == 1
    for bad in ([1.0, math.inf], [math.nan, 2.0], [0.0, 1.0], [-1.0, 1.0], [2.0, 1.0],
                [1.0, 1.0], [1.0, 3.0, 2.0]):
        assert _set(lib, bad) == 1, bad
    for box in ((0, 0, 0, 4), (0, 0, 4, 0), (3, 0, 2, 4), (0, 3, 4, 3), (-1, 0, 4, 4), (0, -1, 4, 4)):
        assert _set(lib, [1.0, 2.0], box) == 1, box
    # NULL turns it off, whatever the rest
    assert lib.neutral_hip_set_spectrum_tally(0, None, 0, 0, 0, 0, None) == 0


def test_wrapper_argument_handling():
    import torch
    from neutral_amd import interface as iface
    out = torch.zeros(16, dtype=torch.float64)
    iface.set_spectrum_tally(EDGES, None, out.data_ptr())      # (an address: not dereferenced here)
    iface.set_spectrum_tally(EDGES, (0, 0, 8, 8), out)
    for edges, box in (([1.0], None), ([2.0, 1.0], None), ([0.0, 1.0], None),
                       (EDGES, (0, 0, 0, 8)), (EDGES, (-1, 0, 8, 8)), (np.geomspace(1, 2, 66), None)):
        with pytest.raises(ValueError):
            iface.set_spectrum_tally(edges, box, torch.zeros(200, dtype=torch.float64))
    with pytest.raises(ValueError):
        iface.set_spectrum_tally(EDGES, None, torch.zeros(4, dtype=torch.float64))  # too short
    with pytest.raises(TypeError):
        iface.set_spectrum_tally(EDGES, None, torch.zeros(16, dtype=torch.float32))
    iface.set_spectrum_tally(EDGES, None, None)                # off
    iface.set_spectrum_tally(None)


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


def dense_box(nx, ny):
    """csp's problem_1 box: cells [0.4 n, 0.6 n) on each axis"""
    return (int(round(0.4 * nx)), int(round(0.4 * ny)), int(round(0.6 * nx)), int(round(0.6 * ny)))


def _run(iface, prob, cs, its, variant, edges=EDGES, box=None, spectrum=True, flux=True,
         keys=None, **kw):
    """steps 1..its (master keys `keys`) -> dict of the results"""
    sim = iface.Simulation(prob, *cs, variant=variant, scalar_flux=flux,
                           spectrum=(edges, box) if spectrum else None, **kw)
    sim.inject()
    steps = [sim.step(k) for k in (keys or range(1, its + 1))]
    out = {"steps": steps, "parts": sim.particle_arrays(), "tally": sim.tally_host(),
           "flux": sim.flux.cpu().numpy() if flux else None}
    if spectrum:
        out["track"], out["coll"] = sim.spectrum_host()
    if kw.get("collision_tallies"):
        out["collisions"], out["absorbed"] = sim.collisions_host(), sim.absorbed_host()
    sim.close()
    return out


def _box_sum(mesh, prob, box):
    m = np.asarray(mesh).reshape(prob.ny, prob.nx)
    return m[box[1]:box[3], box[0]:box[2]].sum()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max() if np.abs(b).max() > 0 else 1.0
    return float(np.abs(a - b).max() / scale)


_CACHE = {}


def _runs(iface, make_problem, cs, deck, box_kind):
    key = (deck, box_kind)
    if key not in _CACHE:
        prob, its = _problem(make_problem, deck)
        box = (0, 0, prob.nx, prob.ny) if box_kind == "mesh" else dense_box(prob.nx, prob.ny)
        _CACHE[key] = (prob, box, {v: _run(iface, prob, cs, its, v, box=box) for v in VARIANTS})
    return _CACHE[key]


@gpu
@needs_gpu
@pytest.mark.parametrize("box_kind", ["mesh", "dense"])
@pytest.mark.parametrize("deck", list(DECKS))
def test_track_length_sums_to_the_flux_over_the_box(iface, make_problem, cs, deck, box_kind):
    """sum over groups of the track-length values = the scalar-flux tally summed over the box's
    cells: the same segments, weights and 1/N (lost or misplaced segments show here)"""
    prob, box, runs = _runs(iface, make_problem, cs, deck, box_kind)
    for v, r in runs.items():
        want = _box_sum(r["flux"], prob, box)
        assert want > 0.0, (v, box)
        assert abs(r["track"].sum() - want) <= 1e-12 * want, (v, r["track"].sum(), want)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_stream_deck_closed_form(iface, make_problem, cs, variant):
    """collision-free, one energy: the initial energy's group holds speed * dt per step (every
    history has weight 1 and flies the whole step), every other value is exactly 0"""
    from closed_form import EV_TO_J, PARTICLE_MASS
    prob, its = _problem(make_problem, "stream")
    r = _run(iface, prob, cs, its, variant, box=None, flux=False)
    e0 = prob.initial_energy
    g0 = int(np.searchsorted(EDGES, e0, side="right")) - 1
    speed = math.sqrt(2.0 * e0 * EV_TO_J / PARTICLE_MASS)
    want = speed * prob.dt * its
    assert abs(r["track"][g0] - want) <= 1e-12 * want, (r["track"][g0], want)
    others = np.delete(r["track"], g0)
    assert not others.any() and not r["coll"].any()


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_merged_groups_are_sums_of_fine_ones(iface, make_problem, cs, variant):
    prob, its = _problem(make_problem, "csp")
    box = dense_box(prob.nx, prob.ny)
    fine = _run(iface, prob, cs, its, variant, box=box, flux=False)
    coarse = _run(iface, prob, cs, its, variant, edges=EDGES[::2], box=box, flux=False)
    for est in ("track", "coll"):
        f, c = fine[est], coarse[est]
        assert c.sum() > 0.0, est
        assert _rel(c, f[0::2] + f[1::2]) <= 1e-12, (est, c, f)


@gpu
@needs_gpu
def test_the_two_estimators_agree(iface, make_problem, cs):
    """The collision value is sum(weight / Sigma_t) / N.  The kernels sample the distance to a
    collision as the reference does (omp3/neutral.c: mfp_to_collision = -log(rn) / Sigma_s of the
    cell where it is drawn, in units of the current cell's cell_mfp = 1 / Sigma_t), so the two
    estimators share their expected value where Sigma_s is 1 / m in every cell a flight crosses:
    the scatter deck (one density everywhere) with a flat table that makes Sigma_s exactly 1 / m.
    Over csp's dense box, per group, the two values then agree within a few standard errors (16
    master keys), and no group above the initial energy is ever scored.  (csp itself does not
    qualify: a history that enters its dense box from the 1e-30 background carries ~1e34 mean
    free paths drawn there.)"""
    prob = make_problem("scatter", nx=64, nparticles=65536, iterations=3)
    its = 3
    box = dense_box(prob.nx, prob.ny)
    avogadros, molar_mass, barns = 6.02214085774e23, 1.0e-2, 1.0e-28
    keys = cs[0]
    flat = np.full_like(cs[1], 1.0 / (1.0e4 * avogadros / molar_mass * barns))  # Sigma_s = 1 / m
    tr, co = [], []
    for k in range(16):
        mkeys = [1000 * (k + 1) + t for t in range(1, its + 1)]
        r = _run(iface, prob, (keys, flat), its, 2, box=box, flux=False, keys=mkeys)
        tr.append(r["track"])
        co.append(r["coll"])
    tr, co = np.array(tr), np.array(co)
    g0 = int(np.searchsorted(EDGES, prob.initial_energy, side="right")) - 1
    assert not tr[:, g0 + 1:].any() and not co[:, g0 + 1:].any()
    diff = tr - co
    mean = diff.mean(axis=0)
    se = diff.std(axis=0, ddof=1) / math.sqrt(len(diff))
    scored = (tr > 0).all(axis=0) & (co > 0).all(axis=0)
    assert scored.any(), (tr.mean(axis=0), co.mean(axis=0))
    for g in np.nonzero(scored)[0]:
        assert abs(mean[g]) <= 5.0 * se[g], (g, tr.mean(axis=0)[g], co.mean(axis=0)[g], se[g])


def _same_histories(on, off, exact_tallies=False):
    for a, b in zip(on["steps"], off["steps"]):
        assert (a.nprocessed, a.facets, a.collisions, a.census) == \
            (b.nprocessed, b.facets, b.collisions, b.census)
    for f in on["parts"]:
        assert np.array_equal(on["parts"][f], off["parts"][f]), f
    for mesh in ("tally", "flux", "collisions", "absorbed"):
        if on.get(mesh) is None:
            continue
        a, b = on[mesh], off[mesh]
        if np.linalg.norm(b) == 0.0:
            assert not a.any(), mesh
        else:
            assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-13, mesh


@gpu
@needs_gpu
@pytest.mark.parametrize("deck", list(DECKS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_spectrum_disturbs_nothing(iface, make_problem, cs, deck, variant):
    prob, its = _problem(make_problem, deck)
    on = _run(iface, prob, cs, its, variant, collision_tallies=True)
    off = _run(iface, prob, cs, its, variant, spectrum=False, collision_tallies=True)
    _same_histories(on, off)


def _agree(runs):
    t0, c0 = runs[0]["track"], runs[0]["coll"]
    assert t0.sum() > 0.0
    for v in VARIANTS[1:]:
        assert _rel(runs[v]["track"], t0) <= 1e-12, (v, runs[v]["track"], t0)
        assert _rel(runs[v]["coll"], c0) <= 1e-12, (v, runs[v]["coll"], c0)


@gpu
@needs_gpu
@pytest.mark.parametrize("policy", ["auto", "checked"])
def test_variants_agree(iface, make_problem, cs, policy):
    prob, its = _problem(make_problem, "csp")
    if policy == "checked":
        iface.set_arithmetic(iface.ARITH_CHECKED)
    box = dense_box(prob.nx, prob.ny)
    _agree({v: _run(iface, prob, cs, its, v, box=box, flux=False) for v in VARIANTS})


@gpu
@needs_gpu
def test_variants_agree_with_a_true_vacuum(iface, make_problem, cs):
    """csp with its background at density 0 (cell_mfp = inf, the checked kernels run): the
    vacuum never collides, and the whole mesh's values agree"""
    prob, its = _problem(make_problem, "csp")
    prob.density[prob.density < 1.0e-20] = 0.0
    runs = {v: _run(iface, prob, cs, its, v, box=None) for v in VARIANTS}
    assert all(s.stats.checked_arithmetic == 1 for s in runs[0]["steps"])
    _agree(runs)
    r = runs[2]
    assert abs(r["track"].sum() - r["flux"].sum()) <= 1e-12 * r["flux"].sum()


@gpu
@needs_gpu
def test_variants_agree_with_requeues_queues_roulette_and_collision_tallies(iface, make_problem, cs,
                                                                           monkeypatch):
    """the collision stage time-sliced (NEUTRAL_K2_MAX_BLOCKS), the stream kernel's tile queues
    on, roulette and the collision tallies on at the same time: nothing lost, nothing doubled"""
    prob = make_problem("csp", nx=100, nparticles=100000, iterations=2, dt=1.0e-6)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    box = dense_box(prob.nx, prob.ny)
    sliced = {v: _run(iface, prob, cs, 2, v, box=box) for v in VARIANTS}
    assert sum(s.stats.requeued for s in sliced[2]["steps"]) > 0
    _agree(sliced)
    # (roulette shortens the chains: the slices then rarely end before them)
    kw = dict(box=box, collision_tallies=True, roulette=(0.25, 0.5))
    runs = {v: _run(iface, prob, cs, 2, v, **kw) for v in VARIANTS}
    assert sum(s.stats.roulette_killed for s in runs[2]["steps"]) > 0
    _agree(runs)
    iface.set_stream_queues(True)
    queued = _run(iface, prob, cs, 2, 2, **kw)
    assert _rel(queued["track"], runs[0]["track"]) <= 1e-12
    assert _rel(queued["coll"], runs[0]["coll"]) <= 1e-12
    for r in list(sliced.values()) + list(runs.values()) + [queued]:
        want = _box_sum(r["flux"], prob, box)
        assert abs(r["track"].sum() - want) <= 1e-12 * want


@gpu
@needs_gpu
def test_zero_tally_and_persistence(iface, make_problem, cs):
    """zero_tally() clears the spectrum; a refused call leaves the previous setting in force"""
    import torch
    prob, _ = _problem(make_problem, "scatter")
    sim = iface.Simulation(prob, *cs, variant=2, spectrum=(EDGES, None))
    sim.inject()
    sim.step(1)
    assert sim.spectrum_host()[0].sum() > 0
    sim.zero_tally()
    assert not sim.spectrum_host()[0].any() and not sim.spectrum_host()[1].any()
    sim.close()
    # library-level setting, persisting across steps
    out = torch.zeros(2 * (len(EDGES) - 1), dtype=torch.float64, device="cuda")
    iface.set_spectrum_tally(EDGES, None, out)
    with pytest.raises(ValueError):
        iface.set_spectrum_tally([2.0, 1.0], None, torch.zeros(2, dtype=torch.float64, device="cuda"))
    streaming, _ = _problem(make_problem, "stream")  # (alive through every step)
    plain = iface.Simulation(streaming, *cs, variant=2)
    plain.inject()
    plain.step(1)
    first = out.cpu().numpy().copy()
    assert first[:len(EDGES) - 1].sum() > 0
    plain.step(2)
    assert out.cpu().numpy()[:len(EDGES) - 1].sum() > first[:len(EDGES) - 1].sum()
    iface.set_spectrum_tally(None)
    plain.close()
    with pytest.raises(RuntimeError):
        plain.spectrum_host()


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


def _table(stdout):
    rows = re.findall(r"^Spectrum group (\d+) \[(\S+), (\S+)\) track (\S+) collision (\S+)$", stdout,
                      flags=re.M)
    return np.array([[float(x) for x in r[1:]] for r in rows])


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_and_two_ranks(tmp_path):
    """`neutral.hip --spectrum`: one line per group; without the flag stdout says nothing of it.
    Two ranks on one GPU -- shards of the particles (the on-device all-reduce) and blocks of the
    mesh (each rank its own cells) -- give the one-rank spectrum."""
    run, rel, sets = _driver_deck(tmp_path)
    plain = run_driver(run, rel, sets)
    assert "Spectrum" not in plain
    flag = ["--spectrum", ",".join(f"{e:.17g}" for e in EDGES) + "@51,51,77,77"]
    one = _table(run_driver(run, rel, sets + flag))
    assert one.shape == (len(EDGES) - 1, 4)
    assert np.allclose(one[:, 0], EDGES[:-1], rtol=1e-6) and one[:, 2].sum() > 0
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    for extra in ([], ["--decompose", "2x1"]):
        two = _table(run_driver(run, rel, sets + ["--gpus", "2"] + flag + extra, env))
        assert _rel(two[:, 2], one[:, 2]) <= 1e-12, (extra, two[:, 2], one[:, 2])
        assert _rel(two[:, 3], one[:, 3]) <= 1e-12, (extra, two[:, 3], one[:, 3])

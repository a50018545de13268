"""The optional tallies and Russian roulette of the HIP path against the CPU oracle's restatement
of their definitions (include/neutral_hip.h; oracle/neutral_oracle.c, itself pinned on the CPU by
tests/test_oracle_tallies.py): collisions, absorbed, Jx, Jy, the scalar flux and the energy tally
cell by cell, the spectrum's two estimators group by group, roulette's decisions one by one.

Bars -- none is new: event counts, cells, death flags, the collision counts and roulette's killed
and survived are exact; a mesh is held to TALLY_L2_TOL of tests/test_hip_parity.py (ocml's log and
sincos against glibc's, summation order) AND to the oracle's zero pattern, cell by cell (for the two
signed meshes, Jx and Jy, up to cells whose terms cancel: see compare()); a
spectrum value to 1e-9 of its estimator's largest, and exactly 0 where the oracle scored nothing;
roulette's weights lost and gained to TALLY_SUM_TOL; particle state to STATE_TOL, and a history
roulette ended holds weight exactly 0.0 on both sides.

Every case states what it is meant to exercise (`expect`), and that is asserted of the ORACLE's
run, so it holds whatever the kernels do; test_every_parity_case_exercises_what_it_is_meant_to
checks the same conditions for every case without a GPU."""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import pytest

import oracle_binding as ob
from gpu_support import gpu, iface, needs_gpu, rel  # noqa: F401


TALLY_L2_TOL = 1e-9       # tests/test_hip_parity.py
TALLY_SUM_TOL = 1e-10
STATE_TOL = 1e-9
SPECTRUM_TOL = 1e-9       # of the estimator's largest group

EVERYTHING = frozenset({"flux", "collision_tallies", "current", "spectrum"})
COLLIDES = frozenset({"roulette", "groups", "cells"})


@dataclass(frozen=True)
class Case:
    deck: str = "csp"
    nx: int = 64
    ny: int = 0                       # 0: square
    n: int = 8192
    steps: int = 3
    dt: Optional[float] = 1.0e-6
    roulette: Optional[Tuple[float, float]] = (0.25, 0.5)
    third: bool = False               # capture = scatter / 2: p_absorb = 1/3
    vacuum: bool = False              # the background at density 0
    uneven: bool = False              # the mesh of test_uneven_mesh_matches_oracle
    edges: str = "fine"
    box: str = "dense"
    zero_between: bool = False        # zero_tally() after every step but the last
    options: frozenset = EVERYTHING
    expect: frozenset = COLLIDES | {"reflection"}
    text: Optional[str] = None        # a deck of its own (the random family)
    edge_values: Optional[tuple] = None
    box_values: Optional[tuple] = None


def edges_of(case, e0):
    if case.edge_values is not None:
        return np.array(case.edge_values)
    return {
        # one wide group below (histories no roulette ends slow down to 1 eV), twelve fine ones
        "fine": lambda: np.concatenate([[0.5], e0 * np.geomspace(0.5, 1.02, 13)]),
        # the initial energy exactly on an edge: as a lower edge it is scored in that group ...
        "lower": lambda: np.concatenate([e0 * np.geomspace(0.5, 0.98, 8), [e0, 2.0 * e0]]),
        # ... as the last upper edge it is not scored at all
        "upper": lambda: np.concatenate([e0 * np.geomspace(0.5, 0.98, 8), [e0]]),
        "one": lambda: np.array([0.5, 2.0 * e0]),
        "64": lambda: np.concatenate([[0.5], e0 * np.geomspace(0.6, 1.02, 64)]),
        # part of the spectrum outside on both sides
        "outside": lambda: e0 * np.geomspace(0.8, 0.97, 7),
    }[case.edges]()


def box_of(case, prob):
    """global cells, half-open; None: the whole mesh"""
    nx, ny = prob.nx, prob.ny
    if case.box_values is not None:
        return case.box_values
    return {
        "mesh": None,
        # csp's dense square, cells [0.4 n, 0.6 n)
        "dense": (int(round(0.4 * nx)), int(round(0.4 * ny)), int(round(0.6 * nx)), int(round(0.6 * ny))),
        # borders on no multiple of 16: straddles tiles of every edge and the LDS windows over them
        "straddle": (nx // 13 + 1, ny // 9 + 2, (5 * nx) // 8 + 3, (3 * ny) // 5 - 1),
        "beyond": (nx // 3 + 1, ny // 3, nx + 50, 2 ** 31 - 1),
    }[case.box]


def problem_of(case, tmp_path):
    from neutral_amd import decks, host
    path = str(tmp_path / f"{case.deck}.params")
    if case.text is not None:
        with open(path, "w") as f:
            f.write(case.text)
    else:
        kw = dict(nx=case.nx, ny=case.ny or case.nx, nparticles=case.n, iterations=case.steps)
        if case.dt is not None:
            kw["dt"] = case.dt
        decks.write_deck(case.deck, path, **kw)
    prob = host.setup_problem(path, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    if case.vacuum:
        prob.density[prob.density < 1.0e-20] = 0.0
        assert (prob.density == 0.0).any()
    if case.uneven:
        tx, ty = np.linspace(0.0, 1.0, prob.nx + 1), np.linspace(0.0, 1.0, prob.ny + 1)
        prob.edgex[:] = prob.edgex[-1] * (0.7 * tx + 0.3 * tx * tx)   # monotone, uneven
        prob.edgey[:] = prob.edgey[-1] * (0.8 * ty + 0.2 * ty ** 3)
        prob.edgedx[:-1] = np.diff(prob.edgex)
        prob.edgedy[:-1] = np.diff(prob.edgey)
    return prob


def run_kwargs(case, prob, cs):
    """the keyword arguments OracleRun and Simulation share"""
    kw = dict(scalar_flux="flux" in case.options, collision_tallies="collision_tallies" in case.options,
              current="current" in case.options, roulette=case.roulette)
    if case.third:
        kw["cs_absorb"] = (cs[0].copy(), cs[1] * 0.5)
    spectrum = (edges_of(case, prob.initial_energy), box_of(case, prob)) if "spectrum" in case.options else None
    return kw, spectrum


def _collect(run, results, spectrum):
    out = dict(steps=results, tally=np.array(run.tally_host() if hasattr(run, "tally_host") else run.tally))
    for name in ("flux", "collisions", "absorbed", "jx", "jy"):
        a = getattr(run, name)
        out[name] = None if a is None else np.array(a.cpu().numpy() if hasattr(a, "cpu") else a).ravel()
    if spectrum is not None:
        out["track"], out["coll"] = spectrum
    return out


def oracle_run(case, prob, cs):
    """the oracle's side of a case, with what the case is meant to exercise asserted of it"""
    kw, spectrum = run_kwargs(case, prob, cs)
    # (the oracle always keeps the flux: it says which cells a segment was scored in)
    ref = ob.OracleRun(prob, *cs, spectrum=spectrum, **dict(kw, scalar_flux=True))
    ref.inject()
    results, reflected = [], 0
    for tt in range(1, case.steps + 1):
        before = {f: ref.particles.as_dict()[f].copy() for f in ("energy", "omega_x", "omega_y", "dead")}
        results.append(ref.step(tt))
        after = ref.particles.as_dict()
        # a history that kept its energy never scattered: its direction changes sign at a wall only
        straight = (before["dead"] == 0) & (after["energy"] == before["energy"])
        reflected += int(np.count_nonzero(straight & ((after["omega_x"] == -before["omega_x"]) |
                                                      (after["omega_y"] == -before["omega_y"]))))
        if case.zero_between and tt < case.steps:
            ref.zero_tally()
    out = _collect(ref, results, ref.spectrum_host() if spectrum is not None else None)
    out["scored"] = out["flux"]
    if "flux" not in case.options:
        out["flux"] = None
    out["parts"] = {f: a.copy() for f, a in ref.particles.as_dict().items()}
    out["reflected"] = reflected
    if "roulette" in case.expect:
        assert case.roulette is not None
        assert sum(s.roulette_killed for s in results) > 0 and sum(s.roulette_survived for s in results) > 0
    if "groups" in case.expect and spectrum is not None:
        need = min(3, len(spectrum[0]) - 1)
        assert np.count_nonzero(out["track"]) >= need and np.count_nonzero(out["coll"]) >= need, \
            (out["track"], out["coll"])
    if "cells" in case.expect:
        assert sum(s.collisions for s in results) > 0
        if out["collisions"] is not None:
            assert np.count_nonzero(out["collisions"]) > 1
    if "reflection" in case.expect:
        assert reflected > 0
    if "no_collisions" in case.expect:
        assert sum(s.collisions for s in results) == 0
    return out


# ---- the cases ----------------------------------------------------------------------------------

DECKS = {
    "csp": Case(),
    # (a mean free path of 1e-10 m far from the walls: nobody reflects)
    "scatter": Case(deck="scatter", n=4096, steps=2, dt=None, box="mesh", expect=COLLIDES),
    "split": Case(deck="split", steps=2, dt=5.0e-7, box="mesh"),
    "stream": Case(deck="stream", n=4096, steps=2, dt=None, box="mesh",
                   expect=frozenset({"reflection", "no_collisions"})),
}

CASES = {f"{deck}": c for deck, c in DECKS.items()}
CASES.update({
    "csp_vacuum": replace(DECKS["csp"], vacuum=True, box="mesh"),
    # weights that are no powers of two: generic operands for `absorbed`, roulette's comparison and
    # the collision estimator
    "third": replace(DECKS["csp"], third=True),
    "third_split": replace(DECKS["split"], third=True, roulette=(0.3, 0.9)),
    "non_square": replace(DECKS["csp"], nx=96, ny=40, box="straddle"),
    "uneven": replace(DECKS["csp"], nx=96, n=20000, uneven=True, box="straddle"),
    "edge_lower": replace(DECKS["csp"], edges="lower"),
    "edge_upper": replace(DECKS["csp"], edges="upper"),
    "edge_lower_stream": replace(DECKS["stream"], edges="lower"),
    "edge_upper_stream": replace(DECKS["stream"], edges="upper"),
    "one_group": replace(DECKS["csp"], edges="one"),
    "groups_64": replace(DECKS["split"], edges="64"),
    "outside": replace(DECKS["csp"], edges="outside", third=True),
    "every_absorption_plays": replace(DECKS["csp"], roulette=(0.75, 1.0)),
    "ws_equals_wc": replace(DECKS["split"], roulette=(0.5, 0.5)),
    "accumulates": replace(DECKS["csp"], steps=4, third=True, box="beyond"),
    "zeroed_between": replace(DECKS["csp"], steps=4, zero_between=True),
})
VARIANTS = (0, 1, 2)

# the same size and slicing as test_collision_stage_time_slicing_is_bitwise_neutral; no roulette,
# which would end the chains before a time slice does
SLICED = Case(nx=100, n=100000, steps=2, roulette=None, box="straddle", expect=frozenset({"groups", "cells", "reflection"}))
SLICED_ROULETTE = replace(SLICED, roulette=(0.25, 0.5), third=True, expect=COLLIDES | {"reflection"})
TILES = Case(nx=400, n=30000, steps=2, box="straddle")
TILES_BEYOND = replace(TILES, box="beyond")

RANDOM_SEEDS = 32
ROULETTE_PAIRS = ((0.25, 0.5), (0.75, 1.0), (0.5, 0.5), (0.1, 0.3), (0.3, 0.9))


def random_case(seed):
    """A second family of decks nobody tuned for, after _random_deck_text of tests/test_hip_parity.py:
    a source inside a dense box (so that every deck collides from its first step), up to two more
    boxes, a mesh that need not be square; and drawn with it which options are on, the spectrum's
    box and edges, the roulette pair, the tables, the variant, the policy and the K2 grid."""
    rng = np.random.default_rng(91000 + seed)
    nx, ny = int(rng.integers(20, 200)), int(rng.integers(20, 200))
    sw, sh = (float(v) for v in rng.uniform(0.1, 0.5, 2))
    sx, sy = float(rng.uniform(0.0, 1.0 - sw)), float(rng.uniform(0.0, 1.0 - sh))
    lines = [f"source xpos={sx!r} ypos={sy!r} width={sw!r} height={sh!r}",
             "problem_0 density=1e-30 energy=0.0 xpos=0.0 ypos=0.0 width=1.0 height=1.0"]
    m = [float(v) for v in rng.uniform(0.02, 0.2, 4)]
    bx, by = max(0.0, sx - m[0]), max(0.0, sy - m[1])
    bw, bh = min(1.0, sx + sw + m[2]) - bx, min(1.0, sy + sh + m[3]) - by
    lines.append(f"problem_1 density={float(10.0 ** rng.uniform(0, 4))!r} energy=1.0 xpos={bx!r} ypos={by!r} "
                 f"width={bw!r} height={bh!r}")
    for i in range(int(rng.integers(0, 3))):
        w, h = (float(v) for v in rng.uniform(0.05, 0.7, 2))
        x, y = float(rng.uniform(0.0, 1.0 - w)), float(rng.uniform(0.0, 1.0 - h))
        lines.append(f"problem_{i + 2} density={float(10.0 ** rng.uniform(-2, 4))!r} energy=1.0 xpos={x!r} "
                     f"ypos={y!r} width={w!r} height={h!r}")
    n = int(rng.integers(500, 12000))
    e0 = float(10.0 ** rng.uniform(2.5, 6))
    dt = float(10.0 ** rng.uniform(-8, -6.3))
    steps = int(rng.integers(1, 4))
    lines += [f"nparticles {n}", f"initial_energy {e0!r}", f"dt {dt!r}", f"nx {nx}", f"ny {ny}",
              f"iterations {steps}", "visit_dump 0"]
    names = sorted(EVERYTHING) + ["roulette"]
    on = {name for name in names if rng.random() < 0.7}
    if not on:
        on = {names[int(rng.integers(0, len(names)))]}
    roulette = ROULETTE_PAIRS[int(rng.integers(0, len(ROULETTE_PAIRS)))] if "roulette" in on else None
    # the box holds the middle half of the source box at least (where the histories start, and in
    # the denser decks stay), and may reach beyond the mesh
    lo_x, lo_y = int((sx + 0.25 * sw) * nx), int((sy + 0.25 * sh) * ny)
    hi_x, hi_y = int((sx + 0.75 * sw) * nx) + 1, int((sy + 0.75 * sh) * ny) + 1
    box = (int(rng.integers(0, lo_x + 1)), int(rng.integers(0, lo_y + 1)),
           int(rng.integers(hi_x, nx + 9)), int(rng.integers(hi_y, ny + 9)))
    ngroups = int(rng.integers(8, 65))
    hi = 1.0 if rng.random() < 0.25 else float(rng.uniform(0.99, 1.2))
    edges = tuple(e0 * np.geomspace(float(rng.uniform(0.3, 0.7)), hi, ngroups + 1))
    expect = {"cells", "groups"} | ({"roulette"} if roulette else set())
    case = Case(deck=f"random{seed}", steps=steps, roulette=roulette, third=bool(rng.random() < 0.5),
                options=frozenset(on - {"roulette"}), expect=frozenset(expect), text="\n".join(lines) + "\n",
                edge_values=edges, box_values=box)
    variant = int(rng.integers(0, 3))
    checked = bool(rng.random() < 0.3)
    blocks = [None, 1, 3, 16][int(rng.integers(0, 4))]
    return case, variant, checked, blocks


# ---- the comparison -----------------------------------------------------------------------------

def gpu_run(iface, case, prob, cs, variant):
    kw, spectrum = run_kwargs(case, prob, cs)
    out_tensor = None
    box = spectrum[1] if spectrum is not None else None
    beyond = box is not None and (box[2] > prob.nx or box[3] > prob.ny)
    if beyond:
        # Simulation keeps its box inside the mesh; the library takes one that reaches beyond it
        import torch
        sim = iface.Simulation(prob, *cs, variant=variant, **kw)
        out_tensor = torch.zeros(2 * (len(spectrum[0]) - 1), dtype=torch.float64, device=sim.device)
        iface.set_spectrum_tally(spectrum[0], box, out_tensor)
    else:
        sim = iface.Simulation(prob, *cs, variant=variant, spectrum=spectrum, **kw)
    try:
        sim.inject()
        results = []
        for tt in range(1, case.steps + 1):
            results.append(sim.step(tt))
            assert results[-1].stats.aborted == 0
            if case.zero_between and tt < case.steps:
                sim.zero_tally()
                if out_tensor is not None:
                    out_tensor.zero_()
        if out_tensor is not None:
            v = out_tensor.cpu().numpy()
            spec = (v[:len(v) // 2].copy(), v[len(v) // 2:].copy())
        else:
            spec = sim.spectrum_host() if spectrum is not None else None
        out = _collect(sim, results, spec)
        out["parts"] = sim.particle_arrays()
    finally:
        iface.set_spectrum_tally(None)
        sim.close()
    return out


def compare(got, want, what=""):
    for tt, (g, c) in enumerate(zip(got["steps"], want["steps"]), 1):
        assert (g.nprocessed, g.facets, g.collisions, g.census) == \
            (c.nprocessed, c.facets, c.collisions, c.census), (what, tt)
        s = g.stats
        assert (s.roulette_killed, s.roulette_survived) == (c.roulette_killed, c.roulette_survived), (what, tt)
        for a, b in ((s.roulette_weight_lost, c.roulette_weight_lost),
                     (s.roulette_weight_gained, c.roulette_weight_gained)):
            print(f"{what} step {tt}: roulette weight {a!r} against {b!r}")
            assert abs(a - b) <= TALLY_SUM_TOL * abs(b), (what, tt, a, b)
    gp, cp = got["parts"], want["parts"]
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(gp[f], cp[f]), (what, f)
    # a history roulette ended holds weight exactly 0.0, on both sides the same histories
    assert np.array_equal(gp["weight"] == 0.0, cp["weight"] == 0.0), what
    for f in ("energy", "weight", "dt_to_census", "x", "y"):
        assert rel(gp[f], cp[f]) < STATE_TOL, (what, f)
    for f in ("omega_x", "omega_y"):
        assert np.max(np.abs(gp[f] - cp[f])) < STATE_TOL, (what, f)
    if want["collisions"] is not None:
        assert np.array_equal(got["collisions"], want["collisions"]), what
    for name in ("tally", "flux", "absorbed", "jx", "jy"):
        g, c = got[name], want[name]
        if c is None:
            continue
        norm = np.linalg.norm(c)
        l2 = np.linalg.norm(g - c) / norm if norm > 0.0 else 0.0
        print(f"{what} {name}: L2 {l2:.3e}, {np.count_nonzero(c)} cells")
        assert l2 < TALLY_L2_TOL, (what, name, l2)
        differ = (g == 0.0) != (c == 0.0)
        if name in ("jx", "jy"):
            # A signed sum: a history that a wall sends back through the cells it came by scores
            # +a and -a there, which cancel to exactly 0 or to a last-bit residue as the roundings
            # fall (the random family's seed 11 has nine such cells).  So: nothing where no segment
            # was scored at all (the oracle's flux is 0 there), and where the patterns differ in a
            # scored cell, the value that is not 0 is such a residue -- below the bar for a mesh,
            # of that cell's flux.
            scored = want["scored"]
            assert not g[scored == 0.0].any(), (what, name)
            assert np.all(np.abs(g - c)[differ] <= TALLY_L2_TOL * scored[differ]), (what, name)
        else:
            assert not differ.any(), (what, name)
    if "track" in want:
        for est in ("track", "coll"):
            g, c = got[est], want[est]
            scale = np.abs(c).max()
            print(f"{what} {est}: worst {np.abs(g - c).max() / scale if scale > 0 else 0.0:.3e}, "
                  f"{np.count_nonzero(c)} groups of {len(c)}")
            assert np.all(np.abs(g - c) <= SPECTRUM_TOL * scale), (what, est, g, c)
            assert not g[c == 0.0].any(), (what, est, g, c)


# ---- CPU: every case exercises what it is meant to, before any kernel is asked ----------------------

def test_every_parity_case_exercises_what_it_is_meant_to(cs, tmp_path):
    """oracle_run asserts each case's `expect` of the oracle's own run: roulette killed and kept
    someone, three groups or more were scored by each estimator, more than one cell collided, a
    history turned round at a wall.  All the named cases and all 32 random decks."""
    named = dict(CASES, sliced=SLICED, sliced_roulette=SLICED_ROULETTE, tiles=TILES, tiles_beyond=TILES_BEYOND,
                 sliced_lower=replace(SLICED_ROULETTE, edges="lower", box="dense"),
                 sliced_upper=replace(SLICED_ROULETTE, edges="upper", box="dense"))
    for name, case in named.items():
        oracle_run(case, problem_of(case, tmp_path), cs)
    for seed in range(RANDOM_SEEDS):
        case = random_case(seed)[0]
        oracle_run(case, problem_of(case, tmp_path), cs)
    # the two edge cases are what they say: the initial energy IS an edge
    prob = problem_of(CASES["edge_lower"], tmp_path)
    assert prob.initial_energy in edges_of(CASES["edge_lower"], prob.initial_energy)[1:-1]
    assert edges_of(CASES["edge_upper"], prob.initial_energy)[-1] == prob.initial_energy
    low = oracle_run(CASES["edge_lower_stream"], problem_of(CASES["edge_lower_stream"], tmp_path), cs)
    assert np.count_nonzero(low["track"]) == 1 and low["track"][-1] > 0.0
    up = oracle_run(CASES["edge_upper_stream"], problem_of(CASES["edge_upper_stream"], tmp_path), cs)
    assert not up["track"].any()


# ---- GPU ----------------------------------------------------------------------------------------

_ORACLE = {}


def _want(name, case, prob, cs):
    if name not in _ORACLE:
        _ORACLE[name] = oracle_run(case, prob, cs)
    return _ORACLE[name]


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(iface, cs, tmp_path, monkeypatch, name, variant):
    case = CASES[name]
    prob = problem_of(case, tmp_path)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")   # small decks under windows too
    want = _want(name, case, prob, cs)
    got = gpu_run(iface, case, prob, cs, variant)
    if case.vacuum:
        assert all(s.stats.checked_arithmetic == 1 for s in got["steps"])
    compare(got, want, f"{name} variant {variant}")


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["csp", "third"])
def test_case_matches_oracle_under_the_checked_policy(iface, cs, tmp_path, monkeypatch, name, variant):
    case = CASES[name]
    prob = problem_of(case, tmp_path)
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    want = _want(name, case, prob, cs)
    iface.set_arithmetic(iface.ARITH_CHECKED)
    got = gpu_run(iface, case, prob, cs, variant)
    assert all(s.stats.checked_arithmetic == 1 for s in got["steps"])
    compare(got, want, f"{name} checked variant {variant}")


@gpu
@needs_gpu
def test_time_sliced_collision_stage_and_tile_queues_match_oracle(iface, cs, tmp_path, monkeypatch):
    """histories set aside in the middle of their collision chains (requeued > 0) carry every
    pending score along; then roulette beside it, and the stream kernel's tile queues on"""
    prob = problem_of(SLICED, tmp_path)
    want = oracle_run(SLICED, prob, cs)
    monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", "4")
    got = gpu_run(iface, SLICED, prob, cs, 2)
    assert sum(s.stats.requeued for s in got["steps"]) > 0
    compare(got, want, "sliced")
    want = oracle_run(SLICED_ROULETTE, prob, cs)
    for variant in (1, 2):
        compare(gpu_run(iface, SLICED_ROULETTE, prob, cs, variant), want, f"sliced, roulette, variant {variant}")
    iface.set_stream_queues(True)
    compare(gpu_run(iface, SLICED_ROULETTE, prob, cs, 2), want, "sliced, roulette, tile queues")
    iface.set_stream_queues(False)
    # lanes that take up one history after another meet the initial energy with another group's
    # scores pending: the edge exactly at it, as a lower edge and as the last upper edge
    for edges in ("lower", "upper"):
        case = replace(SLICED_ROULETTE, edges=edges, box="dense")
        want = oracle_run(case, prob, cs)
        for variant in (1, 2):
            compare(gpu_run(iface, case, prob, cs, variant), want, f"sliced, edges {edges}, variant {variant}")
    iface.set_stream_queues(True)
    monkeypatch.delenv("NEUTRAL_K2_MAX_BLOCKS")
    compare(gpu_run(iface, SLICED_ROULETTE, prob, cs, 2), oracle_run(SLICED_ROULETTE, prob, cs),
            "roulette, tile queues")


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", [16, 32, 64, 128])
def test_tile_edges_match_oracle(iface, cs, tmp_path, monkeypatch, tile):
    """tiles of every edge under the LDS windows, histories changing windows, a spectrum box that
    straddles tile and window borders and one that reaches beyond the mesh"""
    monkeypatch.setenv("NEUTRAL_TILE_CELLS", str(tile))
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    for name, case in (("tiles", TILES), ("tiles_beyond", TILES_BEYOND)):
        prob = problem_of(case, tmp_path)
        want = _want(name, case, prob, cs)
        got = gpu_run(iface, case, prob, cs, 2)
        assert max(s.stats.stream_passes for s in got["steps"]) > 1   # histories did change windows
        compare(got, want, f"{name} tile {tile}")


@gpu
@needs_gpu
@pytest.mark.parametrize("seed", range(RANDOM_SEEDS))
def test_random_decks_match_oracle(iface, cs, tmp_path, monkeypatch, seed):
    case, variant, checked, blocks = random_case(seed)
    prob = problem_of(case, tmp_path)
    if blocks is not None:
        monkeypatch.setenv("NEUTRAL_K2_MAX_BLOCKS", str(blocks))
    if checked:
        iface.set_arithmetic(iface.ARITH_CHECKED)
    want = oracle_run(case, prob, cs)
    got = gpu_run(iface, case, prob, cs, variant)
    compare(got, want, f"seed {seed} variant {variant} {sorted(case.options)} roulette {case.roulette}")

"""Degenerate geometry against the oracle: beams, edges, corners.

Every other run that the suite compares with the oracle starts from injection's random positions
and angles, where a direction cosine that is exactly zero, a start exactly on a cell's edge or
corner, and a flight with dt_x == dt_y through a cell's corner all have measure zero.  These are
the inputs where the kernels stop being straight-line arithmetic (the wave-wide vote of
refresh_direction_plain_or_wrapped, the third case of aim_targets, an infinite reciprocal that a
reflection flips by sign, the tie rule dt_x < dt_y of calc_distance_to_targets, two tile edges
crossed a distance of about 0 apart), and since the described source takes theta_width == 0 and
width == height == 0 a user reaches them in one line of a source file.

tests/degenerate_states.py builds the starts.  CPU (not marked gpu): the corpus is what it claims;
the oracle, the Python replay and a closed form that neither is part of agree among themselves on
it.  GPU: every kernel variant and both arithmetic policies take the oracle's decisions on it, at
the bars of tests/test_hip_parity.py; beams and point sources come out of the described source as
described and run like the oracle's.

Two statements about the corpus that one might expect do not hold, and the tests below assert
what does (test_the_corpus_is_what_it_claims):
  * no row of the corpus has a NaN facet time.  A NaN needs 0 * inf: a zero cosine on an axis
    whose target is where the history already is.  The zero cosines are +0.0, so that axis aims at
    the cell's UPPER edge, and no placement sits on an upper edge.  The 0 * inf decision is tested
    where it can be made to happen, on the device function itself
    (tests/test_hip_parity.py::test_distance_to_facet_matches_oracle: the upper-edge rows);
  * the exact ties are 3/32 of the corpus, not 1/8: of the (s, s) histories those that start on
    the middle of a left edge are a whole cell from the x facet and half a cell from the y facet.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import closed_form
import degenerate_states as ds
import oracle_binding as ob
import replay
from gpu_support import allowed_tile, gpu, iface, l2_of_nonzero, needs_gpu, rel  # noqa: F401

N = 4096
STEPS = 2
W, E, S, NORTH = replay.WEST, replay.EAST, replay.SOUTH, replay.NORTH

# the bars of tests/test_hip_parity.py
TALLY_L2_TOL = 1e-9
STATE_TOL = 1e-9
MESH_TOL = 1e-9            # flux and current: tests/test_scalar_flux.py, tests/test_current.py

OPEN_BOUND_CORRECTION = 1.0e-13   # oracle/neutral_oracle.h, neutral_data.h

# The closed form of the axis beams (closed_form.unfolded_beam) leaves out the open-bound
# correction and the rounding of every landing, so the oracle itself is some way from it.
# Measured on the oracle, two steps, 1024 histories (256 per direction) from cell (5, 9) --
# another cell and another count than the tests' beams -- and asserted at ten times that:
#                                                  64^2       48^2
#   largest per-cell relative flux error           4.7e-12    3.6e-12
#   Jx, Jy error against the largest |Jx|, |Jy|    1.3e-11    9.6e-12
# (test_the_oracles_own_distance_from_the_closed_form measures them again and prints them.)
# A dropped segment costs a cell 1e-2 of its flux and more: four orders above the bars.
BEAM_CALIBRATION = dict(cell=(5, 9), n=256)
BEAM_MEASURED = {64: dict(flux=4.7e-12, current=1.3e-11), 48: dict(flux=3.6e-12, current=9.6e-12)}
BEAM_FLUX_TOL = {nx: 10.0 * m["flux"] for nx, m in BEAM_MEASURED.items()}
BEAM_CURRENT_TOL = {nx: 10.0 * m["current"] for nx, m in BEAM_MEASURED.items()}
BEAM_CELL = (37, 22)       # the tests' beams: 1024 histories per direction from here


def _deck(make_problem, name, nx, n=N):
    kw = dict(nx=nx, nparticles=n, iterations=STEPS)
    if name == "csp":
        kw["dt"] = 1.0e-6
    return make_problem(name, **kw)


def _uneven(prob):
    """the edges of tests/test_hip_parity.py::test_uneven_mesh_matches_oracle: not the host
    layer's formula, so the stream kernel loads them"""
    t = np.linspace(0.0, 1.0, prob.nx + 1)
    prob.edgex[:] = prob.edgex[-1] * (0.7 * t + 0.3 * t * t)
    prob.edgey[:] = prob.edgey[-1] * (0.8 * t + 0.2 * t ** 3)
    prob.edgedx[:-1] = np.diff(prob.edgex)
    prob.edgedy[:-1] = np.diff(prob.edgey)
    return prob


def _events(r):
    return (r.nprocessed, r.facets, r.collisions, r.census)


def _oracle_run(prob, cs, states, steps=STEPS, full=None, **opts):
    """the oracle from `states` (or, full: all eleven fields as given); -> dict of the steps' event
    counts, the final particle arrays and the meshes"""
    ref = ob.OracleRun(prob, *cs, **opts)
    ref.inject()
    if full is not None:
        for f, a in ref.particles.as_dict().items():
            a[:] = full[f]
    else:
        ds.into_oracle(ref, states)
    start = {f: a.copy() for f, a in ref.particles.as_dict().items()}
    events = [_events(ref.step(tt)) for tt in range(1, steps + 1)]
    out = dict(events=events, start=start, parts={f: a.copy() for f, a in ref.particles.as_dict().items()},
               tally=ref.tally.copy(), flux=None if ref.flux is None else ref.flux.copy(),
               collisions=None if ref.collisions is None else ref.collisions.copy(),
               absorbed=None if ref.absorbed is None else ref.absorbed.copy())
    if ref.jx is not None:
        out["jx"], out["jy"] = ref.jx.copy(), ref.jy.copy()
    return out


# ---- CPU: the corpus -------------------------------------------------------------------------

def _facet_times(prob, st):
    """dt_x, dt_y of oracle/neutral_oracle.c: orc_calc_distance_to_facet for every row, the same
    operations in numpy; and the distance and facet they imply"""
    speed = replay.speed_of(prob.initial_energy)
    ex, ey = (np.asarray(e, dtype=np.float64) for e in (prob.edgex, prob.edgey))
    cx, cy = st["cellx"] + prob.pad, st["celly"] + prob.pad
    with np.errstate(divide="ignore", invalid="ignore"):
        ux, uy = 1.0 / (st["omega_x"] * speed), 1.0 / (st["omega_y"] * speed)
        ax = np.where(st["omega_x"] >= 0.0, ex[cx + 1], ex[cx] - OPEN_BOUND_CORRECTION) - st["x"]
        ay = np.where(st["omega_y"] >= 0.0, ey[cy + 1], ey[cy] - OPEN_BOUND_CORRECTION) - st["y"]
        dt_x, dt_y = ax * ux, ay * uy
        x_facet = dt_x < dt_y
        distance = np.where(x_facet, ax * speed * ux, ay * speed * uy)
    return dt_x, dt_y, x_facet.astype(np.int32), distance


def _oracle_facets(prob, st):
    """orc_calc_distance_to_facet itself, row by row"""
    speed = replay.speed_of(prob.initial_energy)
    ex = np.ascontiguousarray(prob.edgex, dtype=np.float64)
    ey = np.ascontiguousarray(prob.edgey, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    n = len(st["x"])
    dist, xf = np.zeros(n), np.zeros(n, dtype=np.int32)
    d, x = C.c_double(), C.c_int()
    for i in range(n):
        ob.lib().orc_calc_distance_to_facet(st["x"][i], st["y"][i], prob.pad, 0, 0, st["omega_x"][i], st["omega_y"][i],
                                            speed, int(st["cellx"][i]), int(st["celly"][i]), C.byref(d), C.byref(x),
                                            ex.ctypes.data_as(dp), ey.ctypes.data_as(dp))
        dist[i], xf[i] = d.value, x.value
    return dist, xf


def test_the_corpus_is_what_it_claims(make_problem):
    """At the first event, with the oracle's own distance to the facet: the oracle's facet is the
    tie rule's (dt_x < dt_y, so a tie and a NaN go to the y facet) and its distance the same bits,
    on every row -- this is the assertion that fails when the oracle's `<` is made `<=` -- and the
    corpus holds the exact ties, infinite times and near ties it is there for."""
    i = np.arange(N)
    diagonal = ds.direction_of(i) == 4                      # (s, s)
    off_edge = ds.placement_of(i) != ds.LEFT_EDGE
    prob = _deck(make_problem, "stream", 64)
    st = ds.corpus(prob, N)
    dt_x, dt_y, x_facet, distance = _facet_times(prob, st)
    dist, xf = _oracle_facets(prob, st)
    assert np.array_equal(xf, x_facet)
    assert np.array_equal(dist.view(np.uint64), distance.view(np.uint64))
    ties = dt_x == dt_y
    infinite = np.isinf(dt_x) | np.isinf(dt_y)
    nan = np.isnan(dt_x) | np.isnan(dt_y)
    print(f"64^2: {int(ties.sum())} exact ties, {int(infinite.sum())} infinite, {int(nan.sum())} NaN of {N}")
    # square cells with power-of-two edges: every (s, s) history from a centre or a corner ties
    # to the bit, 3/4 of 1/8 of the corpus; from the middle of a left edge dt_x = 2 dt_y
    assert np.array_equal(ties, diagonal & off_edge) and ties.sum() == 3 * N // 32
    assert not xf[ties].any()                               # a tie is the y facet's
    # the four axis directions: one zero cosine each, one infinite time
    assert np.array_equal(infinite, ds.direction_of(i) < 4) and infinite.sum() >= N // 4
    # no NaN: see the module's text -- and nothing negative either
    assert not nan.any()
    assert np.all(dist >= 0.0) and np.isfinite(dist).all()
    # on-edge starts that leave at once: towards -x from a left edge, 1e-13 m to fly
    at_once = (ds.placement_of(i) >= ds.CORNER) & (st["omega_x"] < 0.0)
    assert at_once.any() and np.all(dist[at_once] < 2.0 * OPEN_BOUND_CORRECTION) and np.all(dist[at_once] > 0.0)

    # 48^2: the edges are no binary fractions, exact ties become near ties
    prob = _deck(make_problem, "stream", 48)
    st = ds.corpus(prob, N)
    dt_x, dt_y, x_facet, distance = _facet_times(prob, st)
    dist, xf = _oracle_facets(prob, st)
    assert np.array_equal(xf, x_facet)
    assert np.array_equal(dist.view(np.uint64), distance.view(np.uint64))
    near = diagonal & off_edge
    diff = np.abs(dt_x[near] - dt_y[near])
    ulps = diff / np.spacing(np.maximum(dt_x[near], dt_y[near]))
    print(f"48^2: of {int(near.sum())} near ties {int((diff == 0).sum())} exact, largest difference "
          f"{ulps.max():.1f} ulp, median {np.median(ulps):.1f} ulp; both facets taken: "
          f"{int(xf[near].sum())} x, {int((1 - xf[near]).sum())} y")
    # Both ideal differences are half a cell (a whole one from a corner).  Each is off by the
    # rounding of two edges and of the centre, at most 2^-54 each below 1 m, and the subtraction
    # is exact (Sterbenz) or within 2^-54 again: the two differ by at most 8 * 2^-54 = 2^-51 m,
    # 5e-14 of half a cell of 1/48 m -- a few hundred ulps of a time at the very most, nowhere
    # near the half of it that the next facet is away.
    half_cell = 0.5 / 48
    assert np.all(diff <= 2.0 ** -51 / half_cell * np.maximum(dt_x[near], dt_y[near]) * (1.0 + 1e-9))
    assert (diff != 0).sum() > diagonal.sum() // 2          # most of the (s, s) histories
    assert xf[near].any() and not xf[near].all()            # rounding decides, both ways


# ---- CPU: the oracle equals the replay -------------------------------------------------------

@pytest.mark.parametrize("name", ["stream", "csp"])
def test_oracle_equals_the_replay_on_the_corpus(make_problem, cs, name):
    """Every 16th history of the corpus -- which is direction (1, 0) at a centre or a corner --
    and histories 0, 97, 194 ... 3007, one of every direction and placement: each as a run of the
    oracle on that history alone (same id, so same random numbers), two steps, against the Python
    replay.  Event for event: facets and collisions per history and step; the fields of
    replay.FIELDS by bits after the last step; the same bits as the oracle's run of the whole
    corpus.  Wall hits the oracle does not count: the replay's are held to what its own outflow
    says, and for the beams from a cell's centre on the stream deck to the unfolded path."""
    prob = _deck(make_problem, name, 64)
    st = ds.corpus(prob, N)
    whole = _oracle_run(prob, cs, st)
    sample = sorted(set(range(0, N, 16)) | set(range(0, 32 * 97, 97)))
    assert {int(d) for d in ds.direction_of(sample)} == set(range(8))
    assert {(int(d), int(p)) for d, p in zip(ds.direction_of(sample), ds.placement_of(sample))} == \
        {(d, p) for d in range(8) for p in range(4)}
    rep = replay.Replay(prob, cs, fused=True)    # (rounds where the oracle's build rounds: the same bits)
    speed = replay.speed_of(prob.initial_energy)
    hits_so_far = {}   # per history: wall hits of the unfolded path up to this step, up to the one before
    for pid in sample:
        one = ob.OracleRun(prob, *cs, shard=(pid, 1))
        one.inject()
        ds.into_oracle(one, {f: a[pid:pid + 1] for f, a in st.items()})
        replayed = replay.run_steps(rep, dict(one.particles.as_dict(), id=[pid]), STEPS)   # (before the oracle steps)
        (s,) = replayed["states"]
        for tt, grew in enumerate(replayed["per_step"], 1):
            r = one.step(tt)
            assert (r.facets, r.collisions) == (grew["facets"], grew["collisions"]), (pid, tt)
            if name == "stream" and ds.direction_of(pid) < 4 and ds.placement_of(pid) <= ds.CENTRE_AGAIN:
                # (the steps' paths are one path: nothing but the census interrupts it)
                along_x = ds.direction_of(pid) % 2 == 0
                edges = prob.edgex if along_x else prob.edgey
                sign = 1 if ds.direction_of(pid) < 2 else -1
                _, _, low, high, gap = closed_form.unfolded_beam(
                    edges, st["x" if along_x else "y"][pid], sign, Fraction(speed) * Fraction(prob.dt) * tt)
                assert gap > 1e-9
                hits_so_far[pid] = low[0] + high[-1], hits_so_far.get(pid, (0, 0))[0]
                assert grew["wall_hits"] == hits_so_far[pid][0] - hits_so_far[pid][1], (pid, tt)
        end = one.particles.as_dict()
        for f in replay.FIELDS:
            mine, theirs, whole_run = np.array([s[f]]), end[f][:1], whole["parts"][f][pid:pid + 1]
            assert mine.astype(theirs.dtype).tobytes() == theirs.tobytes() == whole_run.tobytes(), (pid, f)
    out_sum = rep.out.sum()
    print(f"{name}: {len(sample)} histories, {rep.nfacets} facets, {rep.ncollisions} collisions, "
          f"{rep.wall_hits} wall hits")
    assert rep.nfacets > 50 * len(sample) and rep.wall_hits > 0
    assert (rep.ncollisions > 0) == (name == "csp")
    if name == "stream":   # every weight 1: the outflow counts the events, the boundary sides the wall hits
        import outflow_reference as orf
        assert np.all(whole["parts"]["weight"] == 1.0)
        assert round(N * out_sum) == rep.nfacets and round(N * orf.wall_hits(rep.out)) == rep.wall_hits
    # the corpus stays sane in the oracle, and the axis-aligned histories of the stream deck stay so
    for f in ob.F64_FIELDS:
        assert np.isfinite(whole["parts"][f]).all(), f
    assert whole["parts"]["cellx"].min() >= 0 and whole["parts"]["cellx"].max() < prob.nx
    assert whole["parts"]["celly"].min() >= 0 and whole["parts"]["celly"].max() < prob.ny
    assert [e[0] for e in whole["events"]][0] == N
    if name == "stream":
        axis = ds.direction_of(np.arange(N)) < 4
        assert np.all((whole["parts"]["omega_x"][axis] == 0.0) != (whole["parts"]["omega_y"][axis] == 0.0))
        assert all(e[2] == 0 and e[3] == N for e in whole["events"])


# ---- the axis beams in closed form -----------------------------------------------------------

def _beam_closed_form(prob, cell, n):
    """what 4 n histories of weight 1 -- n along each axis direction from the centre of `cell` --
    leave on the meshes in STEPS steps, from closed_form.unfolded_beam: flux, jx, jy as (ny, nx)
    arrays of Fractions' floats and the crossing COUNTS by side, (4, ny, nx) integers"""
    cx, cy = cell
    total = 4 * n
    speed = replay.speed_of(prob.initial_energy)
    length = Fraction(speed) * Fraction(prob.dt) * STEPS
    ex, ey = (np.asarray(e, dtype=np.float64) for e in (prob.edgex, prob.edgey))
    x0 = Fraction(0.5 * (ex[cx] + ex[cx + 1]))
    y0 = Fraction(0.5 * (ey[cy] + ey[cy + 1]))
    flux = [[Fraction(0)] * prob.nx for _ in range(prob.ny)]
    jx = [[Fraction(0)] * prob.nx for _ in range(prob.ny)]
    jy = [[Fraction(0)] * prob.nx for _ in range(prob.ny)]
    counts = np.zeros((4, prob.ny, prob.nx), dtype=np.int64)
    for sign in (1, -1):
        track, signed, low, high, gap = closed_form.unfolded_beam(ex, x0, sign, length)
        assert gap > 1e-6 * float(ex[1] - ex[0]), "the path ends on an edge: choose another cell"
        for c in range(prob.nx):
            flux[cy][c] += track[c] * n / total
            jx[cy][c] += signed[c] * n / total
            counts[W, cy, c] += low[c] * n
            counts[E, cy, c] += high[c] * n
        track, signed, low, high, gap = closed_form.unfolded_beam(ey, y0, sign, length)
        assert gap > 1e-6 * float(ey[1] - ey[0]), "the path ends on an edge: choose another cell"
        for c in range(prob.ny):
            flux[c][cx] += track[c] * n / total
            jy[c][cx] += signed[c] * n / total
            counts[S, c, cx] += low[c] * n
            counts[NORTH, c, cx] += high[c] * n
    as_array = lambda m: np.array([[float(v) for v in row] for row in m])  # noqa: E731
    return dict(flux=as_array(flux), jx=as_array(jx), jy=as_array(jy), counts=counts)


def _beam_errors(want, flux, jx, jy):
    """(largest per-cell relative flux error over the cells the closed form touches, largest Jx or
    Jy error against the largest |Jx|, |Jy| of the closed form)"""
    flux, jx, jy = (np.asarray(a).reshape(want["flux"].shape) for a in (flux, jx, jy))
    touched = want["flux"] != 0.0
    flux_err = float(np.max(np.abs(flux[touched] - want["flux"][touched]) / want["flux"][touched]))
    current_err = max(float(np.max(np.abs(got - w)) / np.max(np.abs(w))) for got, w in ((jx, want["jx"]), (jy, want["jy"])))
    return flux_err, current_err


def _check_beams(want, flux, jx, jy, counts, nx, who):
    """(a), (b), (c) of the closed form"""
    flux = np.asarray(flux).reshape(want["flux"].shape)
    assert np.array_equal(flux != 0.0, want["flux"] != 0.0), who                # (a)
    assert np.array_equal(np.asarray(counts), want["counts"]), who               # (b)
    flux_err, current_err = _beam_errors(want, flux, jx, jy)                     # (c)
    print(f"{who} {nx}^2: flux {flux_err:.2e} (bar {BEAM_FLUX_TOL[nx]:.1e}), "
          f"current {current_err:.2e} (bar {BEAM_CURRENT_TOL[nx]:.1e})")
    assert flux_err <= BEAM_FLUX_TOL[nx], who
    assert current_err <= BEAM_CURRENT_TOL[nx], who


def _replayed_counts(prob, cs, st, n):
    """the crossings of each side of each cell as replay.Replay.out counts them: one history of
    each beam replayed (the oracle's run shows that a beam's histories are identical), times n"""
    rep = replay.Replay(prob, cs)
    for pid in range(0, 4 * n, n):
        one = dict({f: st[f][pid:pid + 1] for f in st}, energy=np.array([prob.initial_energy]), weight=np.array([1.0]),
                   dead=np.array([0]), id=[pid])
        replay.run_steps(rep, one, STEPS)
    assert rep.ncollisions == 0
    counts = rep.out * prob.nparticles            # (1/N each, N a power of two: exact)
    assert np.array_equal(counts, np.round(counts))
    return counts.astype(np.int64) * n


@pytest.mark.parametrize("nx", [64, 48])
def test_the_oracles_own_distance_from_the_closed_form(make_problem, cs, nx):
    """the measurement behind BEAM_FLUX_TOL and BEAM_CURRENT_TOL, on the calibration beams: it
    still gives what stands next to the constants (within a factor of two either way)"""
    n, cell = BEAM_CALIBRATION["n"], BEAM_CALIBRATION["cell"]
    prob = _deck(make_problem, "stream", nx, 4 * n)
    st = ds.beams(prob, cell, n)
    got = _oracle_run(prob, cs, st, scalar_flux=True, current=True)
    want = _beam_closed_form(prob, cell, n)
    flux_err, current_err = _beam_errors(want, got["flux"], got["jx"], got["jy"])
    print(f"oracle against the closed form, {nx}^2, cell {cell}, {4 * n} histories: largest per-cell relative "
          f"flux error {flux_err:.2e}, current error against the largest current {current_err:.2e}")
    assert 0.5 * BEAM_MEASURED[nx]["flux"] <= flux_err <= 2.0 * BEAM_MEASURED[nx]["flux"]
    assert 0.5 * BEAM_MEASURED[nx]["current"] <= current_err <= 2.0 * BEAM_MEASURED[nx]["current"]


@pytest.mark.parametrize("nx", [64, 48])
def test_axis_beams_against_the_closed_form(make_problem, cs, nx):
    """1024 histories in each axis direction from the centre of BEAM_CELL, two steps of 1.38 m on
    a mesh of 1 m: every beam hits both of its walls.  The oracle's flux and current, and the
    replay's crossing counts, against the unfolded path."""
    n = N // 4
    prob = _deck(make_problem, "stream", nx)
    st = ds.beams(prob, BEAM_CELL, n)
    got = _oracle_run(prob, cs, st, scalar_flux=True, current=True)
    assert all(e == (N, e[1], 0, N) for e in got["events"])
    for pid in range(0, N, n):        # a beam's histories are one history
        for f in replay.FIELDS:
            assert np.all(got["parts"][f][pid:pid + n] == got["parts"][f][pid]), f
    want = _beam_closed_form(prob, BEAM_CELL, n)
    assert sum(e[1] for e in got["events"]) == want["counts"].sum()
    boundary = want["counts"][W][:, 0].sum() + want["counts"][E][:, -1].sum() + \
        want["counts"][S][0, :].sum() + want["counts"][NORTH][-1, :].sum()
    assert boundary >= 2 * N          # both walls, every beam
    _check_beams(want, got["flux"], got["jx"], got["jy"], _replayed_counts(prob, cs, st, n), nx, "oracle")


# ---- GPU -------------------------------------------------------------------------------------

def _upload(iface, sim, states):
    """the states into the store through the array hooks (which tell the library that the arrays
    changed), before step 1"""
    p = sim.particles.contents
    for f, a in states.items():
        a = np.ascontiguousarray(a)
        assert a.dtype == (np.int32 if f in ("cellx", "celly", "dead") else np.float64) and len(a) == sim.n
        iface.library().neutral_hip_memcpy_h2d(C.c_void_p(getattr(p, f)), a.ctypes.data, a.nbytes)


def _gpu_run(iface, prob, cs, states, variant, checked=False, full=False, source=None, **opts):
    iface.set_arithmetic(iface.ARITH_CHECKED if checked else iface.ARITH_AUTO)
    sim = iface.Simulation(prob, *cs, variant=variant, **opts)
    try:
        if source is not None:
            sim.inject(source=source)
        else:
            sim.inject()
            _upload(iface, sim, states)
        start = sim.particle_arrays()
        steps = [sim.step(tt) for tt in range(1, STEPS + 1)]
        out = dict(steps=steps, events=[_events(r) for r in steps], start=start, parts=sim.particle_arrays(),
                   tally=sim.tally_host().copy(),
                   flux=None if sim.flux is None else sim.flux.cpu().numpy(),
                   collisions=None if sim.collisions is None else sim.collisions_host(),
                   absorbed=None if sim.absorbed is None else sim.absorbed_host(),
                   out=None if sim.outflow is None else sim.outflow_host().copy())
        if sim.jx is not None:
            out["jx"], out["jy"] = (a.ravel() for a in sim.current_host())
    finally:
        sim.close()
        iface.set_arithmetic(iface.ARITH_AUTO)
    return out


def _same_as_the_oracle(got, want, variant, checked=False):
    """the bars of tests/test_hip_parity.py"""
    assert got["events"] == want["events"]
    assert iface_variant(got) == variant
    for r in got["steps"]:
        assert r.stats.aborted == 0
        assert r.stats.checked_arithmetic == (1 if checked else 0)
    gp, cp = got["parts"], want["parts"]
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(gp[f], cp[f]), f
    for f in ("energy", "weight", "dt_to_census", "x", "y"):
        assert rel(gp[f], cp[f]) < STATE_TOL, f
    for f in ("omega_x", "omega_y"):
        assert np.max(np.abs(gp[f] - cp[f])) < STATE_TOL, f
    scale = max(1e-300, float(np.max(np.abs(cp["mfp_to_collision"]))))
    assert np.max(np.abs(gp["mfp_to_collision"] - cp["mfp_to_collision"])) / scale < STATE_TOL
    tg, tc = got["tally"], want["tally"]
    assert np.linalg.norm(tg - tc) / np.linalg.norm(tc) < TALLY_L2_TOL
    assert np.array_equal(tg == 0.0, tc == 0.0)
    for name in ("flux", "jx", "jy"):
        if want.get(name) is not None:
            assert l2_of_nonzero(got[name], want[name]) <= MESH_TOL, name
    if want.get("flux") is not None:
        assert np.array_equal(got["flux"] == 0.0, want["flux"] == 0.0)
    if want.get("collisions") is not None:
        assert np.array_equal(got["collisions"], want["collisions"])
        assert got["collisions"].sum() == float(sum(e[2] for e in got["events"]))
        assert l2_of_nonzero(got["absorbed"], want["absorbed"]) <= TALLY_L2_TOL


def iface_variant(got):
    return got["steps"][-1].stats.variant


_ORACLE = {}


def _oracle_on_the_corpus(make_problem, cs, name, nx, uneven=False, **opts):
    """(problem, corpus, the oracle's run): computed once per deck, shared, left as it is"""
    key = (name, nx, uneven, tuple(sorted(opts)))
    if key not in _ORACLE:
        prob = _deck(make_problem, name, nx)
        if uneven:
            _uneven(prob)
        st = ds.corpus(prob, N)
        _ORACLE[key] = (prob, st, _oracle_run(prob, cs, st, **opts))
    return _ORACLE[key]


@gpu
@needs_gpu
@pytest.mark.parametrize("arith", ["auto", "checked"])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_corpus_on_the_stream_deck(iface, make_problem, cs, variant, arith):
    """a. stream 64^2: exact ties, zero cosines, on-edge starts, in every variant under both
    arithmetic policies, with the flux and the current kept"""
    prob, st, want = _oracle_on_the_corpus(make_problem, cs, "stream", 64, scalar_flux=True, current=True)
    got = _gpu_run(iface, prob, cs, st, variant, checked=arith == "checked", scalar_flux=True, current=True)
    _same_as_the_oracle(got, want, variant, checked=arith == "checked")
    for f in st:   # the hooks put into the store what the oracle started from
        assert got["start"][f].tobytes() == want["start"][f].tobytes(), f


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_corpus_into_the_collision_stage(iface, make_problem, cs, variant):
    """b. csp 64^2 at dt = 1e-6: degenerate histories reach the block and collide -- an absorption
    leaves a zero cosine as it is -- with the collision tallies kept, the collisions exact"""
    prob, st, want = _oracle_on_the_corpus(make_problem, cs, "csp", 64, collision_tallies=True)
    assert want["events"][0][2] > 100000
    got = _gpu_run(iface, prob, cs, st, variant, collision_tallies=True)
    _same_as_the_oracle(got, want, variant)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 2])
def test_corpus_with_near_ties(iface, make_problem, cs, variant):
    """c. stream 48^2: edges that are no binary fractions, ties decided by the last bit"""
    prob, st, want = _oracle_on_the_corpus(make_problem, cs, "stream", 48)
    got = _gpu_run(iface, prob, cs, st, variant)
    _same_as_the_oracle(got, want, variant)


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_corpus_on_loaded_edges(iface, make_problem, cs, lazy):
    """d. csp 48^2 with uneven edges, the corpus built from them: the stream kernel loads its
    edges instead of working them out; again with the lazy export"""
    prob, st, want = _oracle_on_the_corpus(make_problem, cs, "csp", 48, uneven=True)
    iface.set_lazy_export(lazy)
    got = _gpu_run(iface, prob, cs, st, 2)
    _same_as_the_oracle(got, want, 2)


@gpu
@needs_gpu
def test_corpus_where_cell_corners_are_tile_corners(iface, make_problem, cs, monkeypatch):
    """e. stream 64^2 under tiles of 16 cells: a history through a cell's corner crosses two tile
    edges in two events a distance of about 0 apart"""
    monkeypatch.setenv("NEUTRAL_TILE_CELLS", "16")
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob, st, want = _oracle_on_the_corpus(make_problem, cs, "stream", 64)
    assert allowed_tile(16, prob.nx, prob.ny, N) == 16
    got = _gpu_run(iface, prob, cs, st, 2)
    assert all(r.stats.tile_cells == 16 for r in got["steps"])
    _same_as_the_oracle(got, want, 2)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("nx", [64, 48])
def test_axis_beams_on_the_gpu(iface, make_problem, cs, nx, variant):
    """f. the beams of test_axis_beams_against_the_closed_form with the outflow kept: the oracle's
    decisions, and (a), (b), (c) of the closed form at the CPU test's constants -- the crossing
    counts of each side of each cell exact"""
    n = N // 4
    prob = _deck(make_problem, "stream", nx)
    st = ds.beams(prob, BEAM_CELL, n)
    want = _oracle_run(prob, cs, st, scalar_flux=True, current=True)
    got = _gpu_run(iface, prob, cs, st, variant, scalar_flux=True, current=True, outflow=True)
    _same_as_the_oracle(got, want, variant)
    counts = got["out"] * N
    assert np.array_equal(counts, np.round(counts))
    _check_beams(_beam_closed_form(prob, BEAM_CELL, n), got["flux"], got["jx"], got["jy"],
                 counts.astype(np.int64), nx, f"variant {variant}")


# ---- GPU: beams and point sources through the described source -------------------------------

@gpu
@needs_gpu
def test_beams_from_lattice_points_through_the_described_source(iface, make_problem, cs):
    """Four components, each a point (width = height = 0) on a lattice point of the mesh, each a
    beam (theta_width = 0) along theta0 = 0, pi/2, pi, 3 pi/2, each with one energy line.  What
    inject(source=...) leaves in the store is what was described, and the oracle, handed the
    store's own arrays, runs it as variants 0 and 2 do."""
    import described_source_reference as dr
    import source_reference as sr
    prob = _deck(make_problem, "stream", 64)
    ex, ey = (np.asarray(e, dtype=np.float64) for e in (prob.edgex, prob.edgey))
    points = [(ex[9], ey[20]), (ex[31], ey[5]), (ex[50], ey[44]), (ex[17], ey[63])]
    thetas = [0.0, math.pi / 2, math.pi, 3 * math.pi / 2]
    energies = [prob.initial_energy, 2.5e5, 5.0e5, 7.5e5]
    desc = [dr.component(1.0, (px, py, 0.0, 0.0), [(e, 1.0)], theta=(t, 0.0))
            for (px, py), t, e in zip(points, thetas, energies)]
    source = dr.to_interface(iface, desc)
    runs = {}
    for variant in (0, 2):
        runs[variant] = _gpu_run(iface, prob, cs, None, variant, source=source)
    start = runs[0]["start"]
    for f in sr.FIELDS:
        assert runs[2]["start"][f].tobytes() == start[f].tobytes(), f
    assert not start["dead"].any()
    for k, ((px, py), theta, energy) in enumerate(zip(points, thetas, energies)):
        slots = np.flatnonzero(start["energy"] == energy)
        assert len(slots) > N // 8, k                        # shares 1 : 1 : 1 : 1
        for f in sr.FIELDS:                                  # every slot the same eleven fields
            assert np.all(start[f][slots].view(np.uint64 if start[f].dtype == np.float64 else np.int32)
                          == start[f][slots[:1]].view(np.uint64 if start[f].dtype == np.float64 else np.int32)), (k, f)
        i = slots[0]
        assert start["x"][i].tobytes() == np.float64(px).tobytes() and start["y"][i].tobytes() == np.float64(py).tobytes()
        assert start["cellx"][i] == sr.find_cell(ex, np.array([px]))[0]
        assert start["celly"][i] == sr.find_cell(ey, np.array([py]))[0]
        ox, oy = start["omega_x"][i], start["omega_y"][i]
        if k == 0:
            assert ox.tobytes() == np.float64(1.0).tobytes() and oy.tobytes() == np.float64(0.0).tobytes()
        else:
            small, large = sorted((abs(ox), abs(oy)))
            assert small < 2.0 ** -50 and large == 1.0, (k, ox, oy)
            assert abs(ox - math.cos(theta)) < 1e-15 and abs(oy - math.sin(theta)) < 1e-15
        assert (start["weight"][i], start["dt_to_census"][i], start["mfp_to_collision"][i]) == (1.0, prob.dt, 0.0)
    assert sum(int((start["energy"] == e).sum()) for e in energies) == N
    want = _oracle_run(prob, cs, None, full=start)
    assert all(e == (N, e[1], 0, N) for e in want["events"])
    for variant in (0, 2):
        _same_as_the_oracle(runs[variant], want, variant)

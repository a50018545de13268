"""The leakage tally (include/neutral_hip.h: neutral_hip_set_leakage_tally): the escapes through the
vacuum sides by side, energy group and exit cosine, scored on the device where a history escapes.
The reference is tests/leakage_reference.py -- tests/replay.py's loop with its wall hook noting the
side, binned by a restatement of the header -- pinned here on hand-picked values and hand-computed
flights, then held against every kernel variant bin by bin.

The GPU's cosines and energies agree with the replay's to 1e-9, not bit for bit, so a history ON a
boundary could land next door; every deck is therefore asserted to hold NO escape within 1e-7 of an
energy edge or of an interior cosine boundary before anything is compared with it (_conditions).

Tolerances are tests/test_vacuum.py's: counts exact, a weight against its reference TALLY_SUM_TOL
per bin, two runs of the same histories 1e-13.  N times a side's weights against the escape
statistics' weight: both are sums of the same k positive terms in different orders (relative error
(k - 1) u each), one divided and one multiplied by N (u each): (k + 1) * 2^-52 of the weight."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import leakage_reference as lr
import oracle_binding as ob
import replay
import test_vacuum as tv
from gpu_support import OWN_DRIVER, gpu, iface, l2, needs_gpu, run_driver, third_absorb  # noqa: F401
from ranks import launch_ranks
from test_window_roulette import two_valued

TALLY_SUM_TOL = 1e-10
SAME_HISTORIES_TOL = 1e-13
W, E, S, N = replay.WEST, replay.EAST, replay.SOUTH, replay.NORTH
LEAKAGE_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_leakage_worker.py")
NEAR = 1e-7
SETTER = "neutral_hip_set_leakage_tally"


def _edges(prob):
    return prob.initial_energy * np.array([0.5, 0.9, 0.97, 1.0])


def _c_edges(e):
    e = np.ascontiguousarray(e, dtype=np.float64)
    return e, e.ctypes.data_as(C.POINTER(C.c_double))


# ---- CPU: the ABI ------------------------------------------------------------------------------

def test_library_exports_the_setter_at_the_same_abi_version():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, SETTER) and SETTER in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12


def test_every_refusal_changes_nothing_and_null_is_always_accepted():
    """No device is touched: the addresses are never dereferenced by the setter, and no step runs.
    What "changes nothing" can mean without a device is that the setter keeps refusing and accepting
    by its arguments alone, whatever was set before -- and that NULL is accepted beside anything."""
    from neutral_amd import interface as iface
    lib = iface.library()
    set_ = getattr(lib, SETTER)
    out = C.c_void_p(0x1000)   # (an address the library only keeps)
    keep, good = _c_edges([1.0, 2.0, 4.0])
    try:
        assert set_(2, good, 4, out) == 0
        _, one = _c_edges([1.0])
        refused = [(-1, None, 4), (65, good, 4), (2, None, 4), (0, good, 4), (2, good, 0), (2, good, 65), (2, good, -3)]
        for bad in ([1.0, 1.0, 2.0], [2.0, 1.0, 3.0], [0.0, 1.0, 2.0], [-1.0, 1.0, 2.0], [1.0, np.inf, 3.0],
                    [1.0, np.nan, 3.0], [1.0, 2.0, np.inf]):
            kept, ptr = _c_edges(bad)
            refused.append((2, ptr, 4, kept))
        for args in refused:
            assert set_(args[0], args[1], args[2], out) == 1, args[:3]
        # 0 groups, 64 groups, 1 and 64 cosines are the ends of what is taken
        many, many_ptr = _c_edges(np.geomspace(1.0, 2.0e6, 65))
        assert set_(0, None, 1, out) == 0 and set_(64, many_ptr, 64, out) == 0 and set_(1, good, 64, out) == 0
        # NULL turns it off beside anything
        for args in [(0, None, 1), (-1, None, 0), (65, good, 65), (2, None, 100)]:
            assert set_(args[0], args[1], args[2], None) == 0
        with pytest.raises(ValueError):
            iface.set_leakage_tally([1.0], 4, 0x1000)
        with pytest.raises(ValueError):
            iface.set_leakage_tally([1.0, 2.0], 65, 0x1000)
        with pytest.raises(ValueError):
            iface.set_leakage_tally([2.0, 1.0], 4, 0x1000)
        iface.set_leakage_tally([1.0, 2.0], 4, 0x1000)
        iface.set_leakage_tally(None, 1, 0x1000)
        assert iface.leakage_shape([1.0, 2.0, 3.0], 5) == (4, 3, 5) and iface.leakage_shape(None, 1) == (4, 1, 1)
    finally:
        set_(0, None, 1, None)
        del keep, many


# ---- CPU: the reference -------------------------------------------------------------------------

def test_the_references_bins_on_hand_picked_values():
    edges = [1.0, 2.0, 4.0, 8.0]
    assert [lr.group_of(edges, e) for e in (1.0, 1.5, 2.0, 3.999, 4.0, 7.999)] == [0, 0, 1, 1, 2, 2]
    assert lr.group_of(edges, 8.0) == 3            # at edges[G]: no group
    assert lr.group_of(edges, 0.999) == 3 and lr.group_of(edges, 9.0) == 3 and lr.group_of(edges, float("nan")) == 3
    assert lr.group_of([], 5.0) == 0 and lr.group_of([], float("nan")) == 0
    assert lr.cosine_bin(1.0, 4) == 3 and lr.cosine_bin(1.0, 1) == 0 and lr.cosine_bin(1.0, 64) == 63
    assert lr.cosine_bin(0.5, 4) == 2 and lr.cosine_bin(np.nextafter(0.5, 0.0), 4) == 1
    assert lr.cosine_bin(0.25, 4) == 1 and lr.cosine_bin(np.nextafter(0.25, 0.0), 4) == 0
    assert lr.cosine_bin(5e-324, 64) == 0
    assert lr.bin_of(edges, 4, W, 2.0, -0.6, 0.8) == (W, 1, 2) and lr.bin_of(edges, 4, N, 2.0, -0.6, 0.8) == (N, 1, 3)
    assert lr.bin_of(edges, 4, S, 8.0, 0.6, -0.2) == (S, 3, 0)


def _oblique_flights(make_problem, cs, starts, ncosines=4, edges=None, nx=10, length=0.2):
    prob = make_problem("stream", nx=nx, nparticles=4, iterations=1)
    e0 = prob.initial_energy
    edges = [0.5 * e0, e0, 2.0 * e0] if edges is None else edges
    rep = lr.LeakageReplay(prob, cs, dt=length / replay.speed_of(e0), vacuum=15, leak_edges=edges, ncosines=ncosines)
    for pid, (x, y, ox, oy, w) in enumerate(starts):
        s = dict(x=x, y=y, omega_x=ox, omega_y=oy, energy=e0, weight=w, dead=0,
                 cellx=min(int(x * nx), nx - 1), celly=min(int(y * nx), nx - 1))
        rep.history(pid, 1, s)
        assert s["dead"] == 1
    assert rep.ncollisions == 0
    return rep


def test_four_hand_computed_oblique_flights_score_one_bin_each(make_problem, cs):
    """Collision-free flights of 0.2 m on a 10 x 10 mesh of 1 m, every side vacuum, N = 4, edges
    (e0 / 2, e0, 2 e0): the energy e0 is ON the middle edge, so in group 1.  (0.6, 0.8) from
    (0.95, 0.55) reaches x = 1 after 0.0833 m, y = 1 only after 0.5625 m: east, mu 0.6, bin 2 of 4.
    (-0.8, -0.6) from (0.04, 0.55): west after 0.05 m, mu 0.8, bin 3.  (0.6, -0.8) from (0.55, 0.04):
    south after 0.05 m (east after 0.75), mu 0.8, bin 3.  (-0.96, 0.28) from (0.55, 0.98): north after
    0.0714 m (west after 0.57), mu 0.28, bin 1.  The weights 1, 1/2, 1/4, 3/4 over N = 4 are exact."""
    starts = [(0.95, 0.55, 0.6, 0.8, 1.0), (0.04, 0.55, -0.8, -0.6, 0.5), (0.55, 0.04, 0.6, -0.8, 0.25),
              (0.55, 0.98, -0.96, 0.28, 0.75)]
    rep = _oblique_flights(make_problem, cs, starts)
    want_w, want_c = np.zeros((4, 3, 4)), np.zeros((4, 3, 4))
    for (side, m), (_, _, _, _, w) in zip(((E, 2), (W, 3), (S, 3), (N, 1)), starts):
        want_w[side, 1, m] = w / 4
        want_c[side, 1, m] = 1.0
    assert np.array_equal(rep.leak_weight, want_w) and np.array_equal(rep.leak_count, want_c)
    assert rep.escaped == [1, 1, 1, 1] and rep.escape_weight == [0.5, 1.0, 0.25, 0.75]


# ---- the decks, their references and what each must show ------------------------------------------

_REFERENCES = {}


def _reference(prob, cs, injected, steps, vacuum, edges, ncosines, cs_absorb=None, roulette=(0.0, 0.0), window=None):
    """the replay of every history of `injected`, once per configuration: -> run with "rep" and
    "added", what each step added"""
    key = (prob.nx, prob.ny, prob.dt, steps, vacuum, tuple(float(e) for e in edges), ncosines, cs_absorb is not None,
           tuple(roulette), None if window is None else (window.lower.tobytes(), window.ratio),
           prob.density.tobytes(), tuple(injected[f].tobytes() for f in replay.FIELDS))
    if key not in _REFERENCES:
        rep = lr.LeakageReplay(prob, cs, cs_absorb, roulette, vacuum=vacuum, window=window, leak_edges=edges,
                               ncosines=ncosines)
        run = lr.run_steps(rep, injected, steps)
        run["rep"] = rep
        _REFERENCES[key] = run
    return _REFERENCES[key]


def _conditions(case, prob, rep, ncosines=4):
    """what a deck must show before anything is compared with its reference (the issue's list)"""
    escapes = rep.escapes
    near_cosine = lr.nearest_cosine_boundary(escapes, ncosines)
    if case == "stream":
        first = [e for e in escapes if e["key"] == 1]
        assert len(first) == prob.nparticles == len(escapes) and all(e["weight"] == 1.0 for e in escapes)
        _, count = lr.rebinned(escapes, rep.inv_n, (), 16)
        filled = [int(np.count_nonzero(count[s, 0])) for s in range(4)]
        print(f"stream: escaped {rep.escaped}, cosine bins of 16 filled per side {filled}, nearest boundary "
              f"{lr.nearest_cosine_boundary(escapes, 16):.2e} (M = 16), {near_cosine:.2e} (M = {ncosines})")
        assert min(filled) >= 3
        for m in (16, 64, ncosines):
            assert lr.nearest_cosine_boundary(escapes, m) > NEAR
        return
    edges = _edges(prob)
    vacuum = tv.CASES[case]["vacuum"]
    near_edge = lr.nearest_edge(escapes, edges)
    weight, count = lr.rebinned(escapes, rep.inv_n, edges, 4)
    print(f"case {case}: escaped {rep.escaped}, {rep.escaped_not_unit} with weight != 1, rows by side "
          f"{[count[s].sum(axis=1).tolist() for s in range(4) if (vacuum >> s) & 1]}, west cosine bins "
          f"{count[W].sum(axis=0).tolist()}, nearest edge {near_edge:.2e}, nearest cosine boundary {near_cosine:.2e}")
    for side in range(4):
        if (vacuum >> side) & 1:
            assert rep.escaped[side] >= 50, side
            assert np.all(count[side].sum(axis=1) > 0), side      # every row, "no group" included
        else:
            assert rep.escaped[side] == 0 and not count[side].any(), side
    assert rep.escaped_not_unit >= 50
    unscattered = sum(1 for e in escapes if e["energy"] == edges[-1])
    assert unscattered == int(count[:, -1].sum()) and unscattered > 0   # the row "no group" IS the unscattered
    assert np.all(count[W].sum(axis=0) > 0)
    assert near_edge > NEAR and near_cosine > NEAR


def _oracle_reference(make_problem, cs, case, ncosines=4):
    if case == "stream":
        prob = tv._stream_problem(make_problem)
        injected = tv._oracle_injected(prob, cs)
        return prob, _reference(prob, cs, injected, 3, 15, (), ncosines)
    prob = tv._case_problem(make_problem, case)
    injected = tv._oracle_injected(prob, cs)
    return prob, _reference(prob, cs, injected, 3, tv.CASES[case]["vacuum"], _edges(prob), ncosines, third_absorb(cs))


@pytest.mark.parametrize("case", ["a", "b", "stream"])
def test_the_decks_meet_their_conditions_and_the_reference_its_identities(make_problem, cs, case):
    """... on the CPU oracle's injection; and (0, 1) binned from the same escapes reproduces
    rep.escaped and rep.escape_weight, a (G, M) tally summed over its rows is the (0, M) one"""
    prob, run = _oracle_reference(make_problem, cs, case)
    rep = run["rep"]
    _conditions(case, prob, rep)
    n = prob.nparticles
    weight, count = lr.rebinned(rep.escapes, rep.inv_n, (), 1)
    assert count[:, 0, 0].tolist() == [float(c) for c in rep.escaped]
    for side in range(4):
        assert abs(n * weight[side, 0, 0] - rep.escape_weight[side]) <= (rep.escaped[side] + 1) * 2.0 ** -52 * \
            rep.escape_weight[side]
    assert np.array_equal(rep.leak_count.sum(axis=(1, 2)), count[:, 0, 0])
    flat_w, flat_c = lr.rebinned(rep.escapes, rep.inv_n, (), rep.ncosines)
    assert np.array_equal(rep.leak_count.sum(axis=1), flat_c[:, 0])
    assert np.allclose(rep.leak_weight.sum(axis=1), flat_w[:, 0], rtol=1e-13, atol=0.0)
    for key, (w, c) in enumerate(run["added"], 1):
        assert c.sum(axis=(1, 2)).tolist() == [float(v) for v in run["per_step"][key - 1]["escaped"]]
    assert np.array_equal(sum(c for _, c in run["added"]), rep.leak_count)


# ---- the GPU runs -----------------------------------------------------------------------------------

def _run(iface, prob, cs, steps, variant, leakage, states=None, window=None, zero_between=True, **kw):
    """inject (and overwrite with `states`), step; after every step the leakage tally's two halves are
    read -- and zeroed, so that each reading is what the step added, unless zero_between is False"""
    sim = iface.Simulation(prob, *cs, variant=variant, leakage=leakage, **kw)
    try:
        sim.inject()
        if states is not None:
            tv._upload(iface, sim, states)
        if window is not None:
            sim.window_in_step(**window)
        injected = sim.particle_arrays()
        results, snaps, read = [], [injected], []
        for tt in range(1, steps + 1):
            results.append(sim.step(tt))
            assert results[-1].stats.aborted == 0
            snaps.append(sim.particle_arrays())
            if leakage is not None:
                read.append(sim.leakage_host())
                if zero_between:
                    sim.leakage.zero_()
        return dict(steps=results, injected=injected, snaps=snaps, parts=snaps[-1], read=read,
                    tally=sim.tally_host().copy(), flux=tv._host(sim.flux), absorbed=tv._host(sim.absorbed),
                    collisions=tv._host(sim.collisions), jx=tv._host(sim.jx), jy=tv._host(sim.jy),
                    spectrum=tv._host(sim.spectrum),
                    out=sim.outflow_host().copy() if sim.outflow is not None else None)
    finally:
        sim.close()
        assert iface.library().neutral_hip_get_vacuum_sides() == 0


def _assert_bins(got, want, what=""):
    """counts exact in every bin, weights within TALLY_SUM_TOL per bin, 0.0 where the reference has 0"""
    (gw, gc), (ww, wc) = got, want
    assert gw.shape == ww.shape and gc.shape == wc.shape, what
    assert np.array_equal(gc, wc), (what, np.argwhere(gc != wc)[:5].tolist())
    assert not gw[ww == 0.0].any(), what
    assert np.all(np.abs(gw - ww) <= TALLY_SUM_TOL * ww), (what, float(np.max(np.abs(gw - ww) / np.maximum(ww, 1e-300))))


def _assert_identities(got, n):
    """per step and side: the counts sum to the escape statistics' exactly, N times the weights to
    their weight within the summation bound"""
    for tt, (r, (w, c)) in enumerate(zip(got["steps"], got["read"]), 1):
        for side in range(4):
            k, total = r.escape.counts()[side], r.escape.weights()[side]
            assert c[side].sum() == float(k), (tt, side)
            assert abs(n * w[side].sum() - total) <= (k + 1) * 2.0 ** -52 * total, (tt, side)


def _assert_against(got, want, n):
    for tt, (read, added) in enumerate(zip(got["read"], want["added"]), 1):
        _assert_bins(read, added, f"step {tt}")
    tv._assert_events(got, want)
    _assert_identities(got, n)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("arith", ["auto", "checked"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_against_the_reference(iface, make_problem, cs, monkeypatch, variant, arith, case):
    """1. every optional tally on; read after every step: what each step added is the reference's"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, case)
    iface.set_arithmetic(iface.ARITH_CHECKED if arith == "checked" else iface.ARITH_AUTO)
    vacuum = tv.CASES[case]["vacuum"]
    got = _run(iface, prob, cs, 3, variant, (_edges(prob), 4), cs_absorb=third_absorb(cs), outflow=True, vacuum=vacuum,
               **tv._everything(prob))
    want = _reference(prob, cs, got["injected"], 3, vacuum, _edges(prob), 4, third_absorb(cs))
    _conditions(case, prob, want["rep"])
    _assert_against(got, want, prob.nparticles)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("ncosines", [1, 16, 64])
def test_exact_on_the_collision_free_deck(iface, make_problem, cs, monkeypatch, variant, ncosines):
    """2. every weight 1, N = 512: the weights ARE counts / 512, the counts the reference's; steps 2
    and 3 add nothing.  With M = 1 all lanes of a wave share at most four bins, with M = 64 a wave
    holds many bins of one or two lanes: the per-wave aggregation at both ends.  One group whose top
    edge is the source's energy: every history is in the row "no group"."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._stream_problem(make_problem)
    e0 = prob.initial_energy
    edges = (0.5 * e0, e0) if ncosines != 16 else ()
    got = _run(iface, prob, cs, 3, variant, (edges or None, ncosines), outflow=True, vacuum="all")
    want = _reference(prob, cs, got["injected"], 3, 15, edges, ncosines)
    _conditions("stream", prob, want["rep"], ncosines)
    (w1, c1), (ww, wc) = got["read"][0], want["added"][0]
    assert np.array_equal(c1, wc) and c1.sum() == 512.0
    assert np.array_equal(w1, c1 / 512.0)
    if edges:
        assert not c1[:, 0].any() and c1[:, 1].sum() == 512.0
    for w, c in got["read"][1:]:
        assert not w.any() and not c.any()
    _assert_identities(got, prob.nparticles)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_it_changes_nothing_else(iface, make_problem, cs, monkeypatch, variant):
    """3. deck a with the tally on against the run without it: every slot's eleven fields, every
    event count and the escape counts exact; the atomically summed meshes and sums within 1e-13"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    kw = dict(cs_absorb=third_absorb(cs), outflow=True, vacuum="wn", **tv._everything(prob))
    off = _run(iface, prob, cs, 3, variant, None, **kw)
    on = _run(iface, prob, cs, 3, variant, (_edges(prob), 4), zero_between=False, **kw)
    for tt in range(4):
        for f in tv.ALL_FIELDS:
            assert np.array_equal(on["snaps"][tt][f], off["snaps"][tt][f]), (tt, f)
    for a, b in zip(on["steps"], off["steps"]):
        assert (a.nprocessed, a.facets, a.collisions, a.census) == (b.nprocessed, b.facets, b.collisions, b.census)
        assert a.escape.counts() == b.escape.counts() and sum(a.escape.counts()) > 0
        for side in range(4):
            assert abs(a.escape.weights()[side] - b.escape.weights()[side]) <= SAME_HISTORIES_TOL * b.escape.weights()[side]
    assert np.array_equal(on["collisions"], off["collisions"])
    for name in ("tally", "flux", "absorbed", "jx", "jy", "spectrum", "out"):
        assert off[name].any() and l2(on[name], off[name]) <= SAME_HISTORIES_TOL, name
    # (not zeroed between the steps: the array accumulates, and its last reading closes on all three steps)
    total = [sum(r.escape.counts()[s] for r in on["steps"]) for s in range(4)]
    assert on["read"][-1][1].sum(axis=(1, 2)).tolist() == [float(c) for c in total]


@gpu
@needs_gpu
def test_equivalences(iface, make_problem, cs, monkeypatch):
    """4. on the tiled variant: (0, 1) holds the escape statistics; (3 groups, 4) summed over its rows
    is the (0, 4) run; with no side vacuum the array stays zero and the step is a plain step's;
    after device_out = NULL a further step leaves the array untouched"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    n = prob.nparticles
    kw = dict(cs_absorb=third_absorb(cs), vacuum="wn")
    bare = _run(iface, prob, cs, 3, 2, (None, 1), zero_between=False, **kw)
    w, c = bare["read"][-1]
    assert w.shape == (4, 1, 1)
    for side in range(4):
        k = sum(r.escape.counts()[side] for r in bare["steps"])
        total = sum(r.escape.weights()[side] for r in bare["steps"])
        assert c[side, 0, 0] == float(k) and abs(n * w[side, 0, 0] - total) <= (k + 3) * 2.0 ** -52 * total
    assert c[W, 0, 0] >= 50 and c[N, 0, 0] >= 50 and c[E, 0, 0] == c[S, 0, 0] == 0.0
    grouped = _run(iface, prob, cs, 3, 2, (_edges(prob), 4), zero_between=False, **kw)
    flat = _run(iface, prob, cs, 3, 2, (None, 4), zero_between=False, **kw)
    (gw, gc), (fw, fc) = grouped["read"][-1], flat["read"][-1]
    assert np.array_equal(gc.sum(axis=1), fc[:, 0]) and fc.sum() == c.sum()
    assert np.all(np.abs(gw.sum(axis=1) - fw[:, 0]) <= SAME_HISTORIES_TOL * fw[:, 0])
    # no side vacuum: nothing is scored, and the step is the plain step
    plain = _run(iface, prob, cs, 3, 2, None, cs_absorb=third_absorb(cs))
    closed = _run(iface, prob, cs, 3, 2, (_edges(prob), 4), zero_between=False, cs_absorb=third_absorb(cs))
    for w, c in closed["read"]:
        assert not w.any() and not c.any()
    for f in tv.ALL_FIELDS:
        assert np.array_equal(closed["parts"][f], plain["parts"][f]), f
    assert l2(closed["tally"], plain["tally"]) <= SAME_HISTORIES_TOL   # (summed by atomics: no order)
    for a, b in zip(closed["steps"], plain["steps"]):
        assert (a.nprocessed, a.facets, a.collisions, a.census, a.stats.variant) == \
            (b.nprocessed, b.facets, b.collisions, b.census, b.stats.variant)
        assert sum(a.escape.counts()) == 0
    # off: a further step with vacuum sides leaves the caller's array alone
    import torch
    sim = iface.Simulation(prob, *cs, variant=2, **kw)
    out = torch.zeros(2 * 4 * 4 * 4, dtype=torch.float64, device=sim.device)
    try:
        sim.inject()
        iface.set_leakage_tally(_edges(prob), 4, out)   # (the Simulation keeps none: the setting is this test's)
        # (a refusal in between changes nothing: the step scores the (3 groups, 4) tally set before it)
        assert iface.library().neutral_hip_set_leakage_tally(0, None, 0, C.c_void_p(out.data_ptr())) == 1
        assert iface.library().neutral_hip_set_leakage_tally(2, None, 1, C.c_void_p(out.data_ptr())) == 1
        sim.step(1)
        after_one = out.cpu().numpy().copy()
        assert after_one[64:].sum() == float(sum(iface.last_escape().counts())) > 0
        assert np.array_equal(after_one[64:].reshape(4, 4, 4), grouped["read"][0][1])
        iface.set_leakage_tally(out=None)
        r = sim.step(2)
        assert sum(r.escape.counts()) > 0
        assert np.array_equal(out.cpu().numpy(), after_one)
    finally:
        iface.set_leakage_tally(out=None)
        sim.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("how", ["no outflow tally", "lazy export", "stream queues"])
def test_tiled_without_an_outflow_tally_lazy_and_with_queues(iface, make_problem, cs, monkeypatch, how):
    """5. one deck-a run each on the tiled variant, against the reference"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    iface.set_lazy_export(how == "lazy export")
    iface.set_stream_queues(how == "stream queues")
    got = _run(iface, prob, cs, 3, 2, (_edges(prob), 4), cs_absorb=third_absorb(cs), vacuum="wn",
               outflow=(how != "no outflow tally"))
    want = _reference(prob, cs, got["injected"], 3, tv.CASES["a"]["vacuum"], _edges(prob), 4, third_absorb(cs))
    _conditions("a", prob, want["rep"])
    _assert_against(got, want, prob.nparticles)


@gpu
@needs_gpu
@pytest.mark.parametrize("how,variant", [("roulette", 1), ("in-step window", 2), ("roulette", 2), ("in-step window", 0)])
def test_with_roulette_and_with_the_in_step_window(iface, make_problem, cs, monkeypatch, how, variant):
    """6. weights that jump: deck a against the reference built with the same roulette / window"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = tv._case_problem(make_problem, "a")
    kw = dict(cs_absorb=third_absorb(cs), outflow=True, vacuum="wn", scalar_flux=True, collision_tallies=True)
    if how == "roulette":
        got = _run(iface, prob, cs, 3, variant, (_edges(prob), 4), roulette=tv.ROULETTE, **kw)
        want = _reference(prob, cs, got["injected"], 3, tv.CASES["a"]["vacuum"], _edges(prob), 4, third_absorb(cs),
                          roulette=tv.ROULETTE)
    else:
        mesh = two_valued(prob.nx, prob.ny)
        got = _run(iface, prob, cs, 3, variant, (_edges(prob), 4), window=dict(lower=mesh, survival_ratio=2.0), **kw)
        want = _reference(prob, cs, got["injected"], 3, tv.CASES["a"]["vacuum"], _edges(prob), 4, third_absorb(cs),
                          window=replay.Window(mesh, 2.0))
    rep = want["rep"]
    print(f"{how}: killed {rep.killed}, survived {rep.survived}, escaped {rep.escaped}, nearest edge "
          f"{lr.nearest_edge(rep.escapes, _edges(prob)):.2e}, nearest cosine boundary "
          f"{lr.nearest_cosine_boundary(rep.escapes, 4):.2e}")
    assert rep.killed >= 20 and rep.survived >= 20 and min(rep.escaped[W], rep.escaped[N]) >= 50
    assert lr.nearest_edge(rep.escapes, _edges(prob)) > NEAR and lr.nearest_cosine_boundary(rep.escapes, 4) > NEAR
    _assert_against(got, want, prob.nparticles)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_degenerate_geometry(iface, make_problem, cs, monkeypatch, variant):
    """7. the beams, edges and corners of tests/test_vacuum.py's degenerate deck (stream 16^2, 96
    particles), every side vacuum: a history that leaves through a corner is scored once, through the
    side the vacuum rule names; the axis beams have mu == 1 and land in the last cosine bin, the
    diagonal ones sqrt(1/2) in bin 2 of 4."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("stream", nx=16, nparticles=96, iterations=3)
    probe = ob.OracleRun(prob, *cs)
    probe.inject()
    states = tv._degenerate_states(prob, probe.particles.as_dict())
    got = _run(iface, prob, cs, 3, variant, (None, 4), states=states, outflow=True, vacuum="all")
    want = _reference(prob, cs, got["injected"], 3, 15, (), 4)
    rep = want["rep"]
    assert sum(rep.escaped) == 96 and len({e["pid"] for e in rep.escapes}) == 96   # each history once
    assert lr.nearest_cosine_boundary(rep.escapes, 4) > NEAR
    total = sum(c for _, c in want["added"])
    assert total[:, 0, 3].sum() == 64.0 and total[:, 0, 2].sum() == 32.0      # mu == 1: the last bin; the diagonals
    _assert_against(got, want, prob.nparticles)


@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["shard", "domain 2x1"])
def test_two_ranks(iface, make_problem, cs, tmp_path, monkeypatch, mode):
    """8. two ranks on one GPU (host transport): sharded, both ranks hold the one-rank tally; on a
    mesh cut 2 x 1 the ranks' arrays sum to it.  Counts exact, weights TALLY_SUM_TOL per bin."""
    from neutral_amd import decks, host
    steps = 3
    deck = decks.write_deck("csp", str(tmp_path / "csp.params"), nx=24, ny=24, nparticles=600, iterations=steps,
                            dt=1.0e-6)
    prob = host.setup_problem(deck)
    edges = [float(e) for e in _edges(prob)]
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    one = _run(iface, prob, cs, steps, 2, (edges, 4), zero_between=False, cs_absorb=third_absorb(cs), outflow=True,
               vacuum="wn")
    ow, oc = one["read"][-1]
    assert oc[W].sum() >= 20 and oc[N].sum() >= 20
    sim_kw = dict(capture_scale=0.5, outflow=True, vacuum="wn", leakage=[edges, 4])
    argv = [sys.executable, LEAKAGE_WORKER, deck, str(tmp_path), str(steps), mode, json.dumps(sim_kw)]
    launch_ranks(argv, 2)
    ranks = [np.load(os.path.join(str(tmp_path), f"leakage{r}.npz")) for r in range(2)]
    if mode == "shard":
        tallies = [(z["weight"], z["count"]) for z in ranks]
    else:
        tallies = [(ranks[0]["weight"] + ranks[1]["weight"], ranks[0]["count"] + ranks[1]["count"])]
        assert ranks[1]["count"][W].sum() == 0.0 and ranks[0]["count"][W].sum() == oc[W].sum()   # rank 1 owns no west wall
    for w, c in tallies:
        assert np.array_equal(c, oc)
        assert np.all(np.abs(w - ow) <= TALLY_SUM_TOL * ow)


@gpu
@needs_gpu
def test_driver(iface, cs, tmp_path):
    """9. --vacuum all --leakage 4,E0,E1,E2: the totals printed per side are the sums of the per-step
    `Escaped` lines; the rows' weights sum to the side's; --leakage without --vacuum is refused"""
    import subprocess
    assert os.path.exists(OWN_DRIVER), "neutral.hip not built"
    from neutral_amd import cs_table, decks
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
    said = run_driver(str(run), rel, sets + ["--vacuum", "all", "--leakage", "4,1.0e3,1.0e5,1.0e7"])
    pattern = r"^Escaped  west (\d+) \((\S+)\) east (\d+) \((\S+)\) south (\d+) \((\S+)\) north (\d+) \((\S+)\)$"
    steps = [re.match(pattern, ln) for ln in said.splitlines() if ln.startswith("Escaped")]
    assert len(steps) == 3 and all(steps)
    for k, name in enumerate(tv.SIDE_NAMES):
        count = sum(int(m.group(1 + 2 * k)) for m in steps)
        weight = sum(float(m.group(2 + 2 * k)) for m in steps)
        block = [ln for ln in said.splitlines() if ln.startswith(f"Leakage {name} ")]
        assert len(block) == 2 + 1 + 1, block      # two groups, "no group", the totals
        assert block[0].startswith(f"Leakage {name} group 0 [") and block[2].startswith(f"Leakage {name} no group ")
        m = re.match(rf"^Leakage {name} total (\d+) \((\S+)\)$", block[-1])
        assert m, block[-1]
        assert int(m.group(1)) == count and count > 0
        assert abs(float(m.group(2)) - weight) <= 1e-8 * weight
        rows = sum(float(v) for ln in block[:-1] for v in ln.split(")")[-1].split()[-4:])
        assert abs(size["nparticles"] * rows - weight) <= 1e-8 * weight
    refused = subprocess.run([OWN_DRIVER, rel] + sets + ["--leakage", "4"], cwd=str(run), capture_output=True, text=True,
                             timeout=600)
    assert refused.returncode != 0 and "--leakage needs --vacuum" in refused.stdout + refused.stderr

"""The census weight window (include/neutral_hip.h: neutral_hip_window_particles).

CPU: the numpy restatement (tests/window_reference.py) pinned by a hand-computed store and by its
properties, the ABI, the wrapper's argument handling, the driver's usage errors, and the in-run
scenario on the oracle alone (no slot guarded, every branch taken).  GPU: bit for bit against the
restatement at every size where the scans take another path, the identity on a second call, the pid
base, refusals, nothing to do on a tiled store, the window inside a run against the CPU oracle, and
the driver's --window.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import census_ops_support
import window_reference as wr
from census_ops_support import same_bits
from conftest import ROOT
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, scan_sizes, scan_tile  # noqa: F401

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
SEED = wr.WINDOW_SEED_BASE + 7
MESH = 16


def fixed_rn0(values):
    """rn0_of for the restatement: slot -> a given sample"""
    return lambda slots: np.array([values[int(j)] for j in slots], dtype=np.float64)


# ---- CPU: the restatement --------------------------------------------------------------------

def test_hand_computed_store_of_eight():
    """2 x 2 mesh, lower = [[0.5, 0], [0.5, 0.5]], upper_ratio 2 (w_hi 1.0), survival_ratio 1.5
    (w_s 0.75), max_split 3.  Slots: 0 dead; 1 in the cell without a window; 2 light, survives
    (0.1 * 0.75 < 0.25); 3 light, dies (0.9 * 0.75 >= 0.25); 4 at 10: q = 10, m capped at 3, e = 2;
    5 at 2.5: q = 2.5, m = 3, e = 2; 6 inside its window; 7 dead.  Free: 0, 3 (freed by roulette),
    7.  Slot 4 is served in full (copies in 0 and 3), slot 5 in part (one copy, in 7), one copy is
    refused."""
    nan = np.nan
    a = {f: np.arange(8, dtype=np.float64) + 10.0 * (k + 1) for k, f in enumerate(wr.F64_FIELDS)}
    a["weight"] = np.array([nan, 100.0, 0.25, 0.25, 10.0, 2.5, 0.75, 7.0])
    a["cellx"] = np.array([-1, 1, 0, 0, 0, 1, 1, 0], dtype=np.int32)
    a["celly"] = np.array([-1, 0, 0, 1, 1, 1, 1, 0], dtype=np.int32)
    a["dead"] = np.array([1, 0, 0, 0, 0, 0, 0, 5], dtype=np.int32)
    lower = np.array([[0.5, 0.0], [0.5, 0.5]])
    r = wr.window(a, lower, 2, 2, 2.0, 1.5, 3, fixed_rn0({2: 0.1, 3: 0.9}))
    assert r.stats == dict(live_before=6, dead_before=2, below=2, roulette_killed=1, roulette_survived=1,
                           above=2, split=2, copies_made=3, copies_refused=1)
    assert (r.lost, r.gained) == (0.25, 0.5)
    assert r.demand.tolist() == [0, 0, 0, 0, 2, 2, 0, 0] and r.grants.tolist() == [0, 0, 0, 0, 2, 1, 0, 0]
    assert r.free.tolist() == [0, 3, 7]
    assert r.sources.tolist() == [4, 4, 5] and r.destinations.tolist() == [0, 3, 7]
    out = r.arrays
    assert out["dead"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0]
    assert out["weight"].tolist() == [10.0 / 3.0, 100.0, 0.75, 10.0 / 3.0, 10.0 / 3.0, 1.25, 0.75, 1.25]
    for f in wr.COPIED:
        assert out[f].tolist() == a[f][[4, 1, 2, 4, 4, 5, 6, 5]].tolist(), f
    assert not r.guarded.any()
    # without supply beyond roulette's: slot 3, freed, is the only one, and slot 4 gets it
    a["dead"][:] = 0
    a["weight"][[0, 7]] = 0.75
    a["cellx"][0] = a["celly"][0] = 0
    r = wr.window(a, lower, 2, 2, 2.0, 1.5, 3, fixed_rn0({2: 0.1, 3: 0.9}))
    assert r.free.tolist() == [3] and r.grants.tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert r.stats["copies_refused"] == 3 and r.arrays["weight"][[3, 4, 5]].tolist() == [5.0, 5.0, 2.5]
    # on the bounds themselves: inside; an ulp over the upper one: q = 1 + 2^-52, m = 2
    a["weight"][[4, 5, 6]] = [np.nextafter(1.0, 2.0), 1.0, 0.5]
    r = wr.window(a, lower, 2, 2, 2.0, 1.5, 3, fixed_rn0({2: 0.1, 3: 0.9}))
    assert r.demand.tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and r.stats["above"] == 1 and r.guarded[[4, 5, 6]].all()
    # the survival test takes the rounded product: fl(1/3) * 0.75 = 0.25 - 2^-56 rounds to 0.25
    assert wr.window(a, lower, 2, 2, 2.0, 1.5, 3, fixed_rn0({2: 1.0 / 3.0, 3: 0.9})).stats["roulette_killed"] == 2


def random_store(n, seed, dead_share=0.3, factors=None, lower=None, continuous=False):
    """n slots on the MESH x MESH mesh: cells anywhere, weights a factor times the cell's bound (on,
    beside and far from the bounds of upper_ratio 2), the other fields random, the dead slots'
    fields NaN or -1 and their dead words 1..3"""
    rng = np.random.default_rng(seed)
    if lower is None:
        lower = rng.choice([0.0, 0.25, 0.5, 1.0], size=(MESH, MESH), p=[0.1, 0.3, 0.3, 0.3])
    a = {f: rng.random(n) for f in wr.F64_FIELDS}
    a["cellx"] = rng.integers(0, MESH, n).astype(np.int32)
    a["celly"] = rng.integers(0, MESH, n).astype(np.int32)
    w_lo = lower[a["celly"], a["cellx"]]
    if continuous:
        factor = np.exp(rng.uniform(np.log(0.05), np.log(20.0), n))
    else:
        if factors is None:
            factors = [0.1, 0.5, 0.999, 1.0, 1.5, 2.0, np.nextafter(2.0, 3.0), 2.5, 3.7, 4.0, 9.3, 100.0, 1e3]
        factor = rng.choice(factors, size=n)
    a["weight"] = np.where(w_lo > 0.0, factor * w_lo, factor)
    mask = rng.random(n) < dead_share
    for f in wr.F64_FIELDS:
        a[f][mask] = np.nan
    a["cellx"][mask] = a["celly"][mask] = -1
    a["dead"] = np.where(mask, 1 + np.arange(n) % 3, 0).astype(np.int32)
    return a, lower


def numpy_rn0(seed):
    """rn0_of from numpy's generator, a function of the slot alone"""
    def rn0_of(slots):
        return np.array([np.random.default_rng([seed, int(j)]).random() for j in slots])
    return rn0_of


@pytest.mark.parametrize("n", [1, 2, 65, 1000, 20011])
def test_properties_of_the_restatement(n):
    for dead_share in (0.0, 0.05, 0.5):
        a, lower = random_store(n, n, dead_share, continuous=True)
        r = wr.window(a, lower, MESH, MESH, 2.0, 1.5, 64, numpy_rn0(n))
        out, s = r.arrays, r.stats
        live = a["dead"] == 0
        # grants in index order: the demanders are served from the first on, one in part at the most
        served = np.flatnonzero(r.demand > 0)
        full = r.grants[served] == r.demand[served]
        partial = (r.grants[served] > 0) & ~full
        assert partial.sum() <= 1 and np.all(np.diff(full.astype(int)) <= 0)
        if partial.any():
            assert full[:np.flatnonzero(partial)[0]].all() and not full[np.flatnonzero(partial)[0]:].any()
        assert s["copies_made"] == int(r.grants.sum()) == min(int(r.demand.sum()), len(r.free))
        assert s["copies_refused"] == int(r.demand.sum()) - s["copies_made"]
        assert np.array_equal(r.destinations, r.free[:s["copies_made"]]) and np.all(np.diff(r.sources) >= 0)
        assert not np.isin(r.destinations, r.sources).any()
        # a split conserves weight to one rounding per particle: (1 + g) * fl(w / (1 + g)) against w
        split = np.flatnonzero(r.grants > 0)
        assert np.all(out["weight"][split] == a["weight"][split] / (1 + r.grants[split]).astype(np.float64))
        parts = (1 + r.grants[split]) * out["weight"][split]
        assert np.all(np.abs(parts - a["weight"][split]) <= 2 * (1 + r.grants[split]) * np.spacing(out["weight"][split]))
        for f in wr.COPIED:
            assert same_bits(out[f][r.destinations], a[f][r.sources]), f
        assert np.all(out["weight"][r.destinations] == out["weight"][r.sources])
        # nobody else is touched
        touched = np.zeros(n, dtype=bool)
        touched[r.destinations] = touched[split] = True
        touched[np.flatnonzero(live & (out["dead"] != 0))] = True
        touched |= live & (out["dead"] == 0) & (out["weight"] != a["weight"])
        for f in wr.FIELDS:
            assert same_bits(out[f][~touched], a[f][~touched]), f
        # the identity on a second call, whatever the seed, where supply sufficed and max_split did not bind
        if s["copies_refused"] == 0 and not r.guarded.any():
            again = wr.window(out, lower, MESH, MESH, 2.0, 1.5, 64, numpy_rn0(n + 1))
            assert (again.stats["below"], again.stats["above"], again.stats["copies_made"]) == (0, 0, 0)
            for f in wr.FIELDS:
                assert same_bits(again.arrays[f], out[f]), f
    # what the call refuses
    a, lower = random_store(100, 1, 0.3)
    ok = (a, lower, MESH, MESH, 2.0, 1.5, 5, numpy_rn0(0))
    assert wr.window(*ok) is not None
    for k, v in ((4, 1.9), (4, np.inf), (5, 0.9), (5, 2.1), (5, np.nan), (6, 1), (6, 65), (2, 0)):
        bad = list(ok)
        bad[k] = v
        assert wr.window(*bad) is None, (k, v)
    j = int(np.flatnonzero(a["dead"] == 0)[0])
    for f, v in (("cellx", MESH), ("celly", -1), ("weight", -0.5), ("weight", np.nan), ("weight", np.inf)):
        b = {g: a[g].copy() for g in wr.FIELDS}
        b[f][j] = v
        assert wr.window(b, *ok[1:]) is None, (f, v)
    for v in (-0.25, np.nan, np.inf):
        worse = lower.copy()
        worse[a["celly"][j], a["cellx"][j]] = v
        assert wr.window(a, worse, *ok[2:]) is None, v


# ---- CPU: the ABI, the wrapper, the driver ---------------------------------------------------

def test_library_exports_the_window():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_window_particles")
    assert "neutral_hip_window_particles" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.WindowStats._fields_] == [
        "live_before", "dead_before", "below", "roulette_killed", "roulette_survived", "above", "split",
        "copies_made", "copies_refused", "roulette_weight_lost", "roulette_weight_gained", "window_ms"]
    assert C.sizeof(iface.WindowStats) == 96
    assert iface.WINDOW_SEED_BASE == 2 ** 63 + 2 ** 62 == wr.WINDOW_SEED_BASE
    text = open(os.path.join(ROOT, "include", "neutral_hip.h")).read()
    assert "neutral_hip_window_particles" in text and "a second call with any seed is the identity" in text


def test_wrapper_argument_handling():
    from neutral_amd import interface as iface
    with pytest.raises(ValueError):
        iface.window_particles(None, 16, 4, 4, 1, 5.0, 3.0, 5, 0)  # no store
    store = C.pointer(iface.Particle())
    good = dict(n=16, nx=4, ny=4, max_split=5, seed=0)
    for k, v in (("n", 0), ("n", -5), ("n", 2 ** 31), ("nx", 0), ("ny", -1), ("seed", -1), ("seed", 2 ** 64),
                 ("max_split", 2 ** 31)):
        kw = dict(good, **{k: v})
        with pytest.raises(ValueError):
            iface.window_particles(store, kw["n"], kw["nx"], kw["ny"], 1, 5.0, 3.0, kw["max_split"], kw["seed"])
    for k, v in (("n", 16.5), ("nx", 4.0), ("max_split", 2.5), ("seed", 0.5), ("n", True)):
        kw = dict(good, **{k: v})
        with pytest.raises(TypeError):
            iface.window_particles(store, kw["n"], kw["nx"], kw["ny"], 1, 5.0, 3.0, kw["max_split"], kw["seed"])
    # the library itself: refusals that need no device to say so (lower: any non-null address)
    lib, stats = iface.library(), iface.WindowStats()
    mesh = np.ones(16)
    lower = mesh.ctypes.data
    assert lib.neutral_hip_window_particles(None, 16, 4, 4, lower, 5.0, 3.0, 5, 0, C.byref(stats)) == 1
    assert lib.neutral_hip_window_particles(store, 16, 4, 4, None, 5.0, 3.0, 5, 0, None) == 1
    for n, nx, ny in ((0, 4, 4), (-1, 4, 4), (16, 0, 4), (16, 4, 0)):
        assert lib.neutral_hip_window_particles(store, n, nx, ny, lower, 5.0, 3.0, 5, 0, None) == 1
    nan, inf = float("nan"), float("inf")
    for upper, survival, most in ((nan, 3.0, 5), (inf, 3.0, 5), (1.999, 1.5, 5), (5.0, nan, 5), (5.0, inf, 5),
                                  (5.0, 0.999, 5), (5.0, 5.001, 5), (5.0, 3.0, 1), (5.0, 3.0, 65),
                                  (5.0, 3.0, 0), (5.0, 3.0, -3)):
        assert lib.neutral_hip_window_particles(store, 16, 4, 4, lower, upper, survival, most, 0,
                                                C.byref(stats)) == 1, (upper, survival, most)
        assert stats.live_before == 0 and stats.copies_made == 0
    with pytest.raises(iface.WindowRefused) as refused:
        iface.window_particles(store, 16, 4, 4, lower, 1.5, 1.0, 5, 0)
    assert refused.value.code == 1 and issubclass(iface.WindowRefused, ValueError)


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("extra", [["--window"], ["--window", "0"], ["--window", "-0.5"], ["--window", "x"],
                                   ["--window", "0.3,"], ["--window", "0.3,1.5"], ["--window", "0.3,x"],
                                   ["--window", "0.3,2,0.5"], ["--window", "0.3,2,2.5"],
                                   ["--window", "0.3,2,1.5,7"], ["--window", "0.3,2,nan"],
                                   ["--window", "0.3", "--decompose", "1x1"],
                                   ["--decompose", "1x1", "--window", "0.3,2,1.5"]])
def test_driver_usage_errors(tmp_path, extra):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + extra, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    said = out.stderr + out.stdout
    if "--decompose" in extra:
        assert "--window does not work with --decompose" in said
    else:
        assert "--window wants WLOW[,UPPER_RATIO[,SURVIVAL_RATIO]]" in said


# ---- the in-run scenario: steps, window, steps, window, steps --------------------------------

ON = (0.25, 0.5)  # roulette in the collision kernels
RUN = dict(nx=24, nparticles=6000, iterations=9, dt=2.0e-6)
RUN_RATIOS = dict(upper_ratio=2.0, survival_ratio=1.7, max_split=5)
RUN_STEPS = ((1, 2, 3), (4, 5, 6), (7, 8, 9))  # a window after the first two groups


def run_meshes():
    """The two windows of the scenario on the 24 x 24 csp mesh (source box: cells 2..7, dense block:
    cells 9..14).  The block is so dense that a history that collides in it goes on colliding until
    roulette ends it within the step: at a census every live weight is what injection or a window
    gave out -- 1, then 0.5 (split in two), 2.55 (a survivor of the first window), 1.02 (of the
    second) -- and the bounds below stay clear of all of them and of their quotients.
    First: 0.3 outside the block (a history at 1 is split in two where a slot is free; most are
    refused), 1.5 inside (one at 1 plays roulette for 2.55).  Second: 0.3 outside, 0.6 inside (0.5
    plays roulette for 1.02, 2.55 asks for three), 0.1 in the corner that holds the source, where a
    history at 1 asks for five and one at 0.5 for three."""
    first = np.full((24, 24), 0.3)
    first[9:15, 9:15] = 1.5
    second = np.full((24, 24), 0.3)
    second[9:15, 9:15] = 0.6
    second[0:9, 0:9] = 0.1
    return first, second


def apply_to_oracle(ref, lower, tt):
    """the restatement on the oracle's arrays, in place; -> Result"""
    arrays = ref.particles.as_dict()
    r = wr.window(arrays, lower, 24, 24, RUN_RATIOS["upper_ratio"], RUN_RATIOS["survival_ratio"],
                  RUN_RATIOS["max_split"], wr.cpu_rn0(0, wr.WINDOW_SEED_BASE + tt))
    assert r is not None
    for f in wr.FIELDS:
        arrays[f][:] = r.arrays[f]
    return r


def _oracle_run(make_problem, cs):
    import oracle_binding as ob
    keys, values = cs
    absorb = (np.array(keys), 0.5 * np.array(values))  # capture = scatter / 2: p_absorb = 1/3
    prob = make_problem("csp", **RUN)
    ref = ob.OracleRun(prob, keys, values, cs_absorb=absorb, roulette=ON)
    ref.inject()
    return prob, keys, values, absorb, ref


def test_the_scenario_on_the_oracle_takes_every_branch_unguarded(make_problem, cs):
    _, _, _, _, ref = _oracle_run(make_problem, cs)
    results = []
    for steps, lower in zip(RUN_STEPS, run_meshes() + (None,)):
        for tt in steps:
            ref.step(tt)
        if lower is not None:
            results.append(apply_to_oracle(ref, lower, steps[-1]))
    for r in results:
        print(r.stats)
        assert not r.guarded.any(), np.flatnonzero(r.guarded)
        assert r.stats["split"] > 0 and r.stats["roulette_killed"] > 0 and r.stats["roulette_survived"] > 0
    assert results[0].stats["copies_refused"] + results[1].stats["copies_refused"] > 0
    assert results[1].stats["copies_refused"] > 0 and results[1].stats["copies_made"] > 0


# ---- GPU: the window alone -------------------------------------------------------------------


class WindowStore(census_ops_support.Store):
    """the store, on a MESH x MESH mesh, with the window's call"""

    def __init__(self, iface, make_problem, cs, n, pid_base=0):
        super().__init__(iface, make_problem, cs, n, pid_base, nx=MESH)

    def raw(self, lower, upper_ratio=2.0, survival_ratio=1.5, max_split=5, seed=SEED, nx=MESH, ny=MESH,
            null_lower=False):
        """the library's own call: -> (return code, stats)"""
        stats = self.iface.WindowStats()
        self.iface.set_pid_base(self.sim.pid_base)
        d_lower = self.torch.from_numpy(np.ascontiguousarray(lower, dtype=np.float64).ravel()).to(self.sim.device)
        rc = self.iface.library().neutral_hip_window_particles(
            self.sim.particles, self.n, nx, ny, None if null_lower else d_lower.data_ptr(), upper_ratio,
            survival_ratio, max_split, seed, C.byref(stats))
        return rc, stats


def _patterns(n):
    """name -> (arrays, lower, max_split)"""
    tile = scan_tile()
    out = {"mixed": random_store(n, n) + (5,)}
    if n > 200000:
        return out  # (the second level of tile sums: one pattern, for the time it takes)
    heavy_only = [1.0, 1.5, 2.0, 2.5, 3.7, 9.3, 100.0]
    out["demand, no supply"] = random_store(n, n + 1, 0.0, factors=heavy_only) + (5,)
    out["everybody over the bound"] = random_store(n, n + 2, 0.1, factors=[2.5, 4.1, 7.0, 300.0],
                                                   lower=np.full((MESH, MESH), 0.5)) + (64,)
    out["supply from roulette only"] = random_store(n, n + 3, 0.0) + (5,)
    yy, xx = np.mgrid[0:MESH, 0:MESH]
    out["checkerboard"] = random_store(n, n + 4, 0.3, lower=np.where((xx + yy) % 2 == 1, 0.5, 0.0)) + (7,)
    for name, at in (("partial grant before a tile boundary", tile - 1), ("partial grant after a tile boundary", tile)):
        if n > at + 1:
            # slot 3 asks for one copy, slot `at` for four; three slots are free: slot `at` gets two
            a, lower = random_store(n, n + 5, 0.0, factors=[1.5], lower=np.full((MESH, MESH), 0.5))
            a["weight"][3] = 0.5 * 2.0 * 1.5
            a["weight"][at] = 0.5 * 2.0 * 4.5
            for j in (5, at + 1, n - 1) if at + 1 < n - 1 else (5, 6, n - 1):
                a["dead"][j] = 2
                a["weight"][j] = np.nan
                a["cellx"][j] = -1
            out[name] = (a, lower, 5)
    if n == 100003:
        a, lower = random_store(n, n + 6, 1.0, lower=np.full((MESH, MESH), 0.5))
        a["dead"][77777] = 0
        a["cellx"][77777] = a["celly"][77777] = 3
        for f in wr.F64_FIELDS:
            a[f][77777] = 0.125
        a["weight"][77777] = 1e6
        out["one heavy history among the dead"] = (a, lower, 64)
    return out


def _check_against_restatement(iface, st, a, lower, max_split, name, pid_base=0, seed=SEED, upper_ratio=2.0,
                               survival_ratio=1.5, upload=True):
    """upload=False: `a` is what the store holds already"""
    if upload:
        st.upload(a)
    rc, stats = st.raw(lower, upper_ratio, survival_ratio, max_split, seed)
    assert rc == 0, name
    r = wr.window(a, lower, MESH, MESH, upper_ratio, survival_ratio, max_split, wr.probe_rn0(iface, pid_base, seed))
    assert {k: getattr(stats, k) for k in wr.STAT_NAMES} == r.stats, name
    after = st.arrays()
    for f in wr.FIELDS:  # every field of every slot, the untouched ones' NaN scribbles included
        assert same_bits(after[f], r.arrays[f]), (name, f, np.flatnonzero(
            after[f].view(np.uint32 if f in wr.I32_FIELDS else np.uint64) !=
            r.arrays[f].view(np.uint32 if f in wr.I32_FIELDS else np.uint64))[:8])
    live = a["dead"] == 0
    bound = st.n * 2.0 ** -53 * float(np.abs(a["weight"][live]).sum())
    print(f"n={st.n} {name}: {r.stats} lost {stats.roulette_weight_lost!r} ({r.lost!r}) gained "
          f"{stats.roulette_weight_gained!r} ({r.gained!r}) bound {bound:.3e} window_ms {stats.window_ms:.3f}")
    assert abs(stats.roulette_weight_lost - r.lost) <= bound, name
    assert abs(stats.roulette_weight_gained - r.gained) <= bound, name
    return r, stats


@gpu
@needs_gpu
@pytest.mark.parametrize("n", scan_sizes())
def test_bit_for_bit_against_the_restatement(iface, make_problem, cs, n):
    st = WindowStore(iface, make_problem, cs, n)
    seen = dict.fromkeys(("split", "roulette_killed", "roulette_survived", "copies_refused"), 0)
    for name, (a, lower, max_split) in _patterns(n).items():
        r, _ = _check_against_restatement(iface, st, a, lower, max_split, name)
        for k in seen:
            seen[k] += r.stats[k]
        if name.startswith("partial grant"):
            at = scan_tile() - 1 if "before" in name else scan_tile()
            assert r.grants[3] == 1 and r.grants[at] == 2 and r.demand[at] == 4, name
        if name.startswith("one heavy"):
            assert r.stats["copies_made"] == 63 and r.stats["split"] == 1
    if n >= 1000:
        assert all(seen.values()), seen
    st.close()


@gpu
@needs_gpu
def test_identity_on_a_second_call(iface, make_problem, cs):
    n = 100003
    st = WindowStore(iface, make_problem, cs, n)
    a, lower = random_store(n, 11, 0.6, continuous=True)
    r, stats = _check_against_restatement(iface, st, a, lower, 64, "first call")
    assert not r.guarded.any() and stats.copies_refused == 0 and stats.split > 0 and stats.roulette_killed > 0
    assert int(r.demand.max()) + 1 < 64  # (max_split did not bind)
    first = st.arrays()
    rc, again = st.raw(lower, max_split=64, seed=SEED + 12345)
    assert rc == 0
    assert (again.below, again.above, again.split, again.copies_made, again.copies_refused) == (0, 0, 0, 0, 0)
    assert again.live_before == stats.live_before - stats.roulette_killed + stats.copies_made
    second = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(second[f], first[f]), f
    st.close()


@gpu
@needs_gpu
def test_workspace_grows_between_operations_on_one_store(iface, make_problem, cs):
    """One store at the first size with a level of tile sums: a source call, whose workspace is its
    list and tile sums alone, a comb, which needs four times as much per slot, then a window, which
    needs a byte per slot more: the allocation grows between every two of the calls; then a second
    window in the workspace as it stands.  Each window bit
    for bit against the restatement on the arrays read back just before it; of the source and the
    comb, the return codes and what their stats must say."""
    n = scan_tile() + 1
    st = WindowStore(iface, make_problem, cs, n)
    lib = iface.library()
    a, _ = random_store(n, n)
    st.upload(a)
    ndead = int((a["dead"] != 0).sum())
    assert ndead > 100
    iface.set_pid_base(st.sim.pid_base)
    source = iface.SourceStats()
    assert lib.neutral_hip_source_particles(st.sim.particles, n, ndead // 2, 0.5, SEED, *st.sim._inject_args(),
                                            C.byref(source)) == 0
    assert (source.dead_before, source.emitted, source.weight_emitted) == (ndead, ndead // 2, 0.5 * (ndead // 2))
    comb = iface.CombStats()
    assert lib.neutral_hip_comb_particles(st.sim.particles, n, SEED, C.byref(comb)) == 0
    assert comb.live_before == n - ndead + ndead // 2 and comb.weight_each > 0.0
    combed = st.arrays()
    assert not combed["dead"].any() and np.all(combed["weight"] == comb.weight_each)
    # bounds around the one weight: no window, over the bound (two for one), inside, under it
    rng = np.random.default_rng(n)
    first, second = (rng.choice([0.0, 0.3, 0.8, 2.0], size=(MESH, MESH)) * comb.weight_each for _ in range(2))
    r, _ = _check_against_restatement(iface, st, combed, first, 5, "first window", upload=False)
    assert r.stats["roulette_killed"] > 0 and r.stats["roulette_survived"] > 0 and r.stats["copies_made"] > 0
    # ... and the weights the first one left (w / 2, w, 3 w) against other bounds
    r, _ = _check_against_restatement(iface, st, st.arrays(), second, 5, "second window", seed=SEED + 1, upload=False)
    assert r.stats["below"] > 0 and r.stats["copies_made"] > 0
    st.close()


@gpu
@needs_gpu
def test_pid_base_moves_the_draws(iface, make_problem, cs):
    n, base = 5000, 123456789
    a, lower = random_store(n, 12, 0.2, factors=[0.3, 0.5, 0.7, 1.5, 4.5])
    dead = {}
    for pid_base in (0, base):
        st = WindowStore(iface, make_problem, cs, n, pid_base=pid_base)
        _check_against_restatement(iface, st, a, lower, 5, f"pid base {pid_base}", pid_base=pid_base)
        dead[pid_base] = st.arrays()["dead"]
        # ... and through the wrapper, which names the base itself
        st.upload(a)
        stats = st.sim.window(lower, upper_ratio=2.0, survival_ratio=1.5, max_split=5, seed=SEED)
        assert stats.roulette_killed > 100 and np.array_equal(st.arrays()["dead"], dead[pid_base])
        st.close()
    assert not np.array_equal(dead[0], dead[base])  # the same slots, other draws


REFUSALS = ["lower null", "nx 0", "ny 0", "upper nan", "upper inf", "upper 1.9", "survival nan", "survival 0.9",
            "survival over upper", "max_split 1", "max_split 65", "cellx beyond", "celly negative",
            "weight negative", "weight nan", "weight inf", "bound negative", "bound nan", "bound inf"]


@gpu
@needs_gpu
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_the_store_untouched(iface, make_problem, cs, case):
    n = 5000
    st = WindowStore(iface, make_problem, cs, n)
    a, lower = random_store(n, 13, 0.3)
    j = int(np.flatnonzero(a["dead"] == 0)[-1])  # (the last live slot: beyond the first tile)
    kw = {"lower null": dict(null_lower=True), "nx 0": dict(nx=0), "ny 0": dict(ny=0),
          "upper nan": dict(upper_ratio=float("nan")), "upper inf": dict(upper_ratio=float("inf")),
          "upper 1.9": dict(upper_ratio=1.9), "survival nan": dict(survival_ratio=float("nan")),
          "survival 0.9": dict(survival_ratio=0.9), "survival over upper": dict(survival_ratio=2.5),
          "max_split 1": dict(max_split=1), "max_split 65": dict(max_split=65)}.get(case, {})
    if case == "cellx beyond":
        a["cellx"][j] = MESH
    elif case == "celly negative":
        a["celly"][j] = -1
    elif case.startswith("weight"):
        a["weight"][j] = {"negative": -0.5, "nan": np.nan, "inf": np.inf}[case.split()[1]]
    elif case.startswith("bound"):
        lower = lower.copy()
        lower[a["celly"][j], a["cellx"][j]] = {"negative": -0.25, "nan": np.nan, "inf": np.inf}[case.split()[1]]
    st.upload(a)
    rc, stats = st.raw(lower, **kw)
    assert rc == 1
    assert (stats.below, stats.split, stats.copies_made, stats.roulette_killed) == (0, 0, 0, 0)
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], a[f]), f
    if not kw or case in ("upper 1.9", "max_split 65"):  # ... and through the wrapper
        with pytest.raises(iface.WindowRefused) as refused:
            st.sim.window(lower, upper_ratio=kw.get("upper_ratio", 2.0), survival_ratio=1.5,
                          max_split=kw.get("max_split", 5), seed=SEED)
        assert refused.value.code == 1
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_nothing_to_do_on_a_tiled_store_changes_nothing(iface, make_problem, cs, lazy, monkeypatch):
    """A window that every history is inside returns 0, writes nothing and leaves the records of a
    tiled store valid: the next step pays no re-import.  The step's stats show one, as
    tests/test_source.py::test_nobody_dead_on_a_tiled_store_changes_nothing explains: a steady step
    waits for the device once, a step after an import more often."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")

    def call(sim):
        stats = sim.window(0.5)  # every weight is 1: inside [0.5, 2.5]
        assert stats.live_before == 30000
        assert (stats.dead_before, stats.below, stats.above, stats.copies_made, stats.copies_refused) == (0,) * 5
        stats = sim.window(np.zeros((400, 400)))  # no window anywhere
        assert (stats.live_before, stats.below, stats.above) == (30000, 0, 0)

    census_ops_support.check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call)


# ---- GPU: the window in a run, against the oracle --------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_window_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """Steps, window, steps, window, steps: the library (records written back before the window,
    imported again after it, graveyard slots among the refilled) against oracle steps with the
    restatement applied to the oracle's arrays."""
    prob, keys, values, absorb, ref = _oracle_run(make_problem, cs)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=ON, cs_absorb=absorb)
    sim.inject()

    def both_step(tt):
        g, c = sim.step(tt), ref.step(tt)
        assert (g.nprocessed, g.facets, g.collisions, g.census) == \
            (c.nprocessed, c.facets, c.collisions, c.census), tt
        assert (g.stats.roulette_killed, g.stats.roulette_survived) == \
            (c.roulette_killed, c.roulette_survived), tt
        return c

    expect = None
    for steps, lower in zip(RUN_STEPS, run_meshes() + (None,)):
        for tt in steps:
            c = both_step(tt)
            assert expect is None or c.nprocessed == expect  # (the copies are stepped, the killed are not)
            expect = None
        if lower is None:
            break
        live = int((ref.particles.as_dict()["dead"] == 0).sum())
        r = apply_to_oracle(ref, lower, steps[-1])
        assert not r.guarded.any()
        stats = sim.window(lower, **RUN_RATIOS)  # (seed: 2^63 + 2^62 + the last master key)
        assert {k: getattr(stats, k) for k in wr.STAT_NAMES} == r.stats
        assert stats.live_before == live and stats.split > 0 and stats.roulette_killed > 0
        got = sim.particle_arrays()
        want = ref.particles.as_dict()
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(got[f], want[f]), f
        assert np.max(np.abs(got["weight"] - want["weight"])[want["dead"] == 0]) <= 1e-9
        expect = live - stats.roulette_killed + stats.copies_made
    got, want = sim.particle_arrays(), ref.particles.as_dict()
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got[f], want[f]), f
    tg, tc = sim.tally_host(), ref.tally
    print(f"variant {variant} lazy {lazy}: tally rel L2 {np.linalg.norm(tg - tc) / np.linalg.norm(tc):.3e} "
          f"worst cell {np.max(np.abs(tg - tc) / np.maximum(np.abs(tc), 1e-300)):.3e}")
    assert np.linalg.norm(tg - tc) / np.linalg.norm(tc) < TALLY_L2_TOL
    assert np.all(np.abs(tg - tc) <= TALLY_L2_TOL * np.abs(tc))
    sim.close()


# ---- GPU: the driver's --window --------------------------------------------------------------

def _window_totals(stdout):
    names = ("roulette killed", "roulette survived", "split", "copies made", "copies refused")
    totals = {k: int(re.search(rf"^Window {k} (\d+)$", stdout, flags=re.M).group(1)) for k in names}
    facets = [int(x) for x in re.findall(r"^Facets\s+(\d+)", stdout, flags=re.M)]
    return totals, facets


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_window_on_one_rank_and_on_two(tmp_path):
    """`neutral.hip --roulette 0.25,0.5 --window 0.3,2,1.6`: after every step but the last the
    histories at 1 are split in two into the slots roulette has freed; two ranks (both on one GPU)
    window their own shards.  At a census of this deck every live weight is what injection or a
    window gave out (tests above: run_meshes), so a uniform window plays roulette only where it
    lies over them: `--window 1.2,2,1.6` makes every history play for 1.92 after the first step and
    finds the survivors inside from then on.  Without the flag stdout says nothing of a window."""
    from neutral_amd import cs_table, decks
    from gpu_support import run_driver
    run = tmp_path / "run"
    (tmp_path / "arch").mkdir()
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    sets = ["--roulette", "0.25,0.5"]
    for kv in ("nx=64", "ny=64", "nparticles=100001", "iterations=6", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), rel, sets)
    assert "Window" not in plain
    plain_facets = [int(x) for x in re.findall(r"^Facets\s+(\d+)", plain, flags=re.M)]
    totals, facets = _window_totals(run_driver(str(run), rel, sets + ["--window", "0.3,2,1.6"]))
    print(totals)
    assert totals["copies made"] >= totals["split"] > 0 and totals["copies refused"] > 0
    assert totals["roulette killed"] == totals["roulette survived"] == 0
    assert facets[0] == plain_facets[0] and facets[-1] > plain_facets[-1]
    high, high_facets = _window_totals(run_driver(str(run), rel, sets + ["--window", "1.2,2,1.6"]))
    print(high)
    assert high["roulette killed"] > 0 and high["roulette survived"] > 0
    assert high["roulette killed"] + high["roulette survived"] == 100001  # (everybody, once)
    assert high["split"] == high["copies made"] == high["copies refused"] == 0
    assert high_facets[0] == plain_facets[0] and high_facets[-1] < plain_facets[-1]
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    totals2, facets2 = _window_totals(
        run_driver(str(run), rel, sets + ["--gpus", "2", "--window", "0.3,2,1.6"], env))
    print(totals2)
    # (the first window's roulette is the same draws on the same histories; the copies then land in
    # other slots of the two shards, and the runs part)
    assert facets2[0] == plain_facets[0] and facets2[-1] > plain_facets[-1]
    assert totals2["copies made"] >= totals2["split"] > 0 and totals2["roulette killed"] == 0

"""The census tally and the window bounds made from it (include/neutral_hip.h:
neutral_hip_census_tally, neutral_hip_window_bounds).

CPU: the numpy restatement (tests/census_reference.py) pinned by a hand-computed store and by its
properties, the ABI, the wrappers' argument handling, the driver's usage errors, and the two
scenarios of the GPU part on the restatements and the oracle alone (no copy refused; a split and a
roulette in the run).  GPU: the census against the restatement (counts exactly, weights bit for bit
where every partial sum is exact and within the any-order bound elsewhere), snapshot semantics,
refusals, a tiled store, the bounds bit for bit, the loop of census, bounds and window, both inside a
run against the CPU oracle, and the driver's --window auto.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import census_ops_support
import census_reference as cr
import window_reference as wr
from conftest import ROOT
from census_ops_support import same_bits
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, scan_tile  # noqa: F401

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
EPS = 2.0 ** -53
SEED = wr.WINDOW_SEED_BASE + 7
MESHES = ((1, 1), (3, 5), (16, 16))  # (nx, ny): one address; not square; several tiles of nothing


def kernel_constant(name):
    text = open(os.path.join(ROOT, "neutral_amd", "csrc", "neutral_kernels.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def random_store(n, seed, nx, ny, dead_share=0.3, weights="dyadic"):
    """n slots on an nx x ny mesh: cells anywhere; weights multiples of 2^-10 in [2^-10, 8] (every
    partial sum of up to 2^40 of them is exact) or log-uniform in [2^-20, 2^10]; the other fields
    random; the dead slots' f64 fields NaN, their cells -1 and their dead words 1..3"""
    rng = np.random.default_rng(seed)
    a = {f: rng.random(n) for f in wr.F64_FIELDS}
    a["cellx"] = rng.integers(0, nx, n).astype(np.int32)
    a["celly"] = rng.integers(0, ny, n).astype(np.int32)
    if weights == "dyadic":
        a["weight"] = rng.integers(1, 8193, n).astype(np.float64) * 2.0 ** -10
    else:
        a["weight"] = np.exp2(rng.uniform(-20.0, 10.0, n))
    mask = rng.random(n) < dead_share
    for f in wr.F64_FIELDS:
        a[f][mask] = np.nan
    a["cellx"][mask] = a["celly"][mask] = -1
    a["dead"] = np.where(mask, 1 + np.arange(n) % 3, 0).astype(np.int32)
    return a


# ---- CPU: the restatement --------------------------------------------------------------------

def hand_store():
    """2 x 2 mesh.  Slot 0 dead (cell -1, NaN); 1 and 2 in cell 0 (1.0 + 0.5); 3, 4, 5 in cell 1
    (4 + 2 + 2); nobody in cell 2; 6 and 7 in cell 3 (3.5 + 0.5)."""
    nan = np.nan
    a = {f: np.arange(8, dtype=np.float64) for f in wr.F64_FIELDS}
    a["weight"] = np.array([nan, 1.0, 0.5, 4.0, 2.0, 2.0, 3.5, 0.5])
    a["cellx"] = np.array([-1, 0, 0, 1, 1, 1, 1, 1], dtype=np.int32)
    a["celly"] = np.array([-1, 0, 0, 0, 0, 0, 1, 1], dtype=np.int32)
    a["dead"] = np.array([2, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    return a


def test_hand_computed_store_of_eight():
    """Census: counts 2, 3, 0, 2; weights 1.5, 8, 0, 4.  Bounds for 6 histories, upper_ratio 2,
    floor_ratio 0.25, min_count 1: K = 3, M = 8, a = 6, b = 48, d = fl(3 * 6) = 18, peak = fl(48 / 18);
    cell 0: r = 0.1875, held up by the floor: 0.25 * peak; cell 1: r = 1: peak; cell 2: not eligible:
    0; cell 3: r = 0.5: peak / 2."""
    c = cr.census(hand_store(), 2, 2)
    assert c.count.tolist() == [2.0, 3.0, 0.0, 2.0] and c.weight.tolist() == [1.5, 8.0, 0.0, 4.0]
    assert c.stats == dict(live=7, dead=1, occupied_cells=3, max_count=3, weight=13.5, max_cell_weight=8.0)
    b = cr.bounds(c.count, c.weight, 6.0, 2.0, 0.25, 1)
    assert b.peak == 2.6666666666666665 == 48.0 / 18.0
    assert b.lower.tolist() == [0.6666666666666666, 2.6666666666666665, 0.0, 1.3333333333333333]
    assert b.eligible.tolist() == [True, True, False, True]
    assert b.stats == dict(windowed_cells=3, floored_cells=1, max_cell_weight=8.0, lower_at_peak=2.6666666666666665)
    # min_count 3 leaves cell 1 alone: K = 1, peak = fl(16 / 18)
    b = cr.bounds(c.count, c.weight, 6.0, 2.0, 0.25, 3)
    assert b.lower.tolist() == [0.0, 0.8888888888888888, 0.0, 0.0] and b.stats["windowed_cells"] == 1
    # the population the bounds settle: every eligible cell at 2 M / (peak (1 + U)) = T / K histories
    b = cr.bounds(c.count, c.weight, 6.0, 2.0, 0.0, 1)
    settle = c.weight[b.eligible] / (b.lower[b.eligible] * 1.5)
    assert np.allclose(settle, 2.0) and math.isclose(settle.sum(), 6.0)


@pytest.mark.parametrize("n", [1, 2, 65, 1000, 20011])
def test_properties_of_the_restatement(n):
    for nx, ny in MESHES:
        for dead_share in (0.0, 0.3):
            for weights in ("dyadic", "continuous"):
                a = random_store(n, n, nx, ny, dead_share, weights)
                c = cr.census(a, nx, ny)
                live = a["dead"] == 0
                assert c.count.sum() == c.stats["live"] == live.sum() and c.stats["dead"] == n - live.sum()
                assert c.stats["occupied_cells"] == len(set(zip(a["cellx"][live], a["celly"][live])))
                assert np.all((c.weight > 0) == (c.count > 0))  # (every live weight is positive here)
                assert abs(c.weight.sum() - a["weight"][live].sum()) <= 1e-12 * a["weight"][live].sum()
                if not live.any():
                    assert cr.bounds(c.count, c.weight, 10.0, 2.0, 0.0, 1) is None  # K == 0
                    continue
                for floor in (0.0, 0.25, 1.0):
                    for min_count in (1, 3):
                        b = cr.bounds(c.count, c.weight, float(live.sum()), 2.0, floor, min_count)
                        eligible = (c.count >= min_count) & (c.weight > 0)
                        if not eligible.any():
                            assert b is None
                            continue
                        assert np.array_equal(b.lower > 0, eligible) and np.array_equal(b.eligible, eligible)
                        assert b.lower.max() == b.peak == b.stats["lower_at_peak"]
                        m = c.weight[eligible].max()
                        assert np.array_equal(b.lower[eligible] / b.peak, np.maximum(c.weight[eligible] / m, floor)) or \
                            np.allclose(b.lower[eligible] / b.peak, np.maximum(c.weight[eligible] / m, floor), rtol=4 * EPS, atol=0)
                        assert b.stats["windowed_cells"] == eligible.sum()
                        assert b.stats["floored_cells"] == (c.weight[eligible] / m < floor).sum()
    # what the census refuses
    a = random_store(100, 1, 16, 16, 0.3)
    j = int(np.flatnonzero(a["dead"] == 0)[0])
    k = int(np.flatnonzero(a["dead"] != 0)[0])
    for f, v in (("cellx", 16), ("celly", -1), ("weight", -0.5), ("weight", np.nan), ("weight", np.inf)):
        b = {g: a[g].copy() for g in wr.FIELDS}
        b[f][j] = v
        assert cr.census(b, 16, 16) is None, (f, v)
        b = {g: a[g].copy() for g in wr.FIELDS}
        b[f][k] = v
        assert cr.census(b, 16, 16) is not None, (f, v)  # (on a dead slot: no refusal)
    a["dead"][:] = 1
    c = cr.census(a, 16, 16)
    assert c.stats["live"] == 0 and c.stats["occupied_cells"] == 0 and not c.count.any() and not c.weight.any()
    # ... and the bounds
    ok = (np.array([2.0, 1.0]), np.array([1.0, 3.0]), 5.0, 2.0, 0.0, 1)
    assert cr.bounds(*ok) is not None
    for i, v in ((2, 0.0), (2, -1.0), (2, np.inf), (2, np.nan), (3, 1.5), (3, np.inf), (4, -0.1), (4, 1.5),
                 (4, np.nan), (5, 0), (0, np.array([2.0, -1.0])), (1, np.array([np.nan, 3.0])),
                 (1, np.array([np.inf, 3.0])), (1, np.zeros(2))):
        bad = list(ok)
        bad[i] = v
        assert cr.bounds(*bad) is None, (i, v)


# ---- CPU: the ABI, the wrappers, the driver --------------------------------------------------

def test_library_exports_census_and_bounds():
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in ("neutral_hip_census_tally", "neutral_hip_window_bounds"):
        assert hasattr(lib, name) and name in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.CensusStats._fields_] == [
        "live", "dead", "occupied_cells", "max_count", "weight", "max_cell_weight", "census_ms"]
    assert C.sizeof(iface.CensusStats) == 56
    assert [f[0] for f in iface.BoundsStats._fields_] == [
        "windowed_cells", "floored_cells", "max_cell_weight", "lower_at_peak", "bounds_ms"]
    assert C.sizeof(iface.BoundsStats) == 40
    text = open(os.path.join(ROOT, "include", "neutral_hip.h")).read()
    assert "neutral_hip_census_tally(" in text and "neutral_hip_window_bounds(" in text
    assert "A SNAPSHOT, NOT AN ACCUMULATOR" in text and "(m - 1) * 2^-53 * S" in text
    assert all(hasattr(iface.Simulation, m) for m in ("census", "auto_window"))
    assert issubclass(iface.CensusRefused, ValueError) and issubclass(iface.BoundsRefused, ValueError)


def test_wrapper_argument_handling():
    import torch
    from neutral_amd import interface as iface
    with pytest.raises(ValueError):
        iface.census_tally(None, 16, 4, 4)  # no store
    store = C.pointer(iface.Particle())
    good = dict(n=16, nx=4, ny=4)
    for k, v in (("n", 0), ("n", -5), ("n", 2 ** 31), ("nx", 0), ("ny", -1), ("nx", 2 ** 31)):
        kw = dict(good, **{k: v})
        with pytest.raises(ValueError):
            iface.census_tally(store, kw["n"], kw["nx"], kw["ny"])
    for k, v in (("n", 16.5), ("nx", 4.0), ("ny", True)):
        kw = dict(good, **{k: v})
        with pytest.raises(TypeError):
            iface.census_tally(store, kw["n"], kw["nx"], kw["ny"])
    with pytest.raises(ValueError):  # a mesh of another size
        iface.census_tally(store, 16, 4, 4, out=torch.zeros(31, dtype=torch.float64))
    with pytest.raises(ValueError):
        iface.census_tally(store, 16, 4, 4, out=torch.zeros(32, dtype=torch.float32))
    census = torch.ones(32, dtype=torch.float64)
    for kw in (dict(nx=0), dict(ny=-1), dict(min_count=2 ** 31), dict(census=torch.ones(31, dtype=torch.float64)),
               dict(census=torch.ones(32, dtype=torch.float32)), dict(census=None),
               dict(out=torch.zeros(15, dtype=torch.float64))):
        args = dict(dict(nx=4, ny=4, census=census, min_count=1, out=None), **kw)
        with pytest.raises(ValueError):
            iface.window_bounds(args["nx"], args["ny"], args["census"], 16.0, 2.0, 0.0, args["min_count"], args["out"])
    for kw in (dict(nx=4.0), dict(min_count=1.5), dict(min_count=True)):
        args = dict(dict(nx=4, min_count=1), **kw)
        with pytest.raises(TypeError):
            iface.window_bounds(args["nx"], 4, census, 16.0, 2.0, 0.0, args["min_count"])
    # the library itself: refusals that need no device to say so (meshes: any non-null address)
    lib, cstats, bstats = iface.library(), iface.CensusStats(), iface.BoundsStats()
    mesh = np.ones(32)
    out = np.full(16, 7.0)
    assert lib.neutral_hip_census_tally(None, 16, 4, 4, mesh.ctypes.data, C.byref(cstats)) == 1
    assert lib.neutral_hip_census_tally(store, 16, 4, 4, None, None) == 1
    for n, nx, ny in ((0, 4, 4), (-1, 4, 4), (16, 0, 4), (16, 4, 0)):
        assert lib.neutral_hip_census_tally(store, n, nx, ny, mesh.ctypes.data, C.byref(cstats)) == 1
        assert cstats.live == 0 and cstats.occupied_cells == 0
    nan, inf = float("nan"), float("inf")
    good = (4, 4, mesh.ctypes.data, 16.0, 2.0, 0.0, 1, out.ctypes.data)
    for i, v in ((0, 0), (1, -1), (2, None), (7, None), (3, 0.0), (3, -2.0), (3, inf), (3, nan), (4, 1.5),
                 (4, nan), (4, inf), (5, -0.1), (5, 1.5), (5, nan), (6, 0), (6, -3)):
        bad = list(good)
        bad[i] = v
        assert lib.neutral_hip_window_bounds(*bad, C.byref(bstats)) == 1, (i, v)
        assert bstats.windowed_cells == 0 and np.all(out == 7.0)
    with pytest.raises(iface.BoundsRefused) as refused:
        iface.window_bounds(4, 4, census, 16.0, 1.5, 0.0, 1, torch.zeros(16, dtype=torch.float64))
    assert refused.value.code == 1


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("extra", [["--window", "auto,1.5"], ["--window", "auto,x"], ["--window", "auto,"],
                                   ["--window", "auto,2,2.5"], ["--window", "auto,2,1.5,7"],
                                   ["--window", "auto", "--decompose", "1x1"],
                                   ["--decompose", "1x1", "--window", "auto,2,1.5"]])
def test_driver_usage_errors(tmp_path, extra):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + extra, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    said = out.stderr + out.stdout
    if "--decompose" in extra:
        assert "--window does not work with --decompose" in said
    else:
        assert "--window wants auto[,UPPER_RATIO[,SURVIVAL_RATIO]]" in said


# ---- the loop of census, bounds and window on a store of its own ------------------------------

LOOP = dict(n=20011, seed=5, nx=16, ny=16, upper_ratio=2.0, survival_ratio=1.5, max_split=64)


def loop_store():
    return random_store(LOOP["n"], LOOP["seed"], LOOP["nx"], LOOP["ny"], 0.3, "continuous")


def loop_window(a, lower, rn0_of):
    return wr.window(a, lower, LOOP["nx"], LOOP["ny"], LOOP["upper_ratio"], LOOP["survival_ratio"],
                     LOOP["max_split"], rn0_of)


def check_inside_the_windows(count, weight, lower):
    """every live weight of a windowed cell lies in [lower, fl(2 * lower)] after a served window call,
    hence the cell's sum between count times either end; 2^-40 covers the summation bound of any
    count below 2^13"""
    assert count.max() < 2 ** 13
    windowed = lower > 0.0
    slack = 2.0 ** -40
    assert np.all(count[windowed] * lower[windowed] * (1.0 - slack) <= weight[windowed])
    assert np.all(weight[windowed] <= count[windowed] * (2.0 * lower[windowed]) * (1.0 + slack))


def test_the_loop_on_the_restatements_refuses_no_copy():
    """the condition of the GPU test below, on the CPU: with this seed the window that the generated
    bounds ask for finds a free slot for every copy, and max_split does not bind"""
    a = loop_store()
    c = cr.census(a, LOOP["nx"], LOOP["ny"])
    b = cr.bounds(c.count, c.weight, float(c.stats["live"]), LOOP["upper_ratio"], 0.0, 1)
    r = loop_window(a, b.lower, wr.cpu_rn0(0, SEED))
    print(c.stats, b.stats, r.stats)
    assert r.stats["copies_refused"] == 0 and r.stats["split"] > 0 and r.stats["roulette_killed"] > 0
    assert int(r.demand.max()) + 1 < LOOP["max_split"]
    after = cr.census(r.arrays, LOOP["nx"], LOOP["ny"])
    check_inside_the_windows(after.count, after.weight, b.lower)
    # the generated window holds about the population it was made for (roulette is fair, not exact)
    assert 0.6 * c.stats["live"] < after.stats["live"] < 1.4 * c.stats["live"]


# ---- the in-run scenario: steps, auto window, steps, auto window, steps ------------------------

ON = (0.25, 0.5)  # roulette in the collision kernels
RUN = dict(nx=24, nparticles=6000, iterations=9, dt=2.0e-6)
RUN_RATIOS = dict(upper_ratio=2.0, survival_ratio=1.7, max_split=5)
RUN_STEPS = ((1, 2, 3), (4, 5, 6), (7, 8, 9))  # an auto window after the first two groups
RUN_TARGET = 4000.0  # fewer than are alive: bounds high enough for roulette in the crowded cells


def _oracle_run(make_problem, cs):
    import oracle_binding as ob
    keys, values = cs
    absorb = (np.array(keys), 0.5 * np.array(values))  # capture = scatter / 2: p_absorb = 1/3
    prob = make_problem("csp", **RUN)
    ref = ob.OracleRun(prob, keys, values, cs_absorb=absorb, roulette=ON)
    ref.inject()
    return prob, keys, values, absorb, ref


def apply_to_oracle(ref, lower, tt):
    """the window's restatement on the oracle's arrays, in place; -> Result"""
    arrays = ref.particles.as_dict()
    r = wr.window(arrays, lower, RUN["nx"], RUN["nx"], RUN_RATIOS["upper_ratio"], RUN_RATIOS["survival_ratio"],
                  RUN_RATIOS["max_split"], wr.cpu_rn0(0, wr.WINDOW_SEED_BASE + tt))
    assert r is not None
    for f in wr.FIELDS:
        arrays[f][:] = r.arrays[f]
    return r


def test_the_scenario_on_the_oracle_splits_and_plays_roulette(make_problem, cs):
    _, _, _, _, ref = _oracle_run(make_problem, cs)
    results = []
    for steps in RUN_STEPS[:2]:
        for tt in steps:
            ref.step(tt)
        c = cr.census(ref.particles.as_dict(), RUN["nx"], RUN["nx"])
        b = cr.bounds(c.count, c.weight, RUN_TARGET, RUN_RATIOS["upper_ratio"], 0.0, 1)
        results.append(apply_to_oracle(ref, b.lower, steps[-1]))
        print(c.stats, b.stats, results[-1].stats)
    for r in results:
        assert not r.guarded.any(), np.flatnonzero(r.guarded)
        assert r.stats["split"] > 0 and r.stats["roulette_killed"] + r.stats["roulette_survived"] > 0


# ---- GPU: census and bounds alone ------------------------------------------------------------

class CensusStore(census_ops_support.Store):
    """the store with the census's call"""

    def census(self, nx, ny, out=None, n=None, null_store=False, null_out=False):
        """the library's own call: -> (return code, stats, the two meshes on the host)"""
        stats = self.iface.CensusStats()
        self.iface.set_pid_base(self.sim.pid_base)
        if out is None:
            out = self.torch.full((2 * max(nx, 1) * max(ny, 1),), 7.0, dtype=self.torch.float64, device=self.sim.device)
        rc = self.iface.library().neutral_hip_census_tally(
            None if null_store else self.sim.particles, self.n if n is None else n, nx, ny,
            None if null_out else C.c_void_p(out.data_ptr()), C.byref(stats))
        return rc, stats, out.cpu().numpy()


def _check_census(st, a, nx, ny, weights, name):
    rc, stats, got = st.census(nx, ny)
    want = cr.census(a, nx, ny)
    assert rc == 0, name
    count, weight = got[:nx * ny], got[nx * ny:]
    assert same_bits(count, want.count), name
    assert (stats.live, stats.dead, stats.occupied_cells, stats.max_count) == \
        tuple(want.stats[k] for k in ("live", "dead", "occupied_cells", "max_count")), name
    assert stats.max_cell_weight == weight.max(), name  # (a maximum is exact)
    exact_total = math.fsum(a["weight"][a["dead"] == 0])
    worst = float(np.max(np.abs(weight - want.weight) / np.maximum(want.weight, 1e-300)))
    print(f"n={st.n} {nx}x{ny} {name}: {want.stats} worst cell {worst:.3e} total off by "
          f"{abs(stats.weight - exact_total):.3e} census_ms {stats.census_ms:.3f}")
    if weights == "dyadic":  # every partial sum is exact
        assert same_bits(weight, want.weight), name
        assert stats.weight == exact_total and stats.max_cell_weight == want.stats["max_cell_weight"], name
    else:
        assert np.all(np.abs(weight - want.weight) <= (want.count + 1.0) * EPS * want.weight), name
        assert abs(stats.weight - exact_total) <= (stats.live + stats.occupied_cells) * EPS * exact_total, name
    return stats, got


def census_sizes():
    """1 .. 65: a wave and its neighbours; 257: a lane's second turn of the grid-strided pass (one
    workgroup of kCombBlock lanes per tile of slots); tile + 1: the second workgroup"""
    return [1, 2, 63, 64, 65, kernel_constant("kCombBlock") + 1, 1000, scan_tile() + 1, 100003]


@gpu
@needs_gpu
@pytest.mark.parametrize("n", census_sizes())
def test_census_against_the_restatement(iface, make_problem, cs, n):
    st = CensusStore(iface, make_problem, cs, n)
    for nx, ny in MESHES:
        for dead_share in (0.0, 0.3, 1.0):
            for weights in ("dyadic", "continuous"):
                if dead_share == 1.0 and weights == "continuous":
                    continue
                name = f"dead {dead_share} {weights}"
                a = random_store(n, n + 7 * nx, nx, ny, dead_share, weights)
                if dead_share == 1.0:
                    a["dead"][a["dead"] == 0] = 3
                st.upload(a)
                stats, got = _check_census(st, a, nx, ny, weights, name)
                if dead_share == 1.0:
                    assert stats.live == 0 and stats.occupied_cells == 0 and not got.any()
    st.close()


@gpu
@needs_gpu
def test_census_is_a_snapshot_and_writes_nothing_to_the_store(iface, make_problem, cs):
    n = 5000
    st = CensusStore(iface, make_problem, cs, n)
    a = random_store(n, 21, 16, 16, 0.3, "dyadic")
    st.upload(a)
    before = st.arrays()
    out = st.torch.full((512,), 7.0, dtype=st.torch.float64, device=st.sim.device)
    rc, _, first = st.census(16, 16, out=out)
    out.fill_(7.0)
    rc2, _, second = st.census(16, 16, out=out)
    assert rc == rc2 == 0 and same_bits(first, second) and first[:256].sum() == (a["dead"] == 0).sum()
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], a[f]) and same_bits(after[f], before[f]), f  # (NaN bits included)
    # through the wrapper: device tensors, the same meshes
    count, weight, stats = iface.census_tally(st.sim.particles, n, 16, 16)
    assert same_bits(count.cpu().numpy(), first[:256]) and same_bits(weight.cpu().numpy(), first[256:])
    assert stats.live == (a["dead"] == 0).sum()
    st.close()


CENSUS_REFUSALS = ["store null", "out null", "n 0", "n negative", "nx 0", "ny 0", "cellx beyond", "celly negative",
                   "weight negative", "weight inf", "weight nan"]


@gpu
@needs_gpu
@pytest.mark.parametrize("case", CENSUS_REFUSALS)
def test_census_refusals(iface, make_problem, cs, case):
    n = 5000
    st = CensusStore(iface, make_problem, cs, n)
    a = random_store(n, 13, 16, 16, 0.3, "continuous")
    j = int(np.flatnonzero(a["dead"] == 0)[-1])  # (the last live slot: beyond the first tile)
    k = int(np.flatnonzero(a["dead"] != 0)[-1])
    kw = {"store null": dict(null_store=True), "out null": dict(null_out=True), "n 0": dict(n=0),
          "n negative": dict(n=-3)}.get(case, {})
    nx, ny = (0, 16) if case == "nx 0" else (16, 0) if case == "ny 0" else (16, 16)
    field, value = {"cellx beyond": ("cellx", 16), "celly negative": ("celly", -1), "weight negative": ("weight", -1.0),
                    "weight inf": ("weight", np.inf), "weight nan": ("weight", np.nan)}.get(case, (None, None))
    if field:  # on a dead slot: no refusal
        a[field][k] = value
        st.upload(a)
        _check_census(st, a, 16, 16, "continuous", case + " on a dead slot")
        a[field][j] = value
    st.upload(a)
    rc, stats, got = st.census(nx, ny, **kw)
    assert rc == 1 and (stats.occupied_cells, stats.max_count, stats.weight, stats.max_cell_weight) == (0, 0, 0.0, 0.0)
    if field:
        assert not got.any()  # found on the device: the buffer holds zeros
        with pytest.raises(iface.CensusRefused) as refused:
            st.sim.census()
        assert refused.value.code == 1
    else:
        assert np.all(got == 7.0)
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], a[f]), f
    st.close()


@gpu
@needs_gpu
def test_census_of_a_sharded_store_and_of_a_decomposed_one(iface, make_problem, cs):
    """the pid base of a shard does not show in the census; a Simulation over a decomposition takes
    none (code 2, as the window says it)"""
    n = 5000
    a = random_store(n, 12, 16, 16, 0.2, "dyadic")
    seen = []
    for pid_base in (0, 123456789):
        st = CensusStore(iface, make_problem, cs, n, pid_base=pid_base)
        st.upload(a)
        _, got = _check_census(st, a, 16, 16, "dyadic", f"pid base {pid_base}")
        seen.append(got)
        st.close()
    assert same_bits(seen[0], seen[1])
    prob = make_problem("csp", nx=64, nparticles=1000, iterations=1)
    sim = iface.Simulation(prob, *cs, variant=2, domain=(1, 1))
    with pytest.raises(iface.CensusRefused) as refused:
        sim.census()
    assert refused.value.code == 2
    with pytest.raises(iface.CensusRefused):
        sim.auto_window()
    sim.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_census_of_a_tiled_store(iface, make_problem, cs, lazy):
    """After two steps of the tiled variant (records pending; lazy: not even written back) the census
    counts what particle_arrays() shows afterwards: it wrote the pending state back itself and
    changed nothing."""
    prob = make_problem("csp", nx=16, nparticles=20011, iterations=4)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, *cs, variant=2, roulette=ON, cs_absorb=(cs[0].copy(), cs[1] * 0.5))
    sim.inject()
    sim.step(1)
    sim.step(2)
    count, weight, stats = sim.census()
    count, weight = count.cpu().numpy(), weight.cpu().numpy()
    want = cr.census(sim.particle_arrays(), 16, 16)
    sim.close()
    assert same_bits(count, want.count) and count.sum() == 20011 - want.stats["dead"]
    assert (stats.live, stats.dead, stats.occupied_cells, stats.max_count) == \
        tuple(want.stats[k] for k in ("live", "dead", "occupied_cells", "max_count"))
    assert np.all(np.abs(weight - want.weight) <= (want.count + 1.0) * EPS * want.weight)


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_census_costs_the_next_tiled_step_no_import(iface, make_problem, cs, lazy, monkeypatch):
    """The census leaves the records of a tiled store valid: the step after it has the stats of the
    same step of a run that made no census -- one wait for the device -- where a step after an
    import waits more often.  The deck and the fields of
    tests/test_window.py::test_nothing_to_do_on_a_tiled_store_changes_nothing (on the small csp deck
    above a step after an import shows the same three numbers as a steady one)."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    runs = []
    for call in (False, True):
        prob = make_problem("stream", nx=400, nparticles=30000, iterations=4)
        iface.set_lazy_export(lazy)
        sim = iface.Simulation(prob, *cs, variant=2)
        sim.inject()
        first = sim.step(1).stats
        assert first.stream_passes > 2 and first.host_syncs > 1, "the case no longer migrates"
        sim.step(2)
        if call:
            count, _, stats = sim.census()
            assert stats.live == 30000 == int(count.sum().item()) and stats.dead == 0
        third = sim.step(3)
        arrays = sim.particle_arrays()
        iface.library().neutral_hip_invalidate_particles(sim.particles)
        fourth = sim.step(4).stats
        runs.append((arrays, third, fourth))
        sim.close()
    (a, ra, imported), (b, rb, _) = runs
    sa, sb = ra.stats, rb.stats
    assert sb.host_syncs == 1, (sb.host_syncs, sb.stream_passes, sb.stream_passes_enqueued)
    assert (sb.host_syncs, sb.stream_passes_enqueued, sb.stream_passes) == \
        (sa.host_syncs, sa.stream_passes_enqueued, sa.stream_passes)
    assert imported.host_syncs > 1  # (what a step that imports the arrays again looks like)
    for f in wr.FIELDS:
        assert same_bits(a[f], b[f]), f
    assert (ra.nprocessed, ra.facets, ra.collisions, ra.census) == (rb.nprocessed, rb.facets, rb.collisions, rb.census)


def _bounds_raw(iface, torch, device, census, nx, ny, target, upper, floor, min_count, null=None):
    """the library's own call on a census mesh from the host: -> (return code, stats, lower_out,
    which went in filled with -3)"""
    d_census = torch.from_numpy(np.ascontiguousarray(census, dtype=np.float64)).to(device)
    out = torch.full((nx * ny,), -3.0, dtype=torch.float64, device=device)
    stats = iface.BoundsStats()
    rc = iface.library().neutral_hip_window_bounds(
        nx, ny, None if null == "census" else C.c_void_p(d_census.data_ptr()), target, upper, floor, min_count,
        None if null == "out" else C.c_void_p(out.data_ptr()), C.byref(stats))
    return rc, stats, out.cpu().numpy()


@gpu
@needs_gpu
@pytest.mark.parametrize("nx, ny", MESHES + ((scan_tile() + 1, 1),))
def test_bounds_bit_for_bit_against_the_restatement(iface, make_problem, cs, nx, ny):
    """the input is the GPU's own census, read back: the bits are then defined, whatever the order of
    its sums.  (scan_tile + 1) x 1: the reductions take their second level."""
    import torch
    n = 4 * nx * ny + 50
    st = CensusStore(iface, make_problem, cs, n)
    device = st.sim.device
    for weights in ("dyadic", "continuous"):
        a = random_store(n, nx + 3, nx, ny, 0.3, weights)
        st.upload(a)
        rc, cstats, census = st.census(nx, ny)
        assert rc == 0
        count, weight = census[:nx * ny], census[nx * ny:]
        for floor in (0.0, 0.25, 1.0):
            for min_count in (1, 3):
                want = cr.bounds(count, weight, float(cstats.live), 2.0, floor, min_count)
                rc, stats, lower = _bounds_raw(iface, torch, device, census, nx, ny, float(cstats.live), 2.0, floor,
                                               min_count)
                if want is None:
                    assert rc == 1 and np.all(lower == -3.0)
                    continue
                assert rc == 0 and same_bits(lower, want.lower), (weights, floor, min_count)
                assert (stats.windowed_cells, stats.floored_cells, stats.max_cell_weight, stats.lower_at_peak) == \
                    tuple(want.stats[k] for k in ("windowed_cells", "floored_cells", "max_cell_weight", "lower_at_peak"))
                if min_count == 1:
                    assert stats.max_cell_weight == cstats.max_cell_weight
        if nx * ny > 1:
            assert want is not None and 0 < want.stats["windowed_cells"]
        # through the wrapper
        lower_t, stats = iface.window_bounds(nx, ny, torch.from_numpy(census).to(device), float(cstats.live), 2.0, 0.25, 1)
        assert same_bits(lower_t.cpu().numpy(), cr.bounds(count, weight, float(cstats.live), 2.0, 0.25, 1).lower)
    # refusals: lower_out, filled with a sentinel, is untouched
    good = dict(census=census, target=100.0, upper=2.0, floor=0.0, min_count=1, null=None)
    worse = census.copy()
    worse[nx * ny - 1] = -1.0
    nan_in = census.copy()
    nan_in[2 * nx * ny - 1] = np.nan
    for kw in (dict(census=np.zeros(2 * nx * ny)), dict(census=worse), dict(census=nan_in), dict(upper=1.5),
               dict(floor=1.5), dict(min_count=0), dict(target=0.0), dict(target=-5.0), dict(target=np.inf),
               dict(null="census")):
        args = dict(good, **kw)
        rc, stats, lower = _bounds_raw(iface, torch, device, args["census"], nx, ny, args["target"], args["upper"],
                                       args["floor"], args["min_count"], args["null"])
        assert rc == 1 and np.all(lower == -3.0) and stats.windowed_cells == 0, kw
    rc, _, _ = _bounds_raw(iface, torch, device, census, nx, ny, 100.0, 2.0, 0.0, 1, null="out")
    assert rc == 1
    st.close()


@gpu
@needs_gpu
def test_the_loop_closes(iface, make_problem, cs):
    """census, bounds for as many histories as are alive, window with the GPU's bounds: no copy is
    refused (the CPU test above shows that for the restatements), the window's result is the
    restatement's bit for bit, a census afterwards finds every windowed cell's weight between its
    count times the cell's two bounds, and a second window with the same bounds changes nothing
    (the window's identity property; auto_window itself makes new bounds from the new census)."""
    n, nx, ny = LOOP["n"], LOOP["nx"], LOOP["ny"]
    st = CensusStore(iface, make_problem, cs, n)
    a = loop_store()
    st.upload(a)
    count, weight, census = st.sim.census()
    both = st.torch.cat([count, weight])
    lower_t, bounds = iface.window_bounds(nx, ny, both, float(census.live), LOOP["upper_ratio"], 0.0, 1)
    lower = lower_t.cpu().numpy()
    want_bounds = cr.bounds(count.cpu().numpy(), weight.cpu().numpy(), float(census.live), LOOP["upper_ratio"], 0.0, 1)
    assert same_bits(lower, want_bounds.lower) and bounds.windowed_cells == census.occupied_cells == nx * ny
    stats = st.sim.window(lower, LOOP["upper_ratio"], LOOP["survival_ratio"], LOOP["max_split"], seed=SEED)
    assert stats.copies_refused == 0  # (a condition of this test, not a result)
    r = loop_window(a, lower, wr.probe_rn0(iface, 0, SEED))
    assert {k: getattr(stats, k) for k in wr.STAT_NAMES} == r.stats and stats.split > 0 and stats.roulette_killed > 0
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], r.arrays[f]), f
    count2, weight2, census2 = st.sim.census()
    assert census2.live == census.live - stats.roulette_killed + stats.copies_made
    check_inside_the_windows(count2.cpu().numpy(), weight2.cpu().numpy(), lower)
    print(f"live {census.live} -> {census2.live}, counts per cell {int(count.min())}..{int(count.max())} -> "
          f"{int(count2.min())}..{int(count2.max())}")
    again = st.sim.window(lower, LOOP["upper_ratio"], LOOP["survival_ratio"], LOOP["max_split"], seed=SEED + 12345)
    assert (again.below, again.above, again.split, again.copies_made, again.copies_refused) == (0, 0, 0, 0, 0)
    second = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(second[f], after[f]), f
    # auto_window: the three calls in one, on the store as it stands
    c3, b3, w3 = st.sim.auto_window(upper_ratio=LOOP["upper_ratio"], survival_ratio=LOOP["survival_ratio"],
                                    max_split=LOOP["max_split"], seed=SEED + 1)
    assert c3.live == census2.live and b3.windowed_cells == nx * ny and w3.live_before == c3.live
    # (its own census: a cell's weight sum is not the same bits from call to call)
    census3 = st.sim.last_census.cpu().numpy()
    assert same_bits(census3[:nx * ny], count2.cpu().numpy())
    want3 = cr.bounds(census3[:nx * ny], census3[nx * ny:], float(c3.live), LOOP["upper_ratio"], 0.0, 1)
    assert same_bits(st.sim.last_lower.cpu().numpy(), want3.lower)
    st.close()


# ---- GPU: census and auto window in a run, against the oracle ---------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False), (0, True)])
def test_census_and_auto_window_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """Steps, census and auto window, steps, the same again, steps: the census against the oracle's
    arrays, the generated bounds applied to the oracle by the window's restatement."""
    prob, keys, values, absorb, ref = _oracle_run(make_problem, cs)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=ON, cs_absorb=absorb)
    sim.inject()
    nx = RUN["nx"]
    split = played = 0
    for steps in RUN_STEPS:
        for tt in steps:
            g, c = sim.step(tt), ref.step(tt)
            assert (g.nprocessed, g.facets, g.collisions, g.census) == (c.nprocessed, c.facets, c.collisions, c.census), tt
        want = cr.census(ref.particles.as_dict(), nx, nx)
        count, weight, cstats = sim.census()
        count, weight = count.cpu().numpy(), weight.cpu().numpy()
        assert same_bits(count, want.count) and cstats.live == want.stats["live"]
        # (each live weight within 1e-9 of the oracle's: tests/test_window.py; then the sum's own bound)
        assert np.all(np.abs(weight - want.weight) <= 1e-9 * want.count + (want.count + 1.0) * EPS * want.weight)
        if steps is RUN_STEPS[-1]:
            break
        census, bounds, stats = sim.auto_window(target_population=RUN_TARGET, **RUN_RATIOS)
        assert census.live == cstats.live and bounds.windowed_cells == cstats.occupied_cells
        r = apply_to_oracle(ref, sim.last_lower.cpu().numpy(), steps[-1])
        assert not r.guarded.any()
        assert {k: getattr(stats, k) for k in wr.STAT_NAMES} == r.stats
        split += stats.split
        played += stats.roulette_killed + stats.roulette_survived
        got, ours = sim.particle_arrays(), ref.particles.as_dict()
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(got[f], ours[f]), f
        assert np.max(np.abs(got["weight"] - ours["weight"])[ours["dead"] == 0]) <= 1e-9
    assert split > 0 and played > 0
    tg, tc = sim.tally_host(), ref.tally
    print(f"variant {variant} lazy {lazy}: tally rel L2 {np.linalg.norm(tg - tc) / np.linalg.norm(tc):.3e}")
    assert np.linalg.norm(tg - tc) / np.linalg.norm(tc) < TALLY_L2_TOL
    sim.close()


# ---- GPU: the driver's --window auto ----------------------------------------------------------

def _census_lines(stdout):
    return [dict(live=int(m.group(1)), occupied=int(m.group(2)), max_count=int(m.group(3)), max_weight=float(m.group(4)))
            for m in re.finditer(r"^Census live (\d+) occupied (\d+) max_count (\d+) max_weight (\S+)$", stdout, flags=re.M)]


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_window_auto_on_one_rank_and_on_two(tmp_path):
    """`neutral.hip --roulette 0.25,0.5 --window auto,2,1.6`: one Census line per window call (after
    every step but the last), copies made, nothing skipped; without the flag no such line.  Two
    ranks (both on one GPU) tally their shards into one census: the histories are the same before
    the first window, so its line says what the one-rank run's says.  (The plain run prints no
    deaths per step to derive the first live count from: it is bounded instead.)"""
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
    assert "Census" not in plain and "Window" not in plain
    one = run_driver(str(run), rel, sets + ["--window", "auto,2,1.6"])
    lines = _census_lines(one)
    print(lines)
    assert len(lines) == 5
    assert 0 < lines[0]["live"] <= 100001 and 0 < lines[0]["occupied"] <= 64 * 64
    assert int(re.search(r"^Window copies made (\d+)$", one, flags=re.M).group(1)) > 0
    assert re.search(r"^Window auto skipped 0$", one, flags=re.M)
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    two = run_driver(str(run), rel, sets + ["--gpus", "2", "--window", "auto,2,1.6"], env)
    lines2 = _census_lines(two)
    print(lines2)
    assert len(lines2) == 5  # (rank 0 prints: the live count over the ranks, the global stats)
    first, first2 = lines[0], lines2[0]
    assert (first2["live"], first2["occupied"], first2["max_count"]) == (first["live"], first["occupied"], first["max_count"])
    assert abs(first2["max_weight"] - first["max_weight"]) <= (first["max_count"] + 1) * EPS * first["max_weight"] \
        + 1e-15 * first["max_weight"]  # (the line prints sixteen digits)
    assert int(re.search(r"^Window copies made (\d+)$", two, flags=re.M).group(1)) > 0

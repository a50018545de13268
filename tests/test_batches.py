"""Batch statistics: a standard error and a relative error for every tally (include/neutral_hip.h:
neutral_hip_batch_fold, neutral_hip_batch_statistics; neutral_amd.interface.BatchedRun; neutral.hip
--batches).

CPU: the numpy restatement (tests/batch_reference.py) pinned against a two-pass variance and by its
properties, the scenarios of the GPU part on the CPU oracle alone (the batches are shards: their sum
is the run; no relative error near 0; the stream deck's total has none), the ABI, the wrappers'
argument handling, the driver's usage errors.  GPU: fold and statistics bit for bit against the
restatement, refusals, a tiled store between two steps, BatchedRun against the oracle, the stream
deck, the error against the particle count, windows inside the batches, the driver.
"""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import batch_reference as br
import census_reference as cr
import window_reference as wr
from conftest import ROOT
from gpu_support import OWN_DRIVER, gpu, iface, l2, needs_gpu, run_driver, scan_tile, third_absorb  # noqa: F401

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
EPS = 2.0 ** -53
LENGTHS = [1, 63, 64, 65, scan_tile() + 1, 100003]  # a wave and its neighbours; the second tile; two levels
BATCH_COUNTS = [2, 3, 8]
NB = 8           # batches of the runs below
ON = (0.25, 0.5)  # roulette in the collision kernels (tests/test_window.py)


def same_bits(a, b):
    """equal as raw bytes: a NaN equals itself, -0.0 does not equal 0.0"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def batch_data(n, nbatches, kind, seed):
    """nbatches arrays of n doubles.  dyadic: multiples of 2^-10 in [0, 8], so that every sum of them
    is exact; continuous: log-uniform magnitudes over 2^-60 .. 2^60 of either sign.  Both with zeros
    mixed in: a tenth of the entries are 0.0 in every batch (not scored), a fifth of the others in any
    one batch."""
    rng = np.random.default_rng(seed)
    if kind == "dyadic":
        x = rng.integers(0, 8193, (nbatches, n)).astype(np.float64) * 2.0 ** -10
    else:
        x = np.exp2(rng.uniform(-60.0, 60.0, (nbatches, n))) * rng.choice([-1.0, 1.0], (nbatches, n))
    x[rng.random((nbatches, n)) < 0.2] = 0.0
    x[:, rng.random(n) < 0.1] = 0.0
    return [np.ascontiguousarray(row) for row in x]


def any_order_bound(terms, exact):
    """how far a sum of `terms` in any order may lie from their exact sum: the first-order bound of a
    summation tree, (m - 1) * 2^-53 * sum|t|, and half an ulp of the result (tests/test_census.py)"""
    return (len(terms) - 1) * EPS * math.fsum(np.abs(terms)) + EPS * abs(exact)


# ---- CPU: the restatement --------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 65, 5000])
@pytest.mark.parametrize("nbatches", BATCH_COUNTS + [17])
def test_restatement_against_a_two_pass_variance(n, nbatches):
    rng = np.random.default_rng(n + nbatches)
    x = rng.uniform(0.5, 1.5, (nbatches, n)) * np.exp2(rng.uniform(-20.0, 20.0, n))
    moments, folds, s = br.run(list(x), scale=float(nbatches))
    mean, var = x.mean(axis=0), x.var(axis=0, ddof=1)
    assert np.allclose(moments[:n], mean, rtol=1e-12, atol=0)
    assert np.allclose(moments[n:] / (nbatches - 1), var, rtol=1e-12, atol=0)
    assert np.allclose(s.estimate, x.sum(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(s.relerr, np.sqrt(var / nbatches) / mean, rtol=1e-12, atol=0)
    for k, f in enumerate(folds):
        assert math.isclose(f["sum"], math.fsum(x[k]), rel_tol=1e-12) and f["nonzero"] == n
    assert s.stats["scored"] == n and s.stats["max_relerr"] == s.relerr.max()
    assert math.isclose(s.stats["mean_relerr"], s.relerr.mean(), rel_tol=1e-12)
    assert math.isclose(s.stats["estimate_sum"], math.fsum(s.estimate), rel_tol=1e-12)
    assert s.stats["within_5pc"] <= s.stats["within_10pc"] <= n


def test_tile_sum_is_a_sum():
    """the restated order of the library's reductions: exact on dyadic data of every length that
    takes another path, within the any-order bound elsewhere"""
    for n in LENGTHS + [scan_tile() - 1, scan_tile(), 3 * scan_tile() + 5]:
        d, c = batch_data(n, 1, "dyadic", n)[0], batch_data(n, 1, "continuous", n)[0]
        assert br.tile_sum(d) == math.fsum(d)
        assert abs(br.tile_sum(c) - math.fsum(c)) <= any_order_bound(c, math.fsum(c))


def test_properties_of_the_restatement():
    rng = np.random.default_rng(3)
    x = [rng.random(100) for _ in range(4)]
    # k == 1 ignores what moments held
    first, _ = br.fold(x[0], 1, np.full(200, np.nan))
    assert same_bits(first, br.fold(x[0], 1, None)[0]) and same_bits(first[:100], x[0]) and not first[100:].any()
    # all batches agree: relerr is exactly 0, whatever the values
    v = np.exp2(rng.uniform(-60.0, 60.0, 100))
    for nb in BATCH_COUNTS:
        _, _, s = br.run([v] * nb)
        assert not s.relerr.any() and s.stats["max_relerr"] == 0.0 and s.stats["within_5pc"] == 100
        assert same_bits(s.estimate, np.float64(nb) * v)
    # exactly one of B batches scored: relerr is 1 (the mean is v / B, its standard error too)
    for nb in BATCH_COUNTS + [5, 7]:
        for where in range(nb):
            batches = [v if k == where else np.zeros(100) for k in range(nb)]
            _, _, s = br.run(batches)
            assert np.all(np.abs(s.relerr - 1.0) <= 2 * 2.0 ** -52), (nb, where, np.abs(s.relerr - 1.0).max())
    # an entry that never scored: estimate 0, relerr 0, not counted
    _, _, s = br.run([np.array([0.0, 1.0]), np.array([0.0, 3.0])])
    assert s.estimate.tolist() == [0.0, 4.0] and s.relerr[0] == 0.0 and s.stats["scored"] == 1
    assert s.relerr[1] == 0.5 and (s.stats["within_10pc"], s.stats["max_relerr"], s.stats["mean_relerr"]) == (0, 0.5, 0.5)
    # refusals
    assert br.fold(np.array([1.0, np.nan]), 1, None) is None and br.fold(np.array([np.inf]), 2, np.zeros(2)) is None
    assert br.fold(np.zeros(0), 1, None) is None and br.fold(np.ones(3), 0, None) is None
    good = np.array([1.0, 2.0, 0.5, 0.0])
    assert br.statistics(good, 2, 2.0) is not None
    for moments, nb, scale in ((good, 1, 1.0), (good, 2, 0.0), (good, 2, -1.0), (good, 2, np.inf), (good, 2, np.nan),
                               (np.array([1.0, np.nan, 0.5, 0.0]), 2, 2.0), (np.array([1.0, 2.0, -0.5, 0.0]), 2, 2.0),
                               (np.array([1.0, 2.0, 0.5, np.inf]), 2, 2.0), (np.array([np.inf, 2.0, 0.5, 0.0]), 2, 2.0),
                               (np.zeros(0), 2, 2.0)):
        assert br.statistics(moments, nb, scale) is None, (moments, nb, scale)


# ---- the runs: problems, and what the CPU oracle makes of them (computed once) ----------------

_DECKS = tempfile.TemporaryDirectory(prefix="batch_decks_")


@functools.lru_cache(maxsize=None)
def _tables():
    from neutral_amd import cs_table
    return cs_table.load()


@functools.lru_cache(maxsize=None)
def problem(name, nparticles, steps):
    from neutral_amd import decks, host
    path = decks.write_deck(name, os.path.join(_DECKS.name, f"{name}_{nparticles}_{steps}.params"), nx=24, ny=24,
                            nparticles=nparticles, iterations=steps)
    return host.setup_problem(path, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)


def _oracle(name, nparticles, steps, shard, third, between=None):
    import oracle_binding as ob
    keys, values = _tables()
    kw = dict(cs_absorb=third_absorb((keys, values)), roulette=ON) if third else {}
    ref = ob.OracleRun(problem(name, nparticles, steps), keys, values, shard=shard, **kw)
    ref.inject()
    for tt in range(1, steps + 1):
        ref.step(tt)
        if between is not None:
            between(ref, tt)
    return ref.tally.copy()


AUTO = dict(upper_ratio=5.0, survival_ratio=3.0, max_split=5)  # Simulation.auto_window's defaults


def oracle_auto_window(ref, tt):
    """Simulation.auto_window() after steps 1 and 2, restated on the oracle's arrays in place"""
    if tt > 2:
        return None
    arrays = ref.particles.as_dict()
    c = cr.census(arrays, 24, 24)
    b = cr.bounds(c.count, c.weight, float(c.stats["live"]), AUTO["upper_ratio"], 0.0, 1)
    r = wr.window(arrays, b.lower, 24, 24, AUTO["upper_ratio"], AUTO["survival_ratio"], AUTO["max_split"],
                  wr.cpu_rn0(ref.pid_base, wr.WINDOW_SEED_BASE + tt))
    assert r is not None
    for f in wr.FIELDS:
        arrays[f][:] = r.arrays[f]
    return r


@functools.lru_cache(maxsize=None)
def oracle_batches(name, nparticles, steps, third=False, windows=False):
    """-> (the NB shards' tallies, the restatement's statistics of them, (total, its standard error))"""
    per = nparticles // NB
    tallies = [_oracle(name, nparticles, steps, (b * per, per), third, oracle_auto_window if windows else None)
               for b in range(NB)]
    _, folds, stats = br.run(tallies)
    return tallies, stats, br.total_of([f["sum"] * NB for f in folds])


@functools.lru_cache(maxsize=None)
def oracle_whole(name, nparticles, steps):
    return _oracle(name, nparticles, steps, None, False)


def median_ratio(relerr_few, relerr_many):
    """median relerr with the fewer particles over that with the more, over the cells scored in both"""
    both = (relerr_few > 0.0) & (relerr_many > 0.0)
    return float(np.median(relerr_few[both]) / np.median(relerr_many[both]))


CSP = ("csp", 8000, 3)
STREAM = ("stream", 8000, 2)


def test_the_batches_of_the_oracle_are_the_run():
    """what the GPU tests rely on, on the CPU oracle alone.  The sum of the batch tallies is the
    one-run tally (the same deposits, summed per cell in another order: 1e-13 covers eight terms a
    thousand times over); no scored cell's relerr is near 0, so inputs that agree to 1e-9 of a cell's
    mean move it by 1e-7 at the most; no relerr lies within 1e-6 of 0.1, so the counts are exact."""
    tallies, s, total = oracle_batches(*CSP)
    whole = oracle_whole(*CSP)
    print(f"sum of the batches against the run: {l2(sum(tallies), whole):.3e}, estimate: {l2(s.estimate, whole):.3e}")
    assert l2(sum(tallies), whole) <= 1e-13 and l2(s.estimate, whole) <= 1e-13
    scored = s.estimate != 0.0
    print(s.stats, f"min relerr {s.relerr[scored].min():.4e}", "scored in one batch only:",
          int((np.abs(s.relerr - 1.0) <= 2 * 2.0 ** -52).sum()))
    assert s.stats["scored"] == scored.sum() > 200 and np.array_equal(scored, whole != 0.0)
    assert s.relerr[scored].min() >= 1e-3
    assert np.abs(s.relerr[scored] - 0.1).min() > 1e-6 and np.abs(s.relerr[scored] - 0.05).min() > 1e-6
    assert total[1] / total[0] > 0.01  # (the total's own error: 6 %)
    assert math.isclose(total[0], whole.sum(), rel_tol=1e-13)


def test_the_stream_deck_of_the_oracle_has_an_exact_total():
    """no history collides: every particle deposits the same whatever its path, so the batch totals
    agree to rounding, while a cell's relerr is that of how many paths cross it"""
    import closed_form
    _, s, total = oracle_batches(*STREAM)
    scored = s.estimate != 0.0
    print(f"total {total[0]:.15e} relative standard error {total[1] / total[0]:.3e}, relerr "
          f"{s.relerr[scored].min():.4f} .. {s.relerr[scored].max():.4f}")
    assert total[1] / total[0] <= 1e-12
    assert scored.all() and s.relerr.min() >= 1e-3
    assert math.isclose(total[0], closed_form.stream_deck_tally(*_tables(), iterations=2), rel_tol=1e-12)


def test_the_error_of_the_oracle_falls_with_the_particle_count():
    """four times the particles: half the error is the law; the median over the cells scored in both
    runs does about that"""
    ratio = median_ratio(oracle_batches("csp", 4000, 3)[1].relerr, oracle_batches("csp", 16000, 3)[1].relerr)
    print(f"median relerr, 4000 over 16000 particles: {ratio:.4f}")
    assert 1.5 < ratio < 2.5


def test_windows_inside_the_batches_of_the_oracle_keep_the_mean():
    """the scenario of the GPU test: roulette, capture = scatter / 2, an auto window after steps 1 and
    2 of every batch.  The plain run's total has a standard error above 1 %, so that three standard
    errors are a statement; the windowed run's total lies within three of its own of it."""
    _, _, plain = oracle_batches(*CSP, third=True)
    _, _, windowed = oracle_batches(*CSP, third=True, windows=True)
    print(f"plain {plain[0]:.6e} +- {plain[1]:.3e}, windowed {windowed[0]:.6e} +- {windowed[1]:.3e}")
    assert plain[1] / plain[0] > 0.01
    assert abs(windowed[0] - plain[0]) <= 3.0 * windowed[1]


# ---- CPU: the ABI, the wrappers, the driver --------------------------------------------------

def test_library_exports_the_batch_calls():
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in ("neutral_hip_batch_fold", "neutral_hip_batch_statistics"):
        assert hasattr(lib, name) and name in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.BatchFoldStats._fields_] == ["sum", "nonzero", "fold_ms"]
    assert C.sizeof(iface.BatchFoldStats) == 24
    assert [f[0] for f in iface.BatchStats._fields_] == [
        "scored", "within_10pc", "within_5pc", "max_relerr", "mean_relerr", "estimate_sum", "stats_ms"]
    assert C.sizeof(iface.BatchStats) == 56
    text = open(os.path.join(ROOT, "include", "neutral_hip.h")).read()
    assert "neutral_hip_batch_fold(" in text and "neutral_hip_batch_statistics(" in text
    assert issubclass(iface.BatchRefused, ValueError) and hasattr(iface.BatchedRun, "run")


def test_wrapper_argument_handling():
    """everything here raises before any GPU is used: the tensors are the host's"""
    import torch
    from neutral_amd import interface as iface
    x, moments = torch.ones(8, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    for kw in (dict(x=None), dict(x=torch.ones(8, dtype=torch.float32)), dict(x=torch.ones(16, dtype=torch.float64)[::2]),
               dict(moments=torch.zeros(15, dtype=torch.float64)), dict(moments=torch.zeros(16, dtype=torch.float32)),
               dict(k=2, moments=None), dict(k=2 ** 31)):
        args = dict(dict(x=x, k=1, moments=moments), **kw)
        with pytest.raises(ValueError):
            iface.batch_fold(args["x"], args["k"], args["moments"])
    for k in (1.0, True, "1"):
        with pytest.raises(TypeError):
            iface.batch_fold(x, k, moments)
    for kw in (dict(moments=None), dict(moments=torch.zeros(15, dtype=torch.float64)), dict(nbatches=-2 ** 31 - 1),
               dict(moments=torch.zeros(16, dtype=torch.float32)), dict(estimate=torch.zeros(7, dtype=torch.float64)),
               dict(relerr=torch.zeros(8, dtype=torch.float32))):
        args = dict(dict(moments=moments, nbatches=2, estimate=None, relerr=None), **kw)
        with pytest.raises(ValueError):
            iface.batch_statistics(args["moments"], args["nbatches"], None, args["estimate"], args["relerr"])
    with pytest.raises(TypeError):
        iface.batch_statistics(moments, 2.0)
    # the library itself: refusals that need no device to say so (arrays: any non-null address)
    lib, fstats, bstats = iface.library(), iface.BatchFoldStats(), iface.BatchStats()
    h_x, h_m, h_e, h_r = np.ones(8), np.full(16, 7.0), np.full(8, 7.0), np.full(8, 7.0)
    good = (h_x.ctypes.data, 8, 1, h_m.ctypes.data)
    for i, v in ((0, None), (3, None), (1, 0), (1, 2 ** 30 + 1), (2, 0), (2, -1)):
        bad = list(good)
        bad[i] = v
        fstats.nonzero = 99
        assert lib.neutral_hip_batch_fold(*bad, C.byref(fstats)) == 1, (i, v)
        assert fstats.nonzero == 0 and fstats.sum == 0.0 and np.all(h_m == 7.0)
    good = (h_m.ctypes.data, 8, 2, 2.0, h_e.ctypes.data, h_r.ctypes.data)
    nan, inf = float("nan"), float("inf")
    for i, v in ((0, None), (4, None), (5, None), (1, 0), (1, 2 ** 30 + 1), (2, 1), (2, 0), (2, -4), (3, 0.0), (3, -1.0),
                 (3, inf), (3, nan)):
        bad = list(good)
        bad[i] = v
        bstats.scored = 99
        assert lib.neutral_hip_batch_statistics(*bad, C.byref(bstats)) == 1, (i, v)
        assert bstats.scored == 0 and np.all(h_e == 7.0) and np.all(h_r == 7.0)
    for k in (0, -3):
        with pytest.raises(iface.BatchRefused) as refused:
            iface.batch_fold(x, k, moments)
        assert refused.value.code == 1
    with pytest.raises(iface.BatchRefused):
        iface.batch_statistics(moments, 1)
    # BatchedRun: what it refuses, before it makes a Simulation
    prob = problem(*CSP)
    keys, values = _tables()
    for kw in (dict(batches=1), dict(batches=0), dict(batches=-8), dict(batches=3), dict(batches=7),
               dict(batches=16000), dict(batches=8, domain=(1, 1)), dict(batches=8, shard=(0, 1000))):
        with pytest.raises(ValueError):
            iface.BatchedRun(prob, keys, values, **kw)
    with pytest.raises(TypeError):
        iface.BatchedRun(prob, keys, values, batches=8.0)
    assert iface.welford_total([1.0, 2.0, 3.0]) == br.total_of([1.0, 2.0, 3.0]) == (2.0, math.sqrt(1.0 / 3.0))


def _driver_dirs(tmp_path, nparticles=8000, steps=3):
    """a run directory with the tables, the arch file beside it and the csp deck of the runs above"""
    from neutral_amd import cs_table, decks
    run = tmp_path / "run"
    (tmp_path / "arch").mkdir()
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel), nx=24, ny=24, nparticles=nparticles, iterations=steps)
    return str(run), rel


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("extra, says", [
    (["--batches", "1"], "--batches wants B >= 2"), (["--batches", "0"], "--batches wants B >= 2"),
    (["--batches", "-4"], "--batches wants B >= 2"), (["--batches", "x"], "--batches wants B >= 2"),
    (["--batches", "2.5"], "--batches wants B >= 2"), (["--batches"], "--batches wants B >= 2"),
    (["--batches", "7"], "7 does not divide 8000"),
    (["--batches", "8", "--gpus", "2"], "--batches does not work with --gpus"),
    (["--gpus", "2", "--batches", "8"], "--batches does not work with --gpus"),
    (["--batches", "8", "--decompose", "1x1"], "--batches does not work with --decompose"),
    (["--decompose", "1x1", "--batches", "8"], "--batches does not work with --decompose")])
def test_driver_usage_errors(tmp_path, extra, says):
    run, rel = _driver_dirs(tmp_path)
    out = subprocess.run([OWN_DRIVER, rel] + extra, cwd=run, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert says in out.stderr + out.stdout


# ---- GPU: fold and statistics alone ----------------------------------------------------------

def _on_torch_stream(iface, torch):
    """the library works on the stream the tensors of a test without a Simulation are made on"""
    iface.set_device(0)
    iface.set_stream(torch.cuda.current_stream().cuda_stream)


def _device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _fold_raw(iface, x, k, moments, null=None, n=None):
    stats = iface.BatchFoldStats()
    rc = iface.library().neutral_hip_batch_fold(
        None if null == "x" else C.c_void_p(x.data_ptr()), x.numel() if n is None else n, k,
        None if null == "moments" else C.c_void_p(moments.data_ptr()), C.byref(stats))
    return rc, stats


def _stats_raw(iface, moments, nbatches, scale, estimate, relerr, null=None, n=None):
    stats = iface.BatchStats()
    p = {name: None if null == name else C.c_void_p(t.data_ptr())
         for name, t in (("moments", moments), ("estimate", estimate), ("relerr", relerr))}
    rc = iface.library().neutral_hip_batch_statistics(p["moments"], moments.numel() // 2 if n is None else n, nbatches,
                                                      scale, p["estimate"], p["relerr"], C.byref(stats))
    return rc, stats


@gpu
@needs_gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("nbatches", BATCH_COUNTS)
def test_fold_and_statistics_bit_for_bit(iface, n, nbatches):
    """Moments, estimate, relerr, the counts and the maximum: the restatement's bits -- a build that
    contracts fl(d * d2) into the sum, or d / k into the mean, fails here.  The three sums: the
    restated order's bits too (tile_sum); where every partial sum is exact (the fold's sum of dyadic
    data) exactly the sum, and elsewhere within the any-order bound of the exact sum.  (A relerr and
    an estimate are no multiples of 2^-10 even where the batches are: what makes mean_relerr and
    estimate_sum the same bits as the restatement's is the restated order.)"""
    import torch
    _on_torch_stream(iface, torch)
    for kind in ("dyadic", "continuous"):
        batches = batch_data(n, nbatches, kind, 1000 * nbatches + n)
        moments = torch.full((2 * n,), float("nan"), dtype=torch.float64, device="cuda")  # (k == 1 ignores it)
        want = None
        for k, x in enumerate(batches, 1):
            want, wf = br.fold(x, k, want)
            got_moments, fs = iface.batch_fold(_device(torch, x), k, moments)
            assert got_moments is moments
            assert same_bits(moments.cpu().numpy(), want), (kind, k)
            exact = math.fsum(x)
            print(f"n={n} B={nbatches} {kind} k={k}: sum off the exact one by {abs(fs.sum - exact):.3e}, "
                  f"fold_ms {fs.fold_ms:.3f}")
            assert fs.nonzero == wf["nonzero"] and fs.sum == wf["sum"], (kind, k)
            if kind == "dyadic":
                assert fs.sum == exact
            assert abs(fs.sum - exact) <= any_order_bound(x, exact)
        for scale in (float(nbatches), 1.0):
            ws = br.statistics(want, nbatches, scale)
            estimate, relerr, stats = iface.batch_statistics(moments, nbatches, None if scale == nbatches else scale)
            e, r = estimate.cpu().numpy(), relerr.cpu().numpy()
            assert same_bits(e, ws.estimate) and same_bits(r, ws.relerr), (kind, scale)
            scored = want[:n] != 0.0
            exact_e, exact_r = math.fsum(e), math.fsum(r[scored])
            print(f"n={n} B={nbatches} {kind} scale={scale}: {ws.stats} estimate_sum off by "
                  f"{abs(stats.estimate_sum - exact_e):.3e} stats_ms {stats.stats_ms:.3f}")
            assert (stats.scored, stats.within_10pc, stats.within_5pc, stats.max_relerr) == \
                tuple(ws.stats[f] for f in ("scored", "within_10pc", "within_5pc", "max_relerr"))
            assert stats.max_relerr == (r[scored].max() if scored.any() else 0.0)
            assert abs(stats.estimate_sum - exact_e) <= any_order_bound(e, exact_e)
            if scored.any() and np.isfinite(exact_r):
                assert abs(stats.mean_relerr - exact_r / scored.sum()) <= \
                    any_order_bound(r[scored], exact_r) / scored.sum() + 2 * EPS * exact_r / scored.sum()
            assert stats.estimate_sum == ws.stats["estimate_sum"] and stats.mean_relerr == ws.stats["mean_relerr"], \
                (kind, scale)


REFUSALS = ["x null", "moments null", "len 0", "len beyond", "k 0", "k negative", "x nan", "x inf", "x -inf",
            "stats moments null", "estimate null", "relerr null", "stats len 0", "stats len beyond", "nbatches 1",
            "nbatches 0", "scale 0", "scale negative", "scale inf", "scale nan", "mean nan", "mean inf", "M2 negative",
            "M2 nan", "M2 inf"]


@gpu
@needs_gpu
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_leave_everything_untouched(iface, case):
    """the device-found ones sit in the last entry of scan_tile() + 1: in the second workgroup"""
    import torch
    _on_torch_stream(iface, torch)
    n = scan_tile() + 1
    x = batch_data(n, 1, "continuous", 5)[0]
    moments_h = br.run(batch_data(n, 3, "continuous", 6))[0]
    sentinel = np.full(2 * n, -3.0)
    value = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "negative": -1.0e-300}.get(case.split()[-1])
    if case in ("x null", "moments null", "len 0", "len beyond", "k 0", "k negative", "x nan", "x inf", "x -inf"):
        if case.startswith("x ") and value is not None:
            x[-1] = value
        d_x, moments = _device(torch, x), _device(torch, sentinel)
        rc, stats = _fold_raw(iface, d_x, {"k 0": 0, "k negative": -2}.get(case, 2), moments,
                              null=case.split()[0] if case.endswith("null") else None,
                              n={"len 0": 0, "len beyond": 2 ** 30 + 1}.get(case))
        assert rc == 1 and (stats.sum, stats.nonzero) == (0.0, 0)
        assert same_bits(moments.cpu().numpy(), sentinel)
        if case.startswith("x ") and value is not None:  # found on the device
            with pytest.raises(iface.BatchRefused) as refused:
                iface.batch_fold(d_x, 1, moments)
            assert refused.value.code == 1 and same_bits(moments.cpu().numpy(), sentinel)
            x[-1] = 1.0  # ... and without it the same call is served
            assert _fold_raw(iface, _device(torch, x), 1, moments)[0] == 0 and same_bits(moments.cpu().numpy()[:n], x)
        return
    if case.startswith(("mean", "M2")):
        moments_h[n - 1 if case.startswith("mean") else 2 * n - 1] = value
    moments = _device(torch, moments_h)
    estimate, relerr = _device(torch, sentinel[:n]), _device(torch, sentinel[:n])
    null = {"stats moments null": "moments", "estimate null": "estimate", "relerr null": "relerr"}.get(case)
    scale = {"scale 0": 0.0, "scale negative": -3.0, "scale inf": np.inf, "scale nan": np.nan}.get(case, 3.0)
    rc, stats = _stats_raw(iface, moments, {"nbatches 1": 1, "nbatches 0": 0}.get(case, 3), scale, estimate, relerr,
                           null=null, n={"stats len 0": 0, "stats len beyond": 2 ** 30 + 1}.get(case))
    assert rc == 1 and (stats.scored, stats.within_10pc, stats.max_relerr, stats.mean_relerr, stats.estimate_sum) == \
        (0, 0, 0.0, 0.0, 0.0)
    assert same_bits(estimate.cpu().numpy(), sentinel[:n]) and same_bits(relerr.cpu().numpy(), sentinel[:n])
    assert same_bits(moments.cpu().numpy(), moments_h)
    if case.startswith(("mean", "M2")):
        with pytest.raises(iface.BatchRefused):
            iface.batch_statistics(moments, 3, None, estimate, relerr)
        assert same_bits(estimate.cpu().numpy(), sentinel[:n])
        moments_h[n - 1 if case.startswith("mean") else 2 * n - 1] = 1.0  # ... and without it it is served
        assert _stats_raw(iface, _device(torch, moments_h), 3, 3.0, estimate, relerr)[0] == 0
        assert same_bits(estimate.cpu().numpy(), br.statistics(moments_h, 3, 3.0).estimate)


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_the_calls_cost_the_next_tiled_step_no_import(iface, make_problem, cs, lazy, monkeypatch):
    """Two folds and the statistics of the tally between two steps of a tiled store leave its records
    valid: the step after them has the stats of the same step of a run without them -- one wait for
    the device -- and the store ends with the same bits.  The deck and the fields of
    tests/test_census.py::test_census_costs_the_next_tiled_step_no_import."""
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
            moments, _ = iface.batch_fold(sim.tally, 1)
            _, fold = iface.batch_fold(sim.tally, 2, moments)
            estimate, relerr, stats = iface.batch_statistics(moments, 2)
            assert fold.nonzero == stats.scored > 0 and stats.max_relerr == 0.0 and not relerr.any().item()
            assert same_bits(estimate.cpu().numpy(), 2.0 * sim.tally_host())
        third = sim.step(3)
        arrays = sim.particle_arrays()
        iface.library().neutral_hip_invalidate_particles(sim.particles)
        fourth = sim.step(4).stats
        runs.append((arrays, third, fourth, sim.tally_host()))
        sim.close()
    (a, ra, imported, ta), (b, rb, _, tb) = runs
    sa, sb = ra.stats, rb.stats
    assert sb.host_syncs == 1, (sb.host_syncs, sb.stream_passes, sb.stream_passes_enqueued)
    assert (sb.host_syncs, sb.stream_passes_enqueued, sb.stream_passes) == \
        (sa.host_syncs, sa.stream_passes_enqueued, sa.stream_passes)
    assert imported.host_syncs > 1  # (what a step that imports the arrays again looks like)
    for f in wr.FIELDS:
        assert same_bits(a[f], b[f]), f
    assert (ra.nprocessed, ra.facets, ra.collisions, ra.census) == (rb.nprocessed, rb.facets, rb.collisions, rb.census)
    assert l2(tb, ta) <= 1e-13  # (the tally itself: sums of f64 atomics, the same from run to run to rounding only)


# ---- GPU: BatchedRun --------------------------------------------------------------------------

def _batched(iface, deck, each=None, between=None, **options):
    """BatchedRun over one of the decks above: -> (result, every batch's energy tally on the host)"""
    name, nparticles, steps = deck
    run = iface.BatchedRun(problem(*deck), *_tables(), batches=NB, **options)
    seen = []
    result = run.run(steps, between=between, each_batch=lambda sim, b: seen.append(sim.tally_host().copy()))
    run.close()
    return result, seen


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [2, 0])
def test_batched_run_against_the_oracle(iface, variant):
    tallies, want, want_total = oracle_batches(*CSP)
    result, seen = _batched(iface, CSP, variant=variant)
    assert len(seen) == NB == result.nbatches
    for b in range(NB):
        print(f"variant {variant} batch {b}: tally rel L2 {l2(seen[b], tallies[b]):.3e}")
        assert l2(seen[b], tallies[b]) < TALLY_L2_TOL
    # the estimate is the run: one Simulation over all the particles
    sim = iface.Simulation(problem(*CSP), *_tables(), variant=variant)
    sim.inject()
    for tt in range(1, CSP[2] + 1):
        sim.step(tt)
    whole = sim.tally_host()
    sim.close()
    energy = result["energy"]
    estimate, relerr = energy.estimate.cpu().numpy(), energy.relerr.cpu().numpy()
    print(f"estimate against the one-run tally: {l2(estimate, whole):.3e}")
    assert l2(estimate, whole) <= 1e-13
    # relerr: inputs that agree to 1e-9 of a cell's mean move a spread of at least 1e-2 of it (the CPU
    # test above) by 1e-7; the bar is ten times that
    scored = want.estimate != 0.0
    assert np.array_equal(estimate != 0.0, scored) and not relerr[~scored].any()
    print(f"relerr over the scored cells: {l2(relerr[scored], want.relerr[scored]):.3e}")
    assert l2(relerr[scored], want.relerr[scored]) <= 1e-6
    # the counts: no relerr of the oracle lies within 1e-6 of a limit (asserted on the CPU as well)
    assert np.abs(want.relerr[scored] - 0.1).min() > 1e-6
    assert energy.stats.scored == want.stats["scored"] and energy.stats.within_10pc == want.stats["within_10pc"]
    assert math.isclose(energy.stats.mean_relerr, want.stats["mean_relerr"], rel_tol=1e-6)
    assert math.isclose(energy.total, want_total[0], rel_tol=1e-9) and math.isclose(energy.total_se, want_total[1], rel_tol=1e-6)
    assert energy.total == iface.welford_total(energy.batch_totals)[0] and len(energy.batch_totals) == NB
    assert result.wall_seconds > 0.0
    assert math.isclose(result.fom, 1.0 / (energy.stats.mean_relerr ** 2 * result.wall_seconds), rel_tol=1e-12)


@gpu
@needs_gpu
def test_every_kept_tally_gets_its_statistics(iface):
    """flux, collision tallies, current, outflow and a spectrum beside the energy: each folded as one
    array, each estimate the sum of what the batches held"""
    edges = [1.0e-3, 1.0, 1.0e3, 2.0e7]
    sums = {}

    def each(sim, b):
        for name, t in (("flux", sim.flux), ("collisions", sim.collisions), ("jx", sim.jx), ("outflow", sim.outflow),
                        ("spectrum", sim.spectrum)):
            sums[name] = sums.get(name, 0.0) + t.cpu().numpy()

    run = iface.BatchedRun(problem(*CSP), *_tables(), batches=NB, variant=2, scalar_flux=True, collision_tallies=True,
                           current=True, outflow=True, spectrum=(edges, None))
    result = run.run(CSP[2], each_batch=each)
    run.close()
    assert sorted(result.tallies) == sorted(["energy", "flux", "collisions", "absorbed", "jx", "jy", "outflow", "spectrum"])
    assert result["outflow"].estimate.numel() == 4 * 576 and result["spectrum"].estimate.numel() == 6
    for name, total in sums.items():
        got = result[name].estimate.cpu().numpy()
        assert np.abs(total).sum() > 0.0, name
        assert l2(got, total) <= 1e-13, name
        if name != "jx":  # (a tally that is not negative: its mean is 0 where no batch scored)
            assert result[name].stats.scored == np.count_nonzero(total), name


@gpu
@needs_gpu
def test_stream_deck_total_has_no_error(iface):
    """the collision-free deck: the batch totals agree to rounding, the cells do not"""
    _, want, want_total = oracle_batches(*STREAM)
    result, _ = _batched(iface, STREAM, variant=2)
    energy = result["energy"]
    relerr = energy.relerr.cpu().numpy()
    print(f"total {energy.total:.15e} relative standard error {energy.total_relerr:.3e}, relerr {relerr.min():.4f} .. "
          f"{relerr.max():.4f} (oracle {want.relerr.min():.4f} .. {want.relerr.max():.4f})")
    assert energy.total_relerr <= 1e-12
    assert energy.stats.scored == 576 and relerr.min() >= 1e-3 and energy.stats.mean_relerr > 1e-2


@gpu
@needs_gpu
def test_error_falls_with_the_particle_count(iface):
    """4 000 against 16 000 particles: the ratio of the median relerr over the cells scored in both is
    the oracle's for the same two runs -- the same deterministic histories, not a statistical bar"""
    few, many = ("csp", 4000, 3), ("csp", 16000, 3)
    want = median_ratio(oracle_batches(*few)[1].relerr, oracle_batches(*many)[1].relerr)
    got = median_ratio(_batched(iface, few, variant=2)[0]["energy"].relerr.cpu().numpy(),
                       _batched(iface, many, variant=2)[0]["energy"].relerr.cpu().numpy())
    print(f"median relerr, 4000 over 16000 particles: {got:.6f} (oracle {want:.6f}; the law is 2)")
    assert 1.5 < want < 2.5 and math.isclose(got, want, rel_tol=1e-6)


@gpu
@needs_gpu
def test_auto_windows_inside_the_batches(iface):
    """roulette, capture = scatter / 2, auto_window() after steps 1 and 2 of every batch: the run
    completes, every batch's window stats come back, and the estimate's total stays within three of
    its own standard errors of the run without windows -- a fair game keeps the mean.  (The plain
    total's standard error is above 1 %: the CPU test above, and here.)"""
    options = dict(variant=2, roulette=ON, cs_absorb=third_absorb(_tables()))
    plain, _ = _batched(iface, CSP, **options)
    windowed, _ = _batched(iface, CSP, between=lambda sim, tt: sim.auto_window() if tt < 3 else None, **options)
    p, w = plain["energy"], windowed["energy"]
    print(f"plain {p.total:.6e} +- {p.total_se:.3e}, windowed {w.total:.6e} +- {w.total_se:.3e}, mean relerr "
          f"{p.stats.mean_relerr:.4f} -> {w.stats.mean_relerr:.4f}")
    _, _, want_plain = oracle_batches(*CSP, third=True)
    assert want_plain[1] / want_plain[0] > 0.01 and p.total_relerr > 0.01
    assert math.isclose(p.total, want_plain[0], rel_tol=1e-9)
    assert len(windowed.between) == NB
    acted = 0
    for per_batch in windowed.between:
        assert len(per_batch) == 3 and per_batch[2] is None
        for census, bounds, window in per_batch[:2]:
            assert 0 < census.live <= 1000 and bounds.windowed_cells == census.occupied_cells
            assert window.live_before == census.live
            acted += window.split + window.roulette_killed + window.roulette_survived
    assert acted > 0
    assert abs(w.total - p.total) <= 3.0 * w.total_se
    assert math.isclose(w.stats.estimate_sum, w.total, rel_tol=1e-12)


# ---- GPU: the driver ----------------------------------------------------------------------------

def _batch_block(stdout):
    total = re.search(r"^Batch total energy deposition (\S+) \+- (\S+) \(relative (\S+)\)$", stdout, flags=re.M)
    errors = re.search(r"^Batch relative error mean (\S+) max (\S+) over (\d+) scored cells$", stdout, flags=re.M)
    within = re.search(r"^Batch scored cells within 10% (\d+) within 5% (\d+)$", stdout, flags=re.M)
    fom = re.search(r"^Batch FOM (\S+) ", stdout, flags=re.M)
    assert total and errors and within and fom, stdout[-2000:]
    return total.groups(), errors.groups(), within.groups(), float(fom.group(1))


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_batches(iface, tmp_path):
    """`neutral.hip --batches 8` on the csp deck of the runs above prints BatchedRun's total and error
    to the printed digits; with --window auto it runs the windows inside each batch"""
    run, rel = _driver_dirs(tmp_path)
    plain = run_driver(run, rel, ["--variant", "2"])
    assert "Batch" not in plain
    out = run_driver(run, rel, ["--variant", "2", "--batches", "8"])
    total, errors, within, fom = _batch_block(out)
    result, _ = _batched(iface, CSP, variant=2)
    e = result["energy"]
    assert total == ("%.15e" % e.total, "%.6e" % e.total_se, "%.6e" % e.total_relerr)
    assert errors == ("%.6e" % e.stats.mean_relerr, "%.6e" % e.stats.max_relerr, str(e.stats.scored))
    assert within == (str(e.stats.within_10pc), str(e.stats.within_5pc)) and fom > 0.0
    assert re.search(r"^Batches 8 of 1000 particles$", out, flags=re.M)
    assert len(re.findall(r"^Batch \d of 8$", out, flags=re.M)) == 8
    # what is validated is the estimate: the sum of the batch tallies, the run's own total
    final = float(re.search(r"^Final global_energy_tally (\S+)$", out, flags=re.M).group(1))
    final_plain = float(re.search(r"^Final global_energy_tally (\S+)$", plain, flags=re.M).group(1))
    assert math.isclose(final, final_plain, rel_tol=1e-12) and math.isclose(final, e.total, rel_tol=1e-12)
    windowed = run_driver(run, rel, ["--variant", "2", "--batches", "8", "--roulette", "0.25,0.5", "--window", "auto"])
    _batch_block(windowed)
    assert len(re.findall(r"^Census live ", windowed, flags=re.M)) == 8 * 2
    assert re.search(r"^Window auto skipped 0$", windowed, flags=re.M)

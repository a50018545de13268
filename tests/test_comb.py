"""The census weight comb (include/neutral_hip.h: neutral_hip_comb_particles).

CPU: the numpy restatement (tests/comb_reference.py) pinned by hand-computed and structural cases,
the ABI, the wrapper's argument handling, the driver's usage errors.  GPU: the library against the
restatement tooth for tooth at every size where the scans take another path, what the definition
implies (bitwise copies, one weight, determinism, refusals), and the comb inside a run against the
CPU oracle for the variants and export modes that reach it through different states.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import census_ops_support
import comb_reference as cr
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, scan_sizes, scan_tile  # noqa: F401

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
ALL_FIELDS = cr.COPIED_FIELDS + ("weight", "dead")


# ---- CPU: the restatement --------------------------------------------------------------------

def test_hand_computed_comb_of_four():
    # lw = 1, 3, 0, 4; S = 1, 4, 4, 8; W = 8, delta = 2; teeth at 1, 3, 5, 7
    c = cr.comb([1.0, 3.0, 5.0, 4.0], [0, 0, 1, 0], v=0.5)
    assert c.S.tolist() == [1.0, 4.0, 4.0, 8.0]
    assert (c.W, c.delta) == (8.0, 2.0)
    assert c.teeth.tolist() == [1.0, 3.0, 5.0, 7.0]
    assert c.src.tolist() == [1, 1, 3, 3]  # (S_0 <= t_0: the tooth on a boundary goes up)
    assert (c.live_before, c.sources_kept, c.max_copies) == (3, 2, 2)
    arrays = {f: np.arange(4, dtype=np.float64) * 10 for f in cr.COPIED_FIELDS}
    out = c.apply(arrays)
    assert out["x"].tolist() == [10.0, 10.0, 30.0, 30.0]
    assert out["weight"].tolist() == [2.0] * 4 and out["dead"].tolist() == [0] * 4
    # v = 0: teeth at 0, 2, 4, 6 -> 0, 1, 3, 3
    assert cr.comb([1.0, 3.0, 5.0, 4.0], [0, 0, 1, 0], v=0.0).src.tolist() == [0, 1, 3, 3]


def test_offset_is_the_stream_of_the_key_no_particle_carries():
    import oracle_binding as ob
    for pid_base, seed in ((0, 0), (0, 7), (1000, 7), (2 ** 40, 3)):
        rn0, _ = ob.generate_random_numbers(2 ** 64 - 1 - pid_base, seed, 0)
        v = cr.comb_offset(pid_base, seed)
        assert v == 1.0 - rn0 and 0.0 <= v < 1.0
    assert cr.comb_offset(0, 7) != cr.comb_offset(1000, 7) != cr.comb_offset(1000, 8)


@pytest.mark.parametrize("n", [1, 2, 65, 1000, 100003])
def test_copy_counts_are_floor_or_ceil(n):
    w, dead = cr.prototype_weights(n)
    c = cr.comb(w, dead, seed=n)
    share = n * np.where(dead == 0, w, 0.0) / c.W
    assert not c.guarded.any()
    assert np.all((c.copies == np.floor(share)) | (c.copies == np.ceil(share)))
    assert c.copies.sum() == n and np.all(c.copies[dead != 0] == 0)
    assert abs(c.delta * n - c.W) <= 1e-15 * c.W


def test_equal_weights_nobody_dead_is_the_identity():
    for n in (1, 64, 1000, 100003):
        c = cr.comb(np.ones(n), np.zeros(n, dtype=np.int32), seed=5)
        assert np.array_equal(c.src, np.arange(n)) and c.delta == 1.0
        assert (c.sources_kept, c.max_copies, c.live_before) == (n, 1, n)


def test_one_live_particle_fills_the_store():
    n = 100003
    w, dead = np.full(n, 0.25), np.ones(n, dtype=np.int32)
    dead[77777] = 0
    c = cr.comb(w, dead, seed=9)
    assert np.all(c.src == 77777) and c.W == 0.25
    assert (c.live_before, c.sources_kept, c.max_copies) == (1, 1, n)


def test_prefix_sums_are_exact_to_a_rounding():
    import math
    w, dead = cr.prototype_weights(20000)
    lw = np.where(dead == 0, w, 0.0)
    S = cr.prefix_sums(lw)
    for j in (0, 1, 4095, 4096, 4097, 12345, 19999):
        assert S[j] == math.fsum(lw[:j + 1])


# ---- CPU: the ABI, the wrapper, the driver ---------------------------------------------------

def test_library_exports_the_comb():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_comb_particles")
    assert "neutral_hip_comb_particles" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.CombStats._fields_] == [
        "live_before", "sources_kept", "max_copies", "weight_before", "weight_each", "comb_ms"]
    assert C.sizeof(iface.CombStats) == 48


def test_wrapper_mirrors_the_kernels_tile():
    from neutral_amd import interface as iface
    assert iface.COMB_TILE == scan_tile()


def test_wrapper_argument_handling():
    from neutral_amd import interface as iface
    with pytest.raises(ValueError):
        iface.comb_particles(None, 16, 1)  # no store
    store = C.pointer(iface.Particle())
    with pytest.raises(ValueError):
        iface.comb_particles(store, 0, 1)
    with pytest.raises(ValueError):
        iface.comb_particles(store, -5, 1)
    with pytest.raises(ValueError):
        iface.comb_particles(store, 16, -1)  # a seed is a uint64
    with pytest.raises(ValueError):
        iface.comb_particles(store, 16, 2 ** 64)
    with pytest.raises(TypeError):
        iface.comb_particles(store, 16.5, 1)
    # the library itself: nothing to comb, nothing touched, no device needed to say so
    stats = iface.CombStats()
    assert iface.library().neutral_hip_comb_particles(None, 16, 1, C.byref(stats)) == 1
    assert iface.library().neutral_hip_comb_particles(store, 0, 1, None) == 1
    assert issubclass(iface.CombRefused, ValueError)


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("extra", [["--comb"], ["--comb", "0"], ["--comb", "-2"], ["--comb", "x"],
                                   ["--comb", "2", "--decompose", "1x1"],
                                   ["--decompose", "1x1", "--comb", "2"]])
def test_driver_usage_errors(tmp_path, extra):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + extra, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert "--comb" in out.stderr + out.stdout


# ---- GPU: the comb alone ---------------------------------------------------------------------



class CombStore(census_ops_support.Store):
    """the store of n injected particles whose weight and dead the test sets"""

    def set(self, weight, dead):
        pc = self.sim.particles.contents
        lib = self.iface.library()
        w = np.ascontiguousarray(weight, dtype=np.float64)
        d = np.ascontiguousarray(dead, dtype=np.int32)
        lib.neutral_hip_memcpy_h2d(C.c_void_p(pc.weight), w.ctypes.data, w.nbytes)
        lib.neutral_hip_memcpy_h2d(C.c_void_p(pc.dead), d.ctypes.data, d.nbytes)

    def raw_comb(self, seed):
        stats = self.iface.CombStats()
        self.iface.set_pid_base(self.sim.pid_base)
        rc = self.iface.library().neutral_hip_comb_particles(self.sim.particles, self.n, seed,
                                                             C.byref(stats))
        return rc, stats


def _check_against(c, before, after, stats, n):
    """the library's result against the restatement c"""
    share = float(c.guarded.sum()) / n
    print(f"n={n} W={c.W!r} guarded teeth {int(c.guarded.sum())} (share {share:.2e}) "
          f"comb_ms={stats.comb_ms:.3f} max_copies={stats.max_copies}")
    assert share <= 1e-4
    if n <= 100003:
        assert not c.guarded.any()
    # which particle every slot holds: the copied fields of the injected particles tell (x is
    # drawn per particle: distinct); src itself is compared through all nine
    want = c.apply(before)
    free = ~c.guarded
    for f in cr.COPIED_FIELDS:
        assert np.array_equal(after[f][free], want[f][free]), f
    if c.guarded.any():
        k = np.flatnonzero(c.guarded)
        for f in cr.COPIED_FIELDS:
            ok = (after[f][k] == before[f][c.src[k]]) | (after[f][k] == before[f][c.src_below[k]]) | \
                 (after[f][k] == before[f][c.src_above[k]])
            assert np.all(ok), f
        # ... and one particle for all nine fields of a slot
        which = np.where(after["x"][k] == before["x"][c.src[k]], c.src[k],
                         np.where(after["x"][k] == before["x"][c.src_below[k]], c.src_below[k],
                                  c.src_above[k]))
        for f in cr.COPIED_FIELDS:
            assert np.array_equal(after[f][k], before[f][which]), f
    assert np.all(after["weight"] == after["weight"][0])
    assert abs(after["weight"][0] - c.delta) <= 1e-13 * c.delta
    assert not after["dead"].any()
    assert abs(after["weight"].sum() - c.W) <= 1e-12 * c.W
    assert stats.live_before == c.live_before
    assert abs(stats.weight_before - c.W) <= 1e-13 * c.W
    assert stats.weight_each == after["weight"][0]
    if not c.guarded.any():
        assert stats.sources_kept == c.sources_kept
        assert stats.max_copies == c.max_copies
    else:
        assert abs(int(stats.sources_kept) - c.sources_kept) <= int(c.guarded.sum())
        assert abs(int(stats.max_copies) - c.max_copies) <= int(c.guarded.sum())


def _sizes():
    tile = scan_tile()  # (tile^2 + 1 <= 2^24 + 3: 2 049 workgroups)
    return sorted(scan_sizes() + [tile * tile])


@gpu
@needs_gpu
@pytest.mark.parametrize("n", _sizes())
def test_random_weights_against_the_restatement(iface, make_problem, cs, n):
    st = CombStore(iface, make_problem, cs, n)
    w, dead = cr.prototype_weights(n, rng_seed=n)
    st.set(w, dead)
    before = st.arrays()
    assert np.array_equal(before["weight"], w) and np.array_equal(before["dead"], dead)
    assert len(np.unique(before["x"])) == n  # (a slot's x names its source)
    rc, stats = st.raw_comb(seed=11)
    assert rc == 0
    after = st.arrays()
    _check_against(cr.comb(w, dead, 0, 11), before, after, stats, n)
    # the same call on the same input: the same bits
    st.set(w, dead)
    for f in cr.COPIED_FIELDS:
        src = before[f]
        st.iface.library().neutral_hip_memcpy_h2d(
            C.c_void_p(getattr(st.sim.particles.contents, f)), src.ctypes.data, src.nbytes)
    rc2, stats2 = st.raw_comb(seed=11)
    again = st.arrays()
    assert rc2 == 0
    for f in ALL_FIELDS:
        assert np.array_equal(again[f], after[f]), f
    assert (stats2.live_before, stats2.sources_kept, stats2.max_copies, stats2.weight_before,
            stats2.weight_each) == (stats.live_before, stats.sources_kept, stats.max_copies,
                                    stats.weight_before, stats.weight_each)
    # another seed: another offset
    if 1000 <= n <= 100003:
        st.set(w, dead)
        for f in cr.COPIED_FIELDS:
            src = before[f]
            st.iface.library().neutral_hip_memcpy_h2d(
                C.c_void_p(getattr(st.sim.particles.contents, f)), src.ctypes.data, src.nbytes)
        rc3, stats3 = st.raw_comb(seed=12)
        assert rc3 == 0
        _check_against(cr.comb(w, dead, 0, 12), before, st.arrays(), stats3, n)
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [1, 65, 2049, 100003])
def test_equal_weights_nobody_dead_changes_nothing(iface, make_problem, cs, n):
    st = CombStore(iface, make_problem, cs, n)
    before = st.arrays()
    assert np.all(before["weight"] == 1.0) and not before["dead"].any()
    stats = st.sim.comb(seed=3)
    after = st.arrays()
    for f in ALL_FIELDS:
        assert np.array_equal(after[f], before[f]), f
    assert (stats.live_before, stats.sources_kept, stats.max_copies) == (n, n, 1)
    assert (stats.weight_before, stats.weight_each) == (float(n), 1.0)
    st.close()


@gpu
@needs_gpu
def test_one_live_particle_among_many(iface, make_problem, cs):
    n = 100003
    st = CombStore(iface, make_problem, cs, n)
    w, dead = cr.prototype_weights(n)
    st.set(w, dead)
    st.raw_comb(seed=1)  # (first call: the workspace is allocated)
    st.set(w, dead)
    rc, random_case = st.raw_comb(seed=1)
    assert rc == 0
    w1, d1 = np.full(n, 0.25), np.ones(n, dtype=np.int32)
    d1[77777] = 0
    st.set(w1, d1)
    before = st.arrays()
    rc, stats = st.raw_comb(seed=2)
    assert rc == 0
    after = st.arrays()
    for f in cr.COPIED_FIELDS:
        assert np.all(after[f] == before[f][77777]), f
    assert np.all(after["weight"] == 0.25 / n) and not after["dead"].any()
    assert (stats.live_before, stats.sources_kept, stats.max_copies) == (1, 1, n)
    print(f"comb_ms random {random_case.comb_ms:.3f} one live {stats.comb_ms:.3f}")
    # (the same launches either way; a loop over the copies would be 100 003 trips of one lane)
    assert stats.comb_ms <= 3.0 * random_case.comb_ms + 0.5
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("case", ["all dead", "nan", "inf", "negative", "zero weight"])
def test_refused_stores_are_untouched(iface, make_problem, cs, case):
    n = 5000
    st = CombStore(iface, make_problem, cs, n)
    w, dead = cr.prototype_weights(n)
    if case == "all dead":
        dead[:] = 1
    elif case == "zero weight":
        w[dead == 0] = 0.0
    else:
        j = int(np.flatnonzero(dead == 0)[n // 3])
        w[j] = {"nan": float("nan"), "inf": float("inf"), "negative": -0.5}[case]
    st.set(w, dead)
    before = st.arrays()
    rc, stats = st.raw_comb(seed=4)
    assert rc == 1
    after = st.arrays()
    for f in ALL_FIELDS:
        assert np.array_equal(after[f], before[f], equal_nan=(f == "weight")), f
    assert stats.live_before == int((dead == 0).sum())
    with pytest.raises(iface.CombRefused) as refused:
        st.sim.comb(seed=4)
    assert refused.value.code == 1
    # a bad weight in a DEAD slot is nobody's business
    if case in ("nan", "negative"):
        w2, d2 = cr.prototype_weights(n)
        j = int(np.flatnonzero(d2 != 0)[5])
        w2[j] = float("nan") if case == "nan" else -0.5
        st.set(w2, d2)
        rc, _ = st.raw_comb(seed=4)
        assert rc == 0
    st.close()


@gpu
@needs_gpu
def test_pid_base_moves_the_offset(iface, make_problem, cs):
    n, base = 1000, 123456789
    w, dead = cr.prototype_weights(n)
    results = {}
    for pid_base in (0, base):
        st = CombStore(iface, make_problem, cs, n, pid_base=pid_base)
        st.set(w, dead)
        before = st.arrays()
        stats = st.sim.comb(seed=21)
        c = cr.comb(w, dead, pid_base, 21)
        _check_against(c, before, st.arrays(), stats, n)
        results[pid_base] = c.src
        st.close()
    assert cr.comb_offset(0, 21) != cr.comb_offset(base, 21)
    assert not np.array_equal(results[0], results[base])


# ---- GPU: the comb in a run, against the oracle ---------------------------------------------

ON = (0.25, 0.5)
HALF = 3  # steps before the comb, and after it


@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_comb_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """Steps, comb, steps: the library (records written back before the comb and imported again
    after it) against oracle steps, the restatement on the oracle's arrays, oracle steps."""
    import oracle_binding as ob
    keys, values = cs
    absorb = (np.array(keys), 0.5 * np.array(values))  # capture = scatter / 2: p_absorb = 1/3
    prob = make_problem("csp", nx=24, nparticles=6000, iterations=2 * HALF, dt=2.0e-6)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=ON, cs_absorb=absorb)
    ref = ob.OracleRun(prob, keys, values, cs_absorb=absorb, roulette=ON)
    sim.inject()
    ref.inject()

    def both_step(tt):
        g, c = sim.step(tt), ref.step(tt)
        assert (g.nprocessed, g.facets, g.collisions, g.census) == \
            (c.nprocessed, c.facets, c.collisions, c.census), tt
        assert (g.stats.roulette_killed, g.stats.roulette_survived) == \
            (c.roulette_killed, c.roulette_survived), tt
        return c

    killed = sum(both_step(tt).roulette_killed for tt in range(1, HALF + 1))
    assert killed > 0  # roulette has ended histories: there are slots to refill
    arrays = ref.particles.as_dict()
    assert arrays["dead"].any()
    c = cr.comb(arrays["weight"], arrays["dead"], 0, HALF)
    assert not c.guarded.any()
    stats = sim.comb(seed=HALF)
    new = c.apply(arrays)
    for f in ALL_FIELDS:
        arrays[f][:] = new[f]
    assert (stats.live_before, stats.sources_kept, stats.max_copies) == \
        (c.live_before, c.sources_kept, c.max_copies)
    assert stats.live_before < prob.nparticles and stats.max_copies > 1
    for tt in range(HALF + 1, 2 * HALF + 1):
        c_step = both_step(tt)
    assert c_step.nprocessed > stats.live_before  # (the refilled slots are stepped)
    got = sim.particle_arrays()
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got[f], arrays[f]), f
    tg, tc = sim.tally_host(), ref.tally
    print(f"variant {variant} lazy {lazy}: tally rel L2 {np.linalg.norm(tg - tc) / np.linalg.norm(tc):.3e} "
          f"worst cell {np.max(np.abs(tg - tc) / np.maximum(np.abs(tc), 1e-300)):.3e}")
    assert np.linalg.norm(tg - tc) / np.linalg.norm(tc) < TALLY_L2_TOL
    assert np.all(np.abs(tg - tc) <= TALLY_L2_TOL * np.abs(tc))
    sim.close()

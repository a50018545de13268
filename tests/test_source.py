"""The fixed source (include/neutral_hip.h: neutral_hip_source_particles).

CPU: the numpy restatement (tests/source_reference.py) pinned by a hand-computed case and by the
properties of `ranks`, the ABI, the wrapper's argument handling, the driver's usage errors.  GPU:
a refill with injection's key and weight against injection's own bits at every size where the scan
takes another path, which slots are refilled and that nothing else is touched, another seed, weight
and energy against the restatement, refusals, and the source inside a run against the CPU oracle
for the variants and export modes that reach it through different states.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import census_ops_support
import source_reference as sr
from census_ops_support import _source_totals, same_bits
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, rel, scan_sizes, scan_tile  # noqa: F401

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
SEED = 2 ** 63 + 17


# ---- CPU: the restatement --------------------------------------------------------------------

def test_hand_computed_source_of_six():
    dead = np.array([0, 1, 1, 0, 7, 1], dtype=np.int32)  # dead: 1, 2, 4, 5 (any non-zero word)
    assert sr.ranks(dead, 3).tolist() == [1, 2, 4]
    edge = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    args = sr.SourceArgs(0.25, 0.5, 0.5, 0.25, 10, 20, 1e-7, edge, edge, 2.0)
    before = {f: np.arange(6, dtype=np.float64) + 100 for f in sr.F64_FIELDS}
    before.update({f: np.arange(6, dtype=np.int32) + 50 for f in ("cellx", "celly")}, dead=dead)
    # rn[slot, counter] = (rn0, rn1): x = 0.25 + rn0 / 2, y = 0.5 + rn1 / 4, theta = 2 pi rn0 of counter 1
    rn = np.array([[[0.5, 0.5], [0.25, 0.9]], [[1.0, 1.0], [0.5, 0.9]], [[0.25, 0.0], [1.0, 0.9]]])
    out = sr.expected(before, dead, 3, 0.5, 99, 7, args, rn)
    assert out["dead"].tolist() == [0, 0, 0, 0, 0, 1]
    assert out["x"].tolist() == [100.0, 0.5, 0.75, 103.0, 0.375, 105.0]
    assert out["y"].tolist() == [100.0, 0.625, 0.75, 103.0, 0.5, 105.0]
    assert out["cellx"].tolist() == [50, 12, 13, 53, 11, 55]  # 10 + cell of 0.5, 0.75, 0.375
    assert out["celly"].tolist() == [50, 22, 23, 53, 22, 55]  # 20 + cell of 0.625, 0.75, 0.5
    assert np.allclose(out["omega_x"][[1, 2, 4]], [0.0, -1.0, 1.0], atol=1e-15)
    assert np.allclose(out["omega_y"][[1, 2, 4]], [1.0, 0.0, 0.0], atol=1e-15)
    for f, v in (("energy", 2.0), ("weight", 0.5), ("dt_to_census", 1e-7), ("mfp_to_collision", 0.0)):
        assert out[f].tolist() == [100.0, v, v, 103.0, v, 105.0], f
    # a coordinate at or beyond the last edge has no cell: 0, as the reference's scan leaves it
    assert sr.find_cell(edge, np.array([1.0, -0.1, 0.999])).tolist() == [0, 0, 3]
    # the oracle's samples: the streams of keys 7 + slot under master key 99
    import oracle_binding as ob
    cpu = sr.cpu_samples([1, 2, 4], 7, 99)
    assert tuple(cpu[2, 1]) == ob.generate_random_numbers(11, 99, 1)
    assert sr.probe_rows([1, 4], 7, 99).tolist() == [[0, 8, 99], [1, 8, 99], [0, 11, 99], [1, 11, 99]]


@pytest.mark.parametrize("n", [1, 2, 65, 1000, 100003])
def test_ranks_are_the_first_dead_in_ascending_order(n):
    rng = np.random.default_rng(n)
    for share in (0.0, 0.3, 1.0):
        dead = (rng.random(n) < share).astype(np.int32) * rng.integers(1, 9, n).astype(np.int32)
        every = np.flatnonzero(dead)
        ndead = len(every)
        for count in (0, 1, ndead - 1, ndead, ndead + 5):
            r = sr.ranks(dead, count)
            assert len(r) == min(max(count, 0), ndead)
            assert np.all(np.diff(r) > 0) and np.all(dead[r] != 0)
            assert np.array_equal(r, every[:len(r)])  # the first m, nothing skipped
        assert len(sr.ranks(dead, 0)) == 0 and np.array_equal(sr.ranks(dead, n + 1), every)


# ---- CPU: the ABI, the wrapper, the driver ---------------------------------------------------

def test_library_exports_the_source():
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_source_particles")
    assert "neutral_hip_source_particles" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.SourceStats._fields_] == [
        "dead_before", "emitted", "weight_emitted", "source_ms"]
    assert C.sizeof(iface.SourceStats) == 32
    assert iface.SOURCE_SEED_BASE == 2 ** 63


_BOX = (4, 4, 0, 0.0, 0.0, 1.0, 1.0, 0, 0, 1e-7, None, None, 1.0)  # (no mesh: nothing gets that far)


def test_wrapper_argument_handling():
    from neutral_amd import interface as iface
    with pytest.raises(ValueError):
        iface.source_particles(None, 16, 1, 1.0, 0, *_BOX)  # no store
    store = C.pointer(iface.Particle())
    for n, count, seed in ((0, 1, 0), (-5, 1, 0), (16, -1, 0), (16, 2 ** 31, 0), (16, 1, -1),
                           (16, 1, 2 ** 64)):
        with pytest.raises(ValueError):
            iface.source_particles(store, n, count, 1.0, seed, *_BOX)
    for n, count, seed in ((16.5, 1, 0), (16, 1.5, 0), (16, 1, 0.5), (16, True, 0)):
        with pytest.raises(TypeError):
            iface.source_particles(store, n, count, 1.0, seed, *_BOX)
    # the library itself: nothing to refill, nothing touched, no device needed to say so
    lib, stats = iface.library(), iface.SourceStats()
    assert lib.neutral_hip_source_particles(None, 16, 1, 1.0, 0, *_BOX, C.byref(stats)) == 1
    assert lib.neutral_hip_source_particles(store, 0, 1, 1.0, 0, *_BOX, None) == 1
    assert lib.neutral_hip_source_particles(store, 16, -1, 1.0, 0, *_BOX, None) == 1
    for weight in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.neutral_hip_source_particles(store, 16, 1, weight, 0, *_BOX, None) == 1
    with pytest.raises(iface.SourceRefused) as refused:
        iface.source_particles(store, 16, 1, 0.0, 0, *_BOX)
    assert refused.value.code == 1 and issubclass(iface.SourceRefused, ValueError)


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("extra", [["--source"], ["--source", "0"], ["--source", "-2"], ["--source", "x"],
                                   ["--source", "5,0"], ["--source", "5,-1"], ["--source", "5,x"],
                                   ["--source", "5", "--decompose", "1x1"],
                                   ["--decompose", "1x1", "--source", "5,2"]])
def test_driver_usage_errors(tmp_path, extra):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + extra, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    said = out.stderr + out.stdout
    if "--decompose" in extra:
        assert "--source does not work with --decompose" in said
    else:
        assert "--source wants COUNT[,WEIGHT]" in said


# ---- GPU: the source alone -------------------------------------------------------------------


class SourceStore(census_ops_support.Store):
    """the store with the fixed source's call"""

    def raw(self, count, weight=1.0, seed=0, energy=None, dt=None, width=None):
        """the library's own call: -> (return code, stats)"""
        stats = self.iface.SourceStats()
        self.iface.set_pid_base(self.sim.pid_base)
        args = list(self.sim._inject_args())
        if energy is not None:
            args[12] = energy
        if dt is not None:
            args[9] = dt
        if width is not None:
            args[5] = width
        rc = self.iface.library().neutral_hip_source_particles(
            self.sim.particles, self.n, count, weight, seed, *args, C.byref(stats))
        return rc, stats


def _patterns(n):
    rng = np.random.default_rng(n)
    none = np.zeros(n, dtype=bool)
    out = {"none": none, "all": ~none}
    for name, j in (("slot 0", 0), ("last slot", n - 1)):
        out[name] = none.copy()
        out[name][j] = True
    if n >= 2:
        out["alternating"] = np.arange(n) % 2 == 1
    if n >= 10:
        out["random 30 %"] = rng.random(n) < 0.3
    if n >= 64 + 2 * 64:
        out["one wave"] = none.copy()
        out["one wave"][64:128] = True  # lanes 0..63 of the second wave, live slots either side
    return out


@gpu
@needs_gpu
@pytest.mark.parametrize("n", scan_sizes())
def test_seed_0_gives_back_the_injected_particles(iface, make_problem, cs, n):
    st = SourceStore(iface, make_problem, cs, n)
    injected = st.arrays()
    assert not injected["dead"].any() and np.all(injected["weight"] == 1.0)
    for name, mask in _patterns(n).items():
        ndead = int(mask.sum())
        st.kill(injected, mask)
        rc, stats = st.raw(count=n, weight=1.0, seed=0)
        assert rc == 0, name
        assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (ndead, ndead, float(ndead)), name
        after = st.arrays()
        for f in sr.FIELDS:
            assert same_bits(after[f], injected[f]), (name, f)
    print(f"n={n} source_ms (last pattern) {stats.source_ms:.3f}")
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [1000, scan_tile() + 1, 100003])
def test_exactly_the_first_count_dead_slots(iface, make_problem, cs, n):
    st = SourceStore(iface, make_problem, cs, n)
    injected = st.arrays()
    mask = np.random.default_rng(n + 1).random(n) < 0.3
    ndead = int(mask.sum())
    for count in (0, 1, ndead - 1, ndead, ndead + 5):
        killed = st.kill(injected, mask)
        rc, stats = st.raw(count=count, weight=0.25, seed=0)
        assert rc == 0
        m = min(count, ndead)
        assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (ndead, m, m * 0.25)
        after = st.arrays()
        slots = sr.ranks(killed["dead"], count)
        refilled = np.zeros(n, dtype=bool)
        refilled[slots] = True
        for f in sr.FIELDS:
            want = np.full(m, 0.25) if f == "weight" else injected[f][slots]
            assert same_bits(np.ascontiguousarray(after[f][slots]), np.ascontiguousarray(want)), (count, f)
            # every other slot byte for byte, the NaN scribbles and the dead words included
            assert same_bits(np.ascontiguousarray(after[f][~refilled]),
                             np.ascontiguousarray(killed[f][~refilled])), (count, f)
    st.close()


def _check_refilled(iface, after, slots, pid_base, seed, weight, args):
    """the refilled slots of `after` against the restatement, fed the library's own samples"""
    _, rn = iface.probe_threefry(sr.probe_rows(slots, pid_base, seed))
    dead = np.zeros(len(after["dead"]), dtype=np.int32)
    dead[slots] = 1
    want = sr.expected(after, dead, len(slots), weight, seed, pid_base, args, rn)
    for f in ("dead", "energy", "weight", "dt_to_census", "mfp_to_collision"):
        assert np.array_equal(after[f][slots], want[f][slots]), f
    assert not after["dead"][slots].any() and np.all(after["mfp_to_collision"][slots] == 0.0)
    # the tolerances of tests/test_hip_parity.py::test_inject_matches_oracle
    for f in ("x", "y"):
        assert rel(after[f][slots], want[f][slots]) < 1e-15, f
    for f in ("omega_x", "omega_y"):
        assert np.max(np.abs(after[f][slots] - want[f][slots]), initial=0.0) < 1e-15, f
    assert np.array_equal(after["cellx"][slots], args.x_off + sr.find_cell(args.edgex, after["x"][slots]))
    assert np.array_equal(after["celly"][slots], args.y_off + sr.find_cell(args.edgey, after["y"][slots]))


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [65, scan_tile() + 1, 100003])
def test_another_seed_weight_and_energy_against_the_restatement(iface, make_problem, cs, n):
    st = SourceStore(iface, make_problem, cs, n)
    injected = st.arrays()
    mask = np.random.default_rng(n + 2).random(n) < 0.3
    count = int(mask.sum()) - 3
    killed = st.kill(injected, mask)
    slots = sr.ranks(killed["dead"], count)
    rc, stats = st.raw(count=count, weight=0.375, seed=SEED, energy=12345.5)
    assert rc == 0 and stats.emitted == count
    after = st.arrays()
    _check_refilled(iface, after, slots, 0, SEED, 0.375, st.args._replace(energy=12345.5))
    assert np.all(after["energy"][slots] == 12345.5) and np.all(after["weight"][slots] == 0.375)
    assert np.all(after["dt_to_census"][slots] == st.prob.dt)
    # the same call on the same input: the same bits
    st.upload(killed)
    rc, again = st.raw(count=count, weight=0.375, seed=SEED, energy=12345.5)
    assert rc == 0 and again.emitted == count
    second = st.arrays()
    for f in sr.FIELDS:
        assert same_bits(second[f], after[f]), f
    # another seed: other positions (and not injection's)
    st.upload(killed)
    rc, _ = st.raw(count=count, weight=0.375, seed=SEED + 1, energy=12345.5)
    other = st.arrays()
    assert rc == 0
    assert not np.any(other["x"][slots] == after["x"][slots])
    assert not np.any(after["x"][slots] == injected["x"][slots])
    _check_refilled(iface, other, slots, 0, SEED + 1, 0.375, st.args._replace(energy=12345.5))
    st.close()


@gpu
@needs_gpu
def test_pid_base_moves_the_streams(iface, make_problem, cs):
    n, base = 1000, 123456789
    mask = np.random.default_rng(5).random(n) < 0.3
    got = {}
    for pid_base in (0, base):
        st = SourceStore(iface, make_problem, cs, n, pid_base=pid_base)
        killed = st.kill(st.arrays(), mask)
        slots = sr.ranks(killed["dead"], n)
        stats = st.sim.emit(n, seed=SEED, weight=2.0)
        assert stats.emitted == len(slots)
        after = st.arrays()
        _check_refilled(iface, after, slots, pid_base, SEED, 2.0, st.args)
        assert not after["dead"].any()
        got[pid_base] = after["x"][slots]
        st.close()
    assert not np.any(got[0] == got[base])  # the same slots, other particles


@gpu
@needs_gpu
@pytest.mark.parametrize("case", ["count -1", "weight 0", "weight nan", "weight inf", "weight negative",
                                  "energy 0", "dt 0", "width -1"])
def test_refusals_leave_the_store_untouched(iface, make_problem, cs, case):
    n = 5000
    st = SourceStore(iface, make_problem, cs, n)
    killed = st.kill(st.arrays(), np.random.default_rng(6).random(n) < 0.3)
    kw = {"count -1": dict(count=-1), "weight 0": dict(weight=0.0), "weight nan": dict(weight=float("nan")),
          "weight inf": dict(weight=float("inf")), "weight negative": dict(weight=-0.5),
          "energy 0": dict(energy=0.0), "dt 0": dict(dt=0.0), "width -1": dict(width=-1.0)}[case]
    rc, stats = st.raw(**{"count": 10, "seed": SEED, **kw})
    assert rc == 1 and stats.emitted == 0
    after = st.arrays()
    for f in sr.FIELDS:
        assert same_bits(after[f], killed[f]), f
    if "weight" in case or case == "energy 0":  # ... and through the wrapper
        with pytest.raises(iface.SourceRefused) as refused:
            st.sim.emit(10, seed=SEED, weight=kw.get("weight", 1.0), energy=kw.get("energy"))
        assert refused.value.code == 1
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_nobody_dead_on_a_tiled_store_changes_nothing(iface, make_problem, cs, lazy, monkeypatch):
    """emitted == 0 returns 0, writes nothing and leaves the records of a tiled store valid: the next
    step pays no re-import.  The step's stats show one: after an import the plan of stream passes
    starts over, so a deck whose histories migrate through several windows (the stream deck with
    small windows, as tests/test_tiled_pipeline.py uses it) waits for the device more than once and
    enqueues other batches of passes.  A steady step waits once.  The last step of the run, after an
    invalidation, shows that these figures do see an import here."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")

    def call(sim):
        stats = sim.emit(100)
        assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (0, 0, 0.0)

    census_ops_support.check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call)


# ---- GPU: the driver's --source --------------------------------------------------------------

_FACETS = r"^Facets\s+(\d+)"  # (the driver's line of every step)


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_source_on_one_rank_and_on_two(tmp_path, iface, make_problem, cs):
    """`neutral.hip --roulette 0.25,0.5 --source 500,0.5`: from the step at which roulette has ended
    more than 500 histories on, every emit refills 500 slots; two ranks (both on one GPU) emit 250
    each into their shards, the same total.  Without the flag stdout says nothing of a source, and
    the later steps follow fewer histories."""
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
    assert "Source" not in plain
    killed = int(re.search(r"^Roulette killed (\d+)$", plain, flags=re.M).group(1))
    assert killed > 5000, "the case no longer ends histories"
    emitted, weight, facets = _source_totals(run_driver(str(run), rel, sets + ["--source", "500,0.5"]), _FACETS)
    print(f"emitted {emitted} weight {weight}")
    assert 500 <= emitted <= 5 * 500 and emitted % 500 == 0  # (before steps 2 .. 6; none dead at first)
    assert weight == emitted * 0.5
    plain_facets = [int(x) for x in re.findall(r"^Facets\s+(\d+)", plain, flags=re.M)]
    assert facets[0] == plain_facets[0] and facets[-1] > plain_facets[-1]
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    emitted2, weight2, _ = _source_totals(
        run_driver(str(run), rel, sets + ["--gpus", "2", "--source", "500,0.5"], env), _FACETS)
    assert (emitted2, weight2) == (emitted, weight)
    # ... and exactly what the ranks' shares (comms_shard_range of 500: 250 and 250) can emit into
    # their shards (50001 and 50000 slots).  Until the first call that finds a dead slot the
    # histories are the one-rank run's, whose dead slots per shard a Simulation tells: before that
    # call, every earlier call emitted nothing; from it on a shard whose dead slots cover its share
    # times the calls that remain serves every one of them in full, since a call takes its share
    # out of them at the most and the steps between only add to them.
    prob = make_problem("csp", nx=64, nparticles=100001, iterations=6, dt=2.0e-6)
    sim = iface.Simulation(prob, *cs, roulette=ON)
    sim.inject()
    shards, shares = ((0, 50001), (50001, 50000)), (250, 250)
    expected = None
    for tt in range(1, 6):  # (the call before step tt + 1 sees what step tt left)
        sim.step(tt)
        dead = sim.particle_arrays()["dead"] != 0
        by_shard = [int(dead[lo:lo + n].sum()) for lo, n in shards]
        if sum(by_shard) > 0:
            calls = 6 - tt
            print(f"dead by shard after step {tt}: {by_shard}; {calls} calls remain")
            assert all(d >= s * calls for d, s in zip(by_shard, shares)), "the case no longer saturates every call"
            expected = sum(shares) * calls
            break
    sim.close()
    assert emitted2 == expected and weight2 == expected * 0.5


# ---- GPU: the source in a run, against the oracle --------------------------------------------

ON = (0.25, 0.5)


@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_source_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """Steps, emit, steps, emit, steps: the library (records written back before the refill, imported
    again after it, graveyard slots among the refilled) against the oracle, whose arrays receive the
    library's refilled slots."""
    import oracle_binding as ob
    keys, values = cs
    absorb = (np.array(keys), 0.5 * np.array(values))  # capture = scatter / 2: p_absorb = 1/3
    prob = make_problem("csp", nx=24, nparticles=6000, iterations=11, dt=2.0e-6)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=ON, cs_absorb=absorb)
    ref = ob.OracleRun(prob, keys, values, cs_absorb=absorb, roulette=ON)
    sim.inject()
    ref.inject()
    args = sr.args_of(prob)

    def both_step(tt):
        g, c = sim.step(tt), ref.step(tt)
        assert (g.nprocessed, g.facets, g.collisions, g.census) == \
            (c.nprocessed, c.facets, c.collisions, c.census), tt
        assert (g.stats.roulette_killed, g.stats.roulette_survived) == \
            (c.roulette_killed, c.roulette_survived), tt
        return c

    def emit(count, tt):
        """emit into the library's store, check the refilled slots, hand them to the oracle"""
        arrays = ref.particles.as_dict()
        slots = sr.ranks(arrays["dead"], count)
        live = int((arrays["dead"] == 0).sum())
        stats = sim.emit(count)  # (seed: 2^63 + the last master key)
        assert (stats.dead_before, stats.emitted) == (prob.nparticles - live, len(slots))
        got = sim.particle_arrays()
        _check_refilled(iface, got, slots, 0, 2 ** 63 + tt, 1.0, args)
        untouched = np.ones(prob.nparticles, dtype=bool)
        untouched[slots] = False
        assert np.array_equal(got["dead"][untouched], arrays["dead"][untouched])
        for f in sr.FIELDS:
            arrays[f][slots] = got[f][slots]
        return slots, live, stats

    killed = sum(both_step(tt).roulette_killed for tt in range(1, 4))
    assert killed > 0  # histories have died ...
    for tt in (4, 5):  # ... and the tiled variant has moved them into its graveyard
        both_step(tt)
    ndead = int(ref.particles.as_dict()["dead"].astype(bool).sum())
    first, live, stats = emit(ndead // 2, 5)
    assert 0 < stats.emitted < ndead
    assert both_step(6).nprocessed == live + stats.emitted
    for tt in (7, 8):
        both_step(tt)
    ndead = int(ref.particles.as_dict()["dead"].astype(bool).sum())
    second, live, stats = emit(ndead, 8)
    assert len(np.intersect1d(first, second)) > 0  # refilled once, dead again, refilled again
    assert both_step(9).nprocessed == live + stats.emitted == prob.nparticles
    for tt in (10, 11):
        both_step(tt)
    got, want = sim.particle_arrays(), ref.particles.as_dict()
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got[f], want[f]), f
    tg, tc = sim.tally_host(), ref.tally
    print(f"variant {variant} lazy {lazy}: tally rel L2 {np.linalg.norm(tg - tc) / np.linalg.norm(tc):.3e} "
          f"worst cell {np.max(np.abs(tg - tc) / np.maximum(np.abs(tc), 1e-300)):.3e}")
    assert np.linalg.norm(tg - tc) / np.linalg.norm(tc) < TALLY_L2_TOL
    assert np.all(np.abs(tg - tc) <= TALLY_L2_TOL * np.abs(tc))
    sim.close()


@gpu
@needs_gpu
def test_weight_balance_and_a_source_every_step(iface, make_problem, cs):
    keys, values = cs
    absorb = (np.array(keys), 0.5 * np.array(values))
    n = 6000
    prob = make_problem("csp", nx=24, nparticles=n, iterations=13, dt=2.0e-6)
    sim = iface.Simulation(prob, keys, values, variant=2, roulette=ON, cs_absorb=absorb)
    sim.inject()

    def live_and_weight():
        a = sim.particle_arrays()
        alive = a["dead"] == 0
        return int(alive.sum()), float(a["weight"][alive].sum())

    counts = [live_and_weight()[0]]
    for tt in (1, 2, 3):
        sim.step(tt)
        counts.append(live_and_weight()[0])
    assert counts[-1] < counts[0] and all(b <= a for a, b in zip(counts, counts[1:]))  # it only decays
    for tt in range(4, 14):
        live, weight = live_and_weight()
        stats = sim.emit(150, weight=0.75)
        live_after, weight_after = live_and_weight()
        assert stats.weight_emitted == stats.emitted * 0.75
        assert abs(weight_after - (weight + stats.weight_emitted)) <= 1e-12 * weight_after
        assert live_after == live + stats.emitted <= n
        if tt == 4:
            assert stats.emitted == 150 and live_after > live  # it rises where it fell before
        sim.step(tt)
        assert live_and_weight()[0] <= n
    sim.close()

"""Comb, source, window and census on the shards of 2 and 3 ranks, against the CPU oracle.

The reference is ONE oracle run over all the particles.  After a scheduled step the numpy
restatements (tests/comb_reference.py, source_reference.py, window_reference.py,
census_reference.py) are applied to each rank's slice [first, first + count) of the oracle's arrays
with pid_base = first, which is what the library does on several ranks (neutral_abi_store.hip:
resolve_shard); the census is taken over the whole store, which is what its all-reduce makes of
the shards'.  The ranks (tests/gpu_ranks_worker.py with a schedule, all on one GPU, exchanging
through the host) keep their arrays and what every operation returned; each is compared with the
reference slice by slice, every slot of every rank.

CPU: every scenario on the oracle alone -- no slot inside a restatement's guard band, every branch
taken on every slice, the source both saturating a shard and not.

The scenario is that of tests/test_window.py with 6001 particles, which divide by neither rank
count: two ranks hold 3001 and 3000 slots (two scan tiles each, the last one ragged), three hold
2001, 2000 and 2000 (one tile each).  The comb and the second window name 1000 particles in their
calls, not the shard's count: for a sharded store the library takes the shard's own, whatever count
the caller names (include/neutral_hip.h), and a library that took the caller's would stop short.

Margins, taken from the one-rank run tests: live weights 1e-9 absolute (test_window.py), the
tally 1e-9 relative, L2 and per cell (TALLY_L2_TOL), refilled positions 1e-15 relative and
directions 1e-15 absolute (test_source.py), a census cell's weight 1e-9 * count + (count + 1) *
2^-53 * weight (test_census.py).  One margin is derived, not taken over: the comb's run test has no
bar for weight_each, which is the mean over the shard's slots of live weights that are each within
1e-9 of the oracle's, hence within 1e-9 itself.
"""
import collections

import numpy as np
import pytest

import census_reference as cen
import comb_reference as cr
import source_reference as sr
import window_reference as wr
from gpu_support import gpu, needs_gpu
from ranks import launch_gpu_ranks
from test_census import EPS
from test_window import ON, RUN, RUN_RATIOS, RUN_STEPS, TALLY_L2_TOL, _oracle_run, run_meshes, same_bits

N = 6001
NX = RUN["nx"]
WEIGHT_TOL = 1e-9  # absolute, of a live weight: tests/test_window.py::test_window_in_a_run_against_the_oracle
SOURCE_SEED_BASE = 2 ** 63  # include/neutral_hip.h; neutral_amd.interface.SOURCE_SEED_BASE
COMB_HALF = 3  # tests/test_comb.py: steps before the comb, and after it
# The auto window's target: more histories than are alive after three steps (5385), so that the
# bounds come out low, the splits ask for more copies than roulette and the dead leave slots, and
# every shard refuses copies -- and few enough that the crowded cells' bounds still lie over 1 and
# their histories play roulette (at 4000, tests/test_census.py's target, no copy is refused; from
# 10000 on nobody plays).  Chosen on the oracle alone; the CPU test below asserts all of it.
AUTO_TARGET = 6000.0
NAMED = 1000  # a count some calls name instead of the shard's: the library takes the shard's own


def shard_ranges(total, nranks):
    """comms_shard_range (host/comms_ranks.c): contiguous, the first total % nranks one longer"""
    per, rem = divmod(total, nranks)
    return [(r * per + min(r, rem), per + (1 if r < rem else 0)) for r in range(nranks)]


# ---- the reference: one oracle run, the restatements on its slices -----------------------------

Op = collections.namedtuple("Op", "after entry before results")  # before, results: one per rank (census: one)


class Reference:
    def __init__(self, make_problem, cs, nranks, steps):
        self.prob, self.keys, self.values, self.absorb, self.ref = _oracle_run(
            lambda name, **kw: make_problem(name, **dict(kw, nparticles=N, iterations=steps)), cs)
        assert self.prob.nparticles == N
        self.shards = shard_ranges(N, nranks)
        self.arrays = self.ref.particles.as_dict()
        self.steps, self.tallies, self.ops, self.tt = [], [], [], 0

    def step(self):
        self.tt += 1
        c = self.ref.step(self.tt)
        self.steps.append(c)
        self.tallies.append(self.ref.tally.copy())
        return c

    def slices(self):
        """copies of the ranks' slices of the oracle's arrays"""
        return [{f: self.arrays[f][lo:lo + n].copy() for f in wr.FIELDS} for lo, n in self.shards]

    def _put(self, rank, new):
        lo, n = self.shards[rank]
        for f in wr.FIELDS:
            self.arrays[f][lo:lo + n] = new[f]

    def _window_slices(self, before, lower):
        results = []
        for rank, ((lo, _), a) in enumerate(zip(self.shards, before)):
            r = wr.window(a, lower, NX, NX, RUN_RATIOS["upper_ratio"], RUN_RATIOS["survival_ratio"],
                          RUN_RATIOS["max_split"], wr.cpu_rn0(lo, wr.WINDOW_SEED_BASE + self.tt))
            assert r is not None
            self._put(rank, r.arrays)
            results.append(r)
        return results

    def window(self, lower, **more):
        before = self.slices()
        entry = dict(op="window", lower=np.array(lower), **RUN_RATIOS, **more)
        self.ops.append(Op(self.tt, entry, before, self._window_slices(before, lower)))

    def comb(self, seed, **more):
        before, results = self.slices(), []
        for rank, ((lo, _), a) in enumerate(zip(self.shards, before)):
            c = cr.comb(a["weight"], a["dead"], lo, seed)
            self._put(rank, c.apply(a))
            results.append(c)
        self.ops.append(Op(self.tt, dict(op="comb", seed=seed, **more), before, results))

    def emit(self, count, weight, **more):
        before, results = self.slices(), []
        args = sr.args_of(self.prob)
        for rank, ((lo, _), a) in enumerate(zip(self.shards, before)):
            share = shard_ranges(count, len(self.shards))[rank][1]
            new = sr.expected(a, a["dead"], share, weight, SOURCE_SEED_BASE + self.tt, lo, args)
            self._put(rank, new)
            results.append((share, sr.ranks(a["dead"], share), new))
        self.ops.append(Op(self.tt, dict(op="emit", count=count, weight=weight, **more), before, results))

    def census(self):
        c = cen.census(self.arrays, NX, NX)
        assert c is not None
        self.ops.append(Op(self.tt, dict(op="census"), self.slices(), c))
        return c

    def auto_window(self, target, lower=None):
        """lower: the bounds to window with (the ranks' own); None: the restatement's, from the
        oracle's census"""
        before = self.slices()
        c = cen.census(self.arrays, NX, NX)
        b = cen.bounds(c.count, c.weight, target, RUN_RATIOS["upper_ratio"], 0.0, 1)
        assert b is not None
        results = self._window_slices(before, b.lower if lower is None else lower)
        self.ops.append(Op(self.tt, dict(op="auto_window", target=target, **RUN_RATIOS), before, (c, b, results)))

    def keep(self):
        """the worker's operation that does nothing: the ranks keep their arrays as they stand, here
        just before an emit"""
        self.ops.append(Op(self.tt, dict(op="keep"), self.slices(), None))

    def schedule(self, folder):
        """the operations as tests/gpu_ranks_worker.py reads them, meshes in files under `folder`"""
        out = []
        for k, op in enumerate(self.ops):
            entry = dict(op.entry, after=op.after)
            if "lower" in entry:
                path = folder / f"lower{k}.npy"
                np.save(path, entry["lower"].reshape(NX, NX))
                entry["lower"] = str(path)
            out.append(entry)
        return out


def window_scenario(make_problem, cs, nranks):
    """tests/test_window.py's: steps 1-3, window, steps 4-6, window, steps 7-9; the second window's
    call names a count that is not the shard's"""
    ref = Reference(make_problem, cs, nranks, RUN["iterations"])
    for steps, lower, more in zip(RUN_STEPS, run_meshes() + (None,), ({}, dict(named_count=NAMED), {})):
        for _ in steps:
            ref.step()
        if lower is not None:
            ref.window(lower, **more)
    return ref


def source_count(dead_counts):
    """a count whose shares (equal: it is a multiple of the rank count) lie over the fewest dead
    slots of a shard and not over the most"""
    low, high = min(dead_counts), max(dead_counts)
    assert low < high, dead_counts
    return len(dead_counts) * ((low + high + 1) // 2)


def source_scenario(make_problem, cs, nranks):
    """tests/test_source.py's: steps 1-5, emit, steps 6-8, emit, steps 9-11; the arrays are kept
    before each emit"""
    ref = Reference(make_problem, cs, nranks, 11)
    for steps, weight in (((1, 2, 3, 4, 5), 1.0), ((6, 7, 8), 0.5), ((9, 10, 11), None)):
        for _ in steps:
            ref.step()
        if weight is not None:
            ref.keep()
            ref.emit(source_count([int((a["dead"] != 0).sum()) for a in ref.slices()]), weight)
    return ref


def comb_scenario(make_problem, cs, nranks):
    """tests/test_comb.py's: steps 1-3, comb(seed 3), steps 4-6; the call names a count that is not
    the shard's"""
    ref = Reference(make_problem, cs, nranks, 2 * COMB_HALF)
    for _ in range(COMB_HALF):
        ref.step()
    ref.comb(COMB_HALF, named_count=NAMED)
    for _ in range(COMB_HALF):
        ref.step()
    return ref


def census_scenario(make_problem, cs, nranks, lower=None):
    """steps 1-3, census, auto window, steps 4-6, census"""
    ref = Reference(make_problem, cs, nranks, 6)
    for _ in RUN_STEPS[0]:
        ref.step()
    ref.census()
    ref.auto_window(AUTO_TARGET, lower)
    for _ in RUN_STEPS[1]:
        ref.step()
    ref.census()
    return ref


# ---- CPU: the scenarios on the oracle alone ----------------------------------------------------

@pytest.mark.parametrize("nranks", [2, 3])
def test_the_scenarios_on_the_oracle_take_every_branch_unguarded_on_every_slice(make_problem, cs, nranks):
    assert [n for _, n in shard_ranges(N, 2)] == [3001, 3000] and [n for _, n in shard_ranges(N, 3)] == [2001, 2000, 2000]
    assert shard_ranges(N, nranks)[0][0] == 0 and all(
        a[0] + a[1] == b[0] for a, b in zip(shard_ranges(N, nranks), shard_ranges(N, nranks)[1:]))
    # the windows: split, roulette killed and survived on every slice; a refused copy somewhere
    ref = window_scenario(make_problem, cs, nranks)
    assert len(ref.ops) == 2
    for op in ref.ops:
        for rank, r in enumerate(op.results):
            print(nranks, "window after", op.after, "rank", rank, r.stats)
            assert not r.guarded.any(), (rank, np.flatnonzero(r.guarded))
            assert r.stats["split"] > 0 and r.stats["roulette_killed"] > 0 and r.stats["roulette_survived"] > 0, rank
            assert r.stats["copies_made"] > 0, rank
        assert any(r.stats["copies_refused"] > 0 for r in op.results)
    # the auto window: split and roulette (either outcome) on every slice; a refused copy somewhere
    ref = census_scenario(make_problem, cs, nranks)
    c, b, results = ref.ops[1].results
    print(nranks, "census", c.stats, "bounds", b.stats)
    for rank, r in enumerate(results):
        print(nranks, "auto window rank", rank, r.stats)
        assert not r.guarded.any(), (rank, np.flatnonzero(r.guarded))
        assert r.stats["split"] > 0 and r.stats["roulette_killed"] + r.stats["roulette_survived"] > 0, rank
        assert r.stats["copies_made"] > 0, rank
    assert any(r.stats["copies_refused"] > 0 for r in results)
    assert AUTO_TARGET > c.stats["live"]
    assert ref.ops[2].results.stats["live"] != c.stats["live"]  # (the second census sees another store)
    # the comb: no tooth guarded; slots to refill on every slice
    ref = comb_scenario(make_problem, cs, nranks)
    for rank, c in enumerate(ref.ops[0].results):
        print(nranks, "comb rank", rank, c.live_before, c.sources_kept, c.max_copies)
        assert not c.guarded.any(), rank
        assert c.live_before < ref.shards[rank][1] and c.max_copies > 1, rank
    assert min(n for _, n in ref.shards) > NAMED
    # the source: each emit saturates a shard and leaves another unsaturated
    ref = source_scenario(make_problem, cs, nranks)
    emits = [op for op in ref.ops if op.entry["op"] == "emit"]
    assert len(emits) == 2
    for op in emits:
        dead = [int((a["dead"] != 0).sum()) for a in op.before]
        shares = [share for share, _, _ in op.results]
        print(nranks, "emit after", op.after, "count", op.entry["count"], "shares", shares, "dead", dead)
        assert sum(shares) == op.entry["count"]
        assert any(s > d for s, d in zip(shares, dead)) and any(0 < s <= d for s, d in zip(shares, dead))
    first, second = (np.concatenate([lo + slots for (lo, _), (_, slots, _) in zip(ref.shards, op.results)]) for op in emits)
    assert len(np.intersect1d(first, second)) > 0  # refilled once, dead again, refilled again


# ---- GPU: the ranks ----------------------------------------------------------------------------

def run_ranks(ref, tmp_path, nranks, schedule=None):
    """the reference's scenario on nranks ranks -> per rank (its file, what its operations said)"""
    import json
    out = tmp_path / "ranks"
    out.mkdir()
    files, logs = launch_gpu_ranks(ref.prob.deck, out, ref.tt, "shard", nranks, roulette=ON, capture_scale=0.5,
                                   schedule=ref.schedule(out) if schedule is None else schedule)
    for rank, (z, (lo, n)) in enumerate(zip(files, ref.shards)):
        assert (int(z["ids"][0]), len(z["ids"])) == (lo, n), rank
    return files, [json.loads(str(z["ops"])) for z in files], logs


def check_steps(ref, files, logs, name):
    """every step on every rank: the event counts over the ranks are the oracle's, roulette's too,
    and the all-reduced tally is the oracle's, overall and cell by cell"""
    want = [(c.nprocessed, c.facets, c.collisions, c.census) for c in ref.steps]
    worst = 0.0
    for rank, (z, log) in enumerate(zip(files, logs)):
        assert [tuple(int(v) for v in e) for e in z["events"]] == want, rank
        assert log["killed"] == [c.roulette_killed for c in ref.steps], rank
        assert log["survived"] == [c.roulette_survived for c in ref.steps], rank
        for tt, (tg, tc) in enumerate(zip(z["tallies"], ref.tallies), start=1):
            l2 = np.linalg.norm(tg - tc) / np.linalg.norm(tc)
            worst = max(worst, l2)
            assert l2 < TALLY_L2_TOL, (rank, tt, l2)
            assert np.all(np.abs(tg - tc) <= TALLY_L2_TOL * np.abs(tc)), (rank, tt)
        assert same_bits(z["tallies"][-1], z["tally"])
    print(f"{name}: worst tally rel L2 over the ranks and steps {worst:.3e}")


def check_window(said, z, k, r, rank):
    """operation k of a rank against the window's restatement r of its slice"""
    assert said["code"] == 0, (rank, said)
    assert {name: said["stats"][name] for name in wr.STAT_NAMES} == r.stats, rank
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(z[f"op{k}_{f}"], r.arrays[f]), (rank, f)
    live = r.arrays["dead"] == 0
    assert np.max(np.abs(z[f"op{k}_weight"] - r.arrays["weight"])[live]) <= WEIGHT_TOL, rank


def check_final_state(ref, files):
    for z, (lo, n) in zip(files, ref.shards):
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(z[f], ref.arrays[f][lo:lo + n]), f


@gpu
@needs_gpu
@pytest.mark.parametrize("nranks", [2, 3])
def test_window_on_shards_against_the_oracle(make_problem, cs, tmp_path, nranks):
    ref = window_scenario(make_problem, cs, nranks)
    files, ops, logs = run_ranks(ref, tmp_path, nranks)
    for k, op in enumerate(ref.ops):
        for rank, (z, said, r) in enumerate(zip(files, ops, op.results)):
            assert not r.guarded.any()
            assert (said[k]["op"], said[k]["after"]) == ("window", op.after)
            check_window(said[k], z, k, r, rank)
    check_steps(ref, files, logs, f"window on {nranks} ranks")
    check_final_state(ref, files)


@gpu
@needs_gpu
@pytest.mark.parametrize("nranks", [2, 3])
def test_source_on_shards_against_the_oracle(make_problem, cs, tmp_path, nranks):
    ref = source_scenario(make_problem, cs, nranks)
    files, ops, logs = run_ranks(ref, tmp_path, nranks)
    args = sr.args_of(ref.prob)
    for k, op in enumerate(ref.ops):
        if op.entry["op"] != "emit":
            continue
        for rank, (z, said, a, (share, slots, want)) in enumerate(zip(files, ops, op.before, op.results)):
            ndead = int((a["dead"] != 0).sum())
            stats = said[k]["stats"]
            assert (said[k]["code"], said[k]["share"]) == (0, share), rank
            assert len(slots) == min(share, ndead)
            assert (stats["dead_before"], stats["emitted"]) == (ndead, len(slots)), rank
            assert stats["weight_emitted"] == len(slots) * op.entry["weight"], rank
            got = {f: z[f"op{k}_{f}"] for f in sr.FIELDS}
            kept = {f: z[f"op{k - 1}_{f}"] for f in sr.FIELDS}  # (the arrays just before the emit)
            # exactly the first `share` dead slots of the shard ...
            assert np.array_equal(got["dead"], want["dead"]), rank
            assert np.array_equal(np.flatnonzero((kept["dead"] != 0) & (got["dead"] == 0)), slots), rank
            # ... carrying the particles of the streams pid_base + slot (the tolerances of
            # tests/test_source.py::_check_refilled) ...
            for f in ("dead", "energy", "weight", "dt_to_census", "mfp_to_collision"):
                assert np.array_equal(got[f][slots], want[f][slots]), (rank, f)
            for f in ("x", "y"):
                assert np.max(np.abs(got[f][slots] - want[f][slots]) / np.abs(want[f][slots])) < 1e-15, (rank, f)
            for f in ("omega_x", "omega_y"):
                assert np.max(np.abs(got[f][slots] - want[f][slots])) < 1e-15, (rank, f)
            assert np.array_equal(got["cellx"][slots], args.x_off + sr.find_cell(args.edgex, got["x"][slots])), rank
            assert np.array_equal(got["celly"][slots], args.y_off + sr.find_cell(args.edgey, got["y"][slots])), rank
            assert np.array_equal(got["cellx"][slots], want["cellx"][slots]), rank
            assert np.array_equal(got["celly"][slots], want["celly"][slots]), rank
            # ... and every other slot byte for byte what it was
            untouched = np.ones(len(got["dead"]), dtype=bool)
            untouched[slots] = False
            for f in sr.FIELDS:
                assert same_bits(np.ascontiguousarray(got[f][untouched]), np.ascontiguousarray(kept[f][untouched])), (rank, f)
    check_steps(ref, files, logs, f"source on {nranks} ranks")  # (the next step's nprocessed among them)
    check_final_state(ref, files)


@gpu
@needs_gpu
@pytest.mark.parametrize("nranks", [2, 3])
def test_comb_on_shards_against_the_oracle(make_problem, cs, tmp_path, nranks):
    ref = comb_scenario(make_problem, cs, nranks)
    files, ops, logs = run_ranks(ref, tmp_path, nranks)
    op = ref.ops[0]
    for rank, (z, said, a, c) in enumerate(zip(files, ops, op.before, op.results)):
        assert not c.guarded.any()
        stats = said[0]["stats"]
        assert said[0]["code"] == 0, (rank, said[0])
        assert (stats["live_before"], stats["sources_kept"], stats["max_copies"]) == \
            (c.live_before, c.sources_kept, c.max_copies), rank
        want = c.apply(a)
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(z[f"op0_{f}"], want[f]), (rank, f)
        print(f"comb on {nranks} ranks, rank {rank}: weight_each {stats['weight_each']!r} ({c.delta!r})")
        assert abs(stats["weight_each"] - c.delta) <= WEIGHT_TOL, rank
        assert np.all(z["op0_weight"] == stats["weight_each"]), rank
    check_steps(ref, files, logs, f"comb on {nranks} ranks")
    check_final_state(ref, files)


def check_census(said, z, k, c, a, rank):
    """operation k of a rank, a census, against the restatement c of the WHOLE store; a: the rank's slice"""
    stats = said["stats"]
    assert said["code"] == 0, (rank, said)
    assert same_bits(z[f"op{k}_census_count"], c.count), rank
    weight = z[f"op{k}_census_weight"]
    assert np.all(np.abs(weight - c.weight) <= WEIGHT_TOL * c.count + (c.count + 1.0) * EPS * c.weight), rank
    # this rank's own (include/neutral_hip.h; the driver sums live over the ranks itself) ...
    assert (stats["live"], stats["dead"]) == (int((a["dead"] == 0).sum()), int((a["dead"] != 0).sum())), rank
    # ... and the global ones
    assert (stats["occupied_cells"], stats["max_count"]) == (c.stats["occupied_cells"], c.stats["max_count"]), rank
    assert stats["max_cell_weight"] == weight.max(), rank
    live = c.stats["live"]
    assert abs(stats["weight"] - c.stats["weight"]) <= WEIGHT_TOL * live + (live + 1.0) * EPS * c.stats["weight"], rank


@gpu
@needs_gpu
@pytest.mark.parametrize("nranks", [2, 3])
def test_census_and_auto_window_on_shards(make_problem, cs, tmp_path, nranks):
    first = census_scenario(make_problem, cs, nranks)
    files, ops, logs = run_ranks(first, tmp_path, nranks)
    # one census, one mesh of bounds: the same bits on every rank
    for name in ("op0_census_count", "op0_census_weight", "op1_census_count", "op1_census_weight", "op1_lower",
                 "op2_census_count", "op2_census_weight"):
        for z in files[1:]:
            assert same_bits(z[name], files[0][name]), name
    lower = files[0]["op1_lower"]
    b = cen.bounds(files[0]["op1_census_count"], files[0]["op1_census_weight"], AUTO_TARGET, RUN_RATIOS["upper_ratio"], 0.0, 1)
    assert same_bits(lower, b.lower)
    # the oracle's run again, windowed with the bounds the ranks made
    ref = census_scenario(make_problem, cs, nranks, lower=lower)
    c, _, results = ref.ops[1].results
    for rank, (z, said) in enumerate(zip(files, ops)):
        assert [s["op"] for s in said] == ["census", "auto_window", "census"]
        check_census(said[0], z, 0, c, ref.ops[0].before[rank], rank)
        auto = said[1]
        assert auto["code"] == 0, (rank, auto)
        check_census(dict(code=0, stats=auto["census"]), z, 1, c, ref.ops[1].before[rank], rank)
        assert same_bits(z["op1_census_count"], z["op0_census_count"]) and same_bits(z["op1_census_weight"], z["op0_census_weight"])
        assert auto["bounds"]["windowed_cells"] == b.stats["windowed_cells"] == c.stats["occupied_cells"], rank
        assert (auto["bounds"]["max_cell_weight"], auto["bounds"]["lower_at_peak"]) == \
            (b.stats["max_cell_weight"], b.stats["lower_at_peak"]), rank
        assert not results[rank].guarded.any()
        assert results[rank].stats["split"] > 0 and results[rank].stats["copies_made"] > 0
        check_window(auto, z, 1, results[rank], rank)
        check_census(said[2], z, 2, ref.ops[2].results, ref.ops[2].before[rank], rank)
    assert any(r.stats["copies_refused"] > 0 for r in results)  # (a shard ran out of free slots)
    check_steps(ref, files, logs, f"census and auto window on {nranks} ranks")
    check_final_state(ref, files)


@gpu
@needs_gpu
def test_a_census_refusal_on_one_rank_is_every_ranks(make_problem, cs, tmp_path):
    """Rank 1 gives one live slot a NaN weight: the census, collective, returns 1 on both ranks with
    a buffer of zeros, the auto window after it (its census) likewise, no store is written to, and
    both ranks leave through the barrier (launch_ranks waits for every rank's exit code 0).  No step
    runs on the poisoned store."""
    ref = Reference(make_problem, cs, 2, 3)
    for _ in range(3):
        ref.step()
    slices = ref.slices()
    slot = int(np.flatnonzero(slices[1]["dead"] == 0)[-1])  # (the last live slot: in the ragged second tile)
    assert slot > 2048
    schedule = [dict(after=3, op="poke", rank=1, field="weight", slot=slot, value=float("nan")),
                dict(after=3, op="census"),
                dict(after=3, op="auto_window", target=AUTO_TARGET, **RUN_RATIOS)]
    files, ops, logs = run_ranks(ref, tmp_path, 2, schedule)
    for rank, (z, said, a) in enumerate(zip(files, ops, slices)):
        poke, census, auto = said
        assert (poke["code"], census["code"], auto["code"]) == (0, 1, 1), (rank, said)
        assert (census["refused"], auto["refused"]) == ("CensusRefused", "CensusRefused"), rank
        assert not z["op1_census_count"].any() and not z["op1_census_weight"].any(), rank  # (it held -1 everywhere)
        for s in (census["stats"], auto["stats"]):
            assert (s["live"], s["dead"]) == (int((a["dead"] == 0).sum()), int((a["dead"] != 0).sum())), rank
            assert (s["occupied_cells"], s["max_count"], s["weight"], s["max_cell_weight"]) == (0, 0, 0.0, 0.0), rank
        assert np.isnan(z["op0_weight"][slot]) == (rank == 1)
        assert np.array_equal(z["op0_dead"], a["dead"]), rank
        for f in wr.FIELDS:
            assert same_bits(z[f"op1_{f}"], z[f"op0_{f}"]) and same_bits(z[f"op2_{f}"], z[f"op0_{f}"]), (rank, f)
            assert same_bits(z[f], z[f"op0_{f}"]), (rank, f)
    check_steps(ref, files, logs, "refusal on 2 ranks")

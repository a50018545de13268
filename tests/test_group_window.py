"""Energy groups for the census tally and the weight window (include/neutral_hip.h:
neutral_hip_census_tally_groups, neutral_hip_window_particles_groups).

The definition is by equivalence: the plain calls on a virtual store in which a slot's row is
g * ny + celly.  tests/group_window_reference.py builds that store and calls the plain restatements
as they are.  CPU: the helper's edge cases and its degenerate case, the ABI, the wrappers' argument
handling, the driver's usage errors, and the in-run scenario on the oracle alone.  GPU: G = 1 with
all-embracing edges against the plain calls' bits, the grouped calls against the plain calls on the
uploaded virtual store, against the helper, refusals, the identity on a second call, auto_window,
nothing to do on a tiled store, the grouped window inside a run against the CPU oracle, and the
driver's --window-groups.

Two bounds used below, and where they come from.  The two roulette weight sums are f64 atomics in
an order the hardware chooses: tests/test_window.py holds each within n * 2^-53 * sum|w| of the
exact sum, so two calls on one input lie within twice that of each other.  A census bin's weight
lies within (m - 1) * 2^-53 * S of the exact sum S of its m terms (the header's first-order bound);
the helper's math.fsum is S rounded once, one 2^-53 * S more, and one more covers the second order:
(m + 1) * 2^-53 * S, the bound of tests/test_census.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import census_reference as cr
import group_window_reference as gr
import test_census as tc
import test_window as tw
import window_reference as wr
import census_ops_support
from census_ops_support import same_bits
from conftest import ROOT
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, scan_tile  # noqa: F401

EPS = 2.0 ** -53
SEED = tw.SEED
MESH = tw.MESH
EDGES3 = (5.0e2, 5.0e3, 5.0e4, 5.0e5)
EDGES64 = tuple(np.geomspace(1.0e-2, 1.0e8, 65).tolist())
INT_STATS = wr.STAT_NAMES


# ---- CPU: the helper ----------------------------------------------------------------------------

def test_group_of_an_energy_by_hand():
    """on an edge: the group above it; at edges[G], below edges[0], NaN, inf, -0.0, negative: outside"""
    e = EDGES3
    below, last = np.nextafter(e[0], 0.0), np.nextafter(e[3], 0.0)
    energy = np.array([e[0], e[1], e[2], e[3], below, last, 1.0e3, 4.9e5, np.nan, np.inf, -0.0, 0.0, -1.0e3,
                       -np.inf, np.nextafter(e[1], 0.0)])
    assert gr.groups_of(energy, e).tolist() == [0, 1, 2, 3, 3, 2, 0, 2, 3, 3, 3, 3, 3, 3, 0]
    assert gr.groups_of(np.array([5e-324, 1.0, np.finfo(float).max, 0.0, np.inf]), gr.ALL_EMBRACING).tolist() == \
        [0, 0, 1, 1, 1]
    assert gr.near_an_edge(np.array([5.0e3 * (1 + 5e-10), 5.0e3 * (1 + 5e-9), np.nan]), e).tolist() == [True, False, False]
    for bad in ((1.0,), (1.0, 1.0), (2.0, 1.0), (0.0, 1.0), (-1.0, 1.0), (1.0, np.inf), (1.0, np.nan),
                tuple(range(1, 67))):
        assert not gr.valid_edges(bad), bad
    assert gr.valid_edges(EDGES64) and gr.valid_edges(gr.ALL_EMBRACING)


def test_hand_computed_store_in_two_groups():
    """1 x 1 mesh, two groups [1, 10) and [10, 100), lower 0.5 and 2.0, upper_ratio 2, survival 1.5,
    max_split 3.  Slot 0 at E = 5, w = 2.5: over 1.0, q = 2.5, asks for two.  Slot 1 at E = 10 (on
    the edge: group 1), w = 2.5: inside [2, 4].  Slot 2 at E = 50, w = 1: under 2.0, plays for 3.0
    and loses (0.9 * 3 >= 1).  Slot 3 at E = 100 (edges[G]): outside, w = 1e9 left alone.  Slot 4
    dead.  Free: 2 (killed), 4: slot 0's copies."""
    a = {f: np.arange(5, dtype=np.float64) + 10.0 * (k + 1) for k, f in enumerate(wr.F64_FIELDS)}
    a["energy"] = np.array([5.0, 10.0, 50.0, 100.0, np.nan])
    a["weight"] = np.array([2.5, 2.5, 1.0, 1e9, np.nan])
    a["cellx"] = np.array([0, 0, 0, 0, -1], dtype=np.int32)
    a["celly"] = np.array([0, 0, 0, 0, -1], dtype=np.int32)
    a["dead"] = np.array([0, 0, 0, 0, 2], dtype=np.int32)
    r = gr.window(a, (1.0, 10.0, 100.0), [0.5, 2.0], 1, 1, 2.0, 1.5, 3, tw.fixed_rn0({2: 0.9}))
    assert r.stats == dict(live_before=4, dead_before=1, below=1, roulette_killed=1, roulette_survived=0,
                           above=1, split=1, copies_made=2, copies_refused=0)
    assert r.outside == 1 and r.guarded.tolist() == [False, True, False, True, False]  # (1 and 3: on an edge)
    assert r.sources.tolist() == [0, 0] and r.destinations.tolist() == [2, 4]
    w = 2.5 / 3.0
    assert r.arrays["weight"].tolist() == [w, 2.5, w, 1e9, w] and r.arrays["dead"].tolist() == [0] * 5
    assert r.arrays["celly"].tolist() == [0, 0, 0, 0, 0] and r.arrays["energy"].tolist() == [5.0, 10.0, 5.0, 100.0, 5.0]
    c = gr.census(a, (1.0, 10.0, 100.0), 1, 1)
    assert c.count.tolist() == [1.0, 2.0] and c.weight.tolist() == [2.5, 3.5]
    assert c.stats == dict(live=4, dead=1, outside=1, occupied_bins=2, max_count=2, weight=6.0, max_bin_weight=3.5)
    # a live slot off the mesh refuses both, inside a group or not; so does a bad weight outside
    for j, f, v in ((0, "celly", 1), (3, "celly", -1), (3, "cellx", 1), (3, "weight", np.nan), (3, "weight", -1.0)):
        b = {k: a[k].copy() for k in wr.FIELDS}
        b[f][j] = v
        assert gr.window(b, (1.0, 10.0, 100.0), [0.5, 2.0], 1, 1, 2.0, 1.5, 3, tw.fixed_rn0({2: 0.9})) is None, (j, f)
        assert gr.census(b, (1.0, 10.0, 100.0), 1, 1) is None, (j, f)
    # a bound that nobody live and inside looks up is not checked; one that is refuses
    r = gr.window(a, (1.0, 10.0, 100.0, 1000.0, 1.0e4), [0.5, 2.0, 0.0, np.nan], 1, 1, 2.0, 1.5, 3, tw.fixed_rn0({2: 0.9}))
    assert r.outside == 0 and r.stats["copies_made"] == 2 and r.arrays["weight"][3] == 1e9  # (slot 3: no window)
    assert gr.window(a, (1.0, 10.0, 100.0), [0.5, np.nan], 1, 1, 2.0, 1.5, 3, tw.fixed_rn0({2: 0.9})) is None


@pytest.mark.parametrize("n", [1, 65, 5000])
def test_one_all_embracing_group_is_the_plain_restatement(n):
    a, lower = tw.random_store(n, n)
    plain = wr.window(a, lower, MESH, MESH, 2.0, 1.5, 5, tw.numpy_rn0(n))
    grouped = gr.window(a, gr.ALL_EMBRACING, lower, MESH, MESH, 2.0, 1.5, 5, tw.numpy_rn0(n))
    assert grouped.outside == 0 and grouped.stats == plain.stats and (grouped.lost, grouped.gained) == (plain.lost, plain.gained)
    for f in wr.FIELDS:
        assert same_bits(grouped.arrays[f], plain.arrays[f]), f
    assert np.array_equal(grouped.guarded, plain.guarded)
    pc, gc = cr.census(a, MESH, MESH), gr.census(a, gr.ALL_EMBRACING, MESH, MESH)
    assert same_bits(gc.count, pc.count) and same_bits(gc.weight, pc.weight) and gc.stats["outside"] == 0
    assert (gc.stats["live"], gc.stats["dead"], gc.stats["occupied_bins"], gc.stats["max_count"], gc.stats["weight"],
            gc.stats["max_bin_weight"]) == tuple(pc.stats[k] for k in ("live", "dead", "occupied_cells", "max_count",
                                                                       "weight", "max_cell_weight"))


# ---- CPU: the ABI, the wrappers, the driver ------------------------------------------------------

def test_library_exports_the_grouped_calls(tmp_path):
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in ("neutral_hip_census_tally_groups", "neutral_hip_window_particles_groups"):
        assert hasattr(lib, name) and name in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    census_fields = [f[0] for f in iface.GroupCensusStats._fields_]
    assert census_fields == ["live", "dead", "outside", "occupied_bins", "max_count", "weight", "max_bin_weight",
                             "census_ms"]
    assert [f[0] for f in iface.GroupWindowStats._fields_] == ["window", "outside"]
    # the structs as a C compiler lays them out (the method of tests/test_mesh_source.py)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "neutral_hip.h"\n'
                   'int main(void) {\n  printf("%zu %zu\\n", sizeof(NeutralHipGroupCensusStats), '
                   'sizeof(NeutralHipGroupWindowStats));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(NeutralHipGroupCensusStats, {f}));\n' for f in census_fields) +
                   '  printf("window %zu\\n", offsetof(NeutralHipGroupWindowStats, window));\n'
                   '  printf("window.outside %zu\\n", offsetof(NeutralHipGroupWindowStats, outside));\n'
                   "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "layout")])
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(v) for v in lines[0].split()] == [C.sizeof(iface.GroupCensusStats), C.sizeof(iface.GroupWindowStats)] == [64, 104]
    offsets = dict(line.split() for line in lines[1:] if line.strip())
    for f in census_fields:
        assert getattr(iface.GroupCensusStats, f).offset == int(offsets[f]), f
    assert (iface.GroupWindowStats.window.offset, iface.GroupWindowStats.outside.offset) == \
        (int(offsets["window"]), int(offsets["window.outside"])) == (0, 96)
    text = open(os.path.join(ROOT, "include", "neutral_hip.h")).read()
    assert "VIRTUAL STORE" in text and "neutral_hip_window_bounds(nx, G * ny, census, ...)" in text


BAD_EDGES = {"one edge": (1.0,), "none": (), "66 edges": tuple(float(k) for k in range(1, 67)), "nan": (1.0, np.nan),
             "inf": (1.0, np.inf), "zero": (0.0, 1.0), "negative": (-2.0, 1.0), "equal": (1.0, 2.0, 2.0),
             "descending": (1.0, 3.0, 2.0), "two rows": ((1.0, 2.0), (3.0, 4.0)), "text": ("a", "b")}


def test_wrappers_refuse_bad_edges_and_shapes_before_the_library(monkeypatch):
    from neutral_amd import interface as iface

    def touched(*args):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(iface._lib, "neutral_hip_census_tally_groups", touched)
    monkeypatch.setattr(iface._lib, "neutral_hip_window_particles_groups", touched)
    store = C.pointer(iface.Particle())
    for name, edges in BAD_EDGES.items():
        with pytest.raises(ValueError) as refused:
            iface.group_edges(edges)
        assert not isinstance(refused.value, iface.Refused), name
        with pytest.raises(ValueError):
            iface.census_tally_groups(store, 16, 4, 4, edges)
        with pytest.raises(ValueError):
            iface.window_particles_groups(store, 16, 4, 4, edges, 1, 5.0, 3.0, 5, 0)
    assert iface.group_edges(EDGES64).size == 65 and iface.group_edges([1, 2]).dtype == np.float64
    good = (1.0, 10.0, 100.0)
    with pytest.raises(ValueError):
        iface.census_tally_groups(None, 16, 4, 4, good)  # no store
    with pytest.raises(ValueError):
        iface.window_particles_groups(None, 16, 4, 4, good, 1, 5.0, 3.0, 5, 0)
    for n, nx, ny in ((0, 4, 4), (-5, 4, 4), (2 ** 31, 4, 4), (16, 0, 4), (16, 4, -1), (16, 2 ** 15, 2 ** 14)):
        with pytest.raises(ValueError):
            iface.census_tally_groups(store, n, nx, ny, good)
        with pytest.raises(ValueError):
            iface.window_particles_groups(store, n, nx, ny, good, 1, 5.0, 3.0, 5, 0)
    for kw in (dict(n=16.5), dict(n=True), dict(nx=4.0), dict(max_split=2.5), dict(seed=0.5)):
        args = dict(dict(n=16, nx=4, max_split=5, seed=0), **kw)
        with pytest.raises(TypeError):
            iface.window_particles_groups(store, args["n"], args["nx"], 4, good, 1, 5.0, 3.0, args["max_split"], args["seed"])
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            iface.window_particles_groups(store, 16, 4, 4, good, 1, 5.0, 3.0, 5, seed)


def test_library_refuses_without_a_device():
    """refusals that need no device to say so (lower, device_out: any non-null address)"""
    from neutral_amd import interface as iface
    lib = iface.library()
    store = C.pointer(iface.Particle())
    mesh = np.ones(2 * 3 * 16)
    at = C.c_void_p(mesh.ctypes.data)

    def both(ngroups, edges, nx=4, ny=4, n=16, particles=store):
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        ws, cs_ = iface.GroupWindowStats(), iface.GroupCensusStats()
        rc = (lib.neutral_hip_window_particles_groups(particles, n, nx, ny, ngroups, e, at, 5.0, 3.0, 5, 0, C.byref(ws)),
              lib.neutral_hip_census_tally_groups(particles, n, nx, ny, ngroups, e, at, C.byref(cs_)))
        assert (ws.window.live_before, ws.outside, cs_.live, cs_.outside) == (0, 0, 0, 0)
        return rc
    good = (1.0, 10.0, 100.0, 1000.0)
    assert both(0, good) == both(65, tuple(range(1, 67))) == both(-1, good) == both(3, None) == (1, 1)
    for edges in ((1.0, np.nan, 100.0, 1000.0), (1.0, 10.0, 100.0, np.inf), (0.0, 10.0, 100.0, 1000.0),
                  (-1.0, 10.0, 100.0, 1000.0), (1.0, 10.0, 10.0, 1000.0), (1.0, 100.0, 10.0, 1000.0)):
        assert both(3, edges) == (1, 1), edges
    assert both(3, good, particles=None) == both(3, good, n=0) == both(3, good, nx=0) == both(3, good, ny=0) == (1, 1)
    assert both(3, good, nx=2 ** 15, ny=2 ** 14) == (1, 1)  # (nx * ny * G > 0x3fffffff; nx * ny alone is not)
    assert lib.neutral_hip_window_particles_groups(store, 16, 4, 4, 3, np.array(good).ctypes.data_as(C.POINTER(C.c_double)),
                                                   None, 5.0, 3.0, 5, 0, None) == 1
    assert lib.neutral_hip_window_particles_groups(store, 16, 4, 4, 3, np.array(good).ctypes.data_as(C.POINTER(C.c_double)),
                                                   at, 1.5, 1.0, 5, 0, None) == 1
    assert lib.neutral_hip_census_tally_groups(store, 16, 4, 4, 3, np.array(good).ctypes.data_as(C.POINTER(C.c_double)),
                                               None, None) == 1


USAGE = {"no value": ["--window", "0.3", "--window-groups"], "one edge": ["--window", "0.3", "--window-groups", "1.0"],
         "text": ["--window", "0.3", "--window-groups", "1,x"], "trailing comma": ["--window", "auto", "--window-groups", "1,2,"],
         "descending": ["--window", "0.3", "--window-groups", "2,1"], "equal": ["--window-groups", "1,1", "--window", "0.3"],
         "zero": ["--window", "0.3", "--window-groups", "0,1"], "negative": ["--window", "0.3", "--window-groups", "-1,1"],
         "inf": ["--window", "0.3", "--window-groups", "1,inf"], "nan": ["--window", "0.3", "--window-groups", "1,nan"],
         "66 edges": ["--window", "0.3", "--window-groups", ",".join(str(k) for k in range(1, 67))],
         "no --window": ["--window-groups", "1,2,3"],
         "decomposed": ["--window", "0.3", "--window-groups", "1,2,3", "--decompose", "1x1"]}


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("case", sorted(USAGE))
def test_driver_usage_errors(tmp_path, case):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + USAGE[case], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    said = out.stderr + out.stdout
    if case == "no --window":
        assert "--window-groups needs --window" in said
    elif case == "decomposed":
        assert "--window does not work with --decompose" in said
    else:
        assert "--window-groups wants E0,E1,...,EG with 1 to 64 groups" in said


# ---- the in-run scenario: the plain window's, with four energies and three groups ---------------

RUN_ENERGIES = (1.0e3, 1.0e4, 1.0e5, 1.0e6)  # slot j at RUN_ENERGIES[j % 4]; the last lies outside EDGES3
RUN_SCALES = ((1.0, 4.0, 0.0), (1.0, 0.5, 2.0))  # of the first and of the second mesh, group by group


def run_lowers():
    return [np.stack([scale * mesh for scale in scales]) for mesh, scales in zip(tw.run_meshes(), RUN_SCALES)]


def run_energies(n):
    return np.array(RUN_ENERGIES)[np.arange(n) % 4]


def apply_to_oracle(ref, lower, tt):
    """the helper on the oracle's arrays, in place; -> GroupResult"""
    arrays = ref.particles.as_dict()
    r = gr.window(arrays, EDGES3, lower, 24, 24, tw.RUN_RATIOS["upper_ratio"], tw.RUN_RATIOS["survival_ratio"],
                  tw.RUN_RATIOS["max_split"], wr.cpu_rn0(0, wr.WINDOW_SEED_BASE + tt))
    assert r is not None
    for f in wr.FIELDS:
        arrays[f][:] = r.arrays[f]
    return r


def _oracle_run(make_problem, cs):
    prob, keys, values, absorb, ref = tw._oracle_run(make_problem, cs)
    ref.particles.as_dict()["energy"][:] = run_energies(tw.RUN["nparticles"])
    return prob, keys, values, absorb, ref


def check_every_branch(results):
    for r in results:
        print(r.stats, "outside", r.outside)
        assert not r.guarded.any(), np.flatnonzero(r.guarded)
        assert r.stats["split"] > 0 and r.stats["roulette_killed"] > 0 and r.stats["roulette_survived"] > 0
        assert r.outside > 0
    assert results[1].stats["copies_refused"] > 0 and results[1].stats["copies_made"] > 0


def test_the_scenario_on_the_oracle_takes_every_branch_unguarded(make_problem, cs):
    _, _, _, _, ref = _oracle_run(make_problem, cs)
    results = []
    for steps, lower in zip(tw.RUN_STEPS, run_lowers() + [None]):
        for tt in steps:
            ref.step(tt)
        if lower is not None:
            energy = ref.particles.as_dict()["energy"]
            live = ref.particles.as_dict()["dead"] == 0
            assert not gr.near_an_edge(energy[live], EDGES3).any()
            results.append(apply_to_oracle(ref, lower, steps[-1]))
    check_every_branch(results)


# ---- GPU: the grouped calls alone ----------------------------------------------------------------

def _edges_pointer(edges):
    e = np.ascontiguousarray(edges, dtype=np.float64)
    return e, e.ctypes.data_as(C.POINTER(C.c_double))


class GroupStore(tw.WindowStore):
    """the store, on a MESH x MESH mesh, with the two grouped calls and the plain census"""

    def window_groups(self, edges, lower, upper_ratio=2.0, survival_ratio=1.5, max_split=5, seed=SEED, nx=MESH,
                      ny=MESH, ngroups=None, null_edges=False):
        """the library's own call: -> (return code, stats)"""
        e, pointer = _edges_pointer(edges)
        stats = self.iface.GroupWindowStats()
        self.iface.set_pid_base(self.sim.pid_base)
        d_lower = self.torch.from_numpy(np.ascontiguousarray(lower, dtype=np.float64).ravel()).to(self.sim.device)
        rc = self.iface.library().neutral_hip_window_particles_groups(
            self.sim.particles, self.n, nx, ny, e.size - 1 if ngroups is None else ngroups,
            None if null_edges else pointer, d_lower.data_ptr(), upper_ratio, survival_ratio, max_split, seed,
            C.byref(stats))
        return rc, stats

    def census_groups(self, edges, nx=MESH, ny=MESH, ngroups=None, null_edges=False):
        """the library's own call: -> (return code, stats, the 2 * G * nx * ny values on the host,
        which went in filled with 7)"""
        e, pointer = _edges_pointer(edges)
        stats = self.iface.GroupCensusStats()
        self.iface.set_pid_base(self.sim.pid_base)
        out = self.torch.full((2 * max(e.size - 1, 1) * nx * ny,), 7.0, dtype=self.torch.float64, device=self.sim.device)
        rc = self.iface.library().neutral_hip_census_tally_groups(
            self.sim.particles, self.n, nx, ny, e.size - 1 if ngroups is None else ngroups,
            None if null_edges else pointer, C.c_void_p(out.data_ptr()), C.byref(stats))
        return rc, stats, out.cpu().numpy()

    def census_plain(self, nx, ny):
        stats = self.iface.CensusStats()
        self.iface.set_pid_base(self.sim.pid_base)
        out = self.torch.full((2 * nx * ny,), 7.0, dtype=self.torch.float64, device=self.sim.device)
        rc = self.iface.library().neutral_hip_census_tally(self.sim.particles, self.n, nx, ny,
                                                           C.c_void_p(out.data_ptr()), C.byref(stats))
        return rc, stats, out.cpu().numpy()


def window_stats(stats):
    return {k: getattr(stats, k) for k in INT_STATS}


def sum_bound(a):
    """of each roulette weight sum against the exact one (tests/test_window.py)"""
    live = a["dead"] == 0
    return len(a["dead"]) * EPS * float(np.abs(a["weight"][live]).sum())


def check_census_weights(weight, want):
    """want: a Census of either restatement"""
    assert np.all(np.abs(weight - want.weight) <= (want.count + 1.0) * EPS * want.weight)


FACTORS = [0.1, 0.5, 0.999, 1.0, 1.5, 2.0, np.nextafter(2.0, 3.0), 2.5, 3.7, 4.0, 9.3, 100.0, 1e3]


def energy_store(n, seed, edges, dead_share=0.3, continuous=False, specials="all"):
    """tw.random_store's cells, dead slots (NaN scribbles, dead words 1..3) and other fields, with
    energies from a few lines -- the middles of the groups -- and every fifth live slot at one of the
    `specials`: "all": on edges, an ulp beside them and outside the groups; "far": outside the groups
    and far from every edge; None: no such slot.  The weights are a factor times the bound of the
    slot's own bin (on, beside and far from the bounds of upper_ratio 2; continuous: anywhere from
    0.05 to 20 times it).  -> (arrays, lower of shape (G, MESH, MESH))"""
    rng = np.random.default_rng([seed, 77])
    e = np.asarray(edges, dtype=np.float64)
    ngroups = e.size - 1
    a, _ = tw.random_store(n, seed, dead_share)
    lower = rng.choice([0.0, 0.25, 0.5, 1.0], size=(ngroups, MESH, MESH), p=[0.1, 0.3, 0.3, 0.3])
    energy = np.sqrt(e[:-1] * e[1:])[rng.integers(0, ngroups, n)]
    far = [0.5 * e[0], 2.0 * e[-1], np.inf, np.nan, -0.0, 0.0, -e[1]]
    near = [e[0], e[1], e[-2], e[-1], np.nextafter(e[0], 0.0), np.nextafter(e[-1], 0.0), np.nextafter(e[1], 0.0)]
    if specials:
        special = np.array(far + near if specials == "all" else far)
        energy = np.where(rng.random(n) < 0.2, special[rng.integers(0, special.size, n)], energy)
    live = a["dead"] == 0
    a["energy"] = np.where(live, energy, np.nan)
    g = gr.groups_of(a["energy"], e)
    inside = live & (g < ngroups)
    w_lo = np.zeros(n)
    w_lo[inside] = lower[g[inside], a["celly"][inside], a["cellx"][inside]]
    factor = np.exp(rng.uniform(np.log(0.05), np.log(20.0), n)) if continuous else rng.choice(FACTORS, size=n)
    a["weight"] = np.where(live, np.where(w_lo > 0.0, factor * w_lo, factor), np.nan)
    return a, lower


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [1, 64, 65, scan_tile() + 1, 100003])
def test_one_all_embracing_group_gives_the_plain_calls_bits(iface, make_problem, cs, n):
    st = GroupStore(iface, make_problem, cs, n)
    a, lower = tw.random_store(n, n)
    st.upload(a)
    rc, plain = st.raw(lower)
    after_plain = st.arrays()
    st.upload(a)
    rc_g, grouped = st.window_groups(gr.ALL_EMBRACING, lower)
    after_grouped = st.arrays()
    assert rc == rc_g == 0 and grouped.outside == 0
    for f in wr.FIELDS:
        assert same_bits(after_grouped[f], after_plain[f]), f
    assert window_stats(grouped.window) == window_stats(plain)
    print(f"n={n}: {window_stats(plain)} lost {plain.roulette_weight_lost!r} {grouped.window.roulette_weight_lost!r} "
          f"window_ms {plain.window_ms:.3f} {grouped.window.window_ms:.3f}")
    assert abs(grouped.window.roulette_weight_lost - plain.roulette_weight_lost) <= 2 * sum_bound(a)
    assert abs(grouped.window.roulette_weight_gained - plain.roulette_weight_gained) <= 2 * sum_bound(a)
    # the census, of the store as the windows found it
    st.upload(a)
    rc, pstats, pout = st.census_plain(MESH, MESH)
    rc_g, gstats, gout = st.census_groups(gr.ALL_EMBRACING)
    assert rc == rc_g == 0 and gstats.outside == 0
    cells = MESH * MESH
    assert same_bits(gout[:cells], pout[:cells])
    assert (gstats.live, gstats.dead, gstats.occupied_bins, gstats.max_count) == \
        (pstats.live, pstats.dead, pstats.occupied_cells, pstats.max_count)
    want = cr.census(a, MESH, MESH)
    for weight, total, largest in ((pout[cells:], pstats.weight, pstats.max_cell_weight),
                                   (gout[cells:], gstats.weight, gstats.max_bin_weight)):
        check_census_weights(weight, want)
        assert largest == weight.max()
        assert abs(total - want.stats["weight"]) <= (want.stats["live"] + want.stats["occupied_cells"]) * EPS * want.stats["weight"]
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], a[f]), f
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("edges", [EDGES3, EDGES64], ids=["G3", "G64"])
def test_the_grouped_calls_are_the_plain_calls_on_the_virtual_store(iface, make_problem, cs, edges):
    n, ngroups = scan_tile() + 1, len(edges) - 1
    st = GroupStore(iface, make_problem, cs, n)
    a, lower = energy_store(n, 31 + ngroups, edges)
    virtual, g = gr.virtual_store(a, edges, MESH)
    live = a["dead"] == 0
    outside = int((live & (g == ngroups)).sum())
    assert outside > 50 and np.isnan(a["energy"][~live]).all() and (live & (g < ngroups)).sum() > 500
    rows = (ngroups + 1) * MESH
    lower_v = np.concatenate([lower.ravel(), np.zeros(MESH * MESH)])
    # the census first: the store as it stands
    st.upload(virtual)
    rc, pstats, pout = st.census_plain(MESH, rows)
    st.upload(a)
    rc_g, gstats, gout = st.census_groups(edges)
    assert rc == rc_g == 0
    bins, cells_v = ngroups * MESH * MESH, rows * MESH
    assert same_bits(gout[:bins], pout[:bins]) and gstats.outside == outside == int(pout[bins:cells_v].sum())
    assert (gstats.live, gstats.dead) == (pstats.live, pstats.dead) == (int(live.sum()), n - int(live.sum()))
    want = gr.census(a, edges, MESH, MESH)
    assert same_bits(gout[:bins], want.count)
    assert (gstats.occupied_bins, gstats.max_count) == (want.stats["occupied_bins"], want.stats["max_count"])
    check_census_weights(gout[bins:], want)
    assert gstats.max_bin_weight == gout[bins:].max()
    assert abs(gstats.weight - want.stats["weight"]) <= (gstats.live + gstats.occupied_bins) * EPS * want.stats["weight"]
    # the window
    st.upload(virtual)
    rc, plain = st.raw(lower_v, ny=rows)
    after_plain = st.arrays()
    st.upload(a)
    rc_g, grouped = st.window_groups(edges, lower)
    after_grouped = st.arrays()
    assert rc == rc_g == 0 and grouped.outside == outside
    assert window_stats(grouped.window) == window_stats(plain)
    assert plain.split > 0 and plain.roulette_killed > 0 and plain.roulette_survived > 0
    for f in wr.FIELDS:
        if f != "celly":
            assert same_bits(after_grouped[f], after_plain[f]), f
    alive = after_grouped["dead"] == 0
    g_after = gr.groups_of(after_grouped["energy"], edges)
    assert np.array_equal(after_plain["celly"][alive], (g_after * MESH + after_grouped["celly"])[alive])
    assert same_bits(after_grouped["celly"][~alive], a["celly"][~alive])  # (dead, or killed just now: untouched)
    assert abs(grouped.window.roulette_weight_lost - plain.roulette_weight_lost) <= 2 * sum_bound(a)
    assert abs(grouped.window.roulette_weight_gained - plain.roulette_weight_gained) <= 2 * sum_bound(a)
    print(f"G={ngroups}: {window_stats(plain)} outside {outside} window_ms plain {plain.window_ms:.3f} grouped "
          f"{grouped.window.window_ms:.3f} census_ms plain {pstats.census_ms:.3f} grouped {gstats.census_ms:.3f}")
    st.close()


def _check_against_helper(iface, st, a, edges, lower, max_split, name, pid_base=0, seed=SEED):
    st.upload(a)
    rc, cstats, cout = st.census_groups(edges)
    want = gr.census(a, edges, MESH, MESH)
    bins = (len(edges) - 1) * MESH * MESH
    assert rc == 0 and same_bits(cout[:bins], want.count), name
    assert {k: getattr(cstats, k) for k in ("live", "dead", "outside", "occupied_bins", "max_count")} == \
        {k: want.stats[k] for k in ("live", "dead", "outside", "occupied_bins", "max_count")}, name
    check_census_weights(cout[bins:], want)
    rc, stats = st.window_groups(edges, lower, max_split=max_split, seed=seed)
    assert rc == 0, name
    r = gr.window(a, edges, lower, MESH, MESH, 2.0, 1.5, max_split, wr.probe_rn0(iface, pid_base, seed))
    assert window_stats(stats.window) == r.stats and stats.outside == r.outside, name
    after = st.arrays()
    for f in wr.FIELDS:  # every field of every slot, the untouched ones' NaN scribbles included
        assert same_bits(after[f], r.arrays[f]), (name, f)
    print(f"n={st.n} {name}: {r.stats} outside {r.outside}")
    assert abs(stats.window.roulette_weight_lost - r.lost) <= sum_bound(a), name
    assert abs(stats.window.roulette_weight_gained - r.gained) <= sum_bound(a), name
    return r, stats


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [1000, scan_tile() + 1, 20011])
def test_bit_for_bit_against_the_helper(iface, make_problem, cs, n):
    pid_base = 123456789 if n == 1000 else 0
    st = GroupStore(iface, make_problem, cs, n, pid_base=pid_base)
    for edges in (EDGES3, EDGES64):
        a, lower = energy_store(n, n + len(edges), edges)
        r, _ = _check_against_helper(iface, st, a, edges, lower, 5, f"G={len(edges) - 1}", pid_base=pid_base)
        assert r.outside > 0 and r.stats["split"] > 0 and r.stats["roulette_killed"] > 0
    # weights whose every partial sum is exact: the census's weights bit for bit
    a, lower = energy_store(n, n + 3, EDGES3)
    live = a["dead"] == 0
    a["weight"][live] = np.random.default_rng(n).integers(1, 64, int(live.sum())) / 8.0
    st.upload(a)
    rc, cstats, cout = st.census_groups(EDGES3)
    want = gr.census(a, EDGES3, MESH, MESH)
    assert rc == 0 and same_bits(cout, np.concatenate([want.count, want.weight]))
    assert (cstats.weight, cstats.max_bin_weight) == (want.stats["weight"], want.stats["max_bin_weight"])
    st.close()


REFUSALS = ["ngroups 0", "ngroups 65", "edges null", "edge nan", "edge inf", "edge zero", "edge negative",
            "edges equal", "edges descending", "outside slot off the mesh", "outside slot with a nan weight",
            "nan bound nobody live and inside looks up", "nan bound a live inside slot looks up"]


@gpu
@needs_gpu
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals(iface, make_problem, cs, case):
    n = 5000
    st = GroupStore(iface, make_problem, cs, n)
    a, lower = energy_store(n, 13, EDGES3)
    g = gr.groups_of(a["energy"], EDGES3)
    live = a["dead"] == 0
    edges, kw = EDGES3, {}
    if case == "ngroups 0":
        kw = dict(ngroups=0)
    elif case == "ngroups 65":
        edges, kw = tuple(float(k) for k in range(1, 67)), dict(ngroups=65)
        lower = np.ones((65, MESH, MESH))
    elif case == "edges null":
        kw = dict(null_edges=True)
    elif case.startswith("edge"):
        edges = {"edge nan": (5e2, np.nan, 5e4, 5e5), "edge inf": (5e2, 5e3, 5e4, np.inf), "edge zero": (0.0, 5e3, 5e4, 5e5),
                 "edge negative": (-5e2, 5e3, 5e4, 5e5), "edges equal": (5e2, 5e3, 5e3, 5e5),
                 "edges descending": (5e2, 5e4, 5e3, 5e5)}[case]
    before_the_device = bool(kw) or case.startswith("edge")
    if case.startswith("outside slot"):
        j = int(np.flatnonzero(live & (g == 3))[-1])  # (the last of them: beyond the first tile)
        if "mesh" in case:
            a["cellx"][j] = MESH
        else:
            a["weight"][j] = np.nan
    elif case.startswith("nan bound"):
        j = int(np.flatnonzero(live & (g < 3))[-1])
        cell = (a["celly"] == a["celly"][j]) & (a["cellx"] == a["cellx"][j])
        lower = lower.copy()
        lower[g[j], a["celly"][j], a["cellx"][j]] = np.nan
        if "nobody" in case:  # that bin's live slots leave the groups; the dead and the outside stay
            a["energy"][live & cell & (g == g[j])] = 2.0 * EDGES3[-1]
            a["dead"][np.flatnonzero(~live)[0]] = 1
            for f in ("cellx", "celly"):
                a[f][np.flatnonzero(~live)[0]] = a[f][j]  # a dead slot in that very cell
    st.upload(a)
    if case == "nan bound nobody live and inside looks up":
        r, stats = _check_against_helper(iface, st, a, edges, lower, 5, case)
        assert r.outside > 0
        st.close()
        return
    rc, stats = st.window_groups(edges, lower, **kw)
    assert rc == 1 and stats.outside == 0
    assert (stats.window.below, stats.window.split, stats.window.copies_made, stats.window.roulette_killed) == (0, 0, 0, 0)
    assert gr.window(a, edges if not kw else (), lower, MESH, MESH, 2.0, 1.5, 5, wr.probe_rn0(iface, 0, SEED)) is None
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], a[f]), f
    if case.startswith("nan bound"):
        rc, cstats, _ = st.census_groups(edges)  # (the census looks no bound up)
        assert rc == 0 and cstats.outside == gr.census(a, edges, MESH, MESH).stats["outside"]
    else:
        rc, cstats, got = st.census_groups(edges, **kw)
        assert rc == 1 and (cstats.outside, cstats.occupied_bins, cstats.max_count, cstats.weight) == (0, 0, 0, 0.0)
        if before_the_device:
            assert np.all(got == 7.0) and cstats.live == 0
        else:
            assert not got.any() and cstats.live == int((a["dead"] == 0).sum())  # found on the device: zeros
        after = st.arrays()
        for f in wr.FIELDS:
            assert same_bits(after[f], a[f]), f
    if not before_the_device:  # ... and through the wrapper
        with pytest.raises(iface.WindowRefused) as refused:
            st.sim.window(lower, upper_ratio=2.0, survival_ratio=1.5, max_split=5, seed=SEED, groups=edges)
        assert refused.value.code == 1 and isinstance(refused.value.stats, iface.GroupWindowStats)
        if not case.startswith("nan bound"):
            with pytest.raises(iface.CensusRefused) as refused:
                st.sim.census(groups=edges)
            assert refused.value.code == 1
    st.close()


@gpu
@needs_gpu
def test_identity_on_a_second_call(iface, make_problem, cs):
    n = 20011
    st = GroupStore(iface, make_problem, cs, n)
    a, lower = energy_store(n, 11, EDGES3, dead_share=0.6, continuous=True, specials="far")
    r, stats = _check_against_helper(iface, st, a, EDGES3, lower, 64, "first call")
    assert not r.guarded.any() and stats.window.copies_refused == 0 and stats.window.split > 0
    assert stats.window.roulette_killed > 0 and int(r.demand.max()) + 1 < 64  # (max_split did not bind)
    first = st.arrays()
    rc, again = st.window_groups(EDGES3, lower, max_split=64, seed=SEED + 12345)
    w = again.window
    assert rc == 0 and (w.below, w.above, w.split, w.copies_made, w.copies_refused) == (0, 0, 0, 0, 0)
    assert w.live_before == stats.window.live_before - stats.window.roulette_killed + stats.window.copies_made
    # (a copy of an outside slot does not exist: nobody outside demands; the killed were inside)
    assert again.outside == stats.outside
    second = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(second[f], first[f]), f
    st.close()


@gpu
@needs_gpu
def test_auto_window_over_the_bins(iface, make_problem, cs):
    """census, bounds and window over (cell, group) bins in one call: the bounds are the plain
    restatement's on the grouped census as the census of a mesh of nx by G * ny, bit for bit; no
    copy is refused (a condition of this test), so that afterwards every occupied bin's mean weight
    lies inside its window."""
    n, ngroups = 20011, 3
    st = GroupStore(iface, make_problem, cs, n)
    a, _ = energy_store(n, 5, EDGES3, dead_share=0.6, continuous=True, specials="far")
    st.upload(a)
    bins = ngroups * MESH * MESH
    for bad in (np.ones((MESH, MESH)), np.ones((2, MESH, MESH)), np.ones(bins + 1), np.ones((MESH, ngroups * MESH))):
        with pytest.raises(ValueError) as refused:
            st.sim.window(bad, groups=EDGES3)
        assert not isinstance(refused.value, iface.Refused)
    with pytest.raises(ValueError):
        st.sim.census(groups=(1.0, 1.0))
    with pytest.raises(ValueError):
        st.sim.auto_window(groups=(2.0, 1.0))
    for f in wr.FIELDS:
        assert same_bits(st.arrays()[f], a[f]), f
    census, bounds, window = st.sim.auto_window(upper_ratio=2.0, survival_ratio=1.5, max_split=64, seed=SEED, groups=EDGES3)
    want = gr.census(a, EDGES3, MESH, MESH)
    both = st.sim.last_census.cpu().numpy()
    lower = st.sim.last_lower.cpu().numpy()
    assert both.size == 2 * bins and lower.size == bins
    assert same_bits(both[:bins], want.count) and (census.live, census.outside) == (want.stats["live"], want.stats["outside"])
    assert census.outside > 0
    want_bounds = cr.bounds(both[:bins], both[bins:], float(census.live - census.outside), 2.0, 0.0, 1)
    assert same_bits(lower, want_bounds.lower) and bounds.windowed_cells == census.occupied_bins
    r = gr.window(a, EDGES3, lower, MESH, MESH, 2.0, 1.5, 64, wr.probe_rn0(iface, 0, SEED))
    assert window_stats(window.window) == r.stats and window.outside == census.outside
    assert window.window.copies_refused == 0 and int(r.demand.max()) + 1 < 64 and not r.guarded.any()
    assert window.window.split > 0 and window.window.roulette_killed > 0
    count, weight, after = st.sim.census(groups=EDGES3)
    assert after.live == census.live - window.window.roulette_killed + window.window.copies_made
    assert after.outside == census.outside
    tc.check_inside_the_windows(count.cpu().numpy(), weight.cpu().numpy(), lower)
    # lower as (G, ny, nx), as G * ny * nx values and as one number; a second window is the identity
    first = st.arrays()
    for mesh in (lower.reshape(ngroups, MESH, MESH), lower):
        again = st.sim.window(mesh, upper_ratio=2.0, survival_ratio=1.5, max_split=64, seed=SEED + 1, groups=EDGES3)
        assert (again.window.below, again.window.above, again.window.copies_made) == (0, 0, 0)
    for f in wr.FIELDS:
        assert same_bits(st.arrays()[f], first[f]), f
    uniform = st.sim.window(1e-300, groups=EDGES3)
    assert uniform.window.above > 0 and uniform.outside == census.outside
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_nothing_to_do_on_a_tiled_store_changes_nothing(iface, make_problem, cs, lazy, monkeypatch):
    """A grouped census, and a grouped window that every history is inside or that has no window
    anywhere, write nothing and leave the records of a tiled store valid: the next step pays no
    re-import (the deck and the fields of
    tests/test_window.py::test_nothing_to_do_on_a_tiled_store_changes_nothing)."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    edges = (gr.ALL_EMBRACING[0], 1.0, gr.ALL_EMBRACING[1])

    def call(sim):
        count, _, census = sim.census(groups=edges)
        assert (census.live, census.dead, census.outside) == (30000, 0, 0) and int(count.sum().item()) == 30000
        stats = sim.window(0.5, groups=edges)  # every weight is 1: inside [0.5, 2.5]
        w = stats.window
        assert (w.live_before, stats.outside) == (30000, 0)
        assert (w.dead_before, w.below, w.above, w.copies_made, w.copies_refused) == (0,) * 5
        stats = sim.window(np.zeros((2, 400, 400)), groups=edges)  # no window anywhere
        assert (stats.window.live_before, stats.window.below, stats.window.above) == (30000, 0, 0)
        stats = sim.window(0.5, groups=(1e-300, 2e-300))  # everybody outside
        assert (stats.outside, stats.window.below, stats.window.above) == (30000, 0, 0)

    census_ops_support.check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call)


# ---- GPU: the grouped window in a run, against the oracle ----------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_grouped_window_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """tests/test_window.py::test_window_in_a_run_against_the_oracle with the energies of both sides
    overwritten after injection and a bound for every (cell, group) bin: the helper on the oracle's
    arrays against the library's grouped window."""
    prob, keys, values, absorb, ref = _oracle_run(make_problem, cs)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=tw.ON, cs_absorb=absorb)
    sim.inject()
    energy = run_energies(tw.RUN["nparticles"])
    iface.library().neutral_hip_memcpy_h2d(C.c_void_p(sim.particles.contents.energy), energy.ctypes.data, energy.nbytes)
    assert same_bits(sim.particle_arrays()["energy"], ref.particles.as_dict()["energy"])

    def both_step(tt):
        g, c = sim.step(tt), ref.step(tt)
        assert (g.nprocessed, g.facets, g.collisions, g.census) == \
            (c.nprocessed, c.facets, c.collisions, c.census), tt
        assert (g.stats.roulette_killed, g.stats.roulette_survived) == \
            (c.roulette_killed, c.roulette_survived), tt
        return c

    expect = None
    results = []
    for steps, lower in zip(tw.RUN_STEPS, run_lowers() + [None]):
        for tt in steps:
            c = both_step(tt)
            assert expect is None or c.nprocessed == expect  # (the copies are stepped, the killed are not)
            expect = None
        if lower is None:
            break
        live = int((ref.particles.as_dict()["dead"] == 0).sum())
        r = apply_to_oracle(ref, lower, steps[-1])
        results.append(r)
        stats = sim.window(lower, groups=EDGES3, **tw.RUN_RATIOS)  # (seed: 2^63 + 2^62 + the last master key)
        assert window_stats(stats.window) == r.stats and stats.outside == r.outside
        assert stats.window.live_before == live
        got = sim.particle_arrays()
        want = ref.particles.as_dict()
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(got[f], want[f]), f
        assert np.max(np.abs(got["weight"] - want["weight"])[want["dead"] == 0]) <= 1e-9
        expect = live - stats.window.roulette_killed + stats.window.copies_made
    check_every_branch(results)
    got, want = sim.particle_arrays(), ref.particles.as_dict()
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got[f], want[f]), f
    tg, tcpu = sim.tally_host(), ref.tally
    print(f"variant {variant} lazy {lazy}: tally rel L2 {np.linalg.norm(tg - tcpu) / np.linalg.norm(tcpu):.3e} "
          f"worst cell {np.max(np.abs(tg - tcpu) / np.maximum(np.abs(tcpu), 1e-300)):.3e}")
    assert np.linalg.norm(tg - tcpu) / np.linalg.norm(tcpu) < tw.TALLY_L2_TOL
    assert np.all(np.abs(tg - tcpu) <= tw.TALLY_L2_TOL * np.abs(tcpu))
    sim.close()


# ---- GPU: the driver's --window-groups -----------------------------------------------------------

SOURCE_FILE = ("component share=1.0 xpos=0.1 ypos=0.1 width=0.2 height=0.2\n"
               "line energy=2.5e3 share=1.0\n"
               "line energy=1.0e4 share=1.0\n"
               "line energy=4.0e4 share=1.0\n")


def _outside(stdout):
    found = re.findall(r"^Window outside (\d+)$", stdout, flags=re.M)
    assert len(found) == 1
    return int(found[0])


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_window_groups_on_one_rank_and_on_two(tmp_path):
    """`neutral.hip --roulette 0.25,0.5 --source 500,0.5 --source-file F --window auto,2,1.6
    --window-groups ...` with a source of three lines, 2.5e3, 1e4 -- the deck's own energy -- and 4e4.
    Edges from 1e-300 to 1e300 cover whatever energy a history has: nobody is outside.  Edges (2e3,
    5e3) cover the first line alone: the histories at 1e4, the deck's own among them, are met outside
    at every window -- with auto at its census, whose bounds find nobody inside at first and skip that
    window.  The totals are consistent, on one rank and on two (both on one GPU); a run without the
    flag prints no such line."""
    from neutral_amd import cs_table, decks
    from gpu_support import run_driver
    run = tmp_path / "run"
    (tmp_path / "arch").mkdir()
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    (run / "source.params").write_text(SOURCE_FILE)
    sets = ["--roulette", "0.25,0.5", "--source", "500,0.5", "--source-file", "source.params"]
    for kv in ("nx=64", "ny=64", "nparticles=100001", "iterations=6", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), rel, sets + ["--window", "auto,2,1.6"])
    assert "Window outside" not in plain and len(tc._census_lines(plain)) == 5
    wide = ["--window", "auto,2,1.6", "--window-groups", "1e-300,3e3,2e4,1e300"]
    narrow = ["--window", "auto,2,1.6", "--window-groups", "2e3,5e3"]
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    for ranks in (1, 2):
        extra, env_extra = (["--gpus", "2"], env) if ranks == 2 else ([], None)
        covered = run_driver(str(run), rel, sets + extra + wide, env_extra)
        totals, _ = tw._window_totals(covered)
        lines = tc._census_lines(covered)
        print(ranks, totals, lines)
        assert _outside(covered) == 0 and len(lines) == 5
        assert re.search(r"^Window auto skipped 0$", covered, flags=re.M)
        assert totals["copies made"] >= totals["split"] > 0
        assert lines[0]["live"] == tc._census_lines(plain)[0]["live"]  # (the same histories up to the first window)
        assert 0 < lines[0]["occupied"] <= 3 * 64 * 64
        left_out = run_driver(str(run), rel, sets + extra + narrow, env_extra)
        totals, _ = tw._window_totals(left_out)
        print(ranks, totals, _outside(left_out), re.findall(r"^(?:Source emitted|Window auto skipped) \d+$", left_out, flags=re.M))
        assert _outside(left_out) >= 100001 and totals["copies made"] >= totals["split"]
        # uniform bounds: every bin at WLOW
        uniform = run_driver(str(run), rel, sets + extra + ["--window", "0.3,2,1.6"] + narrow[2:], env_extra)
        print(ranks, tw._window_totals(uniform)[0], _outside(uniform), re.findall(r"^Source emitted \d+$", uniform, flags=re.M))
        assert _outside(uniform) >= 100001 and "Census" not in uniform

"""A coarse window mesh: the census tally and the weight window over blocks of cells
(include/neutral_hip.h: neutral_hip_census_tally_blocks, neutral_hip_window_particles_blocks).

The definition is by equivalence: the plain (no groups) or the grouped calls on a virtual store in
which a slot's cell is its block's.  tests/block_window_reference.py builds that store and calls the
restatements as they are.  CPU: blocks by hand, block (1, 1), the ABI, the wrappers' argument
handling, the driver's usage errors, and the in-run scenario on the oracle alone.  GPU: the blocks
calls against the plain or grouped calls on the uploaded virtual store and against the helper, both
forms of the census pass, the division, refusals, the identity on a second call, nothing to do on a
tiled store, what the feature is for (a sparse store that the per-cell bounds refuse), the blocks
window inside a run against the CPU oracle, two ranks, and the driver's --window-block.

The bounds are those of tests/test_group_window.py: two calls' roulette weight sums lie within
2 * n * 2^-53 * sum|w| of each other, and a census bin's weight within (m + 1) * 2^-53 * S of the
exact sum S of its m terms, in whatever order they are added -- the order is what the two forms of
the census pass differ in.  Weights that are multiples of 2^-10 below 2^6 add exactly up to 2^53 /
2^16 terms: every order gives the same bits.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import block_window_reference as bw
import census_ops_support
import census_reference as cr
import group_window_reference as gr
import test_census as tc
import test_group_window as tg
import test_window as tw
import window_reference as wr
from census_ops_support import same_bits
from conftest import ROOT
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, scan_tile  # noqa: F401

EPS = 2.0 ** -53
SEED = tw.SEED
MESH = tw.MESH
EDGES3 = tg.EDGES3
EDGES64 = tg.EDGES64
GROUPS = {0: None, 3: EDGES3, 64: EDGES64}
BLOCKS = [(1, 1), (16, 16), (3, 5), (17, 1)]  # unit cells; one bin; partial last blocks; wider than the mesh
LDS_CAP = 4096  # kCensusLdsBins as shipped
WORKER = os.path.join(ROOT, "tests", "gpu_blocks_worker.py")


def bins_of(block, edges, nx=MESH, ny=MESH):
    cnx, cny = bw.coarse(nx, ny, block)
    return (1 if edges is None else len(edges) - 1) * cny * cnx


# ---- CPU: the helper ----------------------------------------------------------------------------

def test_blocks_by_hand():
    """nx = 10 with block 4 is three blocks, the last two cells wide; ny = 3 with block 2 is two.  Six
    live slots of weight 1, 2, 4, ... and a dead one."""
    assert bw.coarse(10, 3, (4, 2)) == (3, 2) and bw.coarse(16, 16, (17, 1)) == (1, 16)
    assert bw.coarse(16, 16, (16, 16)) == (1, 1) and bw.coarse(16, 16, (3, 5)) == (6, 4)
    a = {f: np.arange(7, dtype=np.float64) for f in wr.F64_FIELDS}
    a["weight"] = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, np.nan])
    a["cellx"] = np.array([0, 3, 4, 7, 8, 9, -1], dtype=np.int32)
    a["celly"] = np.array([0, 1, 2, 0, 1, 2, -1], dtype=np.int32)
    a["dead"] = np.array([0, 0, 0, 0, 0, 0, 1], dtype=np.int32)
    v = bw.virtual_store(a, (4, 2), 10, 3)
    assert v["cellx"][:6].tolist() == [0, 0, 1, 1, 2, 2] and v["celly"][:6].tolist() == [0, 0, 1, 0, 0, 1]
    c = bw.census(a, (4, 2), None, 10, 3)
    assert c.count.tolist() == [2.0, 1.0, 1.0, 0.0, 1.0, 1.0] and c.weight.tolist() == [3.0, 8.0, 16.0, 0.0, 4.0, 32.0]
    assert c.stats == dict(live=6, dead=1, outside=0, occupied_bins=5, max_count=2, weight=63.0, max_bin_weight=32.0)
    # a cell off the true mesh refuses and does not wrap: cellx = 11 div 4 would be block 2 of 3
    for f, value, nx, ny in (("cellx", 11, 10, 3), ("cellx", 10, 10, 3), ("celly", 3, 10, 3), ("cellx", -1, 10, 3)):
        b = {k: a[k].copy() for k in wr.FIELDS}
        b[f][2] = value
        assert value // 4 < 3 and bw.virtual_store(b, (4, 2), nx, ny) is None, (f, value)
        assert bw.census(b, (4, 2), None, nx, ny) is None
        assert bw.window(b, (4, 2), None, np.ones(6), nx, ny, 2.0, 1.5, 3, tw.fixed_rn0({})) is None
    # the window: bound 4 in bin 0 (weights 1 and 2 play roulette for 6: slot 0 loses, slot 1 wins),
    # 1 in bin 5 (32 over 2: q = 16, asks for max_split - 1 = 2 and gets the two free slots 0 and 6)
    lower = np.array([4.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    r = bw.window(a, (4, 2), None, lower, 10, 3, 2.0, 1.5, 3, tw.fixed_rn0({0: 0.9, 1: 0.1}))
    assert r.stats == dict(live_before=6, dead_before=1, below=2, roulette_killed=1, roulette_survived=1, above=1,
                           split=1, copies_made=2, copies_refused=0) and r.outside == 0
    assert r.sources.tolist() == [5, 5] and r.destinations.tolist() == [0, 6]
    w = 32.0 / 3.0
    assert r.arrays["weight"].tolist() == [w, 6.0, 4.0, 8.0, 16.0, w, w]
    assert r.arrays["cellx"].tolist() == [9, 3, 4, 7, 8, 9, 9] and r.arrays["celly"].tolist() == [2, 1, 2, 0, 1, 2, 2]
    # with groups: the bins of group 1 stand behind those of group 0
    a["energy"] = np.array([5.0, 50.0, 5.0, 50.0, 500.0, 5.0, np.nan])
    c = bw.census(a, (4, 2), (1.0, 10.0, 100.0), 10, 3)
    assert c.count.tolist() == [1.0, 0, 0, 0, 1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0] and c.stats["outside"] == 1
    for bad in ((0, 1), (1, 0), (-2, 2), (1.5, 1), (2,)):
        assert not bw.valid_block(bad) and bw.census(a, bad, None, 10, 3) is None


@pytest.mark.parametrize("n", [1, 65, 5000])
def test_block_one_is_the_plain_or_grouped_restatement(n):
    a, lower = tg.energy_store(n, n, EDGES3)
    plain = wr.window(a, lower[0], MESH, MESH, 2.0, 1.5, 5, tw.numpy_rn0(n))
    grouped = gr.window(a, EDGES3, lower, MESH, MESH, 2.0, 1.5, 5, tw.numpy_rn0(n))
    for want, edges, mesh in ((gr.GroupResult(*plain, outside=0), None, lower[0]), (grouped, EDGES3, lower)):
        got = bw.window(a, (1, 1), edges, mesh, MESH, MESH, 2.0, 1.5, 5, tw.numpy_rn0(n))
        assert got.stats == want.stats and got.outside == want.outside and (got.lost, got.gained) == (want.lost, want.gained)
        for f in wr.FIELDS:
            assert same_bits(got.arrays[f], want.arrays[f]), f
    pc, c0 = cr.census(a, MESH, MESH), bw.census(a, (1, 1), None, MESH, MESH)
    assert same_bits(c0.count, pc.count) and same_bits(c0.weight, pc.weight) and c0.stats["outside"] == 0
    assert c0.stats["occupied_bins"] == pc.stats["occupied_cells"] and c0.stats["weight"] == pc.stats["weight"]
    gc, c3 = gr.census(a, EDGES3, MESH, MESH), bw.census(a, (1, 1), EDGES3, MESH, MESH)
    assert same_bits(c3.count, gc.count) and same_bits(c3.weight, gc.weight) and c3.stats == gc.stats


# ---- CPU: the ABI, the wrappers, the driver ------------------------------------------------------

def test_library_exports_the_blocks_calls(tmp_path):
    from neutral_amd import interface as iface
    lib = iface.library()
    for name in ("neutral_hip_census_tally_blocks", "neutral_hip_window_particles_blocks"):
        assert hasattr(lib, name) and name in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.BlockCensusStats._fields_] == ["census", "privatised"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "neutral_hip.h"\n'
                   'int main(void) {\n  printf("%zu %zu %zu\\n", sizeof(NeutralHipBlockCensusStats), '
                   'offsetof(NeutralHipBlockCensusStats, census), offsetof(NeutralHipBlockCensusStats, privatised));\n'
                   "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "layout")])
    said = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in said] == [C.sizeof(iface.BlockCensusStats), iface.BlockCensusStats.census.offset,
                                      iface.BlockCensusStats.privatised.offset] == [72, 0, 64]
    text = open(os.path.join(ROOT, "include", "neutral_hip.h")).read()
    assert "neutral_hip_window_bounds(cnx, max(G, 1) * cny, census, ...)" in text and "NEUTRAL_CENSUS_LDS_BINS" in text


BAD_BLOCKS = {"zero": 0, "negative": -3, "pair with zero": (4, 0), "three": (1, 2, 3), "one in a tuple": (4,),
              "too large": 2 ** 31}
BAD_BLOCK_TYPES = {"float": 2.0, "bool": True, "pair with a float": (2, 2.5), "text": "4"}


def test_wrappers_refuse_bad_blocks_and_shapes_before_the_library(monkeypatch):
    from neutral_amd import interface as iface

    def touched(*args):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(iface._lib, "neutral_hip_census_tally_blocks", touched)
    monkeypatch.setattr(iface._lib, "neutral_hip_window_particles_blocks", touched)
    store = C.pointer(iface.Particle())
    for table, error in ((BAD_BLOCKS, ValueError), (BAD_BLOCK_TYPES, TypeError)):
        for name, block in table.items():
            with pytest.raises(error) as refused:
                iface.window_block(block)
            assert not isinstance(refused.value, iface.Refused), name
            with pytest.raises(error):
                iface.census_tally_blocks(store, 16, 4, 4, block)
            with pytest.raises(error):
                iface.window_particles_blocks(store, 16, 4, 4, block, None, 1, 5.0, 3.0, 5, 0)
    assert iface.window_block(3) == (3, 3) and iface.window_block((2, np.int32(5))) == (2, 5)
    assert iface.block_bins(10, 16, (4, 1)) == (3, 16, 0) and iface.block_bins(10, 16, 17, EDGES3) == (1, 1, 3)
    for name, edges in tg.BAD_EDGES.items():
        with pytest.raises(ValueError):
            iface.census_tally_blocks(store, 16, 4, 4, 2, edges)
        with pytest.raises(ValueError):
            iface.window_particles_blocks(store, 16, 4, 4, 2, edges, 1, 5.0, 3.0, 5, 0)
    with pytest.raises(ValueError):
        iface.census_tally_blocks(None, 16, 4, 4, 2)  # no store
    with pytest.raises(ValueError):
        iface.window_particles_blocks(None, 16, 4, 4, 2, None, 1, 5.0, 3.0, 5, 0)
    for n, nx, ny in ((0, 4, 4), (-5, 4, 4), (2 ** 31, 4, 4), (16, 0, 4), (16, 4, -1)):
        with pytest.raises(ValueError):
            iface.census_tally_blocks(store, n, nx, ny, 2)
        with pytest.raises(ValueError):
            iface.window_particles_blocks(store, n, nx, ny, 2, None, 1, 5.0, 3.0, 5, 0)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            iface.window_particles_blocks(store, 16, 4, 4, 2, None, 1, 5.0, 3.0, 5, seed)
    with pytest.raises(TypeError):
        iface.window_particles_blocks(store, 16, 4, 4, 2, None, 1, 5.0, 3.0, 2.5, 0)


def test_library_refuses_without_a_device():
    """refusals that need no device to say so (lower, device_out: any non-null address)"""
    from neutral_amd import interface as iface
    lib = iface.library()
    store = C.pointer(iface.Particle())
    mesh = np.ones(2 * 3 * 16)
    at = C.c_void_p(mesh.ctypes.data)
    good = (1.0, 10.0, 100.0, 1000.0)

    def both(bx=2, by=2, ngroups=0, edges=None, nx=4, ny=4, n=16, particles=store):
        e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        ws, cs_ = iface.GroupWindowStats(), iface.BlockCensusStats()
        rc = (lib.neutral_hip_window_particles_blocks(particles, n, nx, ny, bx, by, ngroups, e, at, 5.0, 3.0, 5, 0,
                                                      C.byref(ws)),
              lib.neutral_hip_census_tally_blocks(particles, n, nx, ny, bx, by, ngroups, e, at, C.byref(cs_)))
        assert (ws.window.live_before, ws.outside, cs_.census.live, cs_.census.outside, cs_.privatised) == (0,) * 5
        return rc
    assert both(bx=0) == both(by=0) == both(bx=-1) == both(by=-2 ** 31) == (1, 1)
    assert both(ngroups=-1) == both(ngroups=65, edges=tuple(range(1, 67))) == both(ngroups=3) == (1, 1)
    assert both(ngroups=0, edges=good) == (1, 1)  # edges without groups: a caller's mistake
    for edges in ((1.0, np.nan, 100.0, 1000.0), (0.0, 10.0, 100.0, 1000.0), (1.0, 10.0, 10.0, 1000.0)):
        assert both(ngroups=3, edges=edges) == (1, 1), edges
    assert both(particles=None) == both(n=0) == both(nx=0) == both(ny=0) == (1, 1)
    assert both(bx=1, by=1, nx=2 ** 16, ny=2 ** 15) == (1, 1)  # (B = 2^31 > 0x3fffffff)
    assert both(bx=1, by=1, ngroups=3, edges=good, nx=2 ** 15, ny=2 ** 14) == (1, 1)  # (with the groups alone)
    assert lib.neutral_hip_window_particles_blocks(store, 16, 4, 4, 2, 2, 0, None, None, 5.0, 3.0, 5, 0, None) == 1
    assert lib.neutral_hip_window_particles_blocks(store, 16, 4, 4, 2, 2, 0, None, at, 1.5, 1.0, 5, 0, None) == 1
    assert lib.neutral_hip_census_tally_blocks(store, 16, 4, 4, 2, 2, 0, None, None, None) == 1


USAGE = {"no value": ["--window", "0.3", "--window-block"], "zero": ["--window", "0.3", "--window-block", "0"],
         "negative": ["--window", "0.3", "--window-block", "-4"], "text": ["--window", "0.3", "--window-block", "x"],
         "fraction": ["--window", "0.3", "--window-block", "2.5"],
         "trailing comma": ["--window", "auto", "--window-block", "4,"],
         "three": ["--window", "0.3", "--window-block", "4,4,4"], "zero height": ["--window", "0.3", "--window-block", "4,0"],
         "no --window": ["--window-block", "4"], "no --window, with groups": ["--window-block", "4,2", "--window-groups", "1,2"],
         "decomposed": ["--window", "0.3", "--window-block", "4", "--decompose", "1x1"]}


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("case", sorted(USAGE))
def test_driver_usage_errors(tmp_path, case):
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + USAGE[case], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    said = out.stderr + out.stdout
    if case == "no --window":
        assert "--window-block needs --window" in said
    elif case == "no --window, with groups":
        assert "needs --window" in said
    elif case == "decomposed":
        assert "--window does not work with --decompose" in said
    else:
        assert "--window-block wants BX[,BY], integers >= 1" in said


# ---- the in-run scenario: the grouped window's, on blocks of 5 x 7 cells -------------------------

RUN_BLOCK = (5, 7)  # the 24 x 24 mesh in 5 x 4 blocks, the last of a row 4 cells wide, of a column 3 high


def run_lowers():
    """tests/test_window.py's two windows (source box: cells 2..7, dense block: cells 9..14) on the
    coarse mesh -- block column 2 is cells 10..14, block row 1 cells 7..13 --, scaled group by group
    as tests/test_group_window.py scales them.  The weights at a census are what injection or a
    window gave out (run_meshes explains why): the bounds stay clear of them and of their quotients."""
    first = np.full((4, 5), 0.3)
    first[1, 2] = 1.5
    second = np.full((4, 5), 0.3)
    second[1, 2] = 0.6
    second[0:2, 0:2] = 0.1
    return [np.stack([scale * mesh for scale in scales]) for mesh, scales in zip((first, second), tg.RUN_SCALES)]


def apply_to_oracle(ref, lower, tt):
    """the helper on the oracle's arrays, in place; -> GroupResult"""
    arrays = ref.particles.as_dict()
    r = bw.window(arrays, RUN_BLOCK, EDGES3, lower, 24, 24, tw.RUN_RATIOS["upper_ratio"],
                  tw.RUN_RATIOS["survival_ratio"], tw.RUN_RATIOS["max_split"], wr.cpu_rn0(0, wr.WINDOW_SEED_BASE + tt))
    assert r is not None
    for f in wr.FIELDS:
        arrays[f][:] = r.arrays[f]
    return r


def test_the_scenario_on_the_oracle_takes_every_branch_unguarded(make_problem, cs):
    """the condition of the GPU test below, on the oracle alone: no guarded slot, and both windows
    split, kill, let survive and meet histories outside; the second refuses copies and makes some"""
    _, _, _, _, ref = tg._oracle_run(make_problem, cs)
    results = []
    for steps, lower in zip(tw.RUN_STEPS, run_lowers() + [None]):
        for tt in steps:
            ref.step(tt)
        if lower is not None:
            energy = ref.particles.as_dict()["energy"]
            live = ref.particles.as_dict()["dead"] == 0
            assert not gr.near_an_edge(energy[live], EDGES3).any()
            results.append(apply_to_oracle(ref, lower, steps[-1]))
    tg.check_every_branch(results)


# ---- GPU: the blocks calls alone -----------------------------------------------------------------

class BlockStore(tg.GroupStore):
    """the store with the two blocks calls beside the plain and the grouped ones"""

    def window_blocks(self, block, edges, lower, upper_ratio=2.0, survival_ratio=1.5, max_split=5, seed=SEED,
                      nx=MESH, ny=MESH, ngroups=None, null_edges=False):
        """the library's own call: -> (return code, stats)"""
        e, pointer = (None, None) if edges is None else tg._edges_pointer(edges)
        stats = self.iface.GroupWindowStats()
        self.iface.set_pid_base(self.sim.pid_base)
        d_lower = self.torch.from_numpy(np.ascontiguousarray(lower, dtype=np.float64).ravel()).to(self.sim.device)
        rc = self.iface.library().neutral_hip_window_particles_blocks(
            self.sim.particles, self.n, nx, ny, block[0], block[1],
            (0 if e is None else e.size - 1) if ngroups is None else ngroups, None if null_edges else pointer,
            d_lower.data_ptr(), upper_ratio, survival_ratio, max_split, seed, C.byref(stats))
        return rc, stats

    def census_blocks(self, block, edges, nx=MESH, ny=MESH, ngroups=None, null_edges=False, doubles=None):
        """the library's own call: -> (return code, stats, the 2 * B values on the host, which went
        in filled with 7)"""
        e, pointer = (None, None) if edges is None else tg._edges_pointer(edges)
        stats = self.iface.BlockCensusStats()
        self.iface.set_pid_base(self.sim.pid_base)
        doubles = 2 * bins_of(block, edges, nx, ny) if doubles is None else doubles
        out = self.torch.full((doubles,), 7.0, dtype=self.torch.float64, device=self.sim.device)
        rc = self.iface.library().neutral_hip_census_tally_blocks(
            self.sim.particles, self.n, nx, ny, block[0], block[1],
            (0 if e is None else e.size - 1) if ngroups is None else ngroups, None if null_edges else pointer,
            C.c_void_p(out.data_ptr()), C.byref(stats))
        return rc, stats, out.cpu().numpy()

    def census_on_the_virtual_store(self, edges, cnx, cny):
        """the plain or the grouped census: -> (return code, GroupCensusStats by name, values)"""
        if edges is None:
            rc, s, out = self.census_plain(cnx, cny)
            return rc, dict(live=s.live, dead=s.dead, outside=0, occupied_bins=s.occupied_cells,
                            max_count=s.max_count), out
        rc, s, out = self.census_groups(edges, nx=cnx, ny=cny)
        return rc, {k: getattr(s, k) for k in ("live", "dead", "outside", "occupied_bins", "max_count")}, out

    def window_on_the_virtual_store(self, edges, lower, cnx, cny, **kw):
        """the plain or the grouped window: -> (return code, WindowStats, outside)"""
        if edges is None:
            rc, s = self.raw(lower, nx=cnx, ny=cny, **kw)
            return rc, s, 0
        rc, s = self.window_groups(edges, lower, nx=cnx, ny=cny, **kw)
        return rc, s.window, s.outside


def census_stats(stats):
    return {k: getattr(stats.census, k) for k in ("live", "dead", "outside", "occupied_bins", "max_count")}


def block_store(n, seed, block, edges, nx=MESH, ny=MESH, **kw):
    """tests/test_group_window.py's store (cells anywhere on the MESH x MESH mesh, 30 % dead slots of
    NaN and -1, energies on, beside and outside the groups, weights on, beside and far from bounds)
    with a bound for every bin of the coarse mesh, the first of them not 0 -- where there is one bin,
    it has a window.  -> (arrays, lower of shape (max(G, 1), cny, cnx))"""
    a, _ = tg.energy_store(n, seed, EDGES3 if edges is None else edges, **kw)
    cnx, cny = bw.coarse(nx, ny, block)
    rng = np.random.default_rng([seed, 99])
    meshes = 1 if edges is None else len(edges) - 1
    lower = rng.choice([0.0, 0.25, 0.5, 1.0], size=(meshes, cny, cnx), p=[0.1, 0.3, 0.3, 0.3])
    lower[:, 0, 0] = 0.5
    # the weights again: a factor times the bound of the slot's own bin of the coarse mesh
    live = a["dead"] == 0
    g = np.zeros(n, dtype=np.int64) if edges is None else gr.groups_of(a["energy"], edges)
    inside = live & (g < meshes)
    w_lo = np.zeros(n)
    w_lo[inside] = lower[g[inside], a["celly"][inside] % ny // block[1], a["cellx"][inside] % nx // block[0]]
    factor = np.exp(rng.uniform(np.log(0.05), np.log(20.0), n)) if kw.get("continuous") else rng.choice(tg.FACTORS, size=n)
    a["weight"] = np.where(live, np.where(w_lo > 0.0, factor * w_lo, factor), np.nan)
    return a, lower


def with_weights(a, kind, seed):
    """the store with other live weights: "dyadic": multiples of 2^-10 below 64, whose sums are exact
    in any order; "log-uniform": over six decades"""
    rng = np.random.default_rng([seed, 5])
    live = a["dead"] == 0
    b = {f: a[f].copy() for f in wr.FIELDS}
    b["weight"][live] = rng.integers(1, 2 ** 16, int(live.sum())) / 1024.0 if kind == "dyadic" else \
        np.exp(rng.uniform(np.log(1.0e-3), np.log(1.0e3), int(live.sum())))
    return b


@gpu
@needs_gpu
@pytest.mark.parametrize("ngroups", sorted(GROUPS))
@pytest.mark.parametrize("n", [1, 64, 65, scan_tile() + 1, 100003])
def test_the_blocks_calls_are_the_plain_or_grouped_calls_on_the_virtual_store(iface, make_problem, cs, n, ngroups):
    """per block shape: the census (counts exact; weights bit for bit where every sum is exact, inside
    the any-order bound on log-uniform weights) and the window (every field of every slot, the true
    cells restored, copies' included) against the plain or grouped call on the uploaded virtual
    store, and against the helper"""
    edges = GROUPS[ngroups]
    st = BlockStore(iface, make_problem, cs, n)
    for block in BLOCKS:
        cnx, cny = bw.coarse(MESH, MESH, block)
        bins = bins_of(block, edges)
        a, lower = block_store(n, n + 7 * ngroups + block[0], block, edges)
        virtual = bw.virtual_store(a, block, MESH, MESH)
        # the census: dyadic weights bit for bit, log-uniform ones within the bound
        for kind in ("dyadic", "log-uniform"):
            b, bv = with_weights(a, kind, n), with_weights(virtual, kind, n)
            st.upload(bv)
            rc, vstats, vout = st.census_on_the_virtual_store(edges, cnx, cny)
            st.upload(b)
            rc_b, stats, out = st.census_blocks(block, edges)
            assert rc == rc_b == 0 and stats.privatised == (1 if bins <= LDS_CAP else 0), (block, kind)
            want = bw.census(b, block, edges, MESH, MESH)
            assert same_bits(out[:bins], vout[:bins]) and same_bits(out[:bins], want.count), (block, kind)
            assert census_stats(stats) == vstats == {k: want.stats[k] for k in vstats}, (block, kind)
            if kind == "dyadic":
                assert same_bits(out[bins:], vout[bins:2 * bins]) and same_bits(out[bins:], want.weight), block
                assert (stats.census.weight, stats.census.max_bin_weight) == (want.stats["weight"], want.stats["max_bin_weight"])
            else:
                tg.check_census_weights(out[bins:], want)
                tg.check_census_weights(vout[bins:2 * bins], want)
                assert stats.census.max_bin_weight == out[bins:].max()
            after = st.arrays()
            for f in wr.FIELDS:
                assert same_bits(after[f], b[f]), (block, f)  # (the census writes nothing)
        # the window
        st.upload(virtual)
        rc, vstats, voutside = st.window_on_the_virtual_store(edges, lower, cnx, cny)
        after_virtual = st.arrays()
        st.upload(a)
        rc_b, stats = st.window_blocks(block, edges, lower)
        after = st.arrays()
        assert rc == rc_b == 0 and stats.outside == voutside, block
        assert tg.window_stats(stats.window) == tg.window_stats(vstats), block
        for f in wr.FIELDS:
            if f not in ("cellx", "celly"):
                assert same_bits(after[f], after_virtual[f]), (block, f)
        alive = after["dead"] == 0
        assert np.array_equal(after_virtual["cellx"][alive], after["cellx"][alive] // block[0])
        assert np.array_equal(after_virtual["celly"][alive], after["celly"][alive] // block[1])
        r = bw.window(a, block, edges, lower, MESH, MESH, 2.0, 1.5, 5, wr.probe_rn0(iface, 0, SEED))
        assert tg.window_stats(stats.window) == r.stats and stats.outside == r.outside, block
        for f in wr.FIELDS:  # every field of every slot: the true cells, the untouched slots' NaN scribbles
            assert same_bits(after[f], r.arrays[f]), (block, f)
        assert abs(stats.window.roulette_weight_lost - vstats.roulette_weight_lost) <= 2 * tg.sum_bound(a)
        assert abs(stats.window.roulette_weight_gained - vstats.roulette_weight_gained) <= 2 * tg.sum_bound(a)
        assert abs(stats.window.roulette_weight_lost - r.lost) <= tg.sum_bound(a)
        if n >= 1000:
            assert r.stats["split"] > 0 and r.stats["roulette_killed"] > 0 and r.stats["roulette_survived"] > 0, block
        print(f"n={n} G={ngroups} block={block}: {r.stats} outside {r.outside}")
    st.close()


FORMS = {"one bin": (MESH, MESH, (MESH, MESH)), "at the cap": (64, 64, (1, 1)), "one over the cap": (17, 241, (1, 1)),
         "at the cap, blocks of 3 x 2": (192, 128, (3, 2))}


@gpu
@needs_gpu
@pytest.mark.parametrize("case", sorted(FORMS))
def test_both_forms_of_the_census_pass(iface, make_problem, cs, case, monkeypatch):
    """B = 1, B at the cap and B one over it: the pass that keeps its bins in LDS and the pass of two
    global atomics per live slot give the same counts and, on weights whose sums are exact, the same
    weights; `privatised` says which one ran"""
    nx, ny, block = FORMS[case]
    n = 20011
    bins = bins_of(block, None, nx, ny)
    assert bins == {"one bin": 1, "one over the cap": LDS_CAP + 1}.get(case, LDS_CAP)
    st = BlockStore(iface, make_problem, cs, n)
    a, _ = tw.random_store(n, 17)
    rng = np.random.default_rng(bins)
    live = a["dead"] == 0
    a["cellx"] = np.where(live, rng.integers(0, nx, n), -1).astype(np.int32)
    a["celly"] = np.where(live, rng.integers(0, ny, n), -1).astype(np.int32)
    a = with_weights(a, "dyadic", bins)
    st.upload(a)
    want = bw.census(a, block, None, nx, ny)
    monkeypatch.delenv("NEUTRAL_CENSUS_LDS_BINS", raising=False)
    rc, shipped, out = st.census_blocks(block, None, nx=nx, ny=ny)
    assert rc == 0 and shipped.privatised == (1 if bins <= LDS_CAP else 0)
    results = [out]
    for limit, privatised in (("0", 0), (str(bins), 1 if bins <= LDS_CAP else 0), (str(bins - 1), 0), ("1000000", shipped.privatised)):
        monkeypatch.setenv("NEUTRAL_CENSUS_LDS_BINS", limit)
        rc, stats, out = st.census_blocks(block, None, nx=nx, ny=ny)
        assert rc == 0 and stats.privatised == privatised, limit
        assert census_stats(stats) == census_stats(shipped)
        assert (stats.census.weight, stats.census.max_bin_weight) == (shipped.census.weight, shipped.census.max_bin_weight)
        results.append(out)
        print(f"{case}: B={bins} NEUTRAL_CENSUS_LDS_BINS={limit} privatised {stats.privatised} census_ms {stats.census.census_ms:.3f}")
    for out in results:
        assert same_bits(out[:bins], want.count) and same_bits(out[bins:], want.weight)
    assert census_stats(shipped) == {k: want.stats[k] for k in ("live", "dead", "outside", "occupied_bins", "max_count")}
    # with groups, and a slot that the call refuses: zeros from either form
    monkeypatch.delenv("NEUTRAL_CENSUS_LDS_BINS")
    if bins == 1:
        rc, stats, out = st.census_blocks(block, EDGES64, nx=nx, ny=ny)
        want = bw.census(a, block, EDGES64, nx, ny)
        assert rc == 0 and stats.privatised == 1 and same_bits(out, np.concatenate([want.count, want.weight]))
        assert stats.census.outside == want.stats["outside"]
    b = {f: a[f].copy() for f in wr.FIELDS}
    b["cellx"][np.flatnonzero(live)[-1]] = nx
    st.upload(b)
    for limit in ("0", str(LDS_CAP)):
        monkeypatch.setenv("NEUTRAL_CENSUS_LDS_BINS", limit)
        rc, stats, out = st.census_blocks(block, None, nx=nx, ny=ny)
        assert rc == 1 and not out.any() and stats.census.live == int(live.sum()) and stats.census.occupied_bins == 0
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("block_x", [3, 7, 641, 100002, 100003, 100004])
def test_the_division_is_exact(iface, make_problem, cs, block_x, monkeypatch):
    """slot j in cell j of a mesh of 100003 by 1 (and of 1 by 100003): every bin counts its block's
    width, and every slot lands in its own bin -- the bins with an even number have a window that
    everybody is under: their slots, and nobody else, play roulette"""
    n = 100003
    st = BlockStore(iface, make_problem, cs, n)
    a, _ = tw.random_store(n, 3, dead_share=0.0)
    a["weight"][:] = 1.0
    bins = -(-n // block_x)
    width = np.bincount(np.arange(n) // block_x, minlength=bins).astype(np.float64)
    assert width.sum() == n and width[-1] == n - (bins - 1) * block_x
    lower = np.where(np.arange(bins) % 2 == 0, 4.0, 0.0)
    for across in (True, False):
        a["cellx"] = (np.arange(n) if across else np.zeros(n)).astype(np.int32)
        a["celly"] = (np.zeros(n) if across else np.arange(n)).astype(np.int32)
        nx, ny, block = (n, 1, (block_x, 1)) if across else (1, n, (1, block_x))
        st.upload(a)
        for limit in ("0", str(LDS_CAP)):
            monkeypatch.setenv("NEUTRAL_CENSUS_LDS_BINS", limit)
            rc, stats, out = st.census_blocks(block, None, nx=nx, ny=ny)
            assert rc == 0 and same_bits(out[:bins], width) and same_bits(out[bins:], width), (across, limit)
            assert stats.census.max_count == width.max() and stats.census.occupied_bins == bins
        rc, stats = st.window_blocks(block, None, lower, nx=nx, ny=ny)
        after = st.arrays()
        windowed = (np.arange(n) // block_x) % 2 == 0
        assert rc == 0 and stats.window.below == int(windowed.sum()) and stats.window.above == 0
        assert np.all((after["dead"][windowed] != 0) | (after["weight"][windowed] == 6.0))
        assert np.all((after["dead"][~windowed] == 0) & (after["weight"][~windowed] == 1.0))
        r = bw.window(a, block, None, lower, nx, ny, 2.0, 1.5, 5, wr.probe_rn0(iface, 0, SEED))
        for f in wr.FIELDS:
            assert same_bits(after[f], r.arrays[f]), (across, f)
    st.close()


REFUSALS = ["block_x 0", "block_y -1", "ngroups -1", "ngroups 65", "groups and edges null", "edges and no groups",
            "edge nan", "edges descending", "too many bins", "cell off the true mesh, inside the coarse one",
            "celly off the true mesh, inside the coarse one", "outside slot off the true mesh", "nan weight",
            "nan bound nobody live and inside looks up", "nan bound a live inside slot looks up"]


@gpu
@needs_gpu
@pytest.mark.parametrize("case", REFUSALS)
def test_refusals(iface, make_problem, cs, case):
    """on a mesh of 10 x 16 in blocks of 4 x 5: three blocks across, the last two cells wide (cells
    10 and 11 would be in it), four up, the last one cell high"""
    n, nx, ny, block = 5000, 10, MESH, (4, 5)
    st = BlockStore(iface, make_problem, cs, n)
    a, lower = block_store(n, 13, block, EDGES3, nx=nx, ny=ny)
    live = a["dead"] == 0
    a["cellx"] = np.where(live, a["cellx"] % nx, -1).astype(np.int32)
    g = gr.groups_of(a["energy"], EDGES3)
    edges, kw, where = EDGES3, {}, dict(nx=nx, ny=ny)
    if case == "block_x 0":
        block = (0, 5)
    elif case == "block_y -1":
        block = (4, -1)
    elif case == "ngroups -1":
        kw = dict(ngroups=-1)
    elif case == "ngroups 65":
        edges, kw = tuple(float(k) for k in range(1, 67)), dict(ngroups=65)
    elif case == "groups and edges null":
        kw = dict(null_edges=True)
    elif case == "edges and no groups":
        kw = dict(ngroups=0)
    elif case.startswith("edge"):
        edges = {"edge nan": (5e2, np.nan, 5e4, 5e5), "edges descending": (5e2, 5e4, 5e3, 5e5)}[case]
    elif case == "too many bins":
        where, block = dict(nx=2 ** 15, ny=2 ** 14), (1, 1)  # (three groups of 2^29 bins)
    before_the_device = case in REFUSALS[:9]
    if "off the true mesh" in case:
        j = int(np.flatnonzero(live & ((g == 3) if "outside" in case else (g < 3)))[-1])
        if "celly" in case:
            where, block = dict(nx=MESH, ny=10), (5, 4)
            a["cellx"] = np.where(live, tw.random_store(n, 13)[0]["cellx"], -1).astype(np.int32)
            a["celly"] = np.where(live, a["celly"] % 10, -1).astype(np.int32)
            lower = lower.reshape(3, -1)[:, :12].reshape(3, 3, 4)  # (4 blocks across, 3 up)
            a["celly"][j] = 11
        else:
            a["cellx"][j] = 11
    elif case == "nan weight":
        a["weight"][int(np.flatnonzero(live)[-1])] = np.nan
    elif case.startswith("nan bound"):
        j = int(np.flatnonzero(live & (g < 3))[-1])
        bx, by = a["cellx"] // 4, a["celly"] // 5
        in_bin = (bx == bx[j]) & (by == by[j]) & (g == g[j])
        lower = lower.copy()
        lower[g[j], by[j], bx[j]] = np.nan
        if "nobody" in case:  # that bin's live slots leave the groups
            a["energy"][live & in_bin] = 2.0 * EDGES3[-1]
    st.upload(a)
    if case == "nan bound nobody live and inside looks up":
        rc, stats = st.window_blocks(block, edges, lower, **where)
        r = bw.window(a, block, edges, lower, nx, ny, 2.0, 1.5, 5, wr.probe_rn0(iface, 0, SEED))
        assert rc == 0 and tg.window_stats(stats.window) == r.stats and stats.outside == r.outside > 0
        after = st.arrays()
        for f in wr.FIELDS:
            assert same_bits(after[f], r.arrays[f]), f
        st.close()
        return
    rc, stats = st.window_blocks(block, edges, lower, **where, **kw)
    assert rc == 1 and stats.outside == 0
    assert (stats.window.below, stats.window.split, stats.window.copies_made, stats.window.roulette_killed) == (0, 0, 0, 0)
    if not before_the_device:
        assert bw.window(a, block, edges, lower, where["nx"], where["ny"], 2.0, 1.5, 5, wr.probe_rn0(iface, 0, SEED)) is None
        assert stats.window.live_before == int(live.sum())
    after = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(after[f], a[f]), f
    if case.startswith("nan bound"):
        rc, cstats, _ = st.census_blocks(block, edges, **where)  # (the census looks no bound up)
        assert rc == 0 and cstats.census.outside == bw.census(a, block, edges, nx, ny).stats["outside"]
    else:
        rc, cstats, got = st.census_blocks(block, edges, **where, **kw, doubles=2 * 3 * 12)
        assert rc == 1 and (cstats.census.outside, cstats.census.occupied_bins, cstats.census.max_count,
                            cstats.census.weight) == (0, 0, 0, 0.0)
        if before_the_device:
            assert np.all(got == 7.0) and cstats.census.live == 0
        else:
            assert bw.census(a, block, edges, where["nx"], where["ny"]) is None
            assert not got.any() and cstats.census.live == int(live.sum())  # found on the device: zeros
        after = st.arrays()
        for f in wr.FIELDS:
            assert same_bits(after[f], a[f]), f
    st.close()


@gpu
@needs_gpu
def test_identity_on_a_second_call(iface, make_problem, cs):
    n, block = 20011, (3, 5)
    st = BlockStore(iface, make_problem, cs, n)
    a, lower = block_store(n, 11, block, EDGES3, dead_share=0.6, continuous=True, specials="far")
    st.upload(a)
    rc, stats = st.window_blocks(block, EDGES3, lower, max_split=64)
    r = bw.window(a, block, EDGES3, lower, MESH, MESH, 2.0, 1.5, 64, wr.probe_rn0(iface, 0, SEED))
    assert rc == 0 and tg.window_stats(stats.window) == r.stats
    assert stats.window.copies_refused == 0 and stats.window.split > 0 and stats.window.roulette_killed > 0
    assert int(r.demand.max()) + 1 < 64  # (max_split did not bind)
    first = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(first[f], r.arrays[f]), f
    rc, again = st.window_blocks(block, EDGES3, lower, max_split=64, seed=SEED + 12345)
    w = again.window
    assert rc == 0 and (w.below, w.above, w.split, w.copies_made, w.copies_refused) == (0, 0, 0, 0, 0)
    assert w.live_before == stats.window.live_before - stats.window.roulette_killed + stats.window.copies_made
    assert again.outside == stats.outside
    second = st.arrays()
    for f in wr.FIELDS:
        assert same_bits(second[f], first[f]), f
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_nothing_to_do_on_a_tiled_store_changes_nothing(iface, make_problem, cs, lazy, monkeypatch):
    """A blocks census, and a blocks window that every history is inside or that has no window
    anywhere, write nothing and leave the records of a tiled store valid (the deck and the figures
    of tests/test_window.py::test_nothing_to_do_on_a_tiled_store_changes_nothing)."""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    edges = (gr.ALL_EMBRACING[0], 1.0, gr.ALL_EMBRACING[1])

    def call(sim):
        count, _, census = sim.census(block=(50, 30))
        assert (census.census.live, census.census.dead, census.census.outside) == (30000, 0, 0)
        assert count.numel() == 8 * 14 and int(count.sum().item()) == 30000 and census.privatised == 1
        count, _, census = sim.census(groups=edges, block=7)
        assert count.numel() == 2 * 58 * 58 and int(count.sum().item()) == 30000 and census.privatised == 0
        stats = sim.window(0.5, block=50)  # every weight is 1: inside [0.5, 2.5]
        w = stats.window
        assert (w.live_before, stats.outside) == (30000, 0)
        assert (w.dead_before, w.below, w.above, w.copies_made, w.copies_refused) == (0,) * 5
        stats = sim.window(np.zeros((2, 14, 8)), groups=edges, block=(50, 30))  # no window anywhere
        assert (stats.window.live_before, stats.window.below, stats.window.above) == (30000, 0, 0)
        stats = sim.window(0.5, groups=(1e-300, 2e-300), block=50)  # everybody outside
        assert (stats.outside, stats.window.below, stats.window.above) == (30000, 0, 0)

    census_ops_support.check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call)


# ---- GPU: what the feature is for ------------------------------------------------------------------

@gpu
@needs_gpu
def test_a_sparse_store_that_the_cells_cannot_window(iface, make_problem, cs):
    """4000 live histories in 4000 distinct cells of a 400 x 400 mesh, weights over two decades and ten
    times as many histories at one side as at the other (the bins' counts are uneven going in): per
    cell no bin holds min_count = 4 histories and the bounds refuse (K = 0); over blocks of 50 x 50
    cells the same call windows 64 bins, splits and plays roulette, and a second census finds the
    occupied bins' counts closer to even than the first did"""
    n, nx = 12000, 400
    prob = make_problem("csp", nx=nx, nparticles=n, iterations=1)
    sim = iface.Simulation(prob, *cs)
    sim.inject()
    rng = np.random.default_rng(400)
    a = {f: rng.random(n) for f in wr.F64_FIELDS}
    live = np.zeros(n, dtype=bool)
    live[rng.choice(n, 4000, replace=False)] = True
    # distinct cells, one history or none in each, ten times as dense at the left of the mesh as at
    # the right; the weight falls by two decades over the same way, as behind a shield
    density = np.tile(10.0 ** (-np.arange(nx) / nx), nx)
    cells = rng.choice(nx * nx, 4000, replace=False, p=density / density.sum())
    a["cellx"], a["celly"] = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    a["cellx"][live], a["celly"][live] = cells % nx, cells // nx
    a["weight"] = np.where(live, 10.0 ** (-2.0 * a["cellx"] / nx) * rng.uniform(0.8, 1.25, n), np.nan)
    a["dead"] = np.where(live, 0, 1).astype(np.int32)
    pc = sim.particles.contents
    for f in wr.FIELDS:
        v = np.ascontiguousarray(a[f])
        iface.library().neutral_hip_memcpy_h2d(C.c_void_p(getattr(pc, f)), v.ctypes.data, v.nbytes)
    ratios = dict(upper_ratio=2.0, survival_ratio=1.5)
    with pytest.raises(iface.BoundsRefused) as refused:
        sim.auto_window(min_count=4, seed=SEED, **ratios)
    assert refused.value.code == 1
    count, _, per_cell = sim.census()
    assert per_cell.max_count == 1 and per_cell.occupied_cells == 4000
    before, _, stats = sim.census(block=50)
    before = before.cpu().numpy()
    assert before.size == 64 and stats.census.occupied_bins == 64 and before.min() >= 4 and stats.privatised == 1
    for f in wr.FIELDS:
        assert same_bits(sim.particle_arrays()[f], a[f]), f  # (nothing written so far)
    census, bounds, window = sim.auto_window(min_count=4, block=50, seed=SEED, **ratios)
    assert bounds.windowed_cells == 64 and sim.last_lower.numel() == 64 and census.census.live == 4000
    assert window.window.split > 0 and window.window.roulette_killed > 0 and window.window.copies_made > 0
    after, _, stats = sim.census(block=50)
    after = after.cpu().numpy()
    assert stats.census.live == 4000 - window.window.roulette_killed + window.window.copies_made
    print(f"per-bin counts before: {before.min():.0f} .. {before.max():.0f}; after: {after.min():.0f} .. {after.max():.0f}; "
          f"{tg.window_stats(window.window)}")
    assert after.min() > 0 and after.max() / after.min() < before.max() / before.min()
    sim.close()


# ---- GPU: the blocks window in a run, against the oracle -----------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_blocks_window_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """tests/test_group_window.py::test_grouped_window_in_a_run_against_the_oracle with a bound for
    every (block, group) bin of blocks of 5 x 7 cells: the helper on the oracle's arrays against the
    library's blocks window.  The scenario has no guarded slot and takes every branch (the CPU test
    above)."""
    prob, keys, values, absorb, ref = tg._oracle_run(make_problem, cs)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=tw.ON, cs_absorb=absorb)
    sim.inject()
    energy = tg.run_energies(tw.RUN["nparticles"])
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
        stats = sim.window(lower, groups=EDGES3, block=RUN_BLOCK, **tw.RUN_RATIOS)  # (seed: the default)
        assert tg.window_stats(stats.window) == r.stats and stats.outside == r.outside
        assert stats.window.live_before == live
        got = sim.particle_arrays()
        want = ref.particles.as_dict()
        for f in ("cellx", "celly", "dead"):
            assert np.array_equal(got[f], want[f]), f
        assert np.max(np.abs(got["weight"] - want["weight"])[want["dead"] == 0]) <= 1e-9
        expect = live - stats.window.roulette_killed + stats.window.copies_made
    tg.check_every_branch(results)
    got, want = sim.particle_arrays(), ref.particles.as_dict()
    for f in ("cellx", "celly", "dead"):
        assert np.array_equal(got[f], want[f]), f
    tgpu, tcpu = sim.tally_host(), ref.tally
    print(f"variant {variant} lazy {lazy}: tally rel L2 {np.linalg.norm(tgpu - tcpu) / np.linalg.norm(tcpu):.3e} "
          f"worst cell {np.max(np.abs(tgpu - tcpu) / np.maximum(np.abs(tcpu), 1e-300)):.3e}")
    assert np.linalg.norm(tgpu - tcpu) / np.linalg.norm(tcpu) < tw.TALLY_L2_TOL
    assert np.all(np.abs(tgpu - tcpu) <= tw.TALLY_L2_TOL * np.abs(tcpu))
    sim.close()


# ---- GPU: two ranks on the one GPU ---------------------------------------------------------------

@gpu
@needs_gpu
def test_two_ranks_share_the_census_and_window_their_shards(tmp_path, make_problem):
    """tests/gpu_blocks_worker.py on two ranks, the store sharded: the blocks census is collective
    -- both ranks hold the same meshes, the counts the sum of each shard's own census --, and the
    window works per shard: each rank's arrays are the helper's on its slice, keyed from its own
    first particle id"""
    from ranks import launch_ranks
    prob = make_problem("csp", **tw.RUN)
    block, seed = [5, 7], SEED
    lower = run_lowers()[0]  # (the scenario's first window: it follows three steps there too)
    np.save(str(tmp_path / "lower.npy"), lower)
    spec = dict(block=block, edges=list(EDGES3), lower=str(tmp_path / "lower.npy"), seed=seed, steps=3,
                roulette=list(tw.ON), capture_scale=0.5, ratios=tw.RUN_RATIOS, energies=list(tg.RUN_ENERGIES))
    launch_ranks([sys.executable, WORKER, prob.deck, str(tmp_path), json.dumps(spec)], 2)
    files = [np.load(str(tmp_path / f"rank{r}.npz")) for r in range(2)]
    bins = 3 * 4 * 5
    counts, weights, live = np.zeros(bins), [], 0
    for f in files:
        before = {k: f[f"before_{k}"] for k in wr.FIELDS}
        said = json.loads(str(f["said"]))
        want = bw.census(before, block, EDGES3, 24, 24)
        counts += want.count
        weights.append(want.weight)
        live += want.stats["live"]
        assert (said["census"]["census"]["live"], said["census"]["census"]["outside"]) == (want.stats["live"], want.stats["outside"])
        assert said["census"]["privatised"] == 1
        r = bw.window(before, block, EDGES3, lower, 24, 24, tw.RUN_RATIOS["upper_ratio"], tw.RUN_RATIOS["survival_ratio"],
                      tw.RUN_RATIOS["max_split"], wr.cpu_rn0(int(f["pid_base"]), seed))
        assert {k: said["window"]["window"][k] for k in wr.STAT_NAMES} == r.stats and said["window"]["outside"] == r.outside
        assert r.stats["split"] > 0 and r.stats["roulette_killed"] > 0 and r.stats["roulette_survived"] > 0 and r.outside > 0
        for k in wr.FIELDS:
            assert same_bits(f[f"after_{k}"], r.arrays[k]), k
    assert int(files[0]["pid_base"]) == 0 and int(files[1]["pid_base"]) == len(files[0]["before_dead"])
    assert same_bits(files[0]["census"], files[1]["census"])
    got = files[0]["census"]
    assert same_bits(got[:bins], counts) and counts.sum() <= live
    total = weights[0] + weights[1]
    assert np.all(np.abs(got[bins:] - total) <= (counts + 2.0) * EPS * total)


# ---- GPU: the driver's --window-block ------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_window_block_on_one_rank_and_on_two(tmp_path):
    """`neutral.hip --roulette 0.25,0.5 --source 500,0.5 --source-file F --window auto,2,1.6
    --window-block 8 [--window-groups ...]` on the deck of tests/test_group_window.py's driver test:
    the 64 x 64 mesh in 8 x 8 blocks.  `Window blocks` is printed, the census lines count bins of the
    coarse mesh, and the totals are consistent, on one rank and on two (both on one GPU)."""
    from neutral_amd import cs_table, decks
    from gpu_support import run_driver
    run = tmp_path / "run"
    (tmp_path / "arch").mkdir()
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    rel = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / rel))
    (run / "source.params").write_text(tg.SOURCE_FILE)
    sets = ["--roulette", "0.25,0.5", "--source", "500,0.5", "--source-file", "source.params"]
    for kv in ("nx=64", "ny=64", "nparticles=100001", "iterations=6", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), rel, sets + ["--window", "auto,2,1.6"])
    assert "Window blocks" not in plain
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    for ranks in (1, 2):
        extra, env_extra = (["--gpus", "2"], env) if ranks == 2 else ([], None)
        for groups, meshes in (([], 1), (["--window-groups", "1e-300,3e3,2e4,1e300"], 3)):
            said = run_driver(str(run), rel, sets + extra + ["--window", "auto,2,1.6", "--window-block", "8"] + groups,
                              env_extra)
            totals, _ = tw._window_totals(said)
            lines = tc._census_lines(said)
            print(ranks, groups, totals, lines)
            assert re.findall(r"^Window blocks (\d+) x (\d+)$", said, flags=re.M) == [("8", "8")]
            assert len(lines) == 5 and re.search(r"^Window auto skipped 0$", said, flags=re.M)
            assert lines[0]["live"] == tc._census_lines(plain)[0]["live"]  # (the same histories up to the first window)
            assert all(0 < line["occupied"] <= meshes * 64 for line in lines)
            assert totals["copies made"] >= totals["split"] > 0
            assert ("Window outside 0" in said) == bool(groups) and ("Window outside" in said) == bool(groups)
        # blocks of 24 x 64: three across, the last 16 wide, one up; uniform bounds
        uniform = run_driver(str(run), rel, sets + extra + ["--window", "0.3,2,1.6", "--window-block", "24,64"], env_extra)
        assert re.findall(r"^Window blocks (\d+) x (\d+)$", uniform, flags=re.M) == [("3", "1")] and "Census" not in uniform
        assert tw._window_totals(uniform)[0]["copies made"] > 0

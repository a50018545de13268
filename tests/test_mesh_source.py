"""The mesh source (include/neutral_hip.h: neutral_hip_source_mesh).

CPU: the numpy restatement (tests/mesh_source_reference.py) pinned by a hand-computed store, by its
identity with the described source's restatement on a mesh of one non-zero cell, and by what it
chooses: never a cell of strength zero, every cell as often as its share says; that the seeds of the
GPU tests leave no draw guarded; the ABI, the wrapper's argument handling and check(), the driver's
usage errors.  GPU: a mesh of one non-zero cell against the described source's own bits, general
meshes against the restatement fed the library's samples, refusals, decomposed and sharded stores, no
re-import where nobody was dead, a run against the CPU oracle that re-emits what was absorbed, a
closed form on the stream deck, and the driver's --source-mesh on one rank and on two.
"""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import described_source_reference as dr
import mesh_source_reference as mr
import source_reference as sr
from conftest import ROOT
import census_ops_support
from census_ops_support import _junk, _patterns, _source_totals, _unit_mesh, same_bits
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, rel, scan_tile  # noqa: F401
from test_described_source import DescribedStore as Store  # (with the described source's call: what a mesh of one cell is compared with)

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
SEED = 2 ** 63 + 17
ON = (0.25, 0.5)
WEIGHT = 0.375
THETA = (0.3, 0.4)
ENERGIES = [(2.5e3, 3.0), (5.0e3, 2.0e4, 1.0)]  # a line and a bin
BINS = mr.spectrum(ENERGIES)
SIZES = [65, scan_tile() + 1, 100003]


# ---- the meshes and stores of the GPU tests, and their seeds ---------------------------------

MESHES = {"5 x 3": (5, 3), "64 x 33": (64, 33),  # (64 x 33: 2112 cells, just past one scan tile)
          "one row": (scan_tile() ** 2 + 1, 1)}   # (the scan's third level)


def _edges(n):
    return np.arange(n + 1, dtype=np.float64) / n


@functools.lru_cache(maxsize=None)
def _strength(mesh, pattern):
    """(ny, nx) strengths: `random` -- uniform with 40 % zeros; `exact` -- small integers times a power
    of two with 40 % zeros, whose sums are exact in any order.  The one row has three non-zero cells:
    the first, one in the middle, the last."""
    nx, ny = MESHES[mesh]
    rng = np.random.default_rng(nx + (7 if pattern == "exact" else 0))
    if mesh == "one row":
        s = np.zeros((ny, nx))
        at = [0, nx // 2 + 3, nx - 1]
        s[0, at] = rng.integers(1, 16, size=3) * 2.0 ** -7 if pattern == "exact" else 0.25 + rng.random(3)
        return s
    s = rng.integers(1, 16, size=(ny, nx)) * 2.0 ** -7 if pattern == "exact" else 1.0 - rng.random((ny, nx))
    s[rng.random((ny, nx)) < 0.4] = 0.0
    return s


@functools.lru_cache(maxsize=None)
def _table(mesh, pattern):
    return mr.Table(_strength(mesh, pattern))


def _mesh_args(mesh, dt=1e-7):
    nx, ny = MESHES[mesh]
    return mr.MeshArgs(0, 0, dt, _edges(nx), _edges(ny))


def _calls(n):
    """(name of the dead pattern, its mask, count, seed) of the general test's calls on a store of n"""
    out = [(name, mask, int(mask.sum()), SEED) for name, mask in _patterns(n).items()]
    name, mask = "random 30 %", _patterns(n)["random 30 %"]
    return out + [(name, mask, max(int(mask.sum()) - 3, 1), SEED + 1)]


@functools.lru_cache(maxsize=None)
def _cpu_u0(n, name, count, seed, pid_base=0):
    mask = _patterns(n)[name]
    return mr.cpu_u(sr.ranks(mask, count), pid_base, seed)[:, 0]


# ---- CPU: the restatement --------------------------------------------------------------------

def test_hand_computed_store_of_eight():
    dead = np.array([1, 0, 2, 1, 0, 7, 0, 1], dtype=np.int32)  # dead: 0, 2, 3, 5, 7
    edge = np.array([0.0, 0.5, 1.0])
    mesh = mr.MeshArgs(10, 20, 1e-7, edge, edge)
    # cells 0 .. 3 = (0,0) (1,0) (0,1) (1,1): C = [1, 1, 3, 4], S = 4, cell 1 is empty
    table = mr.Table([[1.0, 0.0], [2.0, 1.0]])
    assert (table.K, table.S, table.cells.tolist(), table.at_cells.tolist()) == (3, 4.0, [0, 2, 3], [1.0, 3.0, 4.0])
    bins = mr.spectrum([(2.0, 1.0), (8.0, 16.0, 3.0)])  # B = [1, 4], S_B = 4
    before = {f: np.arange(8, dtype=np.float64) + 100 for f in sr.F64_FIELDS}
    before.update({f: np.arange(8, dtype=np.int32) + 50 for f in ("cellx", "celly")}, dead=dead)
    # rn[slot] = (p0, p1), (d0, d1), (u0, u1)
    rn = np.array([[[0.5, 0.5], [0.25, 0.9], [0.125, 0.125]],  # slot 0: t = 0.5 < 1: cell 0; tb = 0.5 < 1: the line
                   [[1.0, 0.0], [0.5, 0.5], [0.25, 0.25]],     # slot 2: t = C_0 = C_1: not cell 1 but cell 2; tb = 1: the bin
                   [[0.5, 1.0], [0.7, 0.25], [0.75, 0.9]],     # slot 3: t = C_2: cell 3; the bin
                   [[0.25, 0.5], [0.7, 1.0], [1.0, 1.0]],      # slot 5: t = S: the last non-zero cell; tb = S_B: the last bin
                   [[0.5, 0.25], [0.1, 0.3], [0.5, 0.1]]])     # slot 7: 1 <= t = 2 < 3: cell 2; the line
    out, cell, b, guarded = mr.expected(before, dead, 5, 0.5, 99, 7, table, bins, (0.0, 0.0), mesh, rn)
    assert cell.tolist() == [0, 2, 3, 3, 2] and b.tolist() == [0, 1, 1, 1, 0]
    assert guarded.tolist() == [False, True, True, False, False]  # t on a boundary; t == S has one reading
    assert not out["dead"].any()
    # slot 2's x is its cell's upper edge and slot 3's y the mesh's: they stay in the drawn cell
    assert out["x"].tolist() == [0.25, 101.0, 0.5, 0.75, 104.0, 0.625, 106.0, 0.25]
    assert out["y"].tolist() == [0.25, 101.0, 0.5, 1.0, 104.0, 0.75, 106.0, 0.625]
    assert out["cellx"].tolist() == [10, 51, 10, 11, 54, 11, 56, 10]
    assert out["celly"].tolist() == [20, 51, 21, 21, 54, 21, 56, 21]
    assert out["energy"].tolist() == [2.0, 101.0, 12.0, 10.0, 104.0, 16.0, 106.0, 2.0]
    assert out["omega_x"][[0, 2, 3, 5, 7]].tolist() == [1.0] * 5 and out["omega_y"][[0, 2, 3, 5, 7]].tolist() == [0.0] * 5
    for f, v in (("weight", 0.5), ("dt_to_census", 1e-7), ("mfp_to_collision", 0.0)):
        assert out[f].tolist() == [v, 101.0, v, v, 104.0, v, 106.0, v], f
    # fewer than the dead: the first three, nothing else
    out, cell, _, _ = mr.expected(before, dead, 3, 0.5, 99, 7, table, bins, (0.0, 0.0), mesh, rn[:3])
    assert out["dead"].tolist() == [0, 0, 0, 0, 0, 7, 0, 1] and cell.tolist() == [0, 2, 3]
    import oracle_binding as ob
    assert tuple(mr.cpu_u([1, 4], 7, 99)[1]) == ob.generate_random_numbers(11, 99, 2)


def _one_cell(nx, ny, i, j, value=0.75):
    s = np.zeros((ny, nx))
    s[j, i] = value
    return s


def _cell_box(mesh, i, j):
    """cell (i, j) as a described source's box"""
    return (mesh.edgex[i], mesh.edgey[j], mesh.edgex[i + 1] - mesh.edgex[i], mesh.edgey[j + 1] - mesh.edgey[j])


@pytest.mark.parametrize("i, j", [(3, 7), (15, 15), (0, 0)])
def test_one_cell_mesh_is_the_described_source(i, j):
    """a mesh whose only non-zero cell is (i, j): the described source's restatement with one component
    whose box is that cell, bit for bit in all eleven fields"""
    n = 1000
    dead = (np.random.default_rng(3).random(n) < 0.4).astype(np.int32)
    mesh = _unit_mesh()
    before = dict(_junk(n), dead=dead)
    slots = sr.ranks(dead, 300)
    rn = dr.cpu_samples(slots, 5, SEED)
    desc = [dr.Component(1.0, _cell_box(mesh, i, j), BINS, THETA)]
    want, _, want_b = dr.expected(before, dead, 300, 0.75, SEED, 5, desc, mesh, rn)
    got, cell, b, guarded = mr.expected(before, dead, 300, 0.75, SEED, 5, mr.Table(_one_cell(16, 16, i, j)), BINS,
                                        THETA, mesh, rn)
    assert np.all(cell == j * 16 + i) and not guarded.any() and np.array_equal(b, want_b)
    assert not np.any(got["x"][slots] == mesh.edgex[i + 1]) and not np.any(got["y"][slots] == mesh.edgey[j + 1])
    for f in sr.FIELDS:
        assert same_bits(got[f], want[f]), f


@functools.lru_cache(maxsize=None)
def _sparse_draws():
    """a 16 x 16 mesh, 90 % zeros, zero runs at its start and its end, and 1e5 draws from it"""
    rng = np.random.default_rng(11)
    s = 1.0 - rng.random((16, 16))
    s[rng.random((16, 16)) < 0.9] = 0.0
    s.ravel()[:9] = 0.0
    s.ravel()[-21:] = 0.0
    table = mr.Table(s)
    cell, guarded = table.choose(mr.cpu_u(np.arange(100000), 0, SEED)[:, 0])
    return s, table, cell, guarded


def test_a_cell_of_strength_zero_is_never_chosen():
    s, table, cell, guarded = _sparse_draws()
    assert 10 <= table.K <= 60 and not guarded.any()
    assert np.all(s.ravel()[cell] > 0.0)
    assert cell.min() >= 9 and cell.max() < 256 - 21
    assert set(cell.tolist()) == set(table.cells.tolist())  # ... and every other one is


def test_frequencies_follow_the_strengths():
    """every non-zero cell's count within five standard deviations of its binomial mean, the bound of
    test_described_source.test_frequencies_follow_the_shares (the GPU draws the same samples, so its
    counts are the same integers)"""
    s, table, cell, _ = _sparse_draws()
    n = len(cell)
    counts = np.bincount(cell, minlength=256)
    for c in table.cells:
        p = s.ravel()[c] / table.S
        assert abs(int(counts[c]) - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p)), (c, counts[c], n * p)


@pytest.mark.parametrize("n", SIZES)
def test_the_seeds_of_the_gpu_tests_leave_no_draw_guarded(n):
    """what every GPU test below asserts with the library's samples, here with the oracle's Threefry
    for the same inputs: no t within GUARD * S of a boundary, so the exact cell can be demanded"""
    for name, _, count, seed in _calls(n):
        u0 = _cpu_u0(n, name, count, seed)
        for mesh in MESHES:
            for pattern in ("random", "exact"):
                cell, guarded = _table(mesh, pattern).choose(u0)
                assert not guarded.any(), (mesh, pattern, name, seed)
                assert np.all(_strength(mesh, pattern).ravel()[cell] > 0.0)
    # the one-cell meshes, the shard's streams and the closed form's
    assert not mr.Table(_one_cell(16, 16, 15, 15)).choose(_cpu_u0(n, "all", n, SEED))[1].any()
    if n == SIZES[0]:
        for pid_base in (0, 123456789):
            u0 = mr.cpu_u(sr.ranks(np.random.default_rng(5).random(1000) < 0.3, 1000), pid_base, SEED)[:, 0]
            assert not mr.Table(_shard_strength()).choose(u0)[1].any()
        assert not mr.Table(_closed_form_strength()).choose(mr.cpu_u(np.arange(4096), 0, 0)[:, 0])[1].any()


def test_exact_strengths_sum_exactly():
    """small integers times a power of two: numpy's sum, the restatement's S and any other order agree"""
    for mesh in MESHES:
        s = _strength(mesh, "exact")
        assert _table(mesh, "exact").S == float(s.sum()) == float(s.ravel()[::-1].sum())
        zeros = float((s == 0.0).mean())
        assert zeros > 0.99 if mesh == "one row" else 0.2 < zeros < 0.6


# ---- CPU: the ABI, the wrapper, the driver ---------------------------------------------------

def test_library_exports_the_mesh_source(tmp_path):
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_source_mesh")
    assert "neutral_hip_source_mesh" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    fields = [f[0] for f in iface.MeshSourceStats._fields_]
    assert fields == ["dead_before", "emitted", "cells_nonzero", "strength_total", "weight_emitted", "source_ms"]
    # the struct as a C compiler lays it out (the method of test_step_stats_mirror_matches_the_c_struct)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "neutral_hip.h"\n'
                   'int main(void) {\n  printf("%zu\\n", sizeof(NeutralHipMeshSourceStats));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(NeutralHipMeshSourceStats, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "layout")])
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0]) == C.sizeof(iface.MeshSourceStats) == 48
    offsets = dict(line.split() for line in lines[1:] if line.strip())
    assert sorted(offsets) == sorted(fields)
    for f in fields:
        assert getattr(iface.MeshSourceStats, f).offset == int(offsets[f]), f


_MESH = (4, 4, 0, 0, 0, 1e-7, None, None)  # (no edges: nothing gets as far as the device)


def _bin_table(iface, bins=BINS):
    return (iface.SourceBinC * len(bins))(*(iface.SourceBinC(*b) for b in bins))


def test_wrapper_argument_handling():
    from neutral_amd import interface as iface
    table = _bin_table(iface)
    call = (0x1000, THETA, table)  # (a strength nobody reads)
    with pytest.raises(ValueError):
        iface.source_mesh(None, 16, 1, 1.0, 0, *call, *_MESH)  # no store
    store = C.pointer(iface.Particle())
    for n, count, seed in ((0, 1, 0), (-5, 1, 0), (16, -1, 0), (16, 2 ** 31, 0), (16, 1, -1), (16, 1, 2 ** 64)):
        with pytest.raises(ValueError):
            iface.source_mesh(store, n, count, 1.0, seed, *call, *_MESH)
    for n, count, seed in ((16.5, 1, 0), (16, 1.5, 0), (16, 1, 0.5), (16, True, 0)):
        with pytest.raises(TypeError):
            iface.source_mesh(store, n, count, 1.0, seed, *call, *_MESH)
    with pytest.raises(TypeError):
        iface.source_mesh(store, 16, 1, 1.0, 0, np.ones((4, 4)), THETA, table, *_MESH)  # not a device pointer
    with pytest.raises(TypeError):
        iface.source_mesh(store, 16, 1, 1.0, 0, 0x1000, THETA, BINS, *_MESH)  # not a table of SourceBinC
    # the library itself: nothing to refill, nothing touched, no device needed to say so
    lib, stats = iface.library(), iface.MeshSourceStats()
    raw = (C.c_void_p(0x1000), THETA[0], THETA[1], len(table), table)
    assert lib.neutral_hip_source_mesh(None, 16, 1, 1.0, 0, *raw, *_MESH, C.byref(stats)) == 1
    assert lib.neutral_hip_source_mesh(store, 0, 1, 1.0, 0, *raw, *_MESH, None) == 1
    assert lib.neutral_hip_source_mesh(store, 16, -1, 1.0, 0, *raw, *_MESH, None) == 1
    for weight in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.neutral_hip_source_mesh(store, 16, 1, weight, 0, *raw, *_MESH, None) == 1
    assert (stats.dead_before, stats.emitted, stats.cells_nonzero, stats.strength_total) == (0, 0, 0, 0.0)
    with pytest.raises(iface.MeshSourceRefused) as refused:
        iface.source_mesh(store, 16, 1, 0.0, 0, *call, *_MESH)
    assert refused.value.code == 1 and refused.value.stats.emitted == 0
    assert issubclass(iface.MeshSourceRefused, ValueError)


def test_mesh_source_parses_its_energies_like_a_component():
    from neutral_amd import interface as iface
    source = iface.MeshSource(np.ones((4, 4)), ENERGIES)
    assert source.theta == iface.ISOTROPIC == (0.0, 2.0 * math.pi) and source.shape == (4, 4)
    assert [(b.e_lo, b.e_hi, b.share) for b in source.bin_table] == [(2.5e3, 2.5e3, 3.0), (5.0e3, 2.0e4, 1.0)]
    assert iface.MeshSource(np.ones((4, 4)), ENERGIES, theta=THETA).theta == THETA
    mine = np.ones((4, 4))
    source = iface.MeshSource(mine, ENERGIES)
    mine[1, 2] = -1.0  # the source keeps what it was given, not the caller's array
    assert np.array_equal(source.strength, np.ones((4, 4)))
    for kw in (dict(energies=[]), dict(energies=[(1.0,)]), dict(theta=(0.0,)), dict(energies=[(1.0, 1.0)] * 257)):
        with pytest.raises(ValueError):
            iface.MeshSource(**{"strength": np.ones((4, 4)), "energies": ENERGIES, **kw})


def test_check_refuses_what_the_library_does_not_look_at(make_problem, cs):
    from neutral_amd import interface as iface
    prob = make_problem("csp", nx=16, ny=12, nparticles=100, iterations=1)
    keys = cs[0]
    lo, hi = max(1.0, float(keys.min())), float(keys.max())
    good = np.ones((12, 16))
    iface.MeshSource(good, [(1.0e4, 1.0)]).check(prob, keys)
    iface.MeshSource(good, [(lo, hi, 1.0)]).check(prob, keys)
    for shape in ((16, 12), (12 * 16,), (12, 15), (1, 12, 16)):
        with pytest.raises(ValueError, match="the mesh is 12 x 16"):
            iface.MeshSource(np.ones(shape), [(1.0e4, 1.0)]).check(prob, keys)
    for energies in (((lo / 2, 1.0),), ((2 * hi, 1.0),), ((1.0e4, 2 * hi, 1.0),), ((2.0e4, 1.0e4, 1.0),),
                     ((float("nan"), 1.0),)):
        with pytest.raises(ValueError, match="leave the cross-section"):
            iface.MeshSource(good, list(energies)).check(prob, keys)
    for value in (-1.0, float("nan"), float("inf")):
        bad = good.copy()
        bad[5, 7] = value
        with pytest.raises(ValueError, match="negative or not finite"):
            iface.MeshSource(bad, [(1.0e4, 1.0)]).check(prob, keys)
    iface.MeshSource(np.zeros((12, 16)), [(1.0e4, 1.0)]).check(prob, keys)  # (the library's to refuse: S == 0)


MESH_FILE = ("# a 4 x 3 mesh\n"
             "4 3\n"
             "0 0 1.5 0   # the first row\n"
             "0 2.0e0 0 0\n"
             "\n"
             "0.25 0 0 0\n")


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("case", ["no --source", "no path", "unreadable", "not the deck's mesh", "bad number",
                                  "a header too large to hold", "bad size", "too few numbers", "too many numbers",
                                  "with --source-file", "a bad number behind a long line",
                                  "too few numbers on a long line"])
def test_driver_usage_errors(tmp_path, case):
    """(the two long lines: a row of 1200 numbers, 10 799 characters, is read as 1200 numbers and counts
    as one line, whatever buffer the reader has)"""
    from neutral_amd import decks
    nx, ny = (1200, 2) if "long line" in case else (4, 3)
    decks.write_deck("csp", str(tmp_path / "problems" / "csp.params"), nx=nx, ny=ny, nparticles=100, iterations=2)
    row = " ".join(["0.0078125", "1.25e-3"] * 600)
    assert len(row) > 2 * 4096
    path = tmp_path / "source.mesh"
    text, want = {
        "no --source": (MESH_FILE, "--source-mesh needs --source"),
        "no path": (MESH_FILE, "--source-mesh wants PATH"),
        "unreadable": (None, "Could not open the source mesh"),
        "not the deck's mesh": (MESH_FILE.replace("4 3\n", "3 4\n"), "the deck's mesh is 4 x 3"),
        "bad number": (MESH_FILE.replace("2.0e0", "2.0e0x"), "bad number"),
        "a header too large to hold": (MESH_FILE.replace("4 3\n", "2000000 2000000\n"), "the deck's mesh is 4 x 3"),
        "bad size": (MESH_FILE.replace("4 3\n", "4 three\n"), "the first line is `nx ny`"),
        "a bad number behind a long line": (f"# long rows\n1200 2\n{row}\n{row} 1x\n", "source.mesh:4: bad number 1x"),
        "too few numbers on a long line": (f"1200 2\n{row}\n{row[:-8]}\n", "too few numbers"),
        "too few numbers": (MESH_FILE.replace("0.25 0 0 0\n", "0.25 0 0\n"), "too few numbers"),
        "too many numbers": (MESH_FILE + "1\n", "more than 4 x 3 numbers"),
        "with --source-file": (MESH_FILE, "does not work with --source-file"),
    }[case]
    if text is not None:
        path.write_text(text)
    extra = {"no --source": ["--source-mesh", str(path)],
             "no path": ["--source", "5", "--source-mesh"],
             "with --source-file": ["--source", "5", "--source-mesh", str(path), "--source-file", str(path)],
             }.get(case, ["--source", "5", "--source-mesh", str(path)])
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + extra, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert want in out.stderr + out.stdout


# ---- GPU: the call alone ---------------------------------------------------------------------

class DeviceMesh:
    """a mesh of the test's own on the device: its edges, and strengths as the tests upload them"""

    def __init__(self, args: mr.MeshArgs):
        import torch
        self.args = args
        self.nx, self.ny = len(args.edgex) - 1, len(args.edgey) - 1
        self.edgex, self.edgey = (torch.from_numpy(np.ascontiguousarray(e)).cuda() for e in (args.edgex, args.edgey))
        self.kept = []

    def upload(self, strength):
        import torch
        self.kept.append(torch.from_numpy(np.ascontiguousarray(strength, dtype=np.float64)).cuda())
        return self.kept[-1].data_ptr()

    def call_args(self):
        return dict(local_nx=self.nx, local_ny=self.ny, pad=0, x_off=self.args.x_off, y_off=self.args.y_off,
                    dt=self.args.dt, edgex=self.edgex.data_ptr(), edgey=self.edgey.data_ptr())


def store_mesh(st):
    """the mesh of a Store's own problem"""
    return DeviceMesh(dr.mesh_of(st.args))


def raw(st, mesh: DeviceMesh, count, weight=1.0, seed=0, strength=None, theta=THETA, bins=BINS, table=None,
        nparticles=None, **changed):
    """the library's own call on the store of `st`: -> (return code, stats); table = (nbins, bins) as the
    library takes them, in place of `bins`"""
    lib = st.iface.library()
    stats = st.iface.MeshSourceStats()
    st.iface.set_pid_base(st.sim.pid_base)
    nbins, bin_table = table if table is not None else (len(bins), _bin_table(st.iface, bins))
    a = dict(mesh.call_args(), **changed)
    rc = lib.neutral_hip_source_mesh(
        st.sim.particles, st.n if nparticles is None else nparticles, count, weight, seed,
        C.c_void_p(strength) if strength else None, theta[0], theta[1], nbins, bin_table, a["local_nx"],
        a["local_ny"], a["pad"], a["x_off"], a["y_off"], a["dt"], a["edgex"], a["edgey"], C.byref(stats))
    return rc, stats


def _check_refilled(iface, after, before, slots, pid_base, seed, weight, table, bins, theta, mesh: mr.MeshArgs):
    """the refilled slots of `after` against the restatement, fed the library's own samples: no draw
    guarded, the exact cell for every slot; every other slot against `before` (where given), bit for
    bit; -> the flat cell of every refilled slot"""
    _, rn = iface.probe_threefry(dr.probe_rows(slots, pid_base, seed))
    n = len(after["dead"])
    dead = np.zeros(n, dtype=np.int32)
    dead[slots] = 1
    want, cell, b, guarded = mr.expected(after, dead, len(slots), weight, seed, pid_base, table, bins, theta, mesh, rn)
    assert not guarded.any(), int(guarded.sum())
    for f in ("cellx", "celly", "dead", "weight", "dt_to_census", "mfp_to_collision"):
        assert np.array_equal(after[f][slots], want[f][slots]), f
    assert not after["dead"][slots].any() and np.all(after["mfp_to_collision"][slots] == 0.0)
    line = np.array([bins[bi][0] == bins[bi][1] for bi in b], dtype=bool)
    assert np.array_equal(after["energy"][slots][line], want["energy"][slots][line])
    # the tolerances of tests/test_source.py::_check_refilled
    for f in ("x", "y", "energy"):
        assert rel(after[f][slots], want[f][slots]) < 1e-15, f
    for f in ("omega_x", "omega_y"):
        assert np.max(np.abs(after[f][slots] - want[f][slots]), initial=0.0) < 1e-15, f
    # every position inside the cell that was written, edges inclusive
    i, j = after["cellx"][slots] - mesh.x_off, after["celly"][slots] - mesh.y_off
    x, y = after["x"][slots], after["y"][slots]
    assert np.all((mesh.edgex[i] <= x) & (x <= mesh.edgex[i + 1]) & (mesh.edgey[j] <= y) & (y <= mesh.edgey[j + 1]))
    untouched = np.ones(n, dtype=bool)
    untouched[slots] = False
    for f in sr.FIELDS if before is not None else ():
        assert same_bits(np.ascontiguousarray(after[f][untouched]), np.ascontiguousarray(before[f][untouched])), f
    return cell


@gpu
@needs_gpu
@pytest.mark.parametrize("n", SIZES)
def test_one_nonzero_cell_against_the_described_source(iface, make_problem, cs, n):
    """the reference is the described source's own bits, one component whose box is the cell: all
    eleven fields and the untouched slots; a cell in the middle, the mesh's last row and column, and a
    mesh of one cell"""
    st = Store(iface, make_problem, cs, n)
    injected = st.arrays()
    own = store_mesh(st)
    single = DeviceMesh(mr.MeshArgs(0, 0, st.args.dt, np.array([0.25, 0.75]), np.array([0.125, 0.5])))
    cases = [(own, 3, 7), (own, own.nx - 1, own.ny - 1), (single, 0, 0)]
    for mesh, i, j in cases:
        strength = mesh.upload(_one_cell(mesh.nx, mesh.ny, i, j))
        desc = [dr.Component(1.0, _cell_box(mesh.args, i, j), BINS, THETA)]
        for name, mask in _patterns(n).items():
            ndead = int(mask.sum())
            for count, weight, seed in ((n, 1.0, 0), (max(ndead - 3, 1), WEIGHT, SEED)):
                killed = st.kill(injected, mask)
                rc, ds = st.raw(count, weight, seed, desc, **mesh.call_args())
                assert rc == 0
                want = st.arrays()
                st.kill(injected, mask)
                rc, stats = raw(st, mesh, count, weight, seed, strength)
                assert rc == 0, name
                m = min(count, ndead)
                assert (stats.dead_before, stats.emitted, stats.weight_emitted) == \
                    (ds.dead_before, ds.emitted, ds.weight_emitted) == (ndead, m, m * weight), name
                assert (stats.cells_nonzero, stats.strength_total) == (1, 0.75)
                after = st.arrays()
                slots = sr.ranks(killed["dead"], count)
                assert not np.any(after["x"][slots] == mesh.args.edgex[i + 1])
                assert not np.any(after["y"][slots] == mesh.args.edgey[j + 1])
                assert np.all(after["cellx"][slots] == i) and np.all(after["celly"][slots] == j)
                for f in sr.FIELDS:
                    assert same_bits(after[f], want[f]), (name, (i, j), count, f)
    print(f"n={n} source_ms described {ds.source_ms:.3f} mesh {stats.source_ms:.3f}")
    st.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("mesh_name", list(MESHES))
@pytest.mark.parametrize("n", SIZES)
def test_general_mesh_against_the_restatement(iface, make_problem, cs, n, mesh_name):
    st = Store(iface, make_problem, cs, n)
    injected = st.arrays()
    args = _mesh_args(mesh_name, st.args.dt)
    mesh = DeviceMesh(args)
    cells_by_seed = {}
    for pattern in ("random", "exact"):
        s, table = _strength(mesh_name, pattern), _table(mesh_name, pattern)
        strength = mesh.upload(s)
        for name, mask, count, seed in _calls(n):
            killed = st.kill(injected, mask)
            slots = sr.ranks(killed["dead"], count)
            rc, stats = raw(st, mesh, count, WEIGHT, seed, strength)
            assert rc == 0 and (stats.dead_before, stats.emitted) == (int(mask.sum()), count), (pattern, name)
            assert stats.weight_emitted == count * WEIGHT and stats.cells_nonzero == table.K
            if pattern == "exact":
                assert stats.strength_total == float(s.sum())  # bit for bit: the sums are exact in any order
            else:
                assert abs(stats.strength_total - table.S) <= 64 * np.finfo(float).eps * table.S
            after = st.arrays()
            cell = _check_refilled(iface, after, killed, slots, 0, seed, WEIGHT, table, BINS, THETA, args)
            assert np.all(s.ravel()[cell] > 0.0)
            if name == "random 30 %":
                cells_by_seed[pattern, seed] = cell
            if name == "random 30 %" and seed == SEED:
                # the same call on the same input: the same bits
                st.upload(killed)
                rc, again = raw(st, mesh, count, WEIGHT, seed, strength)
                assert rc == 0 and (again.emitted, again.cells_nonzero) == (count, table.K)
                assert again.strength_total == stats.strength_total
                second = st.arrays()
                for f in sr.FIELDS:
                    assert same_bits(second[f], after[f]), f
        # another seed: other cells (one slot fewer dead: the slots the two calls share)
        a, b = cells_by_seed[pattern, SEED], cells_by_seed[pattern, SEED + 1]
        shared = min(len(a), len(b))
        assert shared < 8 or np.any(a[:shared] != b[:shared])
    st.close()


def _shard_strength():
    rng = np.random.default_rng(21)
    s = 1.0 - rng.random((16, 16))
    s[rng.random((16, 16)) < 0.4] = 0.0
    return s


@gpu
@needs_gpu
def test_pid_base_moves_the_streams_and_a_shard_is_refilled(iface, make_problem, cs):
    """a store that is a shard (its own first id, its own count): its slots, its streams -- whatever
    particle count the caller names"""
    n, base = 1000, 123456789
    mask = np.random.default_rng(5).random(n) < 0.3
    s = _shard_strength()
    table = mr.Table(s)
    got = {}
    for pid_base in (0, base):
        st = Store(iface, make_problem, cs, n, pid_base=pid_base)
        killed = st.kill(st.arrays(), mask)
        slots = sr.ranks(killed["dead"], n)
        stats = st.sim.emit(n, seed=SEED, weight=2.0, source=iface.MeshSource(s, ENERGIES, theta=THETA))
        assert isinstance(stats, iface.MeshSourceStats) and stats.emitted == len(slots)
        assert stats.cells_nonzero == table.K
        after = st.arrays()
        got[pid_base] = _check_refilled(iface, after, killed, slots, pid_base, SEED, 2.0, table, BINS, THETA,
                                        dr.mesh_of(st.args))
        assert not after["dead"].any()
        st.close()
    assert np.any(got[0] != got[base])  # the same slots, other particles


def _refusals():
    nan, inf = float("nan"), float("inf")
    cases = {"count -1": dict(count=-1), "weight 0": dict(weight=0.0), "weight nan": dict(weight=nan),
             "weight inf": dict(weight=inf), "weight negative": dict(weight=-0.5), "dt 0": dict(dt=0.0),
             "dt nan": dict(dt=nan), "no edgex": dict(edgex=None), "no edgey": dict(edgey=None),
             "local_nx 0": dict(local_nx=0), "local_ny 0": dict(local_ny=0), "pad -1": dict(pad=-1),
             "no strength": dict(strength=None),
             "theta0 nan": dict(theta=(nan, 0.4)), "theta0 inf": dict(theta=(inf, 0.4)),
             "theta_width -1": dict(theta=(0.3, -1.0)), "theta_width nan": dict(theta=(0.3, nan)),
             "theta_width inf": dict(theta=(0.3, inf))}
    for name, share in (("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
        cases[f"bin share {name}"] = dict(bins=[BINS[0], (5.0e3, 2.0e4, share)])
    cases["shares that sum to inf"] = dict(bins=[(e_lo, e_hi, 1.5e308) for e_lo, e_hi, _ in BINS])
    for name, values in (("e_lo 0", (0.0, 2.0e4, 1.0)), ("e_lo negative", (-1.0, 2.0e4, 1.0)),
                         ("e_lo nan", (nan, 2.0e4, 1.0)), ("e_hi inf", (5.0e3, inf, 1.0)),
                         ("e_hi nan", (5.0e3, nan, 1.0)), ("e_hi below e_lo", (5.0e3, 2.0e3, 1.0))):
        cases[name] = dict(bins=[BINS[0], values])
    return cases


@gpu
@needs_gpu
def test_refusals_leave_the_store_untouched(iface, make_problem, cs):
    n = 5000
    st = Store(iface, make_problem, cs, n)
    killed = st.kill(st.arrays(), np.random.default_rng(6).random(n) < 0.3)
    ndead = int((killed["dead"] != 0).sum())
    mesh = store_mesh(st)
    s = _shard_strength()
    good = mesh.upload(s)

    def untouched(name):
        after = st.arrays()
        for f in sr.FIELDS:
            assert same_bits(after[f], killed[f]), (name, f)

    # found on the device, before anything is written
    for name, value in (("negative", -0.5), ("nan", float("nan")), ("inf", float("inf")), ("-inf", -float("inf"))):
        for at in ((0, 0), (9, 5), (15, 15)):
            bad = s.copy()
            bad[at] = value
            rc, stats = raw(st, mesh, 10, WEIGHT, SEED, mesh.upload(bad))
            assert rc == 1 and (stats.emitted, stats.weight_emitted) == (0, 0.0), (name, at)
            assert stats.dead_before == ndead
            untouched((name, at))
    rc, stats = raw(st, mesh, 10, WEIGHT, SEED, mesh.upload(np.zeros((16, 16))))
    assert rc == 1 and (stats.emitted, stats.cells_nonzero, stats.strength_total) == (0, 0, 0.0)
    untouched("all zero")
    rc, stats = raw(st, mesh, 10, WEIGHT, SEED, mesh.upload(np.full((16, 16), 1.0e307)))  # finite one by one
    assert rc == 1 and stats.emitted == 0 and stats.cells_nonzero == 256
    untouched("a sum that is not finite")
    # the arguments
    cases = [(name, kw) for name, kw in _refusals().items()]
    wide = (iface.SourceBinC * 257)(*([iface.SourceBinC(*BINS[0])] * 257))
    cases += [("nbins 0", dict(table=(0, _bin_table(iface)))), ("nbins 257", dict(table=(257, wide))),
              ("no bins", dict(table=(2, None)))]
    for name, kw in cases:
        rc, stats = raw(st, mesh, **{"count": 10, "weight": WEIGHT, "seed": SEED, "strength": good, **kw})
        assert rc == 1 and (stats.emitted, stats.cells_nonzero) == (0, 0), name
        untouched(name)
    # count = 0 is no refusal, and writes nothing either
    rc, stats = raw(st, mesh, 0, 1.0, SEED, good)
    assert rc == 0 and (stats.dead_before, stats.emitted) == (ndead, 0)
    assert stats.cells_nonzero == int((s > 0).sum())
    untouched("count 0")
    # ... and through the wrapper: the library's refusals, and check()'s before them
    source = iface.MeshSource(s, ENERGIES)
    with pytest.raises(iface.MeshSourceRefused) as refused:
        st.sim.emit(10, seed=SEED, weight=0.0, source=source)
    assert refused.value.code == 1
    import torch
    on_device = torch.zeros(256, dtype=torch.float64, device="cuda")
    on_device[17] = -1.0
    with pytest.raises(iface.MeshSourceRefused) as refused:  # (a device tensor is the library's to look at)
        st.sim.emit(10, seed=SEED, source=iface.MeshSource(on_device, ENERGIES))
    assert refused.value.code == 1 and refused.value.stats.dead_before == ndead
    with pytest.raises(ValueError, match="its own energies and cells"):
        st.sim.emit(10, seed=SEED, energy=1.0e4, source=source)
    with pytest.raises(ValueError, match="its own energies and cells"):
        st.sim.emit(10, seed=SEED, box=(0.1, 0.1, 0.2, 0.2), source=source)
    with pytest.raises(ValueError, match="the mesh is 16 x 16"):
        st.sim.emit(10, seed=SEED, source=iface.MeshSource(np.ones((16, 15)), ENERGIES))
    with pytest.raises(ValueError, match="the mesh is 16 x 16"):
        st.sim.inject(source=iface.MeshSource(np.ones((4, 4)), ENERGIES))
    with pytest.raises(ValueError, match="negative or not finite"):
        st.sim.emit(10, seed=SEED, source=iface.MeshSource(-s, ENERGIES))
    untouched("the wrapper")
    st.close()


@gpu
@needs_gpu
def test_an_injection_the_library_refuses_leaves_the_injected_store(iface, make_problem, cs):
    """inject(source=...) with a mesh that only the device can refuse, or a description that only
    the library does (a negative share: check() does not look at shares): the source's *Refused,
    and the store holds the normal injection, not the dead slots the call had made"""
    import torch
    prob = make_problem("csp", nx=16, nparticles=1000, iterations=1)
    sim = iface.Simulation(prob, *cs)
    sim.inject()
    injected = sim.particle_arrays()
    bad = torch.ones(256, dtype=torch.float64, device="cuda")
    bad[200] = float("nan")
    sources = [(iface.MeshSourceRefused, iface.MeshSource(strength, ENERGIES))
               for strength in (bad, torch.zeros(256, dtype=torch.float64, device="cuda"))]
    negative_share = iface.SourceDescription([iface.SourceComponent(-1.0, (0.4, 0.4, 0.1, 0.1), ENERGIES)])
    for kind, source in sources + [(iface.DescribedSourceRefused, negative_share)]:
        with pytest.raises(kind) as refused:
            sim.inject(source=source)
        assert refused.value.code == 1 and refused.value.stats.emitted == 0
        after = sim.particle_arrays()
        assert not after["dead"].any()
        for f in sr.FIELDS:
            assert same_bits(after[f], injected[f]), f
    # a numpy array on two "devices": one upload each, made once
    source = iface.MeshSource(np.ones((16, 16)), ENERGIES)
    first = source.device_pointer(sim.device)
    assert source.device_pointer("cuda") == first == source.device_pointer(torch.device("cuda", 0))
    assert len(source._uploaded) == 1
    on_host_device = iface.MeshSource(torch.ones(256, dtype=torch.float64, device="cuda"), ENERGIES)
    with pytest.raises(ValueError, match="lives on"):
        on_host_device.device_pointer(torch.device("cuda", 1))
    sim.close()


@gpu
@needs_gpu
def test_a_decomposed_store_takes_no_mesh_source(iface, make_problem, cs):
    import torch
    prob = make_problem("csp", nx=64, nparticles=1000, iterations=1)
    sim = iface.Simulation(prob, *cs, variant=2, domain=(1, 1))
    sim.inject()
    before = sim.particle_arrays()
    with pytest.raises(iface.MeshSourceRefused) as refused:
        sim.emit(10, seed=SEED, source=iface.MeshSource(np.ones((64, 64)), ENERGIES))
    assert refused.value.code == 2 and refused.value.stats.emitted == 0
    on_device = torch.ones(64 * 64, dtype=torch.float64, device="cuda")
    with pytest.raises(iface.MeshSourceRefused) as refused:
        sim.inject(source=iface.MeshSource(on_device, ENERGIES))
    assert refused.value.code == 2
    after = sim.particle_arrays()
    for f in sr.FIELDS:
        assert same_bits(after[f], before[f]), f
    sim.close()


@gpu
@needs_gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_nobody_dead_on_a_tiled_store_changes_nothing(iface, make_problem, cs, lazy, monkeypatch):
    """emitted == 0 returns 0, writes nothing and leaves the records of a tiled store valid: the next
    step pays no re-import (the method of tests/test_source.py's test of the same name: a step that
    imports waits for the device more than once on this deck, a steady one once)"""
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    strength = np.zeros((400, 400))
    strength[180:220, 180:220] = 1.0
    source = iface.MeshSource(strength, [(1.0e6, 1.0), (1.0e5, 5.0e5, 1.0)])

    def call(sim):
        stats = sim.emit(100, source=source)
        assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (0, 0, 0.0)
        assert (stats.cells_nonzero, stats.strength_total) == (1600, 1600.0)

    census_ops_support.check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call)


# ---- GPU: in a run, against the oracle -------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_mesh_source_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """The scenario of tests/test_described_source.py::test_described_source_in_a_run_against_the_oracle
    with MeshSource(sim.absorbed), the device tensor itself: what was absorbed so far is re-emitted.
    The refilled slots are checked against the restatement and handed to the oracle's arrays."""
    import oracle_binding as ob
    keys, values = cs
    absorb = (np.array(keys), 0.5 * np.array(values))  # capture = scatter / 2: p_absorb = 1/3
    prob = make_problem("csp", nx=24, nparticles=6000, iterations=11, dt=2.0e-6)
    iface.set_lazy_export(lazy)
    sim = iface.Simulation(prob, keys, values, variant=variant, roulette=ON, cs_absorb=absorb, collision_tallies=True)
    ref = ob.OracleRun(prob, keys, values, cs_absorb=absorb, roulette=ON)
    sim.inject()
    ref.inject()
    args = sr.args_of(prob)
    energies = [(2.5e3, 1.0), (1.0e4, 1.0), (5.0e3, 2.0e4, 1.0)]
    source = iface.MeshSource(sim.absorbed, energies)
    assert source.on_device and source.device_pointer() == sim.absorbed.data_ptr()

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
        absorbed = sim.absorbed_host().reshape(prob.ny, prob.nx)
        table = mr.Table(absorbed)
        stats = sim.emit(count, source=source)  # (seed: 2^63 + the last master key)
        assert (stats.dead_before, stats.emitted) == (prob.nparticles - live, len(slots))
        assert stats.cells_nonzero == table.K
        assert abs(stats.strength_total - table.S) <= 64 * np.finfo(float).eps * table.S
        assert np.array_equal(sim.absorbed_host().reshape(prob.ny, prob.nx), absorbed)  # (read, not written)
        got = sim.particle_arrays()
        cell = _check_refilled(iface, got, None, slots, 0, 2 ** 63 + tt, 1.0, table, mr.spectrum(energies),
                               mr.ISOTROPIC, dr.mesh_of(args))
        untouched = np.ones(prob.nparticles, dtype=bool)
        untouched[slots] = False
        assert np.array_equal(got["dead"][untouched], arrays["dead"][untouched])
        for f in sr.FIELDS:
            arrays[f][slots] = got[f][slots]
        return slots, live, stats, cell

    killed = sum(both_step(tt).roulette_killed for tt in range(1, 4))
    assert killed > 0  # histories have died ...
    for tt in (4, 5):  # ... and the tiled variant has moved them into its graveyard
        both_step(tt)
    ndead = int(ref.particles.as_dict()["dead"].astype(bool).sum())
    first, live, stats, cell = emit(ndead // 2, 5)
    assert 0 < stats.emitted < ndead and len(np.unique(cell)) > 4
    assert both_step(6).nprocessed == live + stats.emitted
    for tt in (7, 8):
        both_step(tt)
    ndead = int(ref.particles.as_dict()["dead"].astype(bool).sum())
    second, live, stats, _ = emit(ndead, 8)
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


# ---- GPU: a closed form ----------------------------------------------------------------------

def _closed_form_strength():
    rng = np.random.default_rng(64)
    s = rng.integers(1, 9, size=(64, 64)).astype(np.float64)
    s[rng.random((64, 64)) < 0.5] = 0.0
    s[:3, :] = 0.0
    s[:, -2:] = 0.0
    return s


@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 2])
def test_the_census_of_an_injected_mesh_in_closed_form(iface, make_problem, cs, variant):
    """inject(source=MeshSource(strength)) on the stream deck: the census counts per cell are the
    restatement's bincount, exactly; cells of zero strength hold nobody"""
    n = 4096
    s = _closed_form_strength()
    table = mr.Table(s)
    prob = make_problem("stream", nx=64, nparticles=n, iterations=1)
    sim = iface.Simulation(prob, *cs, variant=variant)
    stats = sim.inject(source=iface.MeshSource(s, [(1.0e6, 1.0)]))
    assert isinstance(stats, iface.MeshSourceStats)
    assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (n, n, float(n))
    assert (stats.cells_nonzero, stats.strength_total) == (table.K, float(s.sum()))
    _, rn = iface.probe_threefry(dr.probe_rows(np.arange(n), 0, 0))
    cell, guarded = table.choose(rn.reshape(n, 3, 2)[:, 2, 0])
    assert not guarded.any()
    count, weight, census = sim.census()
    count, weight = count.cpu().numpy(), weight.cpu().numpy()
    sim.close()
    want = np.bincount(cell, minlength=64 * 64)
    assert census.live == n and np.array_equal(count, want.astype(np.float64))
    assert np.array_equal(weight, want.astype(np.float64))  # (weight 1 each)
    assert not count[s.ravel() == 0.0].any() and int((want > 0).sum()) > table.K // 2


# ---- GPU: the driver's --source-mesh ---------------------------------------------------------

_MESH_LINE = r"^Source mesh emitted (\d+) from (\d+) cells$"


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_source_mesh_on_one_rank_and_on_two(tmp_path):
    """`neutral.hip --roulette 0.25,0.5 --source 500,0.5 --source-mesh F` (the run of
    tests/test_described_source.py::test_driver_source_file_on_one_rank_and_on_two): the mesh line
    repeats the emitted total and counts the file's non-zero cells; two ranks, both on one GPU, emit
    the same total into their shards.  Without the file the run says nothing of a mesh."""
    from neutral_amd import cs_table, decks
    from gpu_support import run_driver
    run = tmp_path / "run"
    (tmp_path / "arch").mkdir()
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    deck = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / deck))
    s = _closed_form_strength()
    text = " ".join(repr(float(v)) for v in s.ravel())  # (all of it on one line of 16 000 characters)
    assert len(text) > 3 * 4096
    (run / "source.mesh").write_text("# strengths in row order\n64 64\n" + text + "\n")
    sets = ["--roulette", "0.25,0.5"]
    for kv in ("nx=64", "ny=64", "nparticles=100001", "iterations=6", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), deck, sets + ["--source", "500,0.5"])
    assert "Source mesh" not in plain
    one = run_driver(str(run), deck, sets + ["--source", "500,0.5", "--source-mesh", "source.mesh"])
    emitted, weight, ((mesh_emitted, cells), *_) = _source_totals(one, _MESH_LINE)
    print(f"emitted {emitted} weight {weight} cells {cells}")
    assert 500 <= emitted <= 5 * 500 and emitted % 500 == 0 and weight == emitted * 0.5
    assert mesh_emitted == emitted and cells == int((s > 0).sum())
    # the first step is the deck's own injection, with the file or without it
    facets = [re.findall(r"^Facets\s+(\d+)", out, flags=re.M) for out in (plain, one)]
    assert facets[0][0] == facets[1][0] and facets[0][1:] != facets[1][1:]
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    two = run_driver(str(run), deck, sets + ["--gpus", "2", "--source", "500,0.5", "--source-mesh", "source.mesh"],
                     env)
    emitted2, weight2, ((mesh_emitted2, cells2), *_) = _source_totals(two, _MESH_LINE)
    # Up to the first call that finds a dead slot the two runs follow the same histories, and from
    # it on every call of either is served in full (test_driver_source_on_one_rank_and_on_two shows
    # it for this run): the same number of calls emit 500 each.
    facets2 = re.findall(r"^Facets\s+(\d+)", two, flags=re.M)
    assert facets2[0] == facets[1][0]
    assert (emitted2, weight2, mesh_emitted2, cells2) == (emitted, weight, emitted, cells)

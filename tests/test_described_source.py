"""The described source (include/neutral_hip.h: neutral_hip_source_described).

CPU: the numpy restatement (tests/described_source_reference.py) pinned by a hand-computed store,
by its identity with the fixed source's restatement on the degenerate description, and by the
properties and frequencies of what it emits; the ABI, the wrapper's argument handling and check(),
the driver's usage errors.  GPU: the degenerate description against the fixed source's own bits, a
general description against the restatement fed the library's samples, refusals, decomposed and
sharded stores, no re-import where nobody was dead, a run against the CPU oracle for the variants
and export modes that reach the call through different states, a closed form on the stream deck,
and the driver's --source-file on one rank and on two.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import census_ops_support
import described_source_reference as dr
import source_reference as sr
from conftest import ROOT
from census_ops_support import _junk, _patterns, _source_totals, _unit_mesh, same_bits
from gpu_support import OWN_DRIVER, gpu, iface, needs_gpu, rel, scan_tile  # noqa: F401

TALLY_L2_TOL = 1e-9  # the project's bar (tests/test_hip_parity.py)
SEED = 2 ** 63 + 17
ON = (0.25, 0.5)


def general_description():
    """three components on a unit mesh whose csp block is (0.4, 0.4, 0.2, 0.2): one overlapping the
    block, one beam, one isotropic; lines and bins mixed, no two energy ranges meet (so a slot's
    energy tells its bin) and no two boxes (so its position tells its component)"""
    return [dr.component(1.0, (0.35, 0.35, 0.125, 0.125), [(2.5e3, 3.0), (5.0e3, 2.0e4, 1.0)]),
            dr.component(2.0, (0.05, 0.5, 0.1, 0.25), [(3.0e4, 4.0e4, 3.0), (1.0e3, 1.0)], theta=(0.3, 0.4)),
            dr.component(5.0, (0.6, 0.05, 0.3, 0.2), [(1.0e4, 3.0), (5.0e4, 6.0e4, 0.5), (7.0e4, 0.5)])]


def recover(description, x, y, energy):
    """(component, bin) of every particle from where it is and what energy it has"""
    k = np.full(len(x), -1)
    b = np.full(len(x), -1)
    for i, c in enumerate(description):
        left, bottom, width, height = c.box
        inside = (x >= left) & (x <= left + width) & (y >= bottom) & (y <= bottom + height)
        assert np.all(k[inside] == -1), "boxes overlap"
        k[inside] = i
        for j, (e_lo, e_hi, _) in enumerate(c.bins):
            b[inside & (energy >= e_lo) & (energy <= e_hi)] = j
    return k, b


# ---- CPU: the restatement --------------------------------------------------------------------

def test_hand_computed_store_of_eight():
    dead = np.array([1, 0, 2, 1, 0, 7, 0, 1], dtype=np.int32)  # dead: 0, 2, 3, 5, 7
    edge = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    mesh = dr.MeshArgs(10, 20, 1e-7, edge, edge)
    # C = [1, 4], S = 4; A's bins: B = [1, 4], S_A = 4; B's one bin: S_B = 1
    desc = [dr.component(1.0, (0.0, 0.0, 0.5, 0.5), [(2.0, 1.0), (4.0, 3.0)]),
            dr.component(3.0, (0.5, 0.5, 0.5, 0.25), [(8.0, 16.0, 1.0)], theta=(0.0, 0.0))]
    before = {f: np.arange(8, dtype=np.float64) + 100 for f in sr.F64_FIELDS}
    before.update({f: np.arange(8, dtype=np.int32) + 50 for f in ("cellx", "celly")}, dead=dead)
    # rn[slot] = (p0, p1), (d0, d1), (u0, u1)
    rn = np.array([[[0.5, 0.5], [0.25, 0.9], [0.125, 0.125]],   # slot 0: t = 0.5 < 1: A; tb = 0.5 < 1: line 2
                   [[1.0, 0.0], [0.5, 0.9], [0.125, 0.25]],     # slot 2: A; tb = 1, not below 1: line 4
                   [[0.5, 1.0], [0.7, 0.5], [0.25, 0.9]],       # slot 3: t = 1, not below 1: B; 8 + 0.5 * 8
                   [[0.25, 0.5], [0.7, 1.0], [1.0, 1.0]]])      # slot 5: t = S: the last; tb = S_B: the last
    out, k, b = dr.expected(before, dead, 4, 0.5, 99, 7, desc, mesh, rn)
    assert k.tolist() == [0, 0, 1, 1] and b.tolist() == [0, 1, 0, 0]
    assert out["dead"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert out["x"].tolist() == [0.25, 101.0, 0.5, 0.75, 104.0, 0.625, 106.0, 107.0]
    assert out["y"].tolist() == [0.25, 101.0, 0.0, 0.75, 104.0, 0.625, 106.0, 107.0]
    assert out["cellx"].tolist() == [11, 51, 12, 13, 54, 12, 56, 57]
    assert out["celly"].tolist() == [21, 51, 20, 23, 54, 22, 56, 57]
    assert out["energy"].tolist() == [2.0, 101.0, 4.0, 12.0, 104.0, 16.0, 106.0, 107.0]
    assert np.allclose(out["omega_x"][[0, 2]], [0.0, -1.0], atol=1e-15)
    assert np.allclose(out["omega_y"][[0, 2]], [1.0, 0.0], atol=1e-15)
    assert out["omega_x"][[3, 5]].tolist() == [1.0, 1.0] and out["omega_y"][[3, 5]].tolist() == [0.0, 0.0]
    for f, v in (("weight", 0.5), ("dt_to_census", 1e-7), ("mfp_to_collision", 0.0)):
        assert out[f].tolist() == [v, 101.0, v, v, 104.0, v, 106.0, 107.0], f
    # count beyond the dead: all five, the last one too
    out, k, _ = dr.expected(before, dead, 9, 0.5, 99, 7, desc, mesh, np.concatenate([rn, rn[:1]]))
    assert not out["dead"].any() and len(k) == 5
    assert dr.probe_rows([1, 4], 7, 99).tolist() == [[0, 8, 99], [1, 8, 99], [2, 8, 99],
                                                     [0, 11, 99], [1, 11, 99], [2, 11, 99]]
    import oracle_binding as ob
    assert tuple(dr.cpu_samples([1, 2, 4], 7, 99)[2, 2]) == ob.generate_random_numbers(11, 99, 2)


def test_degenerate_description_is_the_fixed_source():
    """one component with the source's box, every direction and one line: the restatement of the
    fixed source, bit for bit in all eleven fields"""
    n = 1000
    dead = (np.random.default_rng(3).random(n) < 0.4).astype(np.int32)
    mesh = _unit_mesh()
    args = sr.SourceArgs(0.1, 0.1, 0.2, 0.2, 0, 0, mesh.dt, mesh.edgex, mesh.edgey, 1.0e4)
    before = dict(_junk(n), dead=dead)
    slots = sr.ranks(dead, 300)
    rn = dr.cpu_samples(slots, 5, SEED)
    want = sr.expected(before, dead, 300, 0.75, SEED, 5, args, rn[:, :2])
    got, k, b = dr.expected(before, dead, 300, 0.75, SEED, 5, dr.degenerate(args), dr.mesh_of(args), rn)
    assert not k.any() and not b.any()
    for f in sr.FIELDS:
        assert same_bits(got[f], want[f]), f


@pytest.mark.parametrize("n", [1, 2, 65, 1000, 100003])
def test_properties_of_what_is_emitted(n):
    desc = general_description()
    dead = np.ones(n, dtype=np.int32)
    out, k, b = dr.expected(dict(_junk(n), dead=dead), dead, n, 1.0, SEED, 0, desc, _unit_mesh())
    assert not out["dead"].any()
    rk, rb = recover(desc, out["x"], out["y"], out["energy"])
    assert np.array_equal(rk, k) and np.array_equal(rb, b)  # every position in its box, every energy in its bin
    for i, c in enumerate(desc):
        mine = k == i
        for j, (e_lo, e_hi, _) in enumerate(c.bins):
            if e_lo == e_hi:
                assert np.all(out["energy"][mine & (b == j)] == e_lo)  # a line is exact
        theta0, width = c.theta
        if width < 1.0:  # the beam: both cos and sin are monotone over [0.3, 0.7]
            eps = 4 * np.finfo(float).eps
            assert np.all(out["omega_x"][mine] >= math.cos(theta0 + width) - eps)
            assert np.all(out["omega_x"][mine] <= math.cos(theta0) + eps)
            assert np.all(out["omega_y"][mine] >= math.sin(theta0) - eps)
            assert np.all(out["omega_y"][mine] <= math.sin(theta0 + width) + eps)
    assert np.all(np.abs(out["omega_x"] ** 2 + out["omega_y"] ** 2 - 1.0) < 1e-15)


def test_frequencies_follow_the_shares():
    """components at 1 : 2 : 5, each with two lines at 3 : 1: every count within five standard
    deviations of its binomial mean (n and seed chosen here, with the oracle's Threefry; the GPU draws
    the same samples, so its counts are the same integers)"""
    n = 40000
    desc = [dr.component(s, (0.1 * i, 0.0, 0.05, 1.0), [(1.0e3 * (i + 1), 3.0), (2.0e4 * (i + 1), 1.0)])
            for i, s in enumerate((1.0, 2.0, 5.0))]
    u = dr.cpu_samples(np.arange(n), 0, SEED)[:, 2]
    k, b = dr.choose(desc, u)
    for i, share in enumerate((1.0, 2.0, 5.0)):
        for j, bin_share in enumerate((3.0, 1.0)):
            p = share / 8.0 * bin_share / 4.0
            count = int(((k == i) & (b == j)).sum())
            assert abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p)), (i, j, count, n * p)
        p = share / 8.0
        assert abs(int((k == i).sum()) - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


# ---- CPU: the ABI, the wrapper, the driver ---------------------------------------------------

def test_library_exports_the_described_source(tmp_path):
    from neutral_amd import interface as iface
    lib = iface.library()
    assert hasattr(lib, "neutral_hip_source_described")
    assert "neutral_hip_source_described" in iface.ABI_SYMBOLS
    assert lib.neutral_hip_abi_version() == 12
    assert [f[0] for f in iface.DescribedSourceStats._fields_] == [
        "dead_before", "emitted", "emitted_by_component", "weight_emitted", "source_ms"]
    # the three structs as a C compiler lays them out
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "neutral_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(NeutralHipSourceComponent), sizeof(NeutralHipSourceBin),\n'
                   '         sizeof(NeutralHipDescribedSourceStats));\n  return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "layout")])
    sizes = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(s) for s in sizes] == [C.sizeof(iface.SourceComponentC), C.sizeof(iface.SourceBinC),
                                       C.sizeof(iface.DescribedSourceStats)] == [64, 24, 160]


def test_description_flattens_to_the_two_tables():
    from neutral_amd import interface as iface
    desc = dr.to_interface(iface, general_description())
    assert len(desc.component_table) == 3 and len(desc.bin_table) == 7
    assert [(c.bin_first, c.bin_count) for c in desc.component_table] == [(0, 2), (2, 2), (4, 3)]
    assert [(b.e_lo, b.e_hi, b.share) for b in desc.bin_table][:3] == [
        (2.5e3, 2.5e3, 3.0), (5.0e3, 2.0e4, 1.0), (3.0e4, 4.0e4, 3.0)]
    beam = desc.component_table[1]
    assert (beam.share, beam.left, beam.bottom, beam.width, beam.height, beam.theta0, beam.theta_width) == \
        (2.0, 0.05, 0.5, 0.1, 0.25, 0.3, 0.4)
    assert (desc.component_table[0].theta0, desc.component_table[0].theta_width) == (0.0, 2.0 * math.pi)
    one = iface.SourceComponent(1.0, (0, 0, 1, 1), [(1.0, 1.0)])
    for bad in ([], [one] * 17, [iface.SourceComponent(1.0, (0, 0, 1, 1), [(1.0, 1.0)] * 257)]):
        with pytest.raises(ValueError):
            iface.SourceDescription(bad)
    for kw in (dict(box=(0, 0, 1)), dict(energies=[]), dict(energies=[(1.0,)]), dict(theta=(0.0,))):
        with pytest.raises(ValueError):
            iface.SourceComponent(**{"share": 1.0, "box": (0, 0, 1, 1), "energies": [(1.0, 1.0)], **kw})


def test_check_refuses_what_the_library_does_not_look_at(make_problem, cs):
    from neutral_amd import interface as iface
    prob = make_problem("csp", nx=16, nparticles=100, iterations=1)
    keys = cs[0]
    lo, hi = max(1.0, float(keys.min())), float(keys.max())

    def desc(box=(0.1, 0.1, 0.2, 0.2), energies=((1.0e4, 1.0),)):
        return iface.SourceDescription([iface.SourceComponent(1.0, box, list(energies))])

    desc().check(prob, keys)
    desc(box=(0.0, 0.0, 1.0, 1.0), energies=((lo, hi, 1.0),)).check(prob, keys)
    for box in ((-0.1, 0.1, 0.2, 0.2), (0.1, -0.1, 0.2, 0.2), (0.9, 0.1, 0.2, 0.2), (0.1, 0.9, 0.2, 0.2),
                (0.1, 0.1, -0.05, 0.2), (float("nan"), 0.1, 0.2, 0.2)):
        with pytest.raises(ValueError, match="leaves the mesh"):
            desc(box=box).check(prob, keys)
    for energies in (((lo / 2, 1.0),), ((2 * hi, 1.0),), ((1.0e4, 2 * hi, 1.0),), ((2.0e4, 1.0e4, 1.0),),
                     ((float("nan"), 1.0),)):
        with pytest.raises(ValueError, match="leave the cross-section"):
            desc(energies=energies).check(prob, keys)


_MESH = (4, 4, 0, 0, 0, 1e-7, None, None)  # (no mesh: nothing gets that far)


def test_wrapper_argument_handling():
    from neutral_amd import interface as iface
    desc = dr.to_interface(iface, general_description())
    with pytest.raises(ValueError):
        iface.source_described(None, 16, 1, 1.0, 0, desc, *_MESH)  # no store
    store = C.pointer(iface.Particle())
    for n, count, seed in ((0, 1, 0), (-5, 1, 0), (16, -1, 0), (16, 2 ** 31, 0), (16, 1, -1), (16, 1, 2 ** 64)):
        with pytest.raises(ValueError):
            iface.source_described(store, n, count, 1.0, seed, desc, *_MESH)
    for n, count, seed in ((16.5, 1, 0), (16, 1.5, 0), (16, 1, 0.5), (16, True, 0)):
        with pytest.raises(TypeError):
            iface.source_described(store, n, count, 1.0, seed, desc, *_MESH)
    with pytest.raises(TypeError):
        iface.source_described(store, 16, 1, 1.0, 0, general_description(), *_MESH)
    # the library itself: nothing to refill, nothing touched, no device needed to say so
    lib, stats = iface.library(), iface.DescribedSourceStats()
    tables = (3, desc.component_table, 7, desc.bin_table)
    assert lib.neutral_hip_source_described(None, 16, 1, 1.0, 0, *tables, *_MESH, C.byref(stats)) == 1
    assert lib.neutral_hip_source_described(store, 0, 1, 1.0, 0, *tables, *_MESH, None) == 1
    assert lib.neutral_hip_source_described(store, 16, -1, 1.0, 0, *tables, *_MESH, None) == 1
    for weight in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.neutral_hip_source_described(store, 16, 1, weight, 0, *tables, *_MESH, None) == 1
    with pytest.raises(iface.DescribedSourceRefused) as refused:
        iface.source_described(store, 16, 1, 0.0, 0, desc, *_MESH)
    assert refused.value.code == 1 and issubclass(iface.DescribedSourceRefused, ValueError)


SOURCE_FILE = ("# two components\n"
               "component share=1.0 xpos=0.1 ypos=0.1 width=0.2 height=0.2\n"
               "line energy=2.5e3 share=1.0\n"
               "line energy=1.0e4 share=1.0   # the deck's own\n"
               "\n"
               "component share=3.0 xpos=0.45 ypos=0.45 width=0.1 height=0.1 theta0=0.0 theta_width=1.5\n"
               "bin lo=5.0e3 hi=2.0e4 share=1.0\n")


@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
@pytest.mark.parametrize("case", ["no --source", "no path", "unreadable", "line first", "bad number",
                                  "unknown key", "unknown kind", "missing key", "no bins", "empty"])
def test_driver_usage_errors(tmp_path, case):
    path = tmp_path / "source.params"
    text, want = {
        "no --source": (SOURCE_FILE, "--source-file needs --source"),
        "no path": (SOURCE_FILE, "--source-file wants PATH"),
        "unreadable": (None, "Could not open the source file"),
        "line first": ("line energy=1.0e4 share=1.0\n" + SOURCE_FILE, "before any component"),
        "bad number": (SOURCE_FILE.replace("energy=2.5e3", "energy=2.5e3x"), "bad number"),
        "unknown key": (SOURCE_FILE.replace("energy=2.5e3", "e=2.5e3"), "unknown key"),
        "unknown kind": (SOURCE_FILE + "beam energy=1.0\n", "component, line or bin"),
        "missing key": (SOURCE_FILE.replace("hi=2.0e4 ", ""), "bin wants hi="),
        "no bins": (SOURCE_FILE + "component share=1.0 xpos=0.1 ypos=0.1 width=0.2 height=0.2\n",
                    "has no line or bin"),
        "empty": ("# nothing\n", "no component"),
    }[case]
    if text is not None:
        path.write_text(text)
    extra = {"no --source": ["--source-file", str(path)],
             "no path": ["--source", "5", "--source-file"]}.get(case, ["--source", "5", "--source-file", str(path)])
    out = subprocess.run([OWN_DRIVER, "problems/csp.params"] + extra, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert want in out.stderr + out.stdout


# ---- GPU: the call alone ---------------------------------------------------------------------

class DescribedStore(census_ops_support.Store):
    """the store with the fixed source's call and the described source's"""

    def plain(self, count, weight, seed):
        stats = self.iface.SourceStats()
        self.iface.set_pid_base(self.sim.pid_base)
        rc = self.iface.library().neutral_hip_source_particles(
            self.sim.particles, self.n, count, weight, seed, *self.sim._inject_args(), C.byref(stats))
        return rc, stats

    def raw(self, count, weight=1.0, seed=0, description=None, components=None, bins=None, nparticles=None,
            **mesh):
        """the library's own call, its tables from `description` (reference form) or as given:
        -> (return code, stats)"""
        stats = self.iface.DescribedSourceStats()
        self.iface.set_pid_base(self.sim.pid_base)
        if description is not None:
            d = dr.to_interface(self.iface, description)
            components, bins = (len(d.component_table), d.component_table), (len(d.bin_table), d.bin_table)
        a = dict(zip(("local_nx", "local_ny", "pad", "left", "bottom", "width", "height", "x_off", "y_off", "dt",
                      "edgex", "edgey", "energy"), self.sim._inject_args()))
        a.update(mesh)
        rc = self.iface.library().neutral_hip_source_described(
            self.sim.particles, self.n if nparticles is None else nparticles, count, weight, seed, *components,
            *bins, a["local_nx"], a["local_ny"], a["pad"], a["x_off"], a["y_off"], a["dt"], a["edgex"],
            a["edgey"], C.byref(stats))
        return rc, stats


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [65, scan_tile() + 1, 100003])
def test_degenerate_description_against_the_fixed_source(iface, make_problem, cs, n):
    st = DescribedStore(iface, make_problem, cs, n)
    injected = st.arrays()
    desc = dr.degenerate(st.args)
    for name, mask in _patterns(n).items():
        ndead = int(mask.sum())
        for count, weight, seed in ((n, 1.0, 0), (max(ndead - 3, 1), 0.375, SEED)):
            st.kill(injected, mask)
            rc, ps = st.plain(count, weight, seed)
            assert rc == 0
            want = st.arrays()
            st.kill(injected, mask)
            rc, stats = st.raw(count, weight, seed, desc)
            assert rc == 0, name
            m = min(count, ndead)
            assert (stats.dead_before, stats.emitted, stats.weight_emitted) == \
                (ps.dead_before, ps.emitted, ps.weight_emitted) == (ndead, m, m * weight), name
            assert list(stats.emitted_by_component) == [m] + [0] * 15
            after = st.arrays()
            for f in sr.FIELDS:
                assert same_bits(after[f], want[f]), (name, count, f)
                if seed == 0:  # ... and with injection's key and weight, injection's particles
                    assert same_bits(after[f], injected[f]), (name, f)
    print(f"n={n} source_ms plain {ps.source_ms:.3f} described {stats.source_ms:.3f}")
    st.close()


def _check_refilled(iface, after, before, slots, pid_base, seed, weight, description, mesh):
    """the refilled slots of `after` against the restatement, fed the library's own samples; every
    other slot against `before` (where given), bit for bit; -> the component of every refilled slot"""
    _, rn = iface.probe_threefry(dr.probe_rows(slots, pid_base, seed))
    n = len(after["dead"])
    dead = np.zeros(n, dtype=np.int32)
    dead[slots] = 1
    want, k, b = dr.expected(after, dead, len(slots), weight, seed, pid_base, description, mesh, rn)
    got_k, got_b = recover(description, after["x"][slots], after["y"][slots], after["energy"][slots])
    assert np.array_equal(got_k, k) and np.array_equal(got_b, b)
    for f in ("dead", "weight", "dt_to_census", "mfp_to_collision"):
        assert np.array_equal(after[f][slots], want[f][slots]), f
    assert not after["dead"][slots].any() and np.all(after["mfp_to_collision"][slots] == 0.0)
    line = np.array([description[ki].bins[bi][0] == description[ki].bins[bi][1] for ki, bi in zip(k, b)], dtype=bool)
    assert np.array_equal(after["energy"][slots][line], want["energy"][slots][line])
    # the tolerances of tests/test_source.py::_check_refilled
    for f in ("x", "y", "energy"):
        assert rel(after[f][slots], want[f][slots]) < 1e-15, f
    for f in ("omega_x", "omega_y"):
        assert np.max(np.abs(after[f][slots] - want[f][slots]), initial=0.0) < 1e-15, f
    assert np.array_equal(after["cellx"][slots], mesh.x_off + sr.find_cell(mesh.edgex, after["x"][slots]))
    assert np.array_equal(after["celly"][slots], mesh.y_off + sr.find_cell(mesh.edgey, after["y"][slots]))
    untouched = np.ones(n, dtype=bool)
    untouched[slots] = False
    for f in sr.FIELDS if before is not None else ():
        assert same_bits(np.ascontiguousarray(after[f][untouched]), np.ascontiguousarray(before[f][untouched])), f
    return k


@gpu
@needs_gpu
@pytest.mark.parametrize("n", [65, scan_tile() + 1, 100003])
def test_general_description_against_the_restatement(iface, make_problem, cs, n):
    st = DescribedStore(iface, make_problem, cs, n)
    injected = st.arrays()
    desc = general_description()
    dr.to_interface(iface, desc).check(st.prob, cs[0])
    mesh = dr.mesh_of(st.args)
    mask = np.random.default_rng(n + 2).random(n) < 0.6
    count = int(mask.sum()) - 3
    killed = st.kill(injected, mask)
    slots = sr.ranks(killed["dead"], count)
    rc, stats = st.raw(count, 0.375, SEED, desc)
    assert rc == 0 and (stats.dead_before, stats.emitted) == (int(mask.sum()), count)
    assert stats.weight_emitted == count * 0.375
    after = st.arrays()
    k = _check_refilled(iface, after, killed, slots, 0, SEED, 0.375, desc, mesh)
    by_component = np.bincount(k, minlength=16).tolist()
    assert list(stats.emitted_by_component) == by_component and sum(by_component) == count
    if n > 1000:
        assert all(c > 0 for c in by_component[:3])
    # the same call on the same input: the same bits
    st.upload(killed)
    rc, again = st.raw(count, 0.375, SEED, desc)
    assert rc == 0 and list(again.emitted_by_component) == by_component
    second = st.arrays()
    for f in sr.FIELDS:
        assert same_bits(second[f], after[f]), f
    # another seed: other positions
    st.upload(killed)
    rc, _ = st.raw(count, 0.375, SEED + 1, desc)
    other = st.arrays()
    assert rc == 0 and not np.any(other["x"][slots] == after["x"][slots])
    _check_refilled(iface, other, killed, slots, 0, SEED + 1, 0.375, desc, mesh)
    st.close()


@gpu
@needs_gpu
def test_pid_base_moves_the_streams_and_a_shard_is_refilled(iface, make_problem, cs):
    """a store that is a shard (its own first id, its own count): its slots, its streams -- whatever
    particle count the caller names"""
    n, base = 1000, 123456789
    mask = np.random.default_rng(5).random(n) < 0.3
    desc = general_description()
    got = {}
    for pid_base in (0, base):
        st = DescribedStore(iface, make_problem, cs, n, pid_base=pid_base)
        killed = st.kill(st.arrays(), mask)
        slots = sr.ranks(killed["dead"], n)
        stats = st.sim.emit(n, seed=SEED, weight=2.0, source=dr.to_interface(iface, desc))
        assert isinstance(stats, iface.DescribedSourceStats) and stats.emitted == len(slots)
        after = st.arrays()
        _check_refilled(iface, after, killed, slots, pid_base, SEED, 2.0, desc, dr.mesh_of(st.args))
        assert not after["dead"].any()
        got[pid_base] = after["x"][slots]
        st.close()
    assert not np.any(got[0] == got[base])  # the same slots, other particles


def _refusals():
    good = general_description()

    def with_component(i, **kw):
        return [c._replace(**kw) if j == i else c for j, c in enumerate(good)]

    def with_bin(values):
        return [good[0], good[1]._replace(bins=[values, good[1].bins[1]]), good[2]]

    nan, inf = float("nan"), float("inf")
    cases = {"count -1": dict(count=-1), "weight 0": dict(weight=0.0), "weight nan": dict(weight=nan),
             "weight inf": dict(weight=inf), "weight negative": dict(weight=-0.5), "dt 0": dict(dt=0.0),
             "dt nan": dict(dt=nan), "no edgex": dict(edgex=None), "no edgey": dict(edgey=None),
             "local_nx 0": dict(local_nx=0), "local_ny 0": dict(local_ny=0), "pad -1": dict(pad=-1),
             }
    for name, share in (("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
        cases[f"component share {name}"] = dict(description=with_component(1, share=share))
        cases[f"bin share {name}"] = dict(description=with_bin((3.0e4, 4.0e4, share)))
    cases["shares that sum to inf"] = dict(description=[c._replace(share=1.5e308) for c in good])
    for name, box in (("width -1", (0.05, 0.5, -1.0, 0.25)), ("height -1", (0.05, 0.5, 0.1, -1.0)),
                      ("width inf", (0.05, 0.5, inf, 0.25)), ("height nan", (0.05, 0.5, 0.1, nan)),
                      ("left nan", (nan, 0.5, 0.1, 0.25)), ("bottom inf", (0.05, inf, 0.1, 0.25))):
        cases[name] = dict(description=with_component(2, box=box))
    for name, theta in (("theta0 nan", (nan, 0.4)), ("theta0 inf", (inf, 0.4)), ("theta_width -1", (0.3, -1.0)),
                        ("theta_width nan", (0.3, nan))):
        cases[name] = dict(description=with_component(0, theta=theta))
    for name, values in (("e_lo 0", (0.0, 4.0e4, 3.0)), ("e_lo negative", (-1.0, 4.0e4, 3.0)),
                         ("e_lo nan", (nan, 4.0e4, 3.0)), ("e_hi inf", (3.0e4, inf, 3.0)),
                         ("e_hi nan", (3.0e4, nan, 3.0)), ("e_hi below e_lo", (3.0e4, 2.0e4, 3.0))):
        cases[name] = dict(description=with_bin(values))
    return cases


def _table_refusals(iface):
    """refusals of tables that no SourceDescription makes: (components, bins) as raw() takes them"""
    d = dr.to_interface(iface, general_description())
    comps, bins = d.component_table, d.bin_table

    def ranged(first, count):
        t = (iface.SourceComponentC * 3)(*comps)
        t[2].bin_first, t[2].bin_count = first, count
        return t

    many = (iface.SourceComponentC * 17)(*([comps[0]] * 17))
    wide = (iface.SourceBinC * 257)(*([bins[0]] * 257))
    return {"ncomponents 0": ((0, comps), (7, bins)), "ncomponents 17": ((17, many), (7, bins)),
            "nbins 0": ((3, comps), (0, bins)), "nbins 257": ((3, comps), (257, wide)),
            "no components": ((3, None), (7, bins)), "no bins": ((3, comps), (7, None)),
            "bin_count 0": ((3, ranged(4, 0)), (7, bins)), "bin_first -1": ((3, ranged(-1, 3)), (7, bins)),
            "range past the table": ((3, ranged(5, 3)), (7, bins)),
            "bin_count overflows": ((3, ranged(4, 2 ** 31 - 1)), (7, bins))}


@gpu
@needs_gpu
def test_refusals_leave_the_store_untouched(iface, make_problem, cs):
    n = 5000
    st = DescribedStore(iface, make_problem, cs, n)
    killed = st.kill(st.arrays(), np.random.default_rng(6).random(n) < 0.3)
    good = general_description()
    cases = [(name, {"description": good, **kw}) for name, kw in _refusals().items()]
    cases += [(name, dict(components=c, bins=b)) for name, (c, b) in _table_refusals(iface).items()]
    for name, kw in cases:
        rc, stats = st.raw(**{"count": 10, "seed": SEED, **kw})
        assert rc == 1 and stats.emitted == 0 and not any(stats.emitted_by_component), name
    # count = 0 is no refusal, and writes nothing either
    rc, stats = st.raw(0, 1.0, SEED, good)
    assert rc == 0 and (stats.dead_before, stats.emitted) == (int((killed["dead"] != 0).sum()), 0)
    after = st.arrays()
    for f in sr.FIELDS:
        assert same_bits(after[f], killed[f]), f
    # ... and through the wrapper: the library's refusal, and check()'s before it
    source = dr.to_interface(iface, good)
    with pytest.raises(iface.DescribedSourceRefused) as refused:
        st.sim.emit(10, seed=SEED, weight=0.0, source=source)
    assert refused.value.code == 1
    with pytest.raises(ValueError, match="its own energies and boxes"):
        st.sim.emit(10, seed=SEED, energy=1.0e4, source=source)
    with pytest.raises(ValueError, match="its own energies and boxes"):
        st.sim.emit(10, seed=SEED, box=(0.1, 0.1, 0.2, 0.2), source=source)
    outside = dr.to_interface(iface, [good[0]._replace(box=(0.9, 0.9, 0.2, 0.2))])
    with pytest.raises(ValueError, match="leaves the mesh"):
        st.sim.emit(10, seed=SEED, source=outside)
    with pytest.raises(ValueError, match="leaves the mesh"):
        st.sim.inject(source=outside)
    with pytest.raises(TypeError):
        st.sim.emit(10, seed=SEED, source=good)
    after = st.arrays()
    for f in sr.FIELDS:
        assert same_bits(after[f], killed[f]), f
    st.close()


@gpu
@needs_gpu
def test_a_decomposed_store_takes_no_described_source(iface, make_problem, cs):
    prob = make_problem("csp", nx=64, nparticles=1000, iterations=1)
    sim = iface.Simulation(prob, *cs, variant=2, domain=(1, 1))
    sim.inject()
    before = sim.particle_arrays()
    with pytest.raises(iface.DescribedSourceRefused) as refused:
        sim.emit(10, seed=SEED, source=dr.to_interface(iface, general_description()))
    assert refused.value.code == 2 and refused.value.stats.emitted == 0
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
    source = dr.to_interface(iface, [dr.component(1.0, (0.45, 0.45, 0.1, 0.1), [(1.0e6, 1.0), (1.0e5, 5.0e5, 1.0)])])

    def call(sim):
        stats = sim.emit(100, source=source)
        assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (0, 0, 0.0)
        assert not any(stats.emitted_by_component)

    census_ops_support.check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call)


# ---- GPU: in a run, against the oracle -------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant, lazy", [(2, False), (2, True), (0, False)])
def test_described_source_in_a_run_against_the_oracle(iface, make_problem, cs, variant, lazy):
    """The scenario of tests/test_source.py::test_source_in_a_run_against_the_oracle with a described
    source: steps, emit, steps, emit, steps; the refilled slots -- new energies among them, some born
    inside the block -- are checked against the restatement and handed to the oracle's arrays."""
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
    desc = [dr.component(1.0, (args.left, args.bottom, args.width, args.height), [(2.5e3, 1.0), (1.0e4, 1.0)]),
            dr.component(1.0, (0.45, 0.45, 0.1, 0.1), [(5.0e3, 2.0e4, 1.0)])]
    source = dr.to_interface(iface, desc)

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
        stats = sim.emit(count, source=source)  # (seed: 2^63 + the last master key)
        assert (stats.dead_before, stats.emitted) == (prob.nparticles - live, len(slots))
        got = sim.particle_arrays()
        k = _check_refilled(iface, got, None, slots, 0, 2 ** 63 + tt, 1.0, desc, dr.mesh_of(args))
        untouched = np.ones(prob.nparticles, dtype=bool)
        untouched[slots] = False
        assert np.array_equal(got["dead"][untouched], arrays["dead"][untouched])
        assert list(stats.emitted_by_component)[:2] == np.bincount(k, minlength=2).tolist()
        for f in sr.FIELDS:
            arrays[f][slots] = got[f][slots]
        return slots, live, stats

    killed = sum(both_step(tt).roulette_killed for tt in range(1, 4))
    assert killed > 0  # histories have died ...
    for tt in (4, 5):  # ... and the tiled variant has moved them into its graveyard
        both_step(tt)
    ndead = int(ref.particles.as_dict()["dead"].astype(bool).sum())
    first, live, stats = emit(ndead // 2, 5)
    assert 0 < stats.emitted < ndead and all(c > 0 for c in list(stats.emitted_by_component)[:2])
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


# ---- GPU: a closed form ----------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", [0, 2])
def test_two_lines_on_the_stream_deck_in_closed_form(iface, make_problem, cs, variant):
    """inject(source=...) with two lines at shares 1 : 3 on the collision-free deck: after one step
    the track-length spectrum holds count_g * speed(E_g) * dt / N in the group of each line"""
    from closed_form import EV_TO_J, PARTICLE_MASS
    n = 4096
    e1, e2 = 2.5e5, 1.0e6
    edges = [1.0e5, 5.0e5, 2.0e6]
    prob = make_problem("stream", nx=64, nparticles=n, iterations=1)
    desc = [dr.component(1.0, (0.45, 0.45, 0.1, 0.1), [(e1, 1.0), (e2, 3.0)])]
    sim = iface.Simulation(prob, *cs, variant=variant, spectrum=(edges, None))
    stats = sim.inject(source=dr.to_interface(iface, desc))
    assert (stats.dead_before, stats.emitted, stats.weight_emitted) == (n, n, float(n))
    assert list(stats.emitted_by_component) == [n] + [0] * 15
    a = sim.particle_arrays()
    assert not a["dead"].any() and np.all(a["weight"] == 1.0)
    counts = [int((a["energy"] == e).sum()) for e in (e1, e2)]
    assert sum(counts) == n and abs(counts[0] - n / 4) <= 5.0 * math.sqrt(n * 0.25 * 0.75)
    _, rn = iface.probe_threefry(dr.probe_rows(np.arange(n), 0, 0))
    _, b = dr.choose(desc, rn.reshape(n, 3, 2)[:, 2])
    assert np.bincount(b, minlength=2).tolist() == counts
    step = sim.step(1)
    assert step.collisions == 0 and step.nprocessed == n
    track, coll = sim.spectrum_host()
    sim.close()
    assert not coll.any()
    for g, (count, e) in enumerate(zip(counts, (e1, e2))):
        want = count * math.sqrt(2.0 * e * EV_TO_J / PARTICLE_MASS) * prob.dt / n
        print(f"variant {variant} group {g}: count {count} track {track[g]:.17e} closed form {want:.17e}")
        assert abs(track[g] - want) <= 1e-12 * want, (g, track[g], want)


# ---- GPU: the driver's --source-file ---------------------------------------------------------

_COMPONENTS = r"^Source component \d+ emitted (\d+)$"


@gpu
@needs_gpu
@pytest.mark.skipif(not os.path.exists(OWN_DRIVER), reason="neutral.hip not built")
def test_driver_source_file_on_one_rank_and_on_two(tmp_path):
    """`neutral.hip --roulette 0.25,0.5 --source 500,0.5 --source-file F` (the run of
    tests/test_source.py::test_driver_source_on_one_rank_and_on_two): the component lines sum to the
    emitted total; two ranks, both on one GPU, emit the same total into their shards.  Without the
    file the run says nothing of components."""
    from neutral_amd import cs_table, decks
    from gpu_support import run_driver
    run = tmp_path / "run"
    (tmp_path / "arch").mkdir()
    (tmp_path / "arch" / "arch.params").write_text("width 1.0\nheight 1.0\nsim_end 100.0\n")
    cs_table.write_files(str(run))
    deck = os.path.join("problems", "csp.params")
    decks.write_deck("csp", str(run / deck))
    (run / "source.params").write_text(SOURCE_FILE)
    sets = ["--roulette", "0.25,0.5"]
    for kv in ("nx=64", "ny=64", "nparticles=100001", "iterations=6", "dt=2.0e-6"):
        sets += ["--set", kv]
    plain = run_driver(str(run), deck, sets + ["--source", "500,0.5"])
    assert "Source component" not in plain
    one = run_driver(str(run), deck, sets + ["--source", "500,0.5", "--source-file", "source.params"])
    emitted, weight, by_component = _source_totals(one, _COMPONENTS)
    print(f"emitted {emitted} weight {weight} by component {by_component}")
    assert 500 <= emitted <= 5 * 500 and emitted % 500 == 0 and weight == emitted * 0.5
    assert len(by_component) == 2 and sum(by_component) == emitted
    p = 0.25  # shares 1 : 3
    assert abs(by_component[0] - emitted * p) <= 5.0 * math.sqrt(emitted * p * (1.0 - p))
    # the first step is the deck's own injection, with the file or without it
    facets = [re.findall(r"^Facets\s+(\d+)", out, flags=re.M) for out in (plain, one)]
    assert facets[0][0] == facets[1][0] and facets[0][1:] != facets[1][1:]
    env = {"NEUTRAL_HIP_SHARE_DEVICE": "1", "NEUTRAL_COMM_TIMEOUT": "60", "NEUTRAL_HIP_COMM": "host"}
    two = run_driver(str(run), deck, sets + ["--gpus", "2", "--source", "500,0.5", "--source-file",
                                             "source.params"], env)
    emitted2, weight2, by_component2 = _source_totals(two, _COMPONENTS)
    assert len(by_component2) == 2 and sum(by_component2) == emitted2
    # Up to the first call that finds a dead slot the two runs follow the same histories, and from
    # it on every call of either is served in full (test_driver_source_on_one_rank_and_on_two shows
    # it for this run): the same number of calls emit 500 each.
    facets2 = re.findall(r"^Facets\s+(\d+)", two, flags=re.M)
    assert facets2[0] == facets[1][0]
    assert (emitted2, weight2) == (emitted, weight)

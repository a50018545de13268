"""What the tests of the operations between two timesteps share (comb, the three sources, window,
census): the store they work on, the comparison bit for bit, and the small helpers of the sources'
tests.  Plain module, imported like gpu_support: every operation's own raw call stays in its test
module."""
import ctypes as C
import re

import numpy as np

import described_source_reference as dr
import source_reference as sr


def same_bits(a, b):
    """equal as raw bytes: a NaN equals itself, -0.0 does not equal 0.0"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Store:
    """a store of n injected particles on an nx x nx mesh that the test fills with arrays of its own,
    or whose slots it kills and scribbles on"""

    def __init__(self, iface, make_problem, cs, n, pid_base=0, nx=16):
        import torch
        self.iface, self.n, self.torch = iface, n, torch
        self.prob = make_problem("csp", nx=nx, nparticles=n, iterations=1)
        self.sim = iface.Simulation(self.prob, *cs, shard=(pid_base, n))
        self.sim.inject()
        self.args = sr.args_of(self.prob)

    def upload(self, arrays):
        pc = self.sim.particles.contents
        for f in sr.FIELDS:
            a = np.ascontiguousarray(arrays[f])
            self.iface.library().neutral_hip_memcpy_h2d(C.c_void_p(getattr(pc, f)), a.ctypes.data, a.nbytes)

    def kill(self, injected, mask):
        """the injected arrays with the slots of `mask` dead (words 1..3) and their other ten fields
        NaN or -1, uploaded; -> those arrays"""
        a = {f: injected[f].copy() for f in sr.FIELDS}
        for f in sr.F64_FIELDS:
            a[f][mask] = np.nan
        a["cellx"][mask] = a["celly"][mask] = -1
        a["dead"][mask] = 1 + np.flatnonzero(mask) % 3
        self.upload(a)
        return a

    def arrays(self):
        return self.sim.particle_arrays()

    def close(self):
        self.sim.close()


def check_a_call_that_writes_nothing(iface, make_problem, cs, lazy, call):
    """The record mirror's contract for an operation between two steps that has nothing to do:
    `call(sim)` -- the operation on a tiled store of 30 000 live particles after two steps, with the
    test's own assertions on its stats -- writes nothing and leaves the records valid.  The step's
    stats show a re-import: after one the plan of stream passes starts over, so a deck whose histories
    migrate through several windows (the stream deck; the caller sets NEUTRAL_WINDOW_MIN_PARTICLES=32,
    as tests/test_tiled_pipeline.py does) waits for the device more than once and enqueues other
    batches of passes.  A steady step waits once.  The last step of each run, after an invalidation,
    shows that these figures do see an import here."""
    runs = []
    for with_call in (False, True):
        prob = make_problem("stream", nx=400, nparticles=30000, iterations=4)
        iface.set_lazy_export(lazy)
        sim = iface.Simulation(prob, *cs, variant=2)
        sim.inject()
        first = sim.step(1).stats
        assert first.stream_passes > 2 and first.host_syncs > 1, "the case no longer migrates"
        sim.step(2)
        if with_call:
            call(sim)
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
    for f in sr.FIELDS:
        assert same_bits(a[f], b[f]), f
    assert (ra.nprocessed, ra.facets, ra.collisions, ra.census) == (rb.nprocessed, rb.facets, rb.collisions, rb.census)


def _patterns(n):
    """the dead slots of the described and the mesh source's stores, by name"""
    none = np.zeros(n, dtype=bool)
    out = {"all": ~none, "last slot": none.copy(), "random 30 %": np.random.default_rng(n).random(n) < 0.3}
    out["last slot"][n - 1] = True
    return out


def _unit_mesh(nx=16):
    edge = np.arange(nx + 1) / nx
    return dr.MeshArgs(0, 0, 1e-7, edge, edge)


def _junk(n):
    before = {f: np.full(n, np.nan) for f in sr.F64_FIELDS}
    before.update({f: np.full(n, -1, dtype=np.int32) for f in ("cellx", "celly")})
    return before


def _source_totals(stdout, line):
    """what the driver said of its source: (emitted, weight emitted, what every line that matches
    `line` holds, as integers: one per line, or one tuple per line of a pattern with several groups)"""
    emitted = int(re.search(r"^Source emitted (\d+)$", stdout, flags=re.M).group(1))
    weight = float(re.search(r"^Source weight emitted (\S+)$", stdout, flags=re.M).group(1))
    own = [tuple(int(v) for v in m) if isinstance(m, tuple) else int(m)
           for m in re.findall(line, stdout, flags=re.M)]
    return emitted, weight, own

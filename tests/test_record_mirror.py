"""The record mirror of the tiled variant (neutral_abi_state.h: RecordMirror), on a real MI355X
(`-m gpu`): transitions that only show under lazy export, where a step leaves the records ahead of
the caller's arrays and a write-back pending -- a partial read of one array, the owner freed with
the write-back still pending, the whole store rewritten by a second injection.

Each case is the smoke problem (csp, 64^2 cells, 8192 particles, dt = 2e-6, two steps) and is
compared bit for bit with the same steps of the over-particle kernel (variant 0), as
tests/test_tiled_pipeline.py compares."""
import numpy as np

from gpu_support import gpu, iface, needs_gpu  # noqa: F401
from test_tiled_pipeline import _run, _same

pytestmark = [gpu, needs_gpu]


def _problem(make_problem, nparticles=8192):
    return make_problem("csp", nx=64, nparticles=nparticles, iterations=2, dt=2.0e-6)


def _two_lazy_steps(iface, prob, cs):
    """a tiled store after two steps under lazy export: its write-back is pending"""
    iface.set_lazy_export(True)
    sim = iface.Simulation(prob, *cs, variant=2)
    sim.inject()
    events = [sim.step(tt) for tt in (1, 2)]
    return sim, [(r.nprocessed, r.facets, r.collisions, r.census) for r in events]


def test_reading_a_slice_of_one_array_writes_the_records_back(iface, make_problem, cs):
    """No sync call: the copy hook sees that slots 1000..2000 of `weight` lie in the mirrored store
    and writes the records back before it copies.  After that every array is current."""
    prob = _problem(make_problem)
    want = _run(iface, prob, cs, 0, 2)[0]
    try:
        sim, _ = _two_lazy_steps(iface, prob, cs)
        pc = sim.particles.contents
        middle = iface.to_host(pc.weight + 8 * 1000, 1000, np.float64)
        assert np.array_equal(middle, want["weight"][1000:2000])
        for fields, dtype in ((iface.F64_FIELDS, np.float64), (iface.I32_FIELDS, np.int32)):
            for f in fields:
                assert np.array_equal(iface.to_host(getattr(pc, f), sim.n, dtype), want[f]), f
        sim.close()
    finally:
        iface.set_lazy_export(False)


def test_freeing_the_owner_with_a_write_back_pending_leaves_the_next_store_alone(iface, make_problem, cs):
    """The pending state dies with the store: a second store of another size is imported, stepped
    and written back as if the first had never been."""
    other = _problem(make_problem, nparticles=12000)
    want = _run(iface, other, cs, 0, 2)
    try:
        first, _ = _two_lazy_steps(iface, _problem(make_problem), cs)
        first.close()
        second, events = _two_lazy_steps(iface, other, cs)
        _same(want, (second.particle_arrays(), second.tally_host(), events, None))
        second.close()
    finally:
        iface.set_lazy_export(False)


def test_injecting_again_discards_the_pending_state(iface, make_problem, cs):
    """inject() on a store whose write-back is pending rewrites the whole store: the records are
    dropped without being written back, and the arrays are the truth.  (The re-injection at the end of
    tests/test_hip_parity.py::test_tiled_variant_lazy_export_and_variant_switches, on its own.)"""
    prob = _problem(make_problem)
    want = _run(iface, prob, cs, 0, 1)
    try:
        sim, _ = _two_lazy_steps(iface, prob, cs)
        sim.inject()
        sim.zero_tally()
        r = sim.step(1)
        _same(want, (sim.particle_arrays(), sim.tally_host(), [(r.nprocessed, r.facets, r.collisions, r.census)], None))
        sim.close()
    finally:
        iface.set_lazy_export(False)

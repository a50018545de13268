"""The one reset of the library's process-global settings (tests/gpu_support.py: reset_library,
which the `iface` fixture of every GPU test calls before and after the test) does reset them."""
import numpy as np

from gpu_support import SETTINGS, gpu, iface, l2, needs_gpu, reset_library  # noqa: F401

TALLY_L2_TOL = 1e-9   # tests/test_tallies_parity.py: a weighted mesh against its reference


def _run(iface, prob, cs):
    sim = iface.Simulation(prob, *cs, variant=iface.VARIANT_TILED)
    sim.inject()
    steps = [sim.step(tt) for tt in (1, 2)]
    last = iface.last_step()
    out = dict(events=[(s.nprocessed, s.facets, s.collisions, s.census) for s in steps],
               killed=[s.stats.roulette_killed for s in steps], parts=sim.particle_arrays(),
               tally=sim.tally_host().copy(), checked=last.checked_arithmetic)
    sim.close()
    return out


@gpu
@needs_gpu
def test_reset_restores_every_default(iface, make_problem, cs, monkeypatch):
    """csp 64^2, 4096 particles, two steps of the tiled variant under windows: a run from a freshly
    reset library, then EVERY setting of the reset's table turned to something else (placeholder
    device tensors of zeros for the tallies) and reset, then the run again.  Event counts and every
    particle array equal, bit for bit; the energy tally within TALLY_L2_TOL (atomic order keeps a
    mesh from being bitwise at this size); no roulette, no checked arithmetic; and nothing was
    scored into a placeholder.  A setting added to the table without another value fails here."""
    import torch
    monkeypatch.setenv("NEUTRAL_WINDOW_MIN_PARTICLES", "32")
    prob = make_problem("csp", nx=64, nparticles=4096, iterations=2, dt=2.0e-6)
    reset_library(iface)
    first = _run(iface, prob, cs)
    placeholders = []

    def placeholder():
        placeholders.append(torch.zeros(4 * prob.nx * prob.ny, dtype=torch.float64, device="cuda"))
        return placeholders[-1]

    for name, _, to_something_else in SETTINGS:
        assert callable(to_something_else), name
        to_something_else(iface, placeholder)
    assert len(placeholders) >= 7
    reset_library(iface)
    again = _run(iface, prob, cs)
    assert again["events"] == first["events"] and sum(e[1] for e in first["events"]) > 0
    assert again["killed"] == first["killed"] == [0, 0]
    for f in first["parts"]:
        assert np.array_equal(again["parts"][f], first["parts"][f]), f
    print(f"energy tally L2 {l2(again['tally'], first['tally']):.3e}")
    assert l2(again["tally"], first["tally"]) <= TALLY_L2_TOL
    assert first["checked"] == 0 and again["checked"] == 0
    for t in placeholders:
        assert not t.any().item()

"""source_ms of the plain source and the described source on a store with every slot dead."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from neutral_amd import cs_table, decks, host  # noqa: E402
from neutral_amd import interface as iface  # noqa: E402

keys, values = cs_table.load()
SEED = 2 ** 63 + 5


def descriptions(prob):
    box = (prob.local_particle_left_off, prob.local_particle_bottom_off, prob.local_particle_width,
           prob.local_particle_height)
    degenerate = iface.SourceDescription([iface.SourceComponent(1.0, box, [(prob.initial_energy, 1.0)])])
    comps = []
    for k in range(16):
        energies = []
        for b in range(16):
            e = 1.0e3 * (1 + 16 * k + b)
            energies.append((e, 1.0) if b % 2 else (e, e + 500.0, 1.0))
        comps.append(iface.SourceComponent(1.0 + k % 3, (0.05 * k, 0.05 * k, 0.2, 0.2), energies,
                                           theta=(0.1 * k, 0.5) if k % 2 else (0.0, 2.0 * np.pi)))
    return {"degenerate": degenerate, "16 x 16 bins": iface.SourceDescription(comps)}


with tempfile.TemporaryDirectory() as tmp:
    for n in (1_000_000, 10_000_000):
        deck = decks.write_deck("csp", os.path.join(tmp, f"csp{n}.params"), nx=256, ny=256, nparticles=n,
                                iterations=1)
        prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
        sim = iface.Simulation(prob, keys, values, device=0)
        sim.inject()
        descs = descriptions(prob)
        for d in descs.values():
            d.check(prob, keys)
        dead = sim.particles.contents.dead

        def kill():
            iface.library().neutral_hip_memset(C.c_void_p(dead), 1, 4 * n)

        def run(name):
            kill()
            if name == "plain":
                s = sim.emit(n, seed=SEED)
            else:
                s = sim.emit(n, seed=SEED, source=descs[name])
            assert s.emitted == n, (name, s.emitted)
            return s

        names = ["plain"] + list(descs)
        for name in names:  # warm-up: the workspace grows, the kernels load
            run(name)
        for rep in range(3):
            for name in names:
                s = run(name)
                extra = "" if name == "plain" else f" by component {list(s.emitted_by_component)[:4]}..."
                print(f"n={n} run {rep} {name:>14}: source_ms {s.source_ms:.4f}{extra}", flush=True)
        sim.close()

"""source_ms of the mesh source and of the described source with one component, on a store of 1e7
slots with every slot dead and a 400 x 400 mesh.  The library is the one NEUTRAL_HIP_LIB names (a
build with -DNEUTRAL_MESH_SOURCE_COARSE=0 or =1), else the one as built."""
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
N, NX = 10_000_000, 400

with tempfile.TemporaryDirectory() as tmp:
    deck = decks.write_deck("csp", os.path.join(tmp, "csp.params"), nx=NX, ny=NX, nparticles=N, iterations=1)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    sim = iface.Simulation(prob, keys, values, device=0)
    sim.inject()
    energies = [(prob.initial_energy, 1.0)]
    rng = np.random.default_rng(400)
    full = 1.0 - rng.random((NX, NX))
    sparse = np.where(rng.random((NX, NX)) < 0.9, 0.0, full)
    one = np.zeros((NX, NX))
    one[200, 200] = 1.0
    box = (prob.local_particle_left_off, prob.local_particle_bottom_off, prob.local_particle_width,
           prob.local_particle_height)
    sources = {"described, one component": iface.SourceDescription([iface.SourceComponent(1.0, box, energies)]),
               "mesh, every cell": iface.MeshSource(full, energies),
               "mesh, 10 % of the cells": iface.MeshSource(sparse, energies),
               "mesh, one cell": iface.MeshSource(one, energies)}
    dead = sim.particles.contents.dead

    def run(name):
        iface.library().neutral_hip_memset(C.c_void_p(dead), 1, 4 * N)
        s = sim.emit(N, seed=SEED, source=sources[name])
        assert s.emitted == N, (name, s.emitted)
        return s

    for name in sources:  # warm-up: the workspace grows, the kernels load, the meshes are uploaded
        run(name)
    print(f"library {os.path.relpath(iface.LIB_PATH, ROOT)}", flush=True)
    for rep in range(3):
        for name in sources:
            s = run(name)
            extra = f" K {s.cells_nonzero}" if name.startswith("mesh") else ""
            print(f"n={N} run {rep} {name:>26}: source_ms {s.source_ms:.4f}{extra}", flush=True)
    sim.close()

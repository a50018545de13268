"""census_ms and window_ms of the blocks calls beside the plain ones, in one process: a 400 x 400
mesh, a store of 1e7 slots of which 7e6 are live, the live ones in random cells, weights a factor
times 0.5 (the factors of tests/test_window.py).  For every coarse mesh of COARSE, three timed calls
per form:
    census            the census tally
    window, zeros     the window with bounds of 0.0 everywhere: the classification pass and the
                      scans, nothing to write -- the cost of reading the store and of the division
The forms:
    blocks, LDS       neutral_hip_census_tally_blocks as shipped (stats.privatised says whether the
                      pass did keep its bins in LDS: above the cap it is the global form)
    blocks, global    the same with NEUTRAL_CENSUS_LDS_BINS=0: two global atomics per live slot
    plain, virtual    neutral_hip_census_tally / neutral_hip_window_particles on the uploaded virtual
                      store (cellx div block_x, celly div block_y) with the coarse mesh: what a caller
                      had to do before, and the only lines that a library without the blocks calls
                      (the parent commit's) gives
Every time is the library's HIP-event time of the call's kernels.  The library is the one
NEUTRAL_HIP_LIB names, else the one as built.  Arguments: the number of timed calls per line
(default 5)."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from neutral_amd import cs_table, decks, host  # noqa: E402
from neutral_amd import interface as iface  # noqa: E402

import torch  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
NX = 400
N = 10_000_000
SEED = iface.WINDOW_SEED_BASE + 7
FACTORS = [0.1, 0.5, 0.999, 1.0, 1.5, 2.0, np.nextafter(2.0, 3.0), 2.5, 3.7, 4.0, 9.3, 100.0, 1e3]
F64 = ("x", "y", "omega_x", "omega_y", "energy", "weight", "dt_to_census", "mfp_to_collision")
# (block_x, block_y): 1, 64, 4000 and 4096 bins (64 x 64 does not divide 400: 50 x 80 is the nearest
# under the cap, and 4096 = 64 x 64 comes from a call that names a mesh of 384 x 384 -- the cells are
# kept inside it), 6400 bins: over the cap; (1, 1): the transport mesh itself, 160 000 bins
COARSE = [(400, 400, NX), (50, 50, NX), (8, 5, NX), (6, 6, 384), (5, 5, NX), (1, 1, NX)]
blocks_built = hasattr(iface.library(), "neutral_hip_census_tally_blocks")
keys, values = cs_table.load()
lib = iface.library()


def timed(label, what, call):
    ms = []
    for rep in range(REPS + 1):  # (the first: the workspace grows, the kernels load)
        t = call()
        if rep:
            ms.append(t)
    line = dict(label, what=what, median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms), ms=ms)
    print(json.dumps(line), flush=True)


with tempfile.TemporaryDirectory() as tmp:
    deck = decks.write_deck("csp", os.path.join(tmp, "csp.params"), nx=NX, ny=NX, nparticles=N, iterations=1)
    prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
    sim = iface.Simulation(prob, keys, values, device=0)
    sim.inject()
    rng = np.random.default_rng(N)
    a = {f: rng.random(N) for f in F64}
    a["cellx"] = rng.integers(0, NX, N).astype(np.int32)
    a["celly"] = rng.integers(0, NX, N).astype(np.int32)
    a["dead"] = np.zeros(N, dtype=np.int32)
    a["dead"][rng.choice(N, 3_000_000, replace=False)] = 1
    live = a["dead"] == 0
    a["weight"] = np.where(live, rng.choice(FACTORS, size=N) * 0.5, np.nan)
    pc = sim.particles.contents

    def upload(cellx, celly):
        for f in F64 + ("cellx", "celly", "dead"):
            v = np.ascontiguousarray({"cellx": cellx, "celly": celly}.get(f, a[f]))
            lib.neutral_hip_memcpy_h2d(C.c_void_p(getattr(pc, f)), v.ctypes.data, v.nbytes)

    iface.set_pid_base(sim.pid_base)
    for bx, by, mesh in COARSE:
        cellx, celly = a["cellx"] % mesh, a["celly"] % mesh
        cnx, cny = -(-mesh // bx), -(-mesh // by)
        bins = cnx * cny
        out = torch.empty(2 * bins, dtype=torch.float64, device=sim.device)
        zeros = torch.zeros(bins, dtype=torch.float64, device=sim.device)
        label = dict(library=os.path.relpath(iface.LIB_PATH, ROOT), n=N, live=int(live.sum()), block=[bx, by],
                     mesh=mesh, bins=bins)
        if blocks_built:
            upload(cellx, celly)
            for form, limit in (("blocks, LDS", None), ("blocks, global", "0")):
                os.environ.pop("NEUTRAL_CENSUS_LDS_BINS", None)
                if limit is not None:
                    os.environ["NEUTRAL_CENSUS_LDS_BINS"] = limit
                stats = iface.census_tally_blocks(sim.particles, N, mesh, mesh, (bx, by), None, out)[2]
                timed(dict(label, form=form, privatised=int(stats.privatised)), "census",
                      lambda: iface.census_tally_blocks(sim.particles, N, mesh, mesh, (bx, by), None, out)[2].census.census_ms)
            os.environ.pop("NEUTRAL_CENSUS_LDS_BINS", None)
            timed(dict(label, form="blocks"), "window, zeros",
                  lambda: iface.window_particles_blocks(sim.particles, N, mesh, mesh, (bx, by), None, zeros.data_ptr(),
                                                        2.0, 1.5, 5, SEED).window.window_ms)
        upload((cellx // bx).astype(np.int32), (celly // by).astype(np.int32))
        timed(dict(label, form="plain, virtual"), "census",
              lambda: iface.census_tally(sim.particles, N, cnx, cny, out)[2].census_ms)
        timed(dict(label, form="plain, virtual"), "window, zeros",
              lambda: iface.window_particles(sim.particles, N, cnx, cny, zeros.data_ptr(), 2.0, 1.5, 5, SEED).window_ms)
    sim.close()

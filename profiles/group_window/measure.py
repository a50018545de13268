"""census_ms and window_ms of the grouped calls beside the plain ones, in one process: a 400 x 400
mesh, stores of 1e6 and 1e7 slots, G = 1, 8 and 64.  The store is the same for every call: 30 % of
the slots dead, the live ones in random cells, energies log-uniform over [1e-2, 1e8) -- the span of
every set of edges, so nobody is outside --, weights a factor times the bound of the slot's own bin
(the factors of tests/test_window.py: on, beside and far from the bounds of upper_ratio 2).  Three
timed calls per form:
    census            the census tally
    window, zeros     the window with bounds of 0.0 everywhere: the classification pass and the
                      scans, nothing to write -- the cost of reading the store
    window, bounds    the window with random bounds {0, 0.25, 0.5, 1} per bin, on the store
                      uploaded afresh before every call
Every time is the library's HIP-event time of the call's kernels.  The library is the one
NEUTRAL_HIP_LIB names, else the one as built; one that lacks the grouped calls (the parent commit's)
gives the plain lines alone.  Arguments: the number of timed calls per line (default 5)."""
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
SEED = iface.WINDOW_SEED_BASE + 7
FACTORS = [0.1, 0.5, 0.999, 1.0, 1.5, 2.0, np.nextafter(2.0, 3.0), 2.5, 3.7, 4.0, 9.3, 100.0, 1e3]
F64 = ("x", "y", "omega_x", "omega_y", "energy", "weight", "dt_to_census", "mfp_to_collision")
grouped_built = hasattr(iface.library(), "neutral_hip_window_particles_groups")
keys, values = cs_table.load()
lib = iface.library()
results = []


def make_store(n, rng):
    a = {f: rng.random(n) for f in F64}
    a["energy"] = np.clip(10.0 ** rng.uniform(-2.0, 8.0, n), 1.0e-2, np.nextafter(1.0e8, 0.0))
    a["cellx"] = rng.integers(0, NX, n).astype(np.int32)
    a["celly"] = rng.integers(0, NX, n).astype(np.int32)
    a["dead"] = (rng.random(n) < 0.3).astype(np.int32)
    a["factor"] = rng.choice(FACTORS, size=n)
    return a


def measure(label, census, window, upload):
    """census() -> stats; window(zeros: bool) -> stats"""
    rows = {"census": [], "window, zeros": [], "window, bounds": []}
    for rep in range(REPS + 1):  # (the first: the workspace grows, the kernels load)
        upload()
        c = census()
        z = window(True)
        w = window(False)
        if rep:
            rows["census"].append(c.census_ms)
            rows["window, zeros"].append(getattr(z, "window", z).window_ms)
            rows["window, bounds"].append(getattr(w, "window", w).window_ms)
    for what, ms in rows.items():
        line = dict(label, what=what, median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms), ms=ms)
        results.append(line)
        print(json.dumps(line), flush=True)


for n in (1_000_000, 10_000_000):
    with tempfile.TemporaryDirectory() as tmp:
        deck = decks.write_deck("csp", os.path.join(tmp, "csp.params"), nx=NX, ny=NX, nparticles=n, iterations=1)
        prob = host.setup_problem(deck, decks.ARCH_WIDTH, decks.ARCH_HEIGHT)
        sim = iface.Simulation(prob, keys, values, device=0)
        sim.inject()
        rng = np.random.default_rng(n)
        a = make_store(n, rng)
        live = a["dead"] == 0
        pc = sim.particles.contents

        def upload(weight):
            for f in F64 + ("cellx", "celly", "dead"):
                v = np.ascontiguousarray(weight if f == "weight" else a[f])
                lib.neutral_hip_memcpy_h2d(C.c_void_p(getattr(pc, f)), v.ctypes.data, v.nbytes)

        for ngroups in (0, 1, 8, 64) if grouped_built else (0,):  # (0: the plain calls)
            meshes = max(ngroups, 1)
            edges = np.geomspace(1.0e-2, 1.0e8, meshes + 1)
            group = np.clip(np.searchsorted(edges, a["energy"], side="right") - 1, 0, meshes - 1)
            lower = rng.choice([0.0, 0.25, 0.5, 1.0], size=(meshes, NX, NX), p=[0.1, 0.3, 0.3, 0.3])
            w_lo = lower[group, a["celly"], a["cellx"]]
            weight = np.where(live, np.where(w_lo > 0.0, a["factor"] * w_lo, a["factor"]), np.nan)
            d_lower = torch.from_numpy(lower.ravel()).to(sim.device)
            d_zeros = torch.zeros_like(d_lower)
            out = torch.empty(2 * meshes * NX * NX, dtype=torch.float64, device=sim.device)
            iface.set_pid_base(sim.pid_base)
            if ngroups == 0:
                census = lambda: iface.census_tally(sim.particles, n, NX, NX, out)[2]  # noqa: E731
                window = lambda zeros: iface.window_particles(  # noqa: E731
                    sim.particles, n, NX, NX, (d_zeros if zeros else d_lower).data_ptr(), 2.0, 1.5, 5, SEED)
            else:
                census = lambda: iface.census_tally_groups(sim.particles, n, NX, NX, edges, out)[2]  # noqa: E731
                window = lambda zeros: iface.window_particles_groups(  # noqa: E731
                    sim.particles, n, NX, NX, edges, (d_zeros if zeros else d_lower).data_ptr(), 2.0, 1.5, 5, SEED)
            label = dict(library=os.path.relpath(iface.LIB_PATH, ROOT), n=n, form="plain" if ngroups == 0 else "grouped",
                         G=ngroups, live=int(live.sum()))
            measure(label, census, window, lambda: upload(weight))
            if ngroups:
                assert census().outside == 0
        sim.close()

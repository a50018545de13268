"""What the GPU tests share: the markers, the one reset of the library's process-global settings
and the `iface` fixture built on it, the error measures, the small table and tile helpers, and
the runner of the project's own driver, neutral.hip.  Plain module: a test module imports what it
uses, the fixture included (`from gpu_support import iface  # noqa: F401`)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, gpu_available

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not gpu_available(), reason="needs a GPU")

OWN_DRIVER = os.path.join(ROOT, "neutral_amd", "host", "neutral.hip")


# ---- the library's process-global settings ----------------------------------------------------

def _decompose_1x1(interface):
    """a grid of one block on one rank: the only decomposition a process without ranks may name"""
    xo, yo, lx, ly = (C.c_int() for _ in range(4))
    assert interface.library().neutral_hip_set_decomposition(1, 1, 64, 64, C.byref(xo), C.byref(yo), C.byref(lx),
                                                             C.byref(ly)) == 0


# One line per process-global setting of include/neutral_hip.h: its name, the call that puts it
# back to the library's default (quiet apart: on, as every test wants it), and a call that sets
# it to something else, given a function that makes placeholder device tensors of zeros.
# A NEW neutral_hip_set_* GETS A LINE HERE, and with it every test starts and ends at its default
# (tests/test_gpu_support.py walks this table).  Not here: the device, the stream and the tests
# file, which every Simulation and every caller of validate() names itself; the automatic
# sharding, which inject() sets; the source box, which goes with the decomposition.
SETTINGS = [
    ("quiet", lambda i: i.set_quiet(True), lambda i, t: i.set_quiet(False)),
    ("lazy export", lambda i: i.set_lazy_export(False), lambda i, t: i.set_lazy_export(True)),
    ("arithmetic", lambda i: i.set_arithmetic(i.ARITH_AUTO), lambda i, t: i.set_arithmetic(i.ARITH_CHECKED)),
    ("stream queues", lambda i: i.set_stream_queues(False), lambda i, t: i.set_stream_queues(True)),
    ("scalar flux", lambda i: i.library().neutral_hip_set_scalar_flux_tally(None),
     lambda i, t: i.library().neutral_hip_set_scalar_flux_tally(C.c_void_p(t().data_ptr()))),
    ("collision tallies", lambda i: i.set_collision_tallies(None, None),
     lambda i, t: i.set_collision_tallies(t(), t())),
    ("current", lambda i: i.set_current_tally(None, None), lambda i, t: i.set_current_tally(t(), t())),
    ("outflow", lambda i: i.set_outflow_tally(None), lambda i, t: i.set_outflow_tally(t())),
    ("spectrum", lambda i: i.set_spectrum_tally(None), lambda i, t: i.set_spectrum_tally([0.5, 1.0e3, 2.0e6], None, t())),
    ("roulette", lambda i: i.set_roulette(0.0, 0.0), lambda i, t: i.set_roulette(0.25, 0.5)),
    ("pid base", lambda i: i.set_pid_base(0), lambda i, t: i.set_pid_base(12345)),
    ("decomposition", lambda i: i.library().neutral_hip_clear_decomposition(), lambda i, t: _decompose_1x1(i)),
    ("variant", lambda i: i.set_variant(i.VARIANT_OVER_PARTICLE), lambda i, t: i.set_variant(i.VARIANT_EVENT_SORTED)),
]


def reset_library(interface):
    """every process-global setting of the library back to its default"""
    for _, to_default, _ in SETTINGS:
        to_default(interface)


@pytest.fixture()
def iface():
    """neutral_amd.interface with the library at its defaults, before the test and after it"""
    from neutral_amd import interface
    reset_library(interface)
    yield interface
    reset_library(interface)


# ---- error measures ---------------------------------------------------------------------------

def rel(a, b):
    """the largest elementwise relative deviation of a from b"""
    d = np.abs(a - b)
    s = np.maximum(np.abs(b), 1e-300)
    return float(np.max(d / s)) if a.size else 0.0


def l2(a, b):
    """relative L2 of a against b; absolute where b is all zero"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    norm = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / norm) if norm > 0.0 else float(np.linalg.norm(a - b))


def l2_of_nonzero(a, b):
    """relative L2 of a against b with no way out for a reference that is all zero (nan: fails)"""
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


# ---- tables, tiles ------------------------------------------------------------------------------

def third_absorb(cs):
    """capture = scatter / 2: p_absorb = 1/3, the weights are no powers of two"""
    return cs[0].copy(), cs[1] * 0.5


def zero_capture(cs):
    """A capture table of zeros: p_absorb = 0, every collision scatters, every weight stays 1."""
    return cs[0].copy(), np.zeros_like(cs[1])


def scan_tile():
    """elements per workgroup of the scans of comb, source and window, from the kernels' own constants"""
    text = open(os.path.join(ROOT, "neutral_amd", "csrc", "neutral_kernels.h")).read()
    return int(re.search(r"constexpr int kCombBlock = (\d+);", text).group(1)) * \
        int(re.search(r"constexpr int kCombItems = (\d+);", text).group(1))


def scan_sizes():
    """the store sizes at which those scans take another path"""
    tile = scan_tile()
    return [1, 2, 63, 64, 65, 1000,
            tile - 1, tile, tile + 1,  # one workgroup's tile; tile + 1: the first level of tile sums
            100003,
            tile * tile + 1]           # the second level


def allowed_tile(requested, nx, ny, nparticles):
    """With the flux's code (and the current's, the outflow's) several windows share the LDS:
    tiles of at most 64 cells; a request that does not fit is served with the choice by particle
    density, capped the same way."""
    if requested <= 64:
        return requested
    density = nparticles / (nx * ny)
    by_density = 16 if density >= 8.0 else 32 if density >= 2.0 else 64 if density >= 0.5 else 128
    return min(by_density, 64)


# ---- the project's own driver -------------------------------------------------------------------

class DriverOutput(str):
    """the driver's stdout; what it wrote to stderr rides along as .stderr"""
    stderr = ""


def run_driver(run_dir, rel_deck, extra, env_extra=None):
    """neutral.hip on the deck `rel_deck` (relative to run_dir) with the arguments `extra` and the
    environment changed by `env_extra`; asserts that it ended well; -> DriverOutput"""
    env = dict(os.environ)
    env.update(env_extra or {})
    out = subprocess.run([OWN_DRIVER, rel_deck] + list(extra), cwd=run_dir, capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    stdout = DriverOutput(out.stdout)
    stdout.stderr = out.stderr
    return stdout


def untimed_lines(stdout):
    """stdout without the lines that carry a wall-clock time or a rate"""
    timed = ("Step time", "Wallclock", "Final Wallclock", "Facet Events / s",
             "Collision Events / s", "Particle-steps / s", "Final global_energy_tally")
    return [ln for ln in stdout.splitlines() if not ln.startswith(timed)]

"""The arithmetic policy's divisions and roots (neutral_amd/csrc/neutral_device.h) on operands that
sit on rounding boundaries, on a real MI355X (`-m gpu`).

The probes (include/neutral_hip.h: neutral_hip_probe_policy_quotient / _root) evaluate every
operand with the device functions the kernels call, in both instantiations, and report the raw
v_rcp_f64 / v_rsq_f64 seeds.  Checked here:
  * the checked forms are IEEE: numpy's bits on the hard operands of tests/hard_operands.py,
    on random operands, on special values and on the edges of the plain ranges;
  * the fast forms are the sequences their comments describe: the host's exact emulation of
    one Newton / Goldschmidt step and the residual correction, started from the device's own
    seed, bit for bit -- and within one ulp of IEEE;
  * the two-step sequences, from the same seeds, are IEEE on every case."""
import numpy as np
import pytest

import hard_operands as ho
from gpu_support import gpu, needs_gpu

pytestmark = [gpu, needs_gpu]

EV_TO_J = 1.60217646e-19
PARTICLE_MASS = 1.674927471213e-27


@pytest.fixture(scope="module")
def probes():
    """the interface module, for its probes alone: they read no setting of the library"""
    from neutral_amd import interface
    return interface


def _differ(got, want):
    """where the bits differ (any NaN equals any NaN)"""
    return ~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want)))


def _ulps(got, want):
    return np.abs(got.view(np.int64) - want.view(np.int64))


def _edges(powers):
    v = np.ldexp(1.0, np.array(powers, dtype=np.int32))
    return np.concatenate([v, np.nextafter(v, 0.0), np.nextafter(v, np.inf)])


SPECIAL = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072009e-308,
                                    1e-310, 1.0, -1.0, 3.0, 1.7976931348623157e308]),
                          _edges([-500, -300, 300, 500, -1022, 1023])])


def _random_pairs(n, seed):
    """the kind of operands test_hip_parity.py divides: ordinary and 2 - 2^-k mantissas"""
    rng = np.random.default_rng(seed)
    def doubles(lo, hi):
        mant = np.where(rng.integers(0, 4, n) == 0, 2.0 - np.ldexp(1.0, -rng.integers(0, 52, n)), rng.random(n) + 1.0)
        return mant * np.ldexp(1.0, rng.integers(lo, hi, n).astype(np.int32))
    return doubles(-299, 299), doubles(-299, 299)


def _quotient_cases():
    a_h, b_h, _ = ho.division_cases()
    a_r, b_r = _random_pairs(200_000, 11)
    ordinary = np.array([1.0, 3.0, 0.1, 1e8, 1e-6, 2.0 ** 52 - 1.0])
    sa, sb = np.meshgrid(np.concatenate([SPECIAL, ordinary]), np.concatenate([SPECIAL, ordinary]))
    return (np.concatenate([a_h, a_r, sa.ravel()]), np.concatenate([b_h, b_r, sb.ravel()]),
            np.concatenate([np.ones(a_h.size, bool), np.zeros(a_r.size + sa.size, bool)]))


def _plain(v):
    m = np.abs(v)
    return (m >= 2.0 ** -300) & (m < 2.0 ** 300)


def _hard_speed_energies(x):
    """energies E whose argument 2 E eV / m (as numpy and the kernels compute it) is a hard x"""
    x = x[(x >= 2.0 ** -74) & (x < 2.0 ** 127)]
    e0 = x * PARTICLE_MASS / (2.0 * EV_TO_J)
    found = []
    for k in range(-3, 4):
        e = e0.copy()
        for _ in range(abs(k)):
            e = np.nextafter(e, np.inf if k > 0 else 0.0)
        hit = (2.0 * e * EV_TO_J) / PARTICLE_MASS == x
        found.append(e[hit])
    return np.unique(np.concatenate(found))


def _root_cases():
    x_h, _ = ho.sqrt_cases()
    rng = np.random.default_rng(12)
    n = 200_000
    mant = np.where(rng.integers(0, 3, n) == 0, 2.0 - np.ldexp(1.0, -rng.integers(0, 52, n)), rng.random(n) + 1.0)
    x_r = np.concatenate([mant * np.ldexp(1.0, rng.integers(-499, 499, n).astype(np.int32)),
                          1.0 - rng.random(n // 4) ** 2, 1.0 + rng.random(n // 4) * 0.04])
    x = np.concatenate([x_h, x_r, SPECIAL, -np.abs(SPECIAL[np.isfinite(SPECIAL)]) - 1.0])
    hard = np.concatenate([np.ones(x_h.size, bool), np.zeros(x.size - x_h.size, bool)])
    e_h = _hard_speed_energies(x_h)
    e_r = 1.0e-2 * 2.0 ** (rng.random(n) * 33.2)
    e = np.concatenate([e_h, e_r])
    e = np.resize(e, x.size) if e.size < x.size else e[: x.size]
    return x, e, hard, e_h.size


@pytest.fixture(scope="module")
def quotients(probes):
    a, b, hard = _quotient_cases()
    with np.errstate(all="ignore"):
        want = a / b
    return a, b, hard, want, probes.probe_policy_quotient(a, b)


@pytest.fixture(scope="module")
def roots(probes):
    x, e, hard, n_hard_speed = _root_cases()
    assert n_hard_speed > 2000
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
        speed = np.sqrt((2.0 * e * EV_TO_J) / PARTICLE_MASS)
    return x, e, hard, want, speed, probes.probe_policy_root(x, e)


def test_checked_quotients_are_ieee(quotients):
    a, b, hard, want, got = quotients
    counts = {k: (int(_differ(got[k], want)[hard].sum()), int(_differ(got[k], want).sum()))
              for k in ("ieee", "physical_checked", "mfp_checked", "time_checked")}
    print("quotients differing from numpy (hard, all of %d):" % a.size, counts)
    for k in ("ieee", "physical_checked", "mfp_checked", "time_checked"):
        assert counts[k] == (0, 0), k


def test_checked_roots_are_ieee(roots):
    x, e, hard, want, speed, got = roots
    counts = {k: (int(_differ(got[k], want)[hard].sum()), int(_differ(got[k], want).sum()))
              for k in ("ieee", "physical_checked", "sine_checked")}
    counts["speed_checked"] = (0, int(_differ(got["speed_checked"], speed).sum()))
    print("roots differing from numpy (hard, all of %d):" % x.size, counts)
    for k in counts:
        assert counts[k] == (0, 0), k


def _emulated_quotients(a, b, seed, two_steps):
    rec = ho.reciprocal_two_steps if two_steps else ho.reciprocal_one_step
    return ho.emulate(lambda p, q, r: ho.quotient_by_reciprocal(p, q, rec(q, r)), a, b, seed)


def _quotient_subset(quotients):
    """the plain range (where the fast forms are defined): every hard pair, 20 000 random ones"""
    a, b, hard, want, got = quotients
    with np.errstate(all="ignore"):
        keep = _plain(a) & _plain(b) & _plain(want)
    keep &= hard | (np.cumsum(keep) <= 20_000 + int(hard.sum()))
    return keep


def test_fast_quotients_are_the_documented_sequence(quotients):
    a, b, hard, want, got = quotients
    keep = _quotient_subset(quotients)
    emu = _emulated_quotients(a[keep], b[keep], got["rcp_seed"][keep], False)
    for k in ("physical_fast", "mfp_fast", "time_fast"):
        assert not _differ(got[k][keep], emu).any(), k
        assert int(_ulps(got[k][keep], want[keep]).max()) <= 1, k
    off = _differ(got["physical_fast"], want) & keep
    print("fast quotient one ulp off IEEE: %d of %d hard pairs, %d of %d others"
          % (int((off & hard).sum()), int((keep & hard).sum()), int((off & ~hard).sum()), int((keep & ~hard).sum())))


def test_fast_roots_are_the_documented_sequence(roots):
    x, e, hard, want, speed, got = roots
    keep = (x >= 2.0 ** -500) & (x <= 2.0 ** 500)
    keep &= hard | (np.cumsum(keep) <= 20_000 + int(hard.sum()))
    emu = ho.emulate(ho.sqrt_one_step, x[keep], got["rsq_seed"][keep])
    assert not _differ(got["physical_fast"][keep], emu).any()
    assert not _differ(got["sine_fast"][keep], emu).any()
    assert int(_ulps(got["physical_fast"][keep], want[keep]).max()) <= 1
    assert np.all(got["sine_fast"][x == 0.0] == 0.0)
    # the speed: the argument is numpy's quotient, its root the one-step sequence from the device's seed
    with np.errstate(all="ignore"):
        arg = (2.0 * e * EV_TO_J) / PARTICLE_MASS
    assert not _differ(got["speed_arg"], arg).any()
    emu_speed = ho.emulate(ho.sqrt_one_step, arg, got["speed_rsq_seed"])
    assert not _differ(got["speed_fast"], emu_speed).any()
    assert int(_ulps(got["speed_fast"], speed).max()) <= 1
    off = _differ(got["physical_fast"], want) & keep
    print("fast root one ulp off IEEE: %d of %d hard arguments, %d of %d others; speeds: %d of %d"
          % (int((off & hard).sum()), int((keep & hard).sum()), int((off & ~hard).sum()), int((keep & ~hard).sum()),
             int(_differ(got["speed_fast"], speed).sum()), e.size))


def test_two_steps_from_the_device_seeds_are_ieee(quotients, roots):
    a, b, hard, want, got = quotients
    keep = _quotient_subset(quotients)
    emu = _emulated_quotients(a[keep], b[keep], got["rcp_seed"][keep], True)
    q_miss = int(_differ(emu, want[keep]).sum())
    x, e, hard_x, want_x, speed, got_x = roots
    keep_x = (x >= 2.0 ** -500) & (x <= 2.0 ** 500)
    emu_x = ho.emulate(ho.sqrt_two_steps, x[keep_x], got_x["rsq_seed"][keep_x])
    s_miss = int(_differ(emu_x, want_x[keep_x]).sum())
    seed_q = np.abs(got["rcp_seed"][keep] * b[keep] - 1.0).max()
    seed_s = np.abs(got_x["rsq_seed"][keep_x] * np.sqrt(x[keep_x]) - 1.0).max()
    print("two steps from the device's seeds: %d of %d quotients, %d of %d roots differ from IEEE; "
          "seed errors up to 2^%.2f (rcp), 2^%.2f (rsq)"
          % (q_miss, int(keep.sum()), s_miss, int(keep_x.sum()), np.log2(seed_q), np.log2(seed_s)))
    assert q_miss == 0 and s_miss == 0

"""The hard operands of tests/hard_operands.py and the host emulation of the device's division and
square-root sequences, checked with exact arithmetic (no GPU).

tests/test_policy_boundaries.py runs the same operands through the kernels' own device functions;
this file makes sure the yardstick is right before any device is involved: every case lies as close
to a rounding boundary as it says, numpy's `a / b` and `np.sqrt` are the correctly rounded results
there, and the one-step sequences of the fast policy really are caught out by the cases."""
from fractions import Fraction

import numpy as np
import pytest

import hard_operands as ho


@pytest.fixture(scope="module")
def roots():
    return ho.sqrt_cases()


@pytest.fixture(scope="module")
def quotients():
    return ho.division_cases()


def _neighbours(y):
    """the midpoints below and above the double y > 0, exactly"""
    lo = (Fraction(y) + Fraction(float(np.nextafter(y, 0.0)))) / 2
    hi = (Fraction(y) + Fraction(float(np.nextafter(y, np.inf)))) / 2
    return lo, hi


def test_root_arguments_lie_on_rounding_boundaries(roots):
    x, bound = roots
    assert x.size >= 20_000 and int((bound <= -100).sum()) >= 10_000
    assert x.min() >= 2.0 ** -500 and x.max() < 2.0 ** 500 and np.all(np.isfinite(x))
    exps = np.frexp(x)[1]
    assert len(set((exps % 2).tolist())) == 2 and len(set(exps.tolist())) > 900
    # the path's own ranges
    assert int(((x >= 0.96) & (x <= 1.04)).sum()) >= 500
    assert int(((x >= 2.0 ** -53) & (x < 1.0)).sum()) >= 2000
    assert int(((x >= 2.0 ** -74) & (x < 2.0 ** 127)).sum()) >= 5000
    y = np.sqrt(x)
    below = 0
    for xi, yi, b in zip(x.tolist(), y.tolist(), bound.tolist()):
        fx = Fraction(xi)
        lo, hi = _neighbours(yi)
        assert lo * lo < fx < hi * hi                        # numpy's root is correctly rounded
        mid = lo if fx - lo * lo < hi * hi - fx else hi      # the boundary it is close to
        eps = Fraction(1, 2 ** -b)
        assert (mid * (1 - eps)) ** 2 <= fx <= (mid * (1 + eps)) ** 2
        below += fx < mid * mid
    assert 0.3 * x.size < below < 0.7 * x.size               # both sides of the midpoints


def test_division_pairs_lie_on_rounding_boundaries(quotients):
    a, b, bound = quotients
    assert a.size >= 20_000 and np.all(bound <= -100)
    for v in (a, b, a / b):
        m = np.abs(v)
        assert np.all((m >= 2.0 ** -300) & (m < 2.0 ** 300))
    third = a.size // 3
    assert np.all((b[1::3] >= 1e3) & (b[1::3] <= 1e8)) and np.all((b[2::3] >= 1e-6) & (b[2::3] <= 1e29))
    assert third > 7000
    q = a / b
    below = 0
    for ai, bi, qi, e in zip(a.tolist(), b.tolist(), q.tolist(), bound.tolist()):
        exact = Fraction(ai) / Fraction(bi)
        s = 1 if exact > 0 else -1
        lo, hi = _neighbours(abs(qi))
        assert lo < s * exact < hi                           # numpy's quotient is correctly rounded
        mid = lo if s * exact - lo < hi - s * exact else hi
        assert abs(s * exact - mid) <= mid * Fraction(1, 2 ** -e)
        below += s * exact < mid
    assert 0.3 * a.size < below < 0.7 * a.size


def test_exact_fma_is_the_rounded_sum():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        a, b, c = (float(v) for v in (rng.random(3) - 0.5) * np.ldexp(1.0, rng.integers(-60, 60, 3)))
        assert ho.fma(a, b, c) == float(Fraction(a) * Fraction(b) + Fraction(c))
    assert ho.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -(2.0 ** -104)   # a product no double holds


def test_one_step_sequences_miss_hard_cases_and_two_steps_do_not(roots, quotients):
    """The documented sequences, emulated exactly.  From seeds perturbed within the hardware's measured
    2^-24.4 (v_rcp_f64) and 2^-24.2 (v_rsq_f64), one Newton / Goldschmidt step and the correction miss
    the IEEE result on many hard cases: the operands have teeth.  The second step (the compiler's
    sequences) misses none from correctly rounded seeds and few from the perturbed ones -- a uniform
    2^-24 perturbation is harsher than the hardware, whose own seeds leave no miss on the device
    (tests/test_policy_boundaries.py: test_two_steps_from_the_device_seeds_are_ieee)."""
    x, _ = roots
    a, b, _ = quotients
    want_q, want_s = a / b, np.sqrt(x)
    misses = {}
    for name, rcp, rsq in (("exact", 1.0 / b, 1.0 / np.sqrt(x)),
                           ("2^-24", ho.model_seeds(1.0 / b, 7, 2.0 ** -24.4),
                            ho.model_seeds(1.0 / np.sqrt(x), 8, 2.0 ** -24.2))):
        q1 = ho.emulate(lambda p, q, r: ho.quotient_by_reciprocal(p, q, ho.reciprocal_one_step(q, r)), a, b, rcp)
        q2 = ho.emulate(lambda p, q, r: ho.quotient_by_reciprocal(p, q, ho.reciprocal_two_steps(q, r)), a, b, rcp)
        s1 = ho.emulate(ho.sqrt_one_step, x, rsq)
        s2 = ho.emulate(ho.sqrt_two_steps, x, rsq)
        misses[name] = tuple(int((got != want).sum()) for got, want in
                             ((q1, want_q), (q2, want_q), (s1, want_s), (s2, want_s)))
        # every miss is by one ulp
        for got, want in ((q1, want_q), (s1, want_s)):
            assert np.abs(got.view(np.int64) - want.view(np.int64)).max() <= 1
    print("misses (quotient one step, two steps, root one step, two steps):", misses)
    q1, q2, s1, s2 = misses["2^-24"]
    assert q1 > 1000 and s1 > 1000
    assert q2 < q1 // 100 and s2 < s1 // 4
    assert misses["exact"][1] == 0 and misses["exact"][3] == 0

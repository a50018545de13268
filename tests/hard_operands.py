"""Operands on rounding boundaries, and the division / square-root sequences of
neutral_amd/csrc/neutral_device.h emulated exactly on the host.

The cases are built from integers alone (no floating point in the construction):

* square roots.  M, an odd 54-bit integer, is a midpoint between two doubles in
  units of 2^-53 of its binade.  If M^2 = +-r (mod 2^t) for a small odd r, then
  N = (M^2 -+ r) / 2^t is an integer of at most 53 bits, and x = N 2^(t + 2j) is a
  double whose exact root M 2^j sqrt(1 -+ r / M^2) lies within r / (2 M^2) (relative)
  of the midpoint M 2^j, below it (r = 1 mod 8) or above it (-r = 1 mod 8).  t = 54
  gives the binades of even exponent (M^2 in [2^106, 2^107)), t = 55 the odd ones.
  The square roots of r modulo 2^t come from Hensel lifting.
* quotients.  B, a random odd 53-bit integer, and a small odd r: Q = +-r B^-1 (mod
  2^54), kept when it is a 54-bit (odd) midpoint, makes A = (Q B -+ r) / 2^54 an
  integer of at most 53 bits whose quotient A / B lies within r / (Q B) of the
  midpoint Q 2^-54.

Every case carries the bound it is stated to meet (`bound_log2`: the exact root or
quotient lies within 2^bound_log2, relative, of a midpoint).  tests/test_hard_operands.py
checks the bounds and numpy's results with exact rational arithmetic.

The emulations use fma(a, b, c) = RN(a b + c) evaluated exactly: every double is a
ratio of integers with a power-of-two denominator, and Python's int / int is
correctly rounded."""
import random

import numpy as np

# ---- square-root arguments ----------------------------------------------------------


def _sqrt_mod_pow2(r: int, t: int) -> int:
    """a root s of s^2 = r (mod 2^t), r = 1 (mod 8), by Hensel lifting one bit at a time;
    the four roots are +-s and +-s + 2^(t-1)"""
    assert r % 8 == 1
    s = 1
    for k in range(3, t):
        if (s * s - r) % (1 << (k + 1)):
            s += 1 << (k - 1)
    return s % (1 << t)


def _root_mantissas(r_max: int):
    """every (N, t, M, signed r) with M an odd 54-bit midpoint, M^2 = N 2^t + r, |r| < r_max"""
    out = []
    for t in (54, 55):
        lo, hi = 1 << (106 + (t - 54)), 1 << (107 + (t - 54))   # M^2 in [2^(t+52), 2^(t+53))
        mod = 1 << t
        for r in range(1, r_max, 2):
            for sign in (1, -1):        # M^2 = N 2^t + r: the root is below the midpoint
                res = (sign * r) % mod   # (sign 1) or above it (sign -1)
                if res % 8 != 1:
                    continue
                s = _sqrt_mod_pow2(res, t)
                for m in {s, mod - s, (s + (mod >> 1)) % mod, (mod - s + (mod >> 1)) % mod}:
                    if m % 2 == 1 and lo <= m * m < hi:
                        n = (m * m - sign * r) >> t
                        assert n << t == m * m - sign * r and n < (1 << 53)
                        out.append((n, t, m, sign * r))
    return out


def _root_bound_log2(m: int, r: int) -> int:
    """an integer b with |sqrt(M^2 - r) - M| / M <= 2^b: the distance |r| / (M (M + sqrt(M^2 - r)))
    is below |r| / (2 M^2 - 2 |r|)"""
    return -((2 * m * m - 2 * abs(r)) // abs(r)).bit_length() + 1


def sqrt_cases(seed: int = 1):
    """-> (x, bound_log2): arguments whose exact roots lie within 2^bound_log2 (relative) of a
    midpoint between two doubles, on both sides, over [2^-500, 2^500], the plain range's edges
    and the path's own ranges (energy ratios in [0.96, 1.04], 1 - cos^2 in [2^-53, 1], the
    speed's argument 2 E eV / m in [2^-74, 2^127])"""
    rng = random.Random(seed)
    xs, bounds = [], []

    def add(n, t, m, r, j):
        xs.append(float(np.ldexp(float(n), t + 2 * j)))   # (n < 2^53: exact)
        bounds.append(_root_bound_log2(m, r))

    # the closest: every mantissa within 2^-100, at 160 scalings each
    closest = _root_mantissas(256)
    closest = [c for c in closest if _root_bound_log2(c[2], c[3]) <= -100]
    for (n, t, m, r) in closest:
        for _ in range(160):
            add(n, t, m, r, rng.randrange(-303, 197))   # x in [2^-500, 2^500)
        for j in (-303, 196, -53, -54, -79):            # the range's ends, around 1, around 2^-53
            add(n, t, m, r, j)
    # within 2^-95: every mantissa, at eight scalings across the range and one in each path range
    wide = _root_mantissas(4096)
    for (n, t, m, r) in wide:
        for _ in range(8):
            add(n, t, m, r, rng.randrange(-303, 197))
        add(n, t, m, r, rng.randrange(-79, -53))          # 1 - cos^2: x in [2^-53, 1)
        add(n, t, m, r, rng.randrange(-90, 10))           # 2 E eV / m: x in [2^-74, 2^127)
    # energy ratios: mantissas whose x lies in [0.96, 1.04] (a band of the binades [0.5, 1), [1, 2))
    for (n, t, m, r) in _root_mantissas(1 << 16):
        x = n << t
        if t == 54 and x * 25 <= 26 << 106:               # x / 2^106 in [1, 1.04]
            add(n, t, m, r, -53)
        elif t == 55 and x * 25 >= 24 << 108:             # x / 2^108 in [0.96, 1)
            add(n, t, m, r, -54)
    x = np.array(xs, dtype=np.float64)
    return x, np.array(bounds, dtype=np.int32)


# ---- division pairs -------------------------------------------------------------------

SPECIAL_DIVISORS = [(1 << 53) - 1, (1 << 52) + 1, (1 << 53) - 3, (3 << 51) + 1, (3 << 51) - 1]


def _quotient_mantissas(rng: random.Random, count: int, r_max: int):
    """(A, B, Q, signed r) with Q an odd 54-bit midpoint and Q B = A 2^54 + r"""
    out = []
    mod = 1 << 54
    while len(out) < count:
        b = SPECIAL_DIVISORS[len(out) % len(SPECIAL_DIVISORS)] if len(out) < 64 * len(SPECIAL_DIVISORS) \
            else rng.randrange(1 << 52, 1 << 53) | 1
        r = rng.randrange(1, r_max, 2) * rng.choice((1, -1))
        q = (r * pow(b, -1, mod)) % mod
        if not (1 << 53) <= q < mod:
            continue
        a = (q * b - r) >> 54
        assert (a << 54) + r == q * b and a < (1 << 53)
        out.append((a, b, q, r))
    return out


def _quotient_bound_log2(b: int, q: int, r: int) -> int:
    """an integer e with |A / B - Q 2^-54| / (Q 2^-54) = |r| / (Q B) <= 2^e"""
    return -((q * b) // abs(r)).bit_length() + 1


def division_cases(count: int = 24000, seed: int = 2):
    """-> (a, b, bound_log2): pairs whose exact quotient lies within 2^bound_log2 (relative) of a
    midpoint, on both sides.  Both operands and the quotient in the plain range [2^-300, 2^300]:
    a third anywhere, a third the stream kernel's facet distance by a speed (1e3 ... 1e8), a third
    by a mean free path (1e-6 ... 1e29)"""
    rng = random.Random(seed)
    rows = _quotient_mantissas(rng, count, 32)
    a_out, b_out, bounds = [], [], []
    for i, (a, b, q, r) in enumerate(rows):
        kind = i % 3
        if kind == 0:
            ea = rng.randrange(-295, 295)                 # a = A 2^(ea - 52) in [2^-295, 2^295)
            eb = rng.randrange(max(-295, ea - 295), min(295, ea + 295))
        else:
            ea = rng.randrange(-40, 7)                    # a facet distance: 1e-12 ... 1e2
            eb = rng.randrange(10, 26) if kind == 1 else rng.randrange(-19, 96)   # b in [1024, 2^26), [2^-19, 2^96)
        av = float(a) * 2.0 ** (ea - 52)
        bv = float(b) * 2.0 ** (eb - 52)
        if rng.randrange(8) == 0:
            av = -av
        a_out.append(av)
        b_out.append(bv)
        bounds.append(_quotient_bound_log2(b, q, r))
    return (np.array(a_out, dtype=np.float64), np.array(b_out, dtype=np.float64),
            np.array(bounds, dtype=np.int32))


# ---- exact host emulation of the device sequences --------------------------------------


def fma(a: float, b: float, c: float) -> float:
    """RN(a b + c) for finite doubles, exactly"""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    d = da * db
    num = na * nb * dc + nc * d
    den = d * dc
    if num == 0:   # (an exact zero is +0 unless both addends are -0)
        return -0.0 if (np.signbit(a) != np.signbit(b)) and na * nb == 0 and nc == 0 and np.signbit(c) else 0.0
    return num / den


def reciprocal_one_step(b: float, r0: float) -> float:
    """refined_reciprocal(): one Newton step on the seed r0"""
    return fma(r0, fma(-b, r0, 1.0), r0)


def reciprocal_two_steps(b: float, r0: float) -> float:
    """the compiler's division: two Newton steps on the seed"""
    r1 = reciprocal_one_step(b, r0)
    return fma(r1, fma(-b, r1, 1.0), r1)


def quotient_by_reciprocal(a: float, b: float, r: float) -> float:
    """q0 = a r, q = q0 + (a - b q0) r"""
    q0 = a * r
    return fma(fma(-b, q0, a), r, q0)


def sqrt_one_step(x: float, y: float) -> float:
    """sqrt_known_plain(): one coupled Goldschmidt step on the seed y = rsq(x) and the correction"""
    g0 = x * y
    h0 = 0.5 * y
    r0 = fma(-h0, g0, 0.5)
    g1 = fma(g0, r0, g0)
    h1 = fma(h0, r0, h0)
    return fma(fma(-g1, g1, x), h1, g1)


def sqrt_two_steps(x: float, y: float) -> float:
    """the compiler's ten operations: the same and a second correction"""
    g0 = x * y
    h0 = 0.5 * y
    r0 = fma(-h0, g0, 0.5)
    g1 = fma(g0, r0, g0)
    h1 = fma(h0, r0, h0)
    s = fma(fma(-g1, g1, x), h1, g1)
    return fma(fma(-s, s, x), h1, s)


def model_seeds(exact, seed: int, rel: float = 2.0 ** -24):
    """seeds as the hardware's v_rcp_f64 / v_rsq_f64 give them: the exact value times (1 + d),
    |d| < rel (measured: 2^-24.4 and 2^-24.2)"""
    rng = np.random.default_rng(seed)
    return exact * (1.0 + rel * (2.0 * rng.random(exact.size) - 1.0))


def emulate(fn, *columns) -> np.ndarray:
    return np.array([fn(*row) for row in zip(*(c.tolist() for c in columns))], dtype=np.float64)

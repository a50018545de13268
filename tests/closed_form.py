"""The stream deck's global tally in closed form, from reference-held inputs ALONE.

`problems/stream.params` is one near-vacuum density everywhere and a source of 1e6 eV: no
history collides (a free flight of -log(rn)/Sigma_s ~ 1e23 mean free paths), every boundary
reflects, so each particle travels exactly speed * dt per timestep whatever the mesh or the
particle count, and every cell it passes through holds the same material.  The energy
deposition of a track segment (`omp3/neutral.c:474-495`) is linear in its length, so

    global tally per timestep = speed * dt * (sigma_s + sigma_a) * BARNS * heating * n

with speed = sqrt(2 E eV / m) (`:117`), n = rho * AVOGADROS / MOLAR_MASS (`:112-113`),
heating = E - (1 - sigma_a / sigma_t) * E * (A^2 + A + 1) / (A + 1)^2 (`:481-492`), the constants
of `neutral_data.h:17-24`, the deck's own numbers, and the two microscopic cross sections
interpolated from the shipped `.cs` table at E (`omp3/neutral.c:498-517`).

Nothing here goes through `oracle/`: the table lookup is numpy's searchsorted plus the
interpolation formula, the rest is six multiplications.  It pins the oracle (CPU suite) and
the HIP path (GPU suite) at 1e-12 where the reference's own `neutral.tests` holds 1e-3
(the shipped known answer agrees with this closed form to 8e-7).
"""
import math

import numpy as np

# neutral_data.h:17-24
EV_TO_J = 1.60217646e-19
AVOGADROS = 6.02214085774e23
BARNS = 1.0e-28
PARTICLE_MASS = 1.674927471213e-27
MASS_NO = 1.0e2
MOLAR_MASS = 1.0e-2


def microscopic_cs(keys: np.ndarray, values: np.ndarray, energy: float) -> float:
    """omp3/neutral.c:498-517: the bracket keys[i] <= E < keys[i+1], linear interpolation."""
    i = int(np.searchsorted(keys, energy, side="right") - 1)
    assert 0 <= i < len(keys) - 1
    return float(values[i] + ((energy - keys[i]) / (keys[i + 1] - keys[i])) * (values[i + 1] - values[i]))


def collision_free_tally_per_step(keys, values, energy: float, density: float, dt: float) -> float:
    """Global energy-deposition tally of ONE timestep of a collision-free, one-material deck
    (weight 1, both tables the shipped one)."""
    sigma_s = microscopic_cs(keys, values, energy)
    sigma_a = sigma_s  # elastic_scatter.cs and capture.cs hold the same data
    sigma_t = sigma_s + sigma_a
    speed = math.sqrt(2.0 * energy * EV_TO_J / PARTICLE_MASS)
    number_density = density * AVOGADROS / MOLAR_MASS
    exit_energy = energy * (MASS_NO * MASS_NO + MASS_NO + 1.0) / ((MASS_NO + 1.0) * (MASS_NO + 1.0))
    heating = energy - (1.0 - sigma_a / sigma_t) * exit_energy
    return speed * dt * (sigma_t * BARNS) * heating * number_density


def unfolded_beam(edges, start, sign, length):
    """A collision-free flight of `length` along one axis between two reflecting walls, without
    any event loop: the reflections are unfolded, the path is the straight interval
    [u0, u0 + length] over mirror images of the mesh (image k even: the mesh as it is, the
    history moving up the axis; k odd: mirrored, moving down), and every image of every cell is
    intersected with it.  Everything in fractions.Fraction built from the edge doubles, `start`
    and `length` (Fractions or doubles): exact.

    -> (track, signed, low, high, gap): per cell the path length inside it, the same with the sign
    of the motion (the current), how often the path leaves it through its lower and through its
    upper side -- a wall hit counts on the wall side of the wall cell, the end of the path does
    not count -- and the distance from the path's end to the nearest edge (the answer is the
    event loop's only where that is well above rounding).

    Left out on purpose: the open-bound correction (omp3/neutral.c:438-447, 1e-14 m past a
    lower edge) and the rounding of every landing."""
    from fractions import Fraction
    e = [Fraction(v) for v in edges]
    n = len(e) - 1
    lo, hi = e[0], e[n]
    width = hi - lo
    start, length = Fraction(start), Fraction(length)
    assert lo < start < hi and length > 0 and sign in (1, -1)
    u0 = (start - lo) if sign > 0 else width + (hi - start)
    u1 = u0 + length
    track, signed = [Fraction(0)] * n, [Fraction(0)] * n
    low, high = [0] * n, [0] * n
    gap = None
    k = int(u0 // width)
    while k * width < u1:
        for c in range(n):
            if k % 2 == 0:
                a, b = k * width + (e[c] - lo), k * width + (e[c + 1] - lo)
            else:
                a, b = k * width + (hi - e[c + 1]), k * width + (hi - e[c])
            overlap = min(b, u1) - max(a, u0)
            if overlap > 0:
                track[c] += overlap
                signed[c] += overlap if k % 2 == 0 else -overlap
            if u0 < b < u1:
                if k % 2 == 0:
                    high[c] += 1
                else:
                    low[c] += 1
            for edge in (a, b):
                gap = abs(u1 - edge) if gap is None else min(gap, abs(u1 - edge))
        k += 1
    return track, signed, low, high, gap


def stream_deck_tally(keys, values, iterations: int = 1) -> float:
    from neutral_amd import decks
    d = decks.STANDARD_DECKS["stream"]
    (p,) = d["problems"]
    return iterations * collision_free_tally_per_step(keys, values, d["initial_energy"], p["density"],
                                                      d["dt"])

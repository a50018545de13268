"""Pins the CPU oracle (oracle/neutral_oracle.c) to the reference.

Two kinds of pin, kept apart by test name so a reader sees which is which:

REFERENCE-HELD (test_reference_held__*): what the reference tree itself holds or
what can be built from it here without stand-ins --
* Threefry2x64-20 bit for bit against the reference's own Random123 header compiled
  in place (oracle/_ref), through its outputs recorded in tests/golden where it is absent;
* the whole history loop against problems/neutral.tests:1-3 at the decks' default
  sizes (the reference's own known answers, tolerance 1e-3, neutral_data.h:27) --
  all three decks, in the default CPU suite.

RECORDED, NOT REPRODUCIBLE HERE (test_recorded_not_reproducible_here__*): numbers
the survey wrote down (SURVEY.md sections 4, 6, 8c) from an
omp3 binary it built against stand-ins for the absent parent project's headers.
That build is not in this repository and by the rules pins nothing; the numbers are
kept as a regression record -- exact integer event counts, tallies to 1e-13 -- which
the oracle reproduces digit for digit.
"""
import hashlib
import os

import numpy as np
import pytest

import closed_form
import oracle_binding as ob
from neutral_amd import decks


def _h(x):
    return int(x, 16)


def test_recorded_not_reproducible_here__threefry_vectors(pins):
    for v in pins["threefry2x64_20"]:
        out = ob.threefry(_h(v["ctr"][0]), _h(v["ctr"][1]), _h(v["key"][0]), _h(v["key"][1]))
        assert out == (_h(v["out"][0]), _h(v["out"][1]))


def test_reference_held__threefry_matches_reference_random123(pins):
    # the reference header's outputs on the pinned inputs, recorded where it is present
    # (tests/golden/make_threefry_vectors.py) ...
    cases = ob.threefry_cases()
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "ref_threefry_vectors.npz"))
    assert str(z["inputs_sha256"]) == hashlib.sha256(cases.tobytes()).hexdigest()
    want = [(int(a), int(b)) for a, b in z["out"]]
    # ... are what the reference produces wherever oracle/_ref is built ...
    if ob.have_ref_threefry():
        for v in pins["threefry2x64_20"]:
            out = ob.ref_threefry(_h(v["ctr"][0]), _h(v["ctr"][1]), _h(v["key"][0]), _h(v["key"][1]))
            assert out == (_h(v["out"][0]), _h(v["out"][1]))
        for row, w in zip(cases, want):
            assert ob.ref_threefry(*(int(x) for x in row)) == w
    # ... and the restatement agrees with them on 20 000 random and edge inputs
    for row, w in zip(cases, want):
        assert ob.threefry(*(int(x) for x in row)) == w


def test_random_numbers_unit_interval():
    # omp3/neutral.c:646-651: u64 * 2^-64 + 2^-65, so rn in (0, 1]
    r0, r1 = ob.generate_random_numbers(12345, 1, 7)
    a, b = ob.threefry(7, 0, 12345, 1)
    assert r0 == float(a) * 2.0**-64 + 2.0**-65
    assert r1 == float(b) * 2.0**-64 + 2.0**-65
    rs = [ob.generate_random_numbers(p, 3, c) for p in range(200) for c in range(5)]
    flat = np.array(rs).ravel()
    assert flat.min() > 0.0 and flat.max() <= 1.0
    assert 0.45 < flat.mean() < 0.55


def test_a_sample_is_below_one_half_exactly_when_its_integer_is_below_2_63_minus_512():
    """The HIP path decides absorb-or-scatter at probability one half (identical tables) on the
    64-bit integer the first sample is made of (neutral_device.h: sample_below_half) instead of on
    the double omp3/neutral.c:646-651 make of it: float(r) rounds to a multiple of 2^10 up there,
    * 2^-64 + 2^-65 is rounded once more, and the result is < 0.5 exactly for r < 2^63 - 512.
    The boundary walked integer by integer, the ends, and two million random integers."""
    threshold = 0x7FFFFFFFFFFFFE00
    def below_half(r):
        return (float(r) * 2.0 ** -64 + 2.0 ** -65) < 0.5     # the reference's arithmetic, in IEEE doubles
    for r in list(range(2 ** 63 - 5000, 2 ** 63 + 5000)) + [0, 1, 2 ** 63, 2 ** 64 - 1]:
        assert below_half(r) == (r < threshold), hex(r)
    rng = np.random.default_rng(7)
    r = rng.integers(0, 2 ** 64, 2_000_000, dtype=np.uint64)
    as_double = r.astype(np.float64) * 2.0 ** -64 + 2.0 ** -65   # (numpy converts round-to-nearest too)
    assert np.array_equal(as_double < 0.5, r < np.uint64(threshold))
    # the same through the oracle's own conversion
    for c in range(2000):
        a, _ = ob.threefry(c, 0, 99, 1)
        r0, _ = ob.generate_random_numbers(99, 1, c)
        assert (r0 < 0.5) == (a < threshold)


def test_recorded_not_reproducible_here__cs_lookup_values(pins, cs):
    table = ob.CsTable(*cs)
    for e in pins["cs_lookup"]:
        value, index = table.lookup(e["energy"])
        assert index == e["index"]
        assert value == pytest.approx(e["value"], rel=1e-14)


def test_cs_lookup_brackets(cs):
    keys, values = cs
    table = ob.CsTable(keys, values)
    rng = np.random.default_rng(7)
    idx = rng.integers(0, len(keys) - 1, size=500)
    for i in idx:
        # exactly on a key: bracket starts there, value is the tabulated one
        v, ind = table.lookup(float(keys[i]))
        assert ind == i and v == values[i]
        # just below the next key: still the same bracket
        e = np.nextafter(keys[i + 1], 0.0)
        v, ind = table.lookup(float(e))
        assert ind == i
        lo, hi = sorted((values[i], values[i + 1]))
        assert lo <= v <= hi
    # matches numpy's searchsorted bracket + the interpolation formula
    es = np.exp(rng.uniform(np.log(keys[0] * 1.001), np.log(keys[-1] * 0.999), size=2000))
    for e in es:
        v, ind = table.lookup(float(e))
        j = int(np.searchsorted(keys, e, side="right") - 1)
        assert ind == j
        expect = values[j] + ((e - keys[j]) / (keys[j + 1] - keys[j])) * (values[j + 1] - values[j])
        assert v == expect


def _run_oracle(make_problem, cs, name, nx, nparticles, iterations):
    prob = make_problem(name, nx=nx, nparticles=nparticles, iterations=iterations)
    run = ob.OracleRun(prob, *cs)
    run.inject()
    facets = collisions = 0
    last = None
    for tt in range(1, prob.niters + 1):
        last = run.step(tt)
        facets += last.facets
        collisions += last.collisions
    return run, facets, collisions, last


@pytest.mark.parametrize("i", range(5))
def test_recorded_not_reproducible_here__omp3_runs(pins, make_problem, cs, i):
    r = pins["omp3_runs"][i]
    run, facets, collisions, last = _run_oracle(make_problem, cs, r["deck"], r["nx"],
                                                r["nparticles"], r["iterations"])
    if r.get("facets") is not None:
        assert facets == r["facets"]
    if r.get("collisions") is not None:
        assert collisions == r["collisions"]
    if "collisions_rounded" in r:
        assert collisions == pytest.approx(r["collisions_rounded"], rel=5e-4)
    if "last_step_processed" in r:
        assert last.nprocessed == r["last_step_processed"]
    assert run.tally_sum() == pytest.approx(r["tally"], rel=1e-13)


@pytest.mark.parametrize("nx,n,its", [(100, 20000, 1), (37, 5000, 3)])
def test_reference_held__stream_deck_closed_form(make_problem, cs, nx, n, its):
    """The stream deck has a closed form from reference-held inputs alone (tests/closed_form.py:
    the constants of neutral_data.h:17-24, the shipped .cs table, omp3/neutral.c:117,474-495 --
    nothing of the restatement): speed * dt * sigma_t * BARNS * heating * n per timestep, whatever
    the mesh and the particle count.  The oracle reproduces it to 1e-12; the reference's own
    known answer (problems/neutral.tests:2, held at 1e-3) agrees with it to 1e-6."""
    expected = closed_form.stream_deck_tally(*cs, iterations=its)
    assert expected == pytest.approx(5.7600599264841e-24 * its, rel=1e-12)
    assert abs(decks.KNOWN_ANSWERS["stream"] - closed_form.stream_deck_tally(*cs)) < \
        1e-6 * decks.KNOWN_ANSWERS["stream"]
    run, facets, collisions, _ = _run_oracle(make_problem, cs, "stream", nx, n, its)
    assert collisions == 0 and facets > 0
    rel = abs(run.tally_sum() - expected) / expected
    print(f"stream {nx}^2 / {n} x {its}: oracle {run.tally_sum():.15e} closed form {expected:.15e} rel {rel:.2e}")
    assert rel < 1e-12


_default_deck_runs = {}


def _default_deck_run(make_problem, cs, name):
    """The oracle on a deck as shipped (4000^2 cells); run once per session."""
    if name not in _default_deck_runs:
        d = decks.STANDARD_DECKS[name]
        run, facets, collisions, _ = _run_oracle(make_problem, cs, name, d["nx"], d["nparticles"],
                                                 d["iterations"])
        _default_deck_runs[name] = (run.tally_sum(), facets, collisions)
    return _default_deck_runs[name]


# scatter as shipped is 7e9 collisions -- five minutes on the eight cores of the build
# container -- so it runs where the whole CPU suite is asked for (`make test-cpu` sets
# NEUTRAL_FULL_KATS=1; last log: oracle/pins/full_kats.log); stream and csp always run
LONG_KAT = pytest.mark.skipif(os.environ.get("NEUTRAL_FULL_KATS") != "1",
                              reason="five minutes of CPU: `make test-cpu` (NEUTRAL_FULL_KATS=1)")
DEFAULT_DECKS = ["stream", "csp", pytest.param("scatter", marks=[pytest.mark.fullkat, LONG_KAT])]


@pytest.mark.parametrize("name", DEFAULT_DECKS)
def test_reference_held__known_answers_default_decks(make_problem, cs, name):
    """problems/neutral.tests:1-3 at the decks' default sizes (4000^2 cells; 1e6, 1e6,
    1e7 particles; 1, 10, 2 iterations), the reference's own tolerance."""
    tally, facets, collisions = _default_deck_run(make_problem, cs, name)
    expected = decks.KNOWN_ANSWERS[name]
    # (shown by `make test-cpu` / `make pin-kats`: oracle/pins/full_kats.log)
    print(f"{name} as shipped: facets={facets} collisions={collisions} tally={tally:.15e} "
          f"expected={expected:.12e} rel={abs(tally - expected) / expected:.2e}")
    assert abs(tally - expected) / expected < decks.VALIDATE_TOLERANCE
    if name == "stream":
        # ... and, at the deck's own size, the closed form (tests/closed_form.py) at 1e-12
        exact = closed_form.stream_deck_tally(*cs)
        print(f"stream as shipped against the closed form: rel={abs(tally - exact) / exact:.2e}")
        assert abs(tally - exact) / exact < 1e-12


@pytest.mark.parametrize("name", DEFAULT_DECKS)
def test_recorded_not_reproducible_here__omp3_default_decks(make_problem, cs, pins, name):
    """The omp3 backend's own output at the default sizes as the survey recorded it:
    exact event counts, tally to 1e-13."""
    tally, facets, collisions = _default_deck_run(make_problem, cs, name)
    rec = next(r for r in pins["omp3_default_runs"] if r["deck"] == name)
    if rec["facets"] is not None:
        assert facets == rec["facets"]
    if rec["collisions"] is not None:
        assert collisions == rec["collisions"]
    assert tally == pytest.approx(rec["tally"], rel=1e-13)

"""The cone and half-space projections of the oracle (oracle/tinympc_oracle.c: project_soc, project_halfspaces, through their test
entry points) against an extended-precision restatement of the textbook formulas, and the coverage condition of every data set that
test_family_regions_gpu.py compares a kernel on: each of the eight outcomes (cone apex / inside / surface per side, row not violated /
violated) takes at least 2 % of its side's projections in the ORACLE's census, and on each side some iteration of some instance mixes
outcomes over its knots. No GPU."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

import family_region_cases as F
import pyoracle as O

LD = np.longdouble
U = 2.0 ** -53  # unit round-off of the oracle's arithmetic (binary64, round to nearest)

assert np.finfo(LD).eps < np.finfo(np.float64).eps, "numpy.longdouble is no wider than double here: part (a) has no reference"


# ---- (a) the projections against numpy.longdouble

def soc_reference(sv, mu):
    """Projection onto { (w, t) : ||w|| <= mu t }, t last, in extended precision: the textbook case distinction."""
    s = np.array(sv, dtype=LD)
    w, t, mu = s[:-1], s[-1], LD(mu)
    a = np.sqrt(np.sum(w * w))
    if a <= -mu * t:      # in the polar cone: the apex
        return np.zeros_like(s), 0, a
    if a <= mu * t:       # in the cone
        return s, 1, a
    scale = (1 + mu * t / a) / 2
    return np.concatenate([scale * w, [scale * a / mu]]), 2, a


def soc_bound(sv, mu, a):
    """|oracle - exact| per entry, from the operation count of project_soc on n entries (m = n - 1 of them in w), u = 2^-53:
      a2 = sum of m squares, all >= 0: relative error <= m u (one rounding per square, m - 1 additions); a = sqrt(a2): (m/2 + 1) u
      u0 = t mu: u;  u0 / a: (m/2 + 3) u, and |u0 / a| < 1 on the surface branch
      1 + u0/a: absolute error <= (m/2 + 3) u + 2 u (the sum is below 2);  scale = 0.5 (..): exact halving: <= (m/4 + 2.5) u, scale in (0, 1)
      w_i' = scale w_i: <= |w_i| ((m/4 + 2.5) + 1) u
      t'   = scale (a / mu): a / mu carries (m/2 + 2) u relative: <= (a/mu) ((m/4 + 2.5) + (m/2 + 2) + 1) u = (a/mu) (0.75 m + 5.5) u
    so every entry is within (0.75 m + 5.5) u max(max|sv|, a / mu) -- rounded up to (n + 6) u. A point within rounding of a boundary may
    take the neighbouring branch; the branches meet continuously (scale -> 1 at a = u0, scale -> 0 at a = -u0) and the branch the oracle
    then takes is exact (identity, or zeros), so it is off by at most |scale - 1| or |scale| <= (m/4 + 1) u times the same magnitude:
    inside the same bound. The extended-precision side adds 2^-64 terms, three orders below."""
    n = len(sv)
    mag = max(float(np.max(np.abs(sv))), float(a) / mu)
    return (n + 6) * U * mag


def check_soc(sv, mu, expect=None):
    sv = np.asarray(sv, dtype=np.float64)
    got, took = O.project_soc(sv, mu)
    ref, ref_took, a = soc_reference(sv, mu)
    err = float(np.max(np.abs(got.astype(LD) - ref)))
    bound = soc_bound(sv, mu, a)
    assert err <= bound, (sv, mu, err, bound)
    if expect is not None:
        assert took == ref_took == expect, (sv, mu, took, ref_took, expect)
    return took, ref_took


@pytest.mark.parametrize("n", [2, 3, 5, 16])
def test_cone_projection_against_extended_precision(n):
    rng = np.random.default_rng(100 + n)
    seen = set()
    for trial in range(600):
        mu = float(rng.uniform(0.2, 1.5))
        sv = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)
        sv[-1] = rng.standard_normal() * np.linalg.norm(sv[:-1]) / mu * rng.choice([0.3, 1.0, 3.0])  # t around the two boundaries
        took, ref_took = check_soc(sv, mu)
        assert took == ref_took, (sv, mu)  # (random points do not sit within rounding of a boundary)
        seen.add(took)
    assert seen == {0, 1, 2}


# integer vectors w with an integer norm, by dimension of the cone: |w| = 5, 5, 5, 6 -- every product below is exact in binary64
EXACT_W = {2: ([5.0], 5.0), 3: ([3.0, 4.0], 5.0), 5: ([1.0, 2.0, 4.0, 2.0], 5.0), 16: ([1.0] * 8 + [2.0] * 7, 6.0)}


@pytest.mark.parametrize("n", [2, 3, 5, 16])
def test_cone_projection_at_the_named_points(n):
    w, norm = EXACT_W[n]
    assert len(w) == n - 1 and float(np.dot(w, w)) == norm * norm
    mu = 0.5
    # exactly on the cone's surface (||w|| == mu t): `inside`, the point stays bit for bit; one step of t either way crosses over
    on = np.array(w + [norm / mu])
    got, took = O.project_soc(on, mu)
    assert took == 1 and np.array_equal(got, on)
    check_soc(on, mu, expect=1)
    check_soc(np.array(w + [np.nextafter(norm / mu, 0.0)]), mu, expect=2)
    # exactly on the polar cone's surface (||w|| == -mu t): the apex; one step towards the cone: the surface branch, continuous with zero
    polar = np.array(w + [-norm / mu])
    got, took = O.project_soc(polar, mu)
    assert took == 0 and np.array_equal(got, np.zeros(n))
    check_soc(polar, mu, expect=0)
    got, _ = O.project_soc(np.array(w + [np.nextafter(-norm / mu, 0.0)]), mu)
    check_soc(np.array(w + [np.nextafter(-norm / mu, 0.0)]), mu, expect=2)
    assert np.max(np.abs(got)) <= 4 * U * norm / mu
    # w = 0 (no division happens on any branch that is taken): t > 0 stays, t < 0 and t = 0 go to the apex
    for t, expect in ((2.5, 1), (-2.5, 0), (0.0, 0)):
        z = np.array([0.0] * (n - 1) + [t])
        got, took = O.project_soc(z, mu)
        assert took == expect and np.array_equal(got, z if expect == 1 else np.zeros(n)) and np.all(np.isfinite(got)), (t, got)
        check_soc(z, mu, expect=expect)


def halfspace_reference(sv, A, b):
    """Rows one after another in extended precision; also the bound of the oracle's error (below)."""
    s = np.array(sv, dtype=LD)
    A = np.array(A, dtype=LD).reshape(len(b), len(s))
    n = len(s)
    before, own, hit = 0.0, 0.0, 0  # the own bounds of the rows before the last finite one, and that one's
    for k in range(len(b)):
        a = A[k]
        dot, nrm = np.sum(a * s), np.sum(a * a)
        if np.isfinite(b[k]):
            # one row on n entries, u = 2^-53, S = sum |a_c s_c|, |dot - b| <= S + |b|:
            #   dot: n products, n - 1 additions: |error| <= n u S;  nrm (all terms >= 0): relative n u
            #   num = dot - b: <= n u S + u |dot - b| <= (n + 1) u (S + |b|)
            #   dist = num / nrm: nrm's n u and the division's u on top: <= 2 (n + 1) u (S + |b|) / nrm
            #   s_c - dist a_c: <= |a_c| 2 (n + 1) u (S + |b|) / nrm + u |dist a_c| + u |s_c'|  <=  (2 n + 5) u M,
            #   M = max(|s|_inf, (S + |b|) |a|_inf / nrm)                         -- rounded up to (2 n + 6) u M.
            # A row decided the other way within rounding of dot == b moves the point by |dot - b| |a|_inf / nrm <= n u S |a|_inf / nrm:
            # inside the same bound. A projection onto a half-space is 1-Lipschitz in the 2-norm, so what the rows BEFORE this one left
            # (2-norm <= sqrt(n) times their max-norm bounds) passes through this row without growing; this row's own error adds in
            # the max-norm as it is. One row: (2 n + 6) u M, a few ulp of M; K rows: own(K) + sqrt(n) (own(1) + .. + own(K-1)).
            S = float(np.sum(np.abs(a * s)))
            M = max(float(np.max(np.abs(s))), (S + abs(float(b[k]))) * float(np.max(np.abs(a))) / float(nrm))
            before, own = before + own, (2 * n + 6) * U * M
        else:
            before, own = before + own, 0.0  # (a row with b = +inf computes nothing that is used)
        if dot > LD(b[k]):
            s = s - (dot - LD(b[k])) / nrm * a
            hit += 1
    return s, hit, own + np.sqrt(n) * before


def check_halfspaces(sv, A, b, expect_hit=None):
    sv, A, b = np.asarray(sv, dtype=np.float64), np.atleast_2d(np.asarray(A, dtype=np.float64)), np.asarray(b, dtype=np.float64).ravel()
    got, hit = O.project_halfspaces(sv, A, b)
    ref, ref_hit, bound = halfspace_reference(sv, A, b)
    err = float(np.max(np.abs(got.astype(LD) - ref)))
    assert err <= bound, (err, bound, sv, A, b)
    if expect_hit is not None:
        assert hit == ref_hit == expect_hit, (hit, ref_hit, expect_hit)
    return got, hit, ref_hit


@pytest.mark.parametrize("n", [2, 3, 5, 16])
def test_halfspace_projection_against_extended_precision(n):
    rng = np.random.default_rng(200 + n)
    hits = 0
    for trial in range(400):
        rows = int(rng.integers(1, 5))
        A = rng.standard_normal((rows, n))
        sv = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2)
        b = A @ sv + rng.standard_normal(rows) * np.abs(A @ sv)
        got, hit, ref_hit = check_halfspaces(sv, A, b)
        assert hit == ref_hit
        hits += hit
    assert hits > 100


def test_halfspace_projection_at_the_named_points():
    s = np.array([3.0, -2.0, 1.0, 4.0])
    a = np.array([[1.0, 2.0, -2.0, 0.5]])  # a's = 3 - 4 - 2 + 2 = -1, exactly
    # dot == b exactly: not violated (the comparison is strict), the point stays bit for bit; the next b below violates
    got, hit, _ = check_halfspaces(s, a, [-1.0], expect_hit=0)
    assert np.array_equal(got, s)
    got, hit, _ = check_halfspaces(s, a, [np.nextafter(-1.0, -2.0)], expect_hit=1)
    # a row with b = +inf is never violated, whatever the point
    for big in (s, 1e300 * s):
        got, hit, _ = check_halfspaces(big, a, [np.inf], expect_hit=0)
        assert np.array_equal(got, big)
    # two rows that are both violated: the second sees the first one's result, so their order matters
    two = np.array([[1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]])
    b2 = np.array([1.0, -1.0])  # x <= 1 moves (3, -2) to (1, -2): x + y = -1 is then NOT violated; the other way round both are
    fwd, hit_fwd, _ = check_halfspaces(s, two, b2, expect_hit=1)
    rev, hit_rev, _ = check_halfspaces(s, two[::-1], b2[::-1], expect_hit=2)
    assert not np.allclose(fwd, rev)
    both = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 1.0, 1.0, 0.0]])
    bb = np.array([-3.0, -4.0])  # both violated in either order, with different results
    fwd, _, _ = check_halfspaces(s, both, bb, expect_hit=2)
    rev, _, _ = check_halfspaces(s, both[::-1], bb[::-1], expect_hit=2)
    assert np.max(np.abs(fwd - rev)) > 0.1
    # a row inside a mixed list with an infinite b leaves the others as they are
    mixed, _, _ = check_halfspaces(s, np.vstack([both[:1], a, both[1:]]), [bb[0], np.inf, bb[1]], expect_hit=2)
    assert np.array_equal(mixed, fwd)


# ---- the census itself

def test_census_is_off_by_default_and_does_not_change_a_solve(problems):
    prob = problems.rocket(10, with_linear=True)
    settings = F.SETTINGS["converging"]
    plain = O.OraclePort(prob).load_problem(prob, settings)
    counted = O.OraclePort(prob).load_problem(prob, settings)
    counted.enable_census(settings["max_iter"])
    for x0 in (F.ROCKET_X0[:, 1], F.ROCKET_X0[:, 0]):  # a cold and a warm solve
        for o in (plain, counted):
            o.set_x0(x0)
            o.solve()
        assert plain.stats() == counted.stats()
        for a, b in zip(plain.solution(), counted.solution()):
            np.testing.assert_array_equal(a, b)
        off, on = plain.family_census(), counted.family_census()
        assert all(v.size == 0 for v in off.values())
        its = counted.stats()["iter"]
        assert on["cone_x"].shape == (its, 10, 1) and on["cone_u"].shape == (its, 9, 1) and on["lin_x"].shape == (its, 10, 1) and on["lin_u"].shape == (its, 9, 0)
        assert on["cone_x"].max() <= 2 and on["lin_x"].max() <= 1
    # the record holds what the projections did: iteration 0 of a cold solve projects x + 0 and u + 0, which the test can redo itself
    counted.reset_workspace()
    counted.set_x0(F.ROCKET_X0[:, 2])
    counted.update_settings(max_iter=1)
    counted.solve()
    c = counted.family_census()
    # (vcnew is the projected slack; the unprojected one is x, the duals being zero)
    x, u = counted.get("x"), counted.get("u")
    for k in range(10):
        assert c["cone_x"][0, k, 0] == O.project_soc(x[0:3, k], 0.5)[1]
        assert c["lin_x"][0, k, 0] == int(-x[2, k] > 0.0)
    for k in range(9):
        assert c["cone_u"][0, k, 0] == O.project_soc(u[0:3, k], 0.25)[1]
    # beyond its capacity nothing is recorded, and switching it off frees it
    counted.enable_census(3)
    counted.update_settings(max_iter=8)
    counted.solve()
    assert counted.family_census()["cone_x"].shape[0] == 3 and counted.stats()["iter"] == 8
    counted.enable_census(0)
    counted.solve()
    assert counted.family_census()["cone_x"].size == 0


ROCKET_HORIZONS = [10, 20, 28, 30, 44, 100]


# ---- (b), (c) the rocket's six states; (d) the wide and large generators: the coverage condition per data set of the GPU file

def test_every_batched_rocket_horizon_is_asserted_here():
    assert {N for horizons, _ in F.ROCKET_BATCHED.values() for N in horizons} == set(ROCKET_HORIZONS)


@pytest.mark.parametrize("setting", list(F.SETTINGS))
@pytest.mark.parametrize("N", ROCKET_HORIZONS)
def test_rocket_states_cover_every_region(problems, N, setting):
    ref = F.rocket_reference(problems, N, setting)
    F.assert_covered(F.flat(ref), "rocket N=%d %s" % (N, setting))
    for kernel, (horizons, batch) in F.ROCKET_BATCHED.items():  # every weighting the GPU file compares this horizon under
        if N in horizons:
            F.assert_covered(F.flat(ref), "%s rocket N=%d x %d %s" % (kernel, N, batch, setting), weights=F.batch_weights(batch))
    F.assert_covered([pair[0] for pair in ref], "rocket N=%d %s, cold solves alone" % (N, setting))
    for pair in ref:
        for s in pair:
            assert np.all(np.isfinite(s.states)) and np.all(np.isfinite(s.controls)) and np.max(np.abs(s.states)) <= 51.0
    its = [pair[0].iter for pair in ref]
    if setting == "forced":
        assert its == [40] * 6
    else:  # only `nominal` converges from a cold start
        assert its[0] == {10: 35, 20: 70, 28: 113}.get(N, 120) and its[1:] == [120] * 5, its
    # high_rising is the ||w||^2 = 0 case of both cones. x0 has x = y = 0 and the lateral feedback rows of Kinf are exactly decoupled, so in
    # iteration 0 of its cold solve x, y and the lateral thrust are EXACTLY 0 at every knot (inside where t > 0: the state side's first knots;
    # the apex where t <= 0: the input side's first knots), and knot 0 of the state cone keeps w = (0, 0) in every iteration of that solve (its dual stays 0). (From iteration 1 on the
    # reference trajectory, which starts at x = 4, y = 2, pulls the other knots off the axis by 1e-6 and more.) The kernels clamp ||w||^2
    # to 1e-300 before they divide and the oracle does not; the projection is continuous there. This instance is the guard for that clamp.
    k = list(F.ROCKET_STATES).index("high_rising")
    prob = problems.rocket(N, with_linear=True)
    first = F.solve_sequence(prob, dict(F.SETTINGS[setting], max_iter=1), [F.ROCKET_X0[:, k]])[0]
    orc = O.OraclePort(prob).load_problem(prob, dict(F.SETTINGS[setting], max_iter=1))
    orc.set_x0(F.ROCKET_X0[:, k])
    orc.solve()
    x, u = orc.get("x"), orc.get("u")
    assert np.all(x[0:2] == 0.0) and np.all(u[0:2] == 0.0) and u[2, 0] < 0.0 and x[2, 0] > 0.0
    # (with w = 0 the outcome is the sign of t alone: inside for t > 0, the apex otherwise -- never the surface branch and its division)
    np.testing.assert_array_equal(first.census["cone_u"][0, :, 0], (u[2] > 0.0).astype(np.uint8))
    np.testing.assert_array_equal(first.census["cone_x"][0, :, 0], (x[2] > 0.0).astype(np.uint8))
    assert np.all(ref[k][0].states[0:2, 0] == 0.0) and np.all(ref[k][0].census["cone_x"][:, 0, 0] == 1)


@pytest.mark.parametrize("setting", list(F.SETTINGS))
def test_rocket_session_and_per_instance_rows_cover_every_region(problems, setting):
    for N in (10, 20, 44, 100):  # the resident session (N = 10) and the single-instance cases of layouts C and F
        F.assert_covered(F.rocket_session_reference(problems, N, setting), "rocket N=%d %s, twelve ticks of one instance" % (N, setting))
    ref = F.rocket_rows_reference(problems, 10, setting)
    F.assert_covered(F.flat(ref), "rocket N=10 %s, a row of its own per instance" % setting, weights=F.batch_weights(F.ROCKET_ROWS_BATCH))
    never = list(F.ROCKET_ROW_B).index(np.inf)
    assert all(np.all(s.census["lin_x"] == 0) for s in ref[never])
    # the rows matter: instances under another b than the problem's own solve another problem
    shared = F.rocket_reference(problems, 10, setting)
    assert sum(not np.array_equal(a[0].controls, b[0].controls) for a, b in zip(ref, shared)) >= 2


@pytest.mark.parametrize("setting", list(F.SETTINGS))
@pytest.mark.parametrize("shape", F.WIDE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wide_generator_covers_every_region(problems, shape, setting):
    _, _, ref = F.wide_reference(problems, *shape, setting)
    F.assert_covered(F.flat(ref), "wide %s %s" % (shape, setting))


@pytest.mark.parametrize("setting", list(F.SETTINGS))
@pytest.mark.parametrize("shape", F.LARGE_SHAPES, ids=lambda s: "x".join(map(str, s)).replace(" ", "-"))
def test_large_generator_covers_every_region(problems, shape, setting):
    _, _, ref = F.large_reference(problems, *shape, setting)
    F.assert_covered(F.flat(ref), "large %s %s" % (shape, setting))


def _statements(fn):
    """The statements of a generator in family_region_cases.py: its source lines without the signature, the docstring and the return."""
    lines = [line.strip() for line in inspect.getsource(fn).splitlines()]
    end_of_doc = max(i for i, line in enumerate(lines) if line.endswith('"""'))
    return [line for line in lines[end_of_doc + 1:] if line and not line.startswith("return ")]


def test_the_copied_generators_are_still_the_originals():
    """wide_problem and large_problem restate the systems of two existing GPU tests so that the new cases share their run-time
    specialisations. Every statement of the copies must stand, verbatim, in the source of the test it was taken from: if either side
    changes, this fails instead of the cases drifting apart silently."""
    import test_hip_families
    import test_large_systems_gpu
    for copy, original in ((F.wide_problem, test_hip_families.test_families_on_wide_systems),
                           (F.large_problem, test_large_systems_gpu.test_families_on_large_systems)):
        source = [line.strip() for line in inspect.getsource(original).splitlines()]
        statements = _statements(copy)
        assert len(statements) >= 9, statements
        for line in statements:
            assert line in source, "%s: `%s` is not in %s" % (copy.__name__, line, original.__name__)

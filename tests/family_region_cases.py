"""Inputs that reach every outcome of the cone and half-space projections, and the oracle's census of them (helper module of
test_family_regions_cpu.py and test_family_regions_gpu.py; no test lives here).

The second-order-cone projection has three outcomes (apex / inside / surface), the half-space projection two (row not violated /
violated). The rocket landing from its nominal initial state leaves most of them untouched at the short horizons the register-resident
family kernels run at, so these cases start the vehicle underground, flying sideways, below the glide cone's apex and rising fast. What
a case must cover is asserted on the ORACLE's census (OraclePort.family_census), never on the device: `assert_covered`.

Every case is solved twice per setting: cold from its own state, then again from the duals the first solve left with the states
rotated by one, so that the warm start lands in another region."""
from __future__ import annotations

import functools

import numpy as np

import pyoracle as O

ROCKET_STATES = {  # name -> x0 of problems.rocket(N, with_linear=True): x, y, z, vx, vy, vz
    "nominal": [4.4, 2.2, 22.0, -3.3, 2.2, -4.95],
    "underground_rising": [1.0, -1.0, -0.3, 0.0, 0.0, 5.0],
    "fast_lateral": [0.1, 0.1, 1.0, 8.0, -8.0, 0.0],
    "apex_state": [0.05, 0.05, -0.4, 0.0, 0.0, -1.0],
    # x = y = 0: in iteration 0 of a cold solve x, y and the lateral thrust are exactly 0 at every knot, and at knot 0 in every iteration:
    # ||w||^2 = 0 on both cones (inside on the state side, the apex on the input side). The kernels clamp ||w||^2 to 1e-300 before the
    # division, the oracle does not: this instance is the guard for the clamp (test_family_regions_cpu.py asserts the zeros).
    "high_rising": [0.0, 0.0, 30.0, 0.0, 0.0, 15.0],
    "high_rising_offaxis": [2.0, -1.0, 35.0, 1.0, 0.0, 18.0],
}
ROCKET_X0 = np.array(list(ROCKET_STATES.values()), dtype=np.float64).T  # (6, 6): column i = state i

SETTINGS = {
    "forced": dict(max_iter=40, abs_pri_tol=0.0, abs_dua_tol=0.0),          # 40 iterations, whatever the residuals
    "converging": dict(max_iter=120, abs_pri_tol=2e-3, abs_dua_tol=1e-4),   # `nominal` converges, the others run all 120
}
MIN_SHARE = 0.02  # every outcome takes at least this share of its side's projections

# The batched rocket cases of test_family_regions_gpu.py: kernel -> (horizons, batch). The six states are repeated cyclically to the batch,
# so a ragged batch (6 k + 1) weighs state 0 once more: test_family_regions_cpu.py asserts the coverage condition under each weighting.
ROCKET_BATCHED = {
    "layout A": ((10, 30), 13),
    "layout C": ((20,), 6),
    "layout D": ((10, 20), 301),                            # 6 * 50 + 1: beyond the latency kernels' range
    "layout E, cut (the library's choice)": ((28,), 301),   # the horizon layout D no longer holds with the families in registers
    "layout E": ((10, 44, 100), 199),                       # 6 * 33 + 1: a ragged last group of four
    "layout F": ((10, 20, 44, 100), 7),
}
ROCKET_ROWS_BATCH = 13  # k_admm_solve_ifam, N = 10


def batch_weights(batch):
    """How many instances of a batch carry each of the six states, once per Solve of flat(reference) (cold and warm)."""
    return np.repeat(np.bincount(np.arange(batch) % 6, minlength=6), 2)


class Solve:
    """What the oracle returned for one solve of one instance."""

    def __init__(self, orc):
        st = orc.stats()
        self.states, self.controls = (a.copy() for a in orc.solution())
        self.iter, self.status = st["iter"], st["status"]
        self.residuals = np.array([st["pri_x"], st["dua_x"], st["pri_u"], st["dua_u"]])
        self.census = orc.family_census()


def solve_sequence(prob, settings, x0_sequence, rows=None):
    """One oracle, census on, solving x0_sequence one after another without a reset (warm starts) -> [Solve, ...]."""
    orc = O.OraclePort(prob).load_problem(prob, settings)
    if rows is not None:
        orc.set_linear_constraints(*rows)
    orc.enable_census(settings["max_iter"])
    out = []
    for x0 in x0_sequence:
        orc.set_x0(np.asarray(x0, dtype=np.float64))
        orc.solve()
        out.append(Solve(orc))
    return out


def rotated(x0s):
    """The states of the second solve: instance i gets what instance i + 1 had."""
    return np.roll(x0s, -1, axis=1)


@functools.lru_cache(maxsize=None)
def rocket_reference(problems, N, setting):
    """The six states on rocket(N): [state i] -> [cold Solve, warm Solve from those duals on state i + 1]. Computed once, never changed."""
    prob = problems.rocket(N, with_linear=True)
    second = rotated(ROCKET_X0)
    return [solve_sequence(prob, SETTINGS[setting], (ROCKET_X0[:, i], second[:, i])) for i in range(ROCKET_X0.shape[1])]


@functools.lru_cache(maxsize=None)
def rocket_session_reference(problems, N, setting):
    """One instance, twelve warm-started ticks: the six states in turn, then the six again -> [Solve] * 12."""
    prob = problems.rocket(N, with_linear=True)
    return solve_sequence(prob, SETTINGS[setting], [ROCKET_X0[:, k % 6] for k in range(12)])


# The ground-plane row -z <= b with a b of its own per instance (k_admm_solve_ifam): instance j carries ROCKET_ROW_B[j % 6]. One plane
# above the ground, some below it, the problem's own (0), and +inf: a row that is there and can never be violated.
ROCKET_ROW_B = np.array([0.0, 0.25, np.inf, -0.1, -2.0, 0.5])


@functools.lru_cache(maxsize=None)
def rocket_rows_reference(problems, N, setting):
    """As rocket_reference, instance i under the row -z <= ROCKET_ROW_B[i] in both solves."""
    prob = problems.rocket(N, with_linear=True)
    second = rotated(ROCKET_X0)
    A = np.asarray(prob.linear["Alin_x"], dtype=np.float64)
    return [solve_sequence(prob, SETTINGS[setting], (ROCKET_X0[:, i], second[:, i]),
                           rows=(A, np.array([ROCKET_ROW_B[i]]), np.zeros((0, prob.nu)), np.zeros(0))) for i in range(6)]


# ---- the wide (32 / 64 lanes per instance) and large (layout M) random systems

def wide_problem(P, nx, nu, N):
    """The generator of test_hip_families.test_families_on_wide_systems, line for line (test_family_regions_cpu.py holds the two
    together: every statement below must stand in that test's source) -> (problem, its rng after the problem)."""
    rng = np.random.default_rng(nx * 100 + nu)
    A = 0.9 * np.eye(nx) + (0.15 / np.sqrt(nx)) * rng.standard_normal((nx, nx))
    Bm = 0.3 * rng.standard_normal((nx, nu))
    prob = P.Problem("widefam", A, Bm, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(0.5, 2, nu)), N, 1.5, rng.standard_normal(nx))
    prob.x_min, prob.x_max = np.full(nx, -3.0), np.full(nx, 3.0)
    prob.u_min, prob.u_max = np.full(nu, -1.0), np.full(nu, 1.0)
    prob.fdyn = 0.01 * rng.standard_normal(nx)
    prob.cones = dict(Acx=[0, 13, 15], qcx=[3, 5, 3], cx=[0.8, 0.6, 1.1], Acu=[0], qcu=[3], cu=[0.7])  # rows 0-2 | 13-17 | 15-17 (shares rows)
    prob.linear = dict(Alin_x=rng.standard_normal((3, nx)), blin_x=rng.uniform(0.5, 1.5, 3), Alin_u=rng.standard_normal((2, nu)), blin_u=rng.uniform(0.3, 0.8, 2))
    return prob, rng


def large_problem(P, nx, nu, N, form):
    """The generator of test_large_systems_gpu.test_families_on_large_systems, line for line (held together in the same way) ->
    (problem, its rng after the problem)."""
    rng = np.random.default_rng(nx * 10 + nu)
    A = 0.9 * np.eye(nx) + (0.15 / np.sqrt(nx)) * rng.standard_normal((nx, nx))
    if nx >= 256:
        A = 0.6 * np.eye(nx) + (0.1 / np.sqrt(nx)) * rng.standard_normal((nx, nx))
    Bm = 0.3 * rng.standard_normal((nx, nu))
    prob = P.Problem("largefam", A, Bm, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(0.5, 2, nu)), N, 1.5, rng.standard_normal(nx))
    prob.x_min, prob.x_max = np.full(nx, -3.0), np.full(nx, 3.0)
    prob.u_min, prob.u_max = np.full(nu, -1.0), np.full(nu, 1.0)
    prob.fdyn = 0.01 * rng.standard_normal(nx)
    prob.cones = dict(Acx=[0, 13, 15, 20], qcx=[3, 6, 3, 41], cx=[0.8, 0.6, 1.1, 0.9], Acu=[0, 5], qcu=[3, 4], cu=[0.7, 1.3])
    nlx = 10 if form == "ten rows" else 3
    prob.linear = dict(Alin_x=rng.standard_normal((nlx, nx)) / np.sqrt(nx), blin_x=rng.uniform(0.1, 0.4, nlx),
                       Alin_u=rng.standard_normal((2, nu)) / np.sqrt(nu), blin_u=rng.uniform(0.1, 0.3, 2))
    return prob, rng


def shaped_x0(prob, rng, batch):
    """The generators' x0 columns (standard normal, scaled 0.1 .. 1 across the batch), shaped so that every cone outcome occurs: the
    entries on the state cones' t rows (the last row of each cone) are made NEGATIVE for every third instance (the polar cone: apex) and
    POSITIVE and three times as large for every third (inside); the last third keeps the generator's. The input cones see x0 only
    through u = -Kinf x - d, and the generators' columns leave their `inside` outcome near 1 % of the projections: every fourth
    instance therefore starts where the feedback's first control lies ON the input cones' axes, x0 = -pinv(Kinf) e_t scaled by 1 .. 2
    (e_t: ones on the input cones' t rows), with Kinf read from the oracle."""
    x0s = rng.standard_normal((prob.nx, batch)) * np.linspace(0.1, 1.0, batch)[None, :]
    t_rows = sorted({int(a) + int(q) - 1 for a, q in zip(prob.cones["Acx"], prob.cones["qcx"])})
    axis = np.zeros(prob.nu)
    axis[sorted({int(a) + int(q) - 1 for a, q in zip(prob.cones["Acu"], prob.cones["qcu"])})] = 1.0
    on_axis = -np.linalg.pinv(O.OraclePort(prob).get("Kinf")) @ axis
    for b in range(batch):
        if b % 3 == 0:
            x0s[t_rows, b] = -np.abs(x0s[t_rows, b]) - 0.5
        elif b % 3 == 1:
            x0s[t_rows, b] = 3.0 * np.abs(x0s[t_rows, b]) + 0.5
        if b % 4 == 3:
            x0s[:, b] = on_axis * (1.0 + b / batch)
    return np.asfortranarray(x0s)


WIDE_SHAPES = [(24, 8, 10, 19), (48, 16, 6, 19)]  # nx, nu, N, batch: 32 and 64 lanes per instance, batch >= 16 (layout D's wide kernels)
LARGE_SHAPES = [(70, 10, 8, 5, "one-pass"), (70, 10, 8, 5, "ten rows")]  # the smallest shape of each form of layout M's cone phase


def _random_reference(prob, rng, batch, setting):
    x0s = shaped_x0(prob, rng, batch)
    second = rotated(x0s)
    return x0s, [solve_sequence(prob, SETTINGS[setting], (x0s[:, b], second[:, b])) for b in range(batch)]


@functools.lru_cache(maxsize=None)
def wide_reference(problems, nx, nu, N, batch, setting):
    """-> (problem, x0s (nx, batch), [instance b] -> [cold Solve, warm Solve on instance b + 1's state])."""
    prob, rng = wide_problem(problems, nx, nu, N)
    return (prob,) + _random_reference(prob, rng, batch, setting)


@functools.lru_cache(maxsize=None)
def large_reference(problems, nx, nu, N, batch, form, setting):
    prob, rng = large_problem(problems, nx, nu, N, form)
    return (prob,) + _random_reference(prob, rng, batch, setting)


# ---- the coverage condition

SIDES = {"state cone": (("cone_x",), 3), "input cone": (("cone_u",), 3), "rows": (("lin_x", "lin_u"), 2)}
OUTCOMES = {3: ("apex", "inside", "surface"), 2: ("not violated", "violated")}


def region_counts(solves, weights=None):
    """{side: counts per outcome} over `solves` (Solve objects); weights[i] = how many instances of the batch solve i stands for."""
    counts = {side: np.zeros(n, dtype=np.int64) for side, (_, n) in SIDES.items()}
    for i, s in enumerate(solves):
        w = 1 if weights is None else int(weights[i])
        for side, (keys, n) in SIDES.items():
            for key in keys:
                c = s.census[key]
                assert c.shape[0] == s.iter, (key, c.shape, s.iter)  # every iteration of the solve was recorded
                assert not c.size or int(c.max()) < n, (key, int(c.max()))   # ... and every projection in it
                counts[side] += w * np.bincount(c.ravel(), minlength=n)[:n]
    return counts


def has_mixed_iteration(solves, side):
    """Some solve has an iteration in which one cone (or row) takes different outcomes at different knots: the lane-divergent select."""
    for s in solves:
        for key in SIDES[side][0]:
            c = s.census[key]  # [iteration, knot, cone or row]
            if c.size and np.any(c.min(axis=1) != c.max(axis=1)):
                return True
    return False


def format_counts(counts):
    return "state cone %d / %d / %d, input cone %d / %d / %d, rows %d / %d" % (*counts["state cone"], *counts["input cone"], *counts["rows"])


def assert_covered(solves, tag, weights=None):
    """The coverage condition on the oracle's census of exactly the solves a test compares. Prints the eight counts, returns them."""
    counts = region_counts(solves, weights)
    print(tag, "census (apex / inside / surface, not violated / violated):", format_counts(counts))
    for side, c in counts.items():
        total = int(c.sum())
        assert total > 0, (tag, side)
        for name, n in zip(OUTCOMES[len(c)], c):
            assert n >= MIN_SHARE * total, "%s: %s '%s' takes %d of %d projections, less than %g" % (tag, side, name, n, total, MIN_SHARE)
        assert has_mixed_iteration(solves, side), "%s: no iteration of any instance mixes outcomes of the %s over its knots" % (tag, side)
    return counts


def flat(reference):
    """[instance] -> [Solve, Solve]  ->  every Solve, and nothing else."""
    return [s for pair in reference for s in pair]

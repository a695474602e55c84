"""Data and oracle references of the per-instance cone-slope tests (test_instance_cones_cpu / _gpu / _d_gpu): no test lives here.

The recipe (seed SEED = 11, looked at with the plain-C oracle alone): x0_b = x0 * (1 + 0.1 randn); every slope is the shared value times
exp(U(ln 0.4, ln 2.5)), drawn for the state side first and then the input side; the problem is problems.rocket(N) with its shared
ground-plane row and fdyn left in; the converging cases run CONV, the others FORCED iterations; the samples are the instances
{0, 1, B//2, B-2, B-1}.

Sample conditions of a CONV case, asserted on the oracle's own results (assert_sample_conditions): at least two samples converge before
max_iter and at least one does not; at least half of the samples move their controls by more than 1e-3 (relative) against the shared
slopes, and at least half against the next sample's slopes; on each side at least 20 % of the sampled cone projections are "inside"
and at least 20 % "surface" (OraclePort.family_census)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
from conftest import rel_err

import pyoracle as O

SEED = 11
CONV = dict(max_iter=300, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
FORCED = dict(max_iter=60, abs_pri_tol=0.0, abs_dua_tol=0.0)
TWO_ROUNDS = dict(Acx=[0, 2], qcx=[3, 3], cx=[0.5, 2.0])  # two state cones that share row 2: two rounds


def sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1})


def with_cones(prob, **cones):
    return dataclasses.replace(prob, cones=dict(prob.cones, **cones))


def held(prob):
    """The problem with its reference held at the trajectory's first column: layout D's per-instance forms take references that are
    constant over the horizon (test_instance_lin_d_gpu._rocket does the same)."""
    return dataclasses.replace(prob, x_ref=np.repeat(prob.x_ref[:, :1], prob.N, axis=1))


def slopes(prob, batch, seed=SEED):
    """-> x0s (nx, batch), cx (ncx, batch), cu (ncu, batch): the recipe of the module docstring."""
    rng = np.random.default_rng(seed)
    x0s = np.asfortranarray(prob.x0[:, None] * (1.0 + 0.1 * rng.standard_normal((prob.nx, batch))))
    out = []
    for key in ("cx", "cu"):
        shared = np.asarray(prob.cones.get(key, []), dtype=np.float64)
        out.append(np.asfortranarray(shared[:, None] * np.exp(rng.uniform(np.log(0.4), np.log(2.5), (shared.size, batch)))))
    return x0s, out[0], out[1]


def oracle(prob, settings, cx=None, cu=None, **flags):
    """The oracle of one instance: the problem (its cone structure, rows and fdyn included) under the slopes cx | cu (None: the shared ones)."""
    pb = prob if cx is None and cu is None else with_cones(prob, cx=list(prob.cones["cx"] if cx is None else cx),
                                                           cu=list(prob.cones["cu"] if cu is None else cu))
    orc = O.OraclePort(pb).load_problem(pb, settings)
    if flags:
        orc.update_settings(**flags)
    return orc


def resend(orc, prob, cx, cu):
    """New slopes on a live oracle: the workspace, the cones' duals included, is kept (as the verb keeps it)."""
    c = prob.cones
    orc.set_cone_constraints(c["Acx"], c["qcx"], list(cx), c["Acu"], c["qcu"], list(cu))
    orc.update_settings()


def run(orc, x0, census=False):
    if census:
        orc.enable_census(orc._settings["max_iter"])
    orc.set_x0(x0)
    orc.solve()
    st = orc.stats()
    out = (orc.solution()[0].copy(), orc.solution()[1].copy(), st["iter"], st["status"],
           np.array([st[k] for k in ("pri_x", "dua_x", "pri_u", "dua_u")]))  # (the order of get_stats_batch()["residuals"])
    return out + ((orc.family_census(),) if census else ())


@functools.lru_cache(maxsize=None)
def reference(pkg, name):
    """Computed once per case and shared: per sampled instance the oracle's cold solve under its own slopes (with the census), under the
    shared slopes and under the next sample's slopes."""
    prob, batch, settings, x0s, cx, cu = data(pkg, name)
    samples = sample(batch)
    own, shared, other = {}, {}, {}
    for i, b in enumerate(samples):
        nb = samples[(i + 1) % len(samples)]
        own[b] = run(oracle(prob, settings, cx[:, b], cu[:, b]), x0s[:, b], census=True)
        shared[b] = run(oracle(prob, settings), x0s[:, b])
        other[b] = run(oracle(prob, settings, cx[:, nb], cu[:, nb]), x0s[:, b])
    return own, shared, other


def _wide(pkg, nx, nu, N):
    """test_instance_bounds_gpu._wide(P, nx, nu, N) -- the wide systems of the per-instance tests, which carry neither cones nor rows -- with
    the cone list of the families' wide tests (family_region_cases.wide_problem: the second and third state cone share rows 15-17, so the
    reduced path walks two rounds) and two shared rows per side: instance 0 of the rows test_instance_lin_gpu draws for the system."""
    from test_instance_bounds_gpu import _wide as wide
    from test_instance_lin_gpu import _of, _rows
    prob = wide(pkg.problems, nx, nu, N)
    prob.cones = dict(Acx=[0, 13, 15], qcx=[3, 5, 3], cx=[0.8, 0.6, 1.1], Acu=[0], qcu=[3], cu=[0.7])
    Ax, bx, Au, bu = _of(_rows(prob, 2, 2, 3)[1:], 0)
    prob.linear = dict(Alin_x=Ax, blin_x=bx, Alin_u=Au, blin_u=bu)
    return prob


def solver(pkg, prob, batch, settings):
    """A handle on the whole problem: bounds, references, the cone structure with its shared slopes, the shared rows, fdyn."""
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if prob.x_ref is not None:
        s.set_x_ref(prob.x_ref)
    if prob.u_ref is not None:
        s.set_u_ref(prob.u_ref)
    if prob.cones:
        s.set_cone_constraints(**prob.cones)
    if prob.linear:
        s.set_linear_constraints(**prob.linear)
    return s


def assert_matches(s, expect, tag, tol=1e-9):
    """Per sampled instance: states and controls within tol, equal iteration counts and status, the four residuals within 1e-6."""
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, ref in expect.items():
        ox, ou, it, status, res = ref[:5]
        ex, eu, er = rel_err(sol["states"][:, :, b], ox), rel_err(sol["controls"][:, :, b], ou), rel_err(st["residuals"][:, b], res)
        print(tag, "instance", b, "iter", st["iter"][b], it, "status", st["status"][b], status, "rel_err x %.2e u %.2e residuals %.2e" % (ex, eu, er))
        assert st["iter"][b] == it and st["status"][b] == status, (tag, b)
        assert ex < tol and eu < tol and er < 1e-6, (tag, b, ex, eu, er)


def bits(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return [sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()]


def assert_same_bits(a, b):
    """Solution, iterations, status and the four residuals of two handles (or recorded bits()) are equal bit for bit."""
    a, b = (x if isinstance(x, list) else bits(x) for x in (a, b))
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


HELD_SEED = 32  # the held-reference cases: the first seed from 0 at which all three meet the sample conditions (seed 11 leaves 9-16 % of the state-cone projections inside)
CASES = {  # name -> (problem, batch, settings, seed); batches are ragged on purpose
    "rocket10": (lambda pkg: pkg.problems.rocket(10), 37, CONV, SEED),
    "rocket20": (lambda pkg: pkg.problems.rocket(20), 37, CONV, SEED),
    "rocket30": (lambda pkg: pkg.problems.rocket(30), 21, FORCED, SEED),                                       # a horizon layout D does not take
    "rocket20-two-rounds": (lambda pkg: with_cones(pkg.problems.rocket(20), **TWO_ROUNDS), 21, FORCED, SEED),  # slopes in both rounds
    "wide32": (lambda pkg: _wide(pkg, 24, 8, 20), 21, FORCED, SEED),                                           # 32 lanes: the reduced path
    "wide64": (lambda pkg: _wide(pkg, 48, 16, 12), 9, FORCED, SEED),                                           # 64 lanes
    "rocket10-no-rows": (lambda pkg: pkg.problems.rocket(10, with_linear=False), 37, CONV, SEED),              # the slope half with no linear family
    # layout D's cases: references constant over the horizon
    "rocket10-held": (lambda pkg: held(pkg.problems.rocket(10)), 37, CONV, HELD_SEED),
    "rocket20-held": (lambda pkg: held(pkg.problems.rocket(20)), 37, CONV, HELD_SEED),
    "rocket10-held-no-rows": (lambda pkg: held(pkg.problems.rocket(10, with_linear=False)), 37, CONV, HELD_SEED),
    "rocket20-held-two-rounds": (lambda pkg: held(with_cones(pkg.problems.rocket(20), **TWO_ROUNDS)), 21, FORCED, SEED),
}
# the converging cases: their sample conditions are asserted on the oracle alone (the issue's recipe for the first two; the others were
# looked at with the oracle only)
CONDITIONED = ["rocket10", "rocket20", "rocket10-no-rows", "rocket10-held", "rocket20-held", "rocket10-held-no-rows"]


def case(pkg, name):
    make, batch, settings, _ = CASES[name]
    return make(pkg), batch, settings


def data(pkg, name):
    """-> problem, batch, settings, x0s, cx, cu of a case (its own seed)."""
    prob, batch, settings = case(pkg, name)
    return (prob, batch, settings) + slopes(prob, batch, CASES[name][3])


def census_shares(own):
    """-> {side: (inside share, surface share)} over the sampled instances' cone projections (0 apex / 1 inside / 2 surface; 255: none ran)."""
    out = {}
    for side in ("cone_x", "cone_u"):
        a = np.concatenate([own[b][5][side].ravel() for b in own])
        a = a[a != 255]
        out[side] = (float(np.mean(a == 1)), float(np.mean(a == 2))) if a.size else (0.0, 0.0)
    return out


def assert_sample_conditions(name, settings, own, shared, other):
    its = [own[b][2] for b in own]
    moved = [rel_err(own[b][1], shared[b][1]) for b in own]
    differ = [rel_err(own[b][1], other[b][1]) for b in own]
    shares = census_shares(own)
    print(name, "oracle iterations", its, "moved", moved, "differ", differ, "census (inside, surface)", shares)
    assert sum(i < settings["max_iter"] for i in its) >= 2 and sum(i >= settings["max_iter"] for i in its) >= 1
    assert 2 * sum(m > 1e-3 for m in moved) >= len(moved) and 2 * sum(d > 1e-3 for d in differ) >= len(differ)
    for side, (inside, surface) in shares.items():
        assert inside >= 0.2 and surface >= 0.2, (side, inside, surface)

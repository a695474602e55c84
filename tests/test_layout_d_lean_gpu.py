"""Layout D's lean kernels (tinympc_lean_d.hip; tinympc_plan.hip: lean_applies) against the plain ones.

An iteration whose residuals nothing can read -- no termination check falls on it, or the tolerances cannot be met and a later check
overwrites its snapshot -- runs a forward sweep without the residual maxima, without the "can this sweep still converge" tests and
without R1:  need_res(it1) = check(it1) && (reachable || it1 + check_termination > max_iter).  What remains of a sweep is the same
instructions on the same operands, so everything a solve returns -- states, controls, iteration counts, status, the four
residuals, and the stale v|z a converged instance leaves behind (seen through the next, warm solve) -- must EQUAL the plain kernel's
(TINYMPC_LEAN=0) bit for bit; a sample of the converging batch is checked against the oracle as well (iteration counts exact, 1e-9 on
the trajectories: the bar of test_slot_refill_gpu.py)."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
WHAT = ("states", "controls", "iterations", "status", "residuals")


def _everything(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


def _both(pkg, monkeypatch, prob, batch, settings, x0s, configure=None, warm_scale=1.0, rho=None):
    """{lean?: (cold solve, warm solve)} of two fresh handles, the plain kernel (TINYMPC_LEAN=0) and the lean one (=1)."""
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")  # (small batches would go to the latency layouts)
    monkeypatch.setenv("TINYMPC_REFILL", "0")
    got = {}
    for lean in (False, True):
        monkeypatch.setenv("TINYMPC_LEAN", "1" if lean else "0")
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho if rho is None else rho, fdyn=prob.fdyn, **settings)
        if prob.has_bounds():
            s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if configure:
            configure(s)
        s.set_x0_batch(x0s)
        s.solve()
        # (asked after the first solve: the kernel for per-knot tables is decided when a launch first needs it)
        assert s.launch_info()["layout"] == "D" and "compiled-in" in s.jit_info(), s.jit_info()
        assert ("lean" in s.jit_info().split()) == lean, s.jit_info()
        cold = _everything(s)
        if warm_scale != 1.0:
            s.set_x0_batch(np.asfortranarray(warm_scale * x0s))
        s.solve()
        got[lean] = (cold, _everything(s))
        s.reset()
    return got


def _assert_equal(got, tag=""):
    for k, name in enumerate(("cold", "warm")):
        for a, b, what in zip(got[False][k], got[True][k], WHAT):
            np.testing.assert_array_equal(a, b, err_msg=f"{tag} {name} solve: {what}")


@pytest.mark.parametrize("batch", [256, 1001])
def test_headline_configuration_is_bit_identical(pkg, monkeypatch, batch):
    """Tolerances 0, a check in every iteration, 200 iterations: 199 lean sweeps and the one whose residuals are returned."""
    P = pkg.problems
    prob = P.quadrotor(50)
    settings = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=200, check_termination=1)
    got = _both(pkg, monkeypatch, prob, batch, settings, P.quadrotor_batch_x0(batch))
    _assert_equal(got)
    cold = got[True][0]
    assert np.all(cold[2] == 200) and np.all(cold[3] != 1)
    assert np.all(np.isfinite(cold[4])) and np.all(cold[4].max(axis=0) > 0)  # (the residuals of iteration 200, from the one full sweep)


@pytest.mark.parametrize("max_iter", [1, 7, 50])
@pytest.mark.parametrize("ct", [0, 2, 3, 7, 10])
def test_forced_iteration_counts_with_any_check_interval(pkg, monkeypatch, ct, max_iter):
    """The last check of a launch is rarely its last iteration, and there may be none at all (check_termination 0, or larger than
    max_iter): the statistics are then left as the plain kernel leaves them."""
    P = pkg.problems
    prob = P.quadrotor(50)
    batch = 517
    settings = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=max_iter, check_termination=ct)
    got = _both(pkg, monkeypatch, prob, batch, settings, P.quadrotor_batch_x0(batch), warm_scale=0.9)
    _assert_equal(got, f"ct={ct} max_iter={max_iter}")
    assert np.all(got[True][0][2] == max_iter) and np.all(got[True][0][3] != 1)


@pytest.mark.parametrize("ct", [3, 10])
def test_converging_batch_is_bit_identical_and_matches_the_oracle(pkg, monkeypatch, ct):
    """Tolerances that can be met: the sweeps between two checks are lean, the checked ones keep residuals, stale copies and the
    early verdicts. Instances converge at different checks (their wavefront's other rows go on as before), some never; the warm
    solve starts from the state -- the stale v|z of the converged ones included -- that the cold one left."""
    P = pkg.problems
    prob = P.quadrotor(50)
    B = 2051
    rng = np.random.default_rng(B + ct)
    x0s = np.asfortranarray(P.quadrotor_batch_x0(B) * rng.uniform(0.05, 3.0, B)[None, :])
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=ct)
    got = _both(pkg, monkeypatch, prob, B, settings, x0s, warm_scale=0.9)
    _assert_equal(got, f"ct={ct}")
    st, sc, it, status, _ = got[True][0]
    assert it.min() < 60 and len(np.unique(it)) > 1  # (instances stop at different checks)
    assert np.all(it[status == 1] % ct == 0) and np.all(status[it < 60] == 1)
    sample = np.random.default_rng(1).choice(B, size=16, replace=False)
    orc = O.OraclePort(prob).load_problem(prob, settings)
    ox, ou, oit, ost, _ = orc.solve_batch(x0s[:, sample])
    np.testing.assert_array_equal(it[sample], oit)
    np.testing.assert_array_equal(status[sample] == 1, np.asarray(ost) == 1)
    assert rel_err(st[:, :, sample], ox) < TOL
    assert rel_err(sc[:, :, sample], ou) < TOL


def _goal_refs(prob, batch, seed):
    rng = np.random.default_rng(seed)
    return 0.4 * rng.standard_normal((prob.nx, batch)), 0.05 * rng.standard_normal((prob.nu, batch))


@pytest.mark.parametrize("form", ["shared_refs", "goals", "bounds", "goals_and_bounds"])
@pytest.mark.parametrize("tol,ct", [(0.0, 1), (1e-3, 4)])
def test_table_forms_are_bit_identical(pkg, monkeypatch, form, tol, ct):
    """The shared constant table with nonzero references, and the per-instance goal form: one goal and / or one box per instance."""
    P = pkg.problems
    prob = P.quadrotor(50)
    batch = 777
    gx, gu = _goal_refs(prob, batch, seed=5)
    rng = np.random.default_rng(6)
    wx, wu = rng.uniform(0.6, 1.4, (prob.nx, batch)), rng.uniform(0.6, 1.4, (prob.nu, batch))
    xmin, xmax = np.asarray(prob.x_min).reshape(-1, 1), np.asarray(prob.x_max).reshape(-1, 1)
    umin, umax = np.asarray(prob.u_min).reshape(-1, 1), np.asarray(prob.u_max).reshape(-1, 1)

    def configure(s):
        if form == "shared_refs":
            s.set_x_ref(np.repeat(gx[:, :1], prob.N, axis=1))
            s.set_u_ref(np.repeat(gu[:, :1], prob.N - 1, axis=1))
        if form in ("goals", "goals_and_bounds"):
            s.set_x_ref_batch(gx)
            s.set_u_ref_batch(gu)
        if form in ("bounds", "goals_and_bounds"):
            s.set_bound_constraints_batch(xmin * wx, xmax * wx, umin * wu, umax * wu)

    settings = dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=40, check_termination=ct)
    x0s = np.asfortranarray(P.quadrotor_batch_x0(batch) * rng.uniform(0.05, 3.0, batch)[None, :])
    got = _both(pkg, monkeypatch, prob, batch, settings, x0s, configure, warm_scale=0.9, rho=0.37)
    _assert_equal(got, form)


@pytest.mark.parametrize("tol,ct", [(0.0, 1), (1e-4, 3)])
def test_reference_trajectory_is_bit_identical(pkg, monkeypatch, tol, ct):
    """References that vary over the horizon: the kernels with per-knot tables (CT false; compiled in for the cartpole)."""
    P = pkg.problems
    prob = P.cartpole(20, True)
    batch = 523
    rng = np.random.default_rng(9)
    X = 0.3 * np.sin(0.4 * np.arange(prob.N)[None, :] + np.arange(prob.nx)[:, None])
    U = 0.05 * np.cos(0.3 * np.arange(prob.N - 1)[None, :]) * np.ones((prob.nu, 1))

    def configure(s):
        s.set_x_ref(X)
        s.set_u_ref(U)

    x0s = np.asfortranarray(np.asarray(prob.x0).reshape(-1, 1) + 0.2 * rng.standard_normal((prob.nx, batch)))
    settings = dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=50, check_termination=ct)
    got = _both(pkg, monkeypatch, prob, batch, settings, x0s, configure, warm_scale=0.8)
    _assert_equal(got)


def test_the_plan_takes_the_lean_kernel_only_where_some_residuals_cannot_be_read(pkg, monkeypatch):
    monkeypatch.delenv("TINYMPC_LEAN", raising=False)
    monkeypatch.delenv("TINYMPC_REFILL", raising=False)
    P = pkg.problems
    prob = P.quadrotor(50)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=8192, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=20, check_termination=1)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    lean = lambda: "lean" in s.jit_info().split()
    assert s.launch_info()["layout"] == "D" and lean()            # forced iteration counts (the headline)
    s.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    assert not lean()                                                # a check in every iteration, tolerances that can be met
    s.update_settings(check_termination=10)
    assert lean()                                                    # nine of ten sweeps are not checked
    s.update_settings(check_termination=0)
    assert lean()                                                    # no check at all
    s.update_settings(check_termination=1, abs_pri_tol=1e-3, abs_dua_tol=0.0)
    assert lean()                                                    # one tolerance nothing can meet
    monkeypatch.setenv("TINYMPC_LEAN", "0")
    assert not lean()
    s.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    monkeypatch.setenv("TINYMPC_LEAN", "1")
    assert lean()
    s.reset()
    # slot refill (a converging batch beyond one resident set) keeps its own kernel
    monkeypatch.delenv("TINYMPC_LEAN", raising=False)
    big = pkg.TinyMPC()
    big.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=9001, rho=prob.rho, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=20, check_termination=3)
    big.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    assert "slot-refill" in big.jit_info() and "lean" not in big.jit_info().split()
    big.reset()

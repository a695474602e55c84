"""Layout D's box path with the work that does not change within a launch taken out of the sweeps (tinympc_solve_d.hip, K0 / FOLD):
forward step 0 starts from c0 = cf + Mf[:, :nx] * x_0, and with references constant over the horizon the backward operator's input
columns carry -rho while the accumulator starts carry Mb[:, nx:] * lr. The headline runs with zero references and rho = 5, so the
fold's accumulator term is exercised here: constant NONZERO references, rho that is not a power of two, cold and warm starts, the
compiled-in kernels and a run-time specialised one -- against the oracle (iteration counts and statuses exact, 1e-9 on the
trajectories: the bar of test_hip_parity.py) -- and the kernels that must agree bit for bit still do: shared references against the
per-instance goal kernel, the plain kernel against slot refill (folded backward tail, full chain at knot 0)."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
SETTINGS = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)

CASES = {  # name -> (problem, batch, compiled into the library?)
    "quadrotor50": (lambda P: P.quadrotor(50), 1031, True),
    "cartpole20": (lambda P: P.cartpole(20, True), 517, True),
    "quadrotor30": (lambda P: P.quadrotor(30), 1031, False),  # run-time specialised (TINY_JIT_CT=1)
}


def _goal(prob, seed=7):
    rng = np.random.default_rng(seed)
    return 0.4 * rng.standard_normal(prob.nx), 0.05 * rng.standard_normal(prob.nu)


def _constant_refs(prob, gx, gu):
    return np.repeat(gx[:, None], prob.N, axis=1), np.repeat(gu[:, None], prob.N - 1, axis=1)


def _solver(pkg, prob, batch, rho, settings=SETTINGS):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=rho, fdyn=prob.fdyn, **settings)
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    return s


def _x0s(prob, batch, scale, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(prob.x0[:, None] * scale + 0.2 * rng.standard_normal((prob.nx, batch)))


def _everything(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


@pytest.mark.parametrize("rho", ["problem", 0.37])
@pytest.mark.parametrize("case", list(CASES))
def test_constant_references_match_the_oracle(pkg, monkeypatch, case, rho):
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")  # (small batches would go to layout F)
    P = pkg.problems
    make, batch, compiled_in = CASES[case]
    prob = make(P)
    rho = prob.rho if rho == "problem" else rho
    X, U = _constant_refs(prob, *_goal(prob))
    s = _solver(pkg, prob, batch, rho)
    s.set_x_ref(X)
    s.set_u_ref(U)
    prob.rho = rho
    sample = sorted({0, 1, batch // 2, batch - 2, batch - 1})
    orcs = {b: O.OraclePort(prob).load_problem(prob, SETTINGS) for b in sample}  # (one per instance: each warm-starts from its own state)
    for orc in orcs.values():
        orc.set_x_ref(X)
        orc.set_u_ref(U)
    iters = []
    for rnd in range(3):  # a cold start, then two warm starts from the state the previous solve left
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        sol, st = s.get_solution_batch(), s.get_stats_batch()
        for b, orc in orcs.items():
            orc.set_x0(x0s[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (case, rnd, b)
            assert st["status"][b] == orc.stats()["status"], (case, rnd, b)
            assert rel_err(sol["states"][:, :, b], orc.solution()[0]) < TOL, (case, rnd, b)
            assert rel_err(sol["controls"][:, :, b], orc.solution()[1]) < TOL, (case, rnd, b)
        iters.append(st["iter"].copy())
    assert s.launch_info()["layout"] == "D" and not s.launch_info()["tables_in_lds"]
    assert ("compiled-in" in s.jit_info()) == compiled_in, s.jit_info()
    assert any(np.any(it < SETTINGS["max_iter"]) for it in iters)  # (some instances converge: the iteration counts mean something)
    s.reset()


@pytest.mark.parametrize("case", ["quadrotor50", "quadrotor30"])
def test_shared_references_and_per_instance_goals_are_bit_identical(pkg, case):
    """The shared constant-table kernel and the goal kernel fold lr the same way: every instance given the shared goal returns the
    same bits, cold and warm."""
    P = pkg.problems
    make, batch, _ = CASES[case]
    prob = make(P)
    gx, gu = _goal(prob, seed=11)
    X, U = _constant_refs(prob, gx, gu)
    shared, inst = _solver(pkg, prob, batch, 0.37), _solver(pkg, prob, batch, 0.37)
    shared.set_x_ref(X)
    shared.set_u_ref(U)
    inst.set_x_ref_batch(np.repeat(gx[:, None], batch, axis=1))
    inst.set_u_ref_batch(np.repeat(gu[:, None], batch, axis=1))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, inst):
            h.set_x0_batch(x0s)
            h.solve()
        for a, b, what in zip(_everything(shared), _everything(inst), ("states", "controls", "iterations", "status", "residuals")):
            np.testing.assert_array_equal(a, b, err_msg=f"solve {rnd}: {what}")
    assert shared.launch_info()["layout"] == inst.launch_info()["layout"] == "D"
    assert "goal" in inst.jit_info() and "per-instance-refs" not in shared.jit_info()
    shared.reset()
    inst.reset()


def test_slot_refill_with_constant_references_is_bit_identical_to_the_plain_kernel(pkg, monkeypatch):
    """Slot refill folds the backward tail like the plain kernel but keeps knot 0's full chain (no c0: the variant has no registers to
    spare); with nonzero constant references and rho = 0.37 everything must still equal the plain kernel's, cold and warm."""
    P = pkg.problems
    prob = P.quadrotor(50)
    B = 9001
    X, U = _constant_refs(prob, *_goal(prob, seed=3))
    rng = np.random.default_rng(B)
    x0s = np.asfortranarray(P.quadrotor_batch_x0(B) * rng.uniform(0.05, 3.0, B)[None, :])
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=1)
    got = {}
    for refill in (False, True):
        monkeypatch.setenv("TINYMPC_REFILL", "1" if refill else "0")
        s = _solver(pkg, prob, B, 0.37, settings)
        s.set_x_ref(X)
        s.set_u_ref(U)
        s.set_x0_batch(x0s)
        assert s.launch_info()["layout"] == "D"
        assert ("slot-refill" in s.jit_info()) == refill
        s.solve()
        cold = _everything(s)
        s.set_x0_batch(np.asfortranarray(0.9 * x0s))
        s.solve()
        got[refill] = (cold, _everything(s))
        s.reset()
    for k, name in enumerate(("cold", "warm")):
        for a, b, what in zip(got[False][k], got[True][k], ("states", "controls", "iterations", "status", "residuals")):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} solve: {what}")
    it = got[True][0][2]
    assert it.min() < 60 and len(np.unique(it)) > 5  # (rows were refilled at different times)

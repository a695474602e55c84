"""Slot refill for layout D's per-instance goal form (`REFILL && IGOAL`; tinympc_solve_d.hip / tinympc_plan.hip): a handle whose
instances have their own goals (set_x_ref_batch / set_u_ref_batch, one column per instance) and / or their own boxes
(set_bound_constraints_batch, one column per instance) runs a batch beyond one resident set as ONE resident set of wavefronts; a
16-lane row that takes the next instance takes that instance's four lane constants and folded accumulator start with it. The
arithmetic of an instance does not change: everything a solve returns is BIT-IDENTICAL to the plain goal kernel's
(TINYMPC_REFILL=0), cold and warm, and a seeded sample matches the oracle with every instance's own goal and box (iterations and
solved flags exact, 1e-9 on the trajectories: the bar of test_slot_refill_gpu.py)."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
WHAT = ("states", "controls", "iterations", "status", "residuals")


def _x0s(P, prob, B):
    scale = np.random.default_rng(B + prob.N).uniform(0.05, 3.0, B)
    base = P.quadrotor_batch_x0(B) if prob.nx == 12 else np.repeat(prob.x0[:, None], B, axis=1)
    return np.asfortranarray(base * scale[None, :])


def _tables(prob, B):
    """-> (state goals nx x B, input goals nu x B, the four bounds, one column per instance), drawn in this order from rng(7)."""
    g = np.random.default_rng(7)
    nx, nu = prob.nx, prob.nu
    gx = np.zeros((nx, B))
    gx[:3] = 0.1 * g.standard_normal((3, B))
    gu = 0.02 * g.standard_normal((nu, B))
    w = g.uniform(0.6, 1.0, B)
    xl, xh, ul, uh = (a[:, 0] for a in prob.expanded_bounds())  # (the problem's own, constant over the horizon)
    box = (np.repeat(xl[:, None], B, axis=1), np.repeat(xh[:, None], B, axis=1), ul[:, None] * w[None, :], uh[:, None] * w[None, :])
    return gx, gu, box


def _handle(pkg, prob, B, settings, x0s, tables, refs=True, boxes=True):
    gx, gu, box = tables
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=B, rho=prob.rho, **settings)
    s.set_bound_constraints(*(a[:, 0] for a in prob.expanded_bounds()))
    if refs:
        s.set_x_ref_batch(gx)
        s.set_u_ref_batch(gu)
    if boxes:
        s.set_bound_constraints_batch(*box)
    s.set_x0_batch(x0s)
    return s


def _everything(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


def _same(a, b, tag):
    for x, y, what in zip(a, b, WHAT):
        np.testing.assert_array_equal(x, y, err_msg=f"{tag}: {what}")


def _oracle_sample(prob, settings, x0s, tables, got, B):
    """A seeded sample of 16 instances, each with its own goal and box, against the C restatement (cold solve)."""
    gx, gu, box = tables
    N = prob.N
    for b in np.random.default_rng(1).choice(B, size=16, replace=False):
        orc = O.OraclePort(prob).load_problem(prob, settings)
        orc.set_x_ref(np.repeat(gx[:, b:b + 1], N, axis=1))
        orc.set_u_ref(np.repeat(gu[:, b:b + 1], N - 1, axis=1))
        orc.set_bound_constraints(np.repeat(box[0][:, b:b + 1], N, axis=1), np.repeat(box[1][:, b:b + 1], N, axis=1),
                                  np.repeat(box[2][:, b:b + 1], N - 1, axis=1), np.repeat(box[3][:, b:b + 1], N - 1, axis=1))
        orc.set_x0(x0s[:, b])
        orc.solve()
        assert got[2][b] == orc.stats()["iter"], b
        assert (got[3][b] == 1) == (orc.stats()["status"] == 1), b
        assert rel_err(got[0][:, :, b], orc.solution()[0]) < TOL, b
        assert rel_err(got[1][:, :, b], orc.solution()[1]) < TOL, b


def _both_kernels(pkg, monkeypatch, prob, B, settings, x0s, tables, compiled_in, **halves):
    """Cold, then warm from 0.9 x0, under TINYMPC_REFILL 0 and 1 -> {refill: (cold, warm)}; layout D and the goal form on both sides,
    `slot-refill` exactly where refill is on (a run-time specialised shape names its kernel from the first solve on)."""
    got = {}
    for refill in (False, True):
        monkeypatch.setenv("TINYMPC_REFILL", "1" if refill else "0")
        s = _handle(pkg, prob, B, settings, x0s, tables, **halves)
        if compiled_in:  # (before the first solve as well)
            assert s.launch_info()["layout"] == "D"
            assert ("slot-refill" in s.jit_info()) == refill and "goal" in s.jit_info(), s.jit_info()
        s.solve()
        assert s.launch_info()["layout"] == "D"
        assert ("slot-refill" in s.jit_info()) == refill and "goal" in s.jit_info(), s.jit_info()
        cold = _everything(s)
        s.set_x0_batch(np.asfortranarray(0.9 * x0s))
        s.solve()
        got[refill] = (cold, _everything(s))
        s.reset()
    _same(got[False][0], got[True][0], "cold solve")
    _same(got[False][1], got[True][1], "warm solve")
    return got


@pytest.mark.parametrize("N,B,ct,max_iter", [(50, 9001, 1, 60), (20, 10000, 3, 45)])
def test_goal_refill_is_bit_identical_to_the_plain_goal_kernel(pkg, monkeypatch, N, B, ct, max_iter):
    """N=50 is the compiled-in kernel (k_admm_solve_d_refill_gbnd), N=20 its run-time specialisation. Ragged batches, a check interval
    that divides nothing, instances that converge after a few iterations next to ones that run max_iter -- the condition below holds
    for these inputs by the algorithm alone: on the oracle the 64-instance sample rng(1).choice(B, 64) runs 8..60 iterations (15
    distinct counts) for N=50 and 9..45 (8 distinct) for N=20, every instance below max_iter solved."""
    P = pkg.problems
    prob = P.quadrotor(N)
    x0s, tables = _x0s(P, prob, B), _tables(prob, B)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=max_iter, check_termination=ct)
    got = _both_kernels(pkg, monkeypatch, prob, B, settings, x0s, tables, compiled_in=N == 50)
    it, status = got[True][0][2], got[True][0][3]
    assert it.min() < max_iter and it.max() == max_iter and len(np.unique(it)) > 5  # (a spread worth refilling for)
    assert np.all(status[it < max_iter] == 1)
    _oracle_sample(prob, settings, x0s, tables, got[True][0], B)


def test_goal_refill_compiled_in_cartpole(pkg, monkeypatch):
    """The cartpole N=20 (compiled in, one input: the folded accumulator start sums one column)."""
    P = pkg.problems
    prob, B = P.cartpole(20), 8500
    x0s, tables = _x0s(P, prob, B), _tables(prob, B)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=1)
    got = _both_kernels(pkg, monkeypatch, prob, B, settings, x0s, tables, compiled_in=True)
    _oracle_sample(prob, settings, x0s, tables, got[True][0], B)


@pytest.mark.parametrize("half", ["bounds", "x_ref_range"])
def test_goal_refill_with_only_one_half_per_instance(pkg, monkeypatch, half):
    """Only boxes per instance beside a shared constant reference; only state goals, for instances 100..4099 -- the rest keep the
    shared goal. The goal form all the same (the shared values fill the other rows): refill is taken, bit-identical."""
    P = pkg.problems
    prob, B = P.quadrotor(50), 9001
    x0s, (gx, gu, box) = _x0s(P, prob, B), _tables(prob, B)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=1)
    got = {}
    for refill in (False, True):
        monkeypatch.setenv("TINYMPC_REFILL", "1" if refill else "0")
        s = _handle(pkg, prob, B, settings, x0s, (gx, gu, box), refs=False, boxes=half == "bounds")
        if half == "x_ref_range":
            s.set_x_ref_batch(gx[:, 100:4100], first=100)
        assert s.launch_info()["layout"] == "D"
        assert ("slot-refill" in s.jit_info()) == refill and "goal" in s.jit_info(), s.jit_info()
        s.solve()
        cold = _everything(s)
        s.set_x0_batch(np.asfortranarray(0.9 * x0s))
        s.solve()
        got[refill] = (cold, _everything(s))
        s.reset()
    _same(got[False][0], got[True][0], "cold solve")
    _same(got[False][1], got[True][1], "warm solve")


@pytest.mark.parametrize("B,ct,max_iter,tol", [(8193, 1, 30, 1e-3), (9100, 1, 1, 1e-3), (9100, 5, 3, 1e-3), (8200, 1, 25, 1e3)])
def test_goal_refill_edges(pkg, monkeypatch, B, ct, max_iter, tol):
    """One instance more than a resident set; max_iter 1; a check interval beyond max_iter (nobody is ever tested); tolerances
    everything meets at the first check. A first solve and a warm one on the same x0: the plain goal kernel's bits."""
    P = pkg.problems
    prob = P.quadrotor(50)
    x0s, tables = _x0s(P, prob, B), _tables(prob, B)
    settings = dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=max_iter, check_termination=ct)
    got = {}
    for refill in (False, True):
        monkeypatch.setenv("TINYMPC_REFILL", "1" if refill else "0")
        s = _handle(pkg, prob, B, settings, x0s, tables)
        assert ("slot-refill" in s.jit_info()) == refill and "goal" in s.jit_info(), s.jit_info()
        s.solve()
        first = _everything(s)
        s.solve()  # warm, same x0
        got[refill] = (first, _everything(s))
        s.reset()
    _same(got[False][0], got[True][0], "first solve")
    _same(got[False][1], got[True][1], "second solve")
    if ct > max_iter:
        assert np.all(got[True][0][2] == max_iter) and np.all(got[True][0][3] != 1)
    if tol >= 1e3:
        assert np.all(got[True][0][2] == ct) and np.all(got[True][0][3] == 1)


def test_goal_refill_is_only_taken_where_it_can_pay(pkg, monkeypatch):
    """One resident set, forced iteration counts without TINYMPC_REFILL=1, and TINYMPC_REFILL=0 keep the plain goal kernel; forced
    on with tolerances nothing meets, the variant returns the plain kernel's bits."""
    P = pkg.problems
    prob = P.quadrotor(50)
    reach = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=12, check_termination=1)
    forced = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=12, check_termination=1)
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    small = _handle(pkg, prob, 8192, reach, _x0s(P, prob, 8192), _tables(prob, 8192))
    assert "slot-refill" not in small.jit_info() and "goal" in small.jit_info()  # one resident set: nothing to refill with
    small.reset()
    B = 9000
    x0s, tables = _x0s(P, prob, B), _tables(prob, B)
    monkeypatch.delenv("TINYMPC_REFILL", raising=False)
    s = _handle(pkg, prob, B, forced, x0s, tables)
    assert "slot-refill" not in s.jit_info() and "goal" in s.jit_info()  # nothing converges: nothing to balance
    s.solve()
    plain = _everything(s)
    monkeypatch.setenv("TINYMPC_REFILL", "0")
    s.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    assert "slot-refill" not in s.jit_info()
    s.reset()
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    s = _handle(pkg, prob, B, forced, x0s, tables)
    assert "slot-refill" in s.jit_info() and "goal" in s.jit_info()
    s.solve()
    _same(plain, _everything(s), "forced iteration counts")
    assert np.all(plain[2] == 12) and np.all(plain[3] == 11)
    s.reset()


def test_goal_refill_mode_switches_on_one_handle(pkg, monkeypatch):
    """Goals -> a trajectory per instance (layout A) -> goals again -> everything shared (the shared refill kernel), on the one ADMM
    state of a run-time specialised shape; a twin handle under TINYMPC_REFILL=0 receives the same calls and returns the same bits."""
    P = pkg.problems
    prob, B = P.quadrotor(20), 9000
    N = prob.N
    x0s, (gx, gu, box) = _x0s(P, prob, B), _tables(prob, B)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40, check_termination=1)
    traj = np.asfortranarray(gx[:, None, :] * np.linspace(0.0, 1.0, N)[None, :, None])
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    pair = [_handle(pkg, prob, B, settings, x0s, (gx, gu, box)) for _ in range(2)]  # [refill, twin]

    def step(call, tag, layout, refill, goal):
        for k, h in enumerate(pair):
            monkeypatch.setenv("TINYMPC_REFILL", "1" if k == 0 else "0")
            call(h)
            h.solve()
            info = h.jit_info()
            assert h.launch_info()["layout"] == layout, (tag, info)
            assert ("slot-refill" in info) == (refill and k == 0), (tag, info)
            assert (" goal" in info) == goal, (tag, info)
        _same(_everything(pair[1]), _everything(pair[0]), tag)

    def shared(h):
        h.set_x_ref(np.zeros((prob.nx, N)))
        h.set_u_ref(np.zeros((prob.nu, N - 1)))
        h.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)

    step(lambda h: None, "goals", "D", True, True)
    step(lambda h: h.set_x_ref_batch(traj), "trajectories", "A", False, False)

    def goals_again(h):  # (a half that held trajectories stays one until it leaves per-instance mode: through the shared verb)
        h.set_x_ref(np.zeros((prob.nx, N)))
        h.set_x_ref_batch(gx)

    step(goals_again, "goals again", "D", True, True)
    step(shared, "shared again", "D", True, False)
    for h in pair:
        h.reset()

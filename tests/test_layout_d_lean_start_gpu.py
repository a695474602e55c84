"""Layout D's lean kernels with the accumulator starts read from LDS and the loop control out of the lean inner loop
(tinympc_lstart_d.hip; tinympc_plan.hip: lean_start_applies) against the lean kernels they replace and against the plain ones.

Both changes keep every instruction of the arithmetic, its order and its operands, so the three builds of one handle configuration --
TINYMPC_LEAN=0 (plain), TINYMPC_LEAN=1 TINYMPC_LEAN_START=0 (the lean kernels of tinympc_lean_d.hip) and TINYMPC_LEAN=1 (the new
ones) -- must return the same bits: states, controls, iteration counts, status and the four residuals of a cold solve and of the
warm solve that follows it (which starts from everything the cold one left, the stale v|z of converged instances included).

Every case has `fdyn` nonzero on every state row: the table holds cf, the forward operator's constant term, and with cf = 0 a wrong
or missing table could not show. Small batches: 5 is a partial wavefront, 17 a second workgroup with one partial wavefront, 9 three
wavefronts of one workgroup. The converging batch is checked against the oracle as well (iteration counts exact, 1e-9 on the
trajectories: the bar of test_layout_d_lean_gpu.py); its seed was chosen on the CPU so that the ORACLE gives instances that converge at
different checks and instances that do not converge -- asserted on the oracle's output before anything is compared."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
WHAT = ("states", "controls", "iterations", "status", "residuals")
BUILDS = {  # name -> (TINYMPC_LEAN, TINYMPC_LEAN_START or None, the words jit_info must / must not have)
    "plain": ("0", None, (), ("lean", "lds-start")),
    "lean": ("1", "0", ("lean",), ("lds-start",)),
    "start": ("1", None, ("lean", "lds-start"), ()),
}


def _fdyn(nx):
    return 0.01 * np.array([(1 + (i % 5)) * (-1.0) ** i for i in range(nx)])  # nonzero on every state row


def _quadrotor(P):
    prob = P.quadrotor(50)
    prob.fdyn = _fdyn(prob.nx)
    return prob


def _cartpole(P, N):
    prob = P.cartpole(N, True)
    prob.fdyn = _fdyn(prob.nx)
    return prob


def _everything(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


def _three(pkg, monkeypatch, prob, batch, settings, x0s, configure=None, warm_scale=0.9, word=None):
    """{build: (cold solve, warm solve)} of three fresh handles; which kernel ran is asserted through jit_info."""
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")  # (small batches would go to the latency layouts)
    monkeypatch.setenv("TINYMPC_REFILL", "0")
    got = {}
    for name, (lean, start, has, has_not) in BUILDS.items():
        monkeypatch.setenv("TINYMPC_LEAN", lean)
        if start is None:
            monkeypatch.delenv("TINYMPC_LEAN_START", raising=False)
        else:
            monkeypatch.setenv("TINYMPC_LEAN_START", start)
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if configure:
            configure(s)
        s.set_x0_batch(x0s)
        s.solve()
        # (asked after the first solve: the kernel for per-knot tables is decided when a launch first needs it)
        words = s.jit_info().split()
        assert s.launch_info()["layout"] == "D" and "compiled-in" in words, s.jit_info()
        assert all(w in words for w in has) and not any(w in words for w in has_not), (name, s.jit_info())
        assert word is None or word in words, s.jit_info()
        cold = _everything(s)
        s.set_x0_batch(np.asfortranarray(warm_scale * x0s))
        s.solve()
        got[name] = (cold, _everything(s))
        s.reset()
    return got


def _assert_equal(got, tag=""):
    for other in ("plain", "lean"):
        for k, name in enumerate(("cold", "warm")):
            for a, b, what in zip(got[other][k], got["start"][k], WHAT):
                np.testing.assert_array_equal(a, b, err_msg=f"{tag} {name} solve, against the {other} kernel: {what}")


def _scaled_x0(P, batch, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(P.quadrotor_batch_x0(batch) * rng.uniform(0.05, 3.0, batch)[None, :])


@pytest.mark.parametrize("max_iter,ct", [(1, 1), (2, 1), (3, 0), (25, 4), (25, 10)])
@pytest.mark.parametrize("batch", [5, 17])
def test_forced_iteration_counts_are_bit_identical(pkg, monkeypatch, batch, max_iter, ct):
    """Quadrotor N=50 (24 slack slots in registers, 25 in LDS), tolerances 0: no lean round at all (1, 1), one in front of the round
    with residuals (2, 1), only lean rounds (3, 0), runs of lean rounds between and behind the rounds with residuals."""
    P = pkg.problems
    prob = _quadrotor(P)
    settings = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=max_iter, check_termination=ct)
    got = _three(pkg, monkeypatch, prob, batch, settings, _scaled_x0(P, batch, 3))
    _assert_equal(got, f"batch={batch} max_iter={max_iter} ct={ct}")
    assert np.all(got["start"][0][2] == max_iter) and np.all(got["start"][0][3] != 1)


CONVERGING_SEED = 0  # (chosen with OraclePort, see the assertions on the oracle's output below)


def test_converging_batch_is_bit_identical_and_matches_the_oracle(pkg, monkeypatch):
    """Tolerances that can be met, a check in every fourth iteration: instances converge at different checks, their write-back is the
    hoisted one in front of the next run of lean rounds, their rows go on as zombies next to the instances that never converge, and
    the warm solve starts from the stale copies."""
    P = pkg.problems
    prob = _quadrotor(P)
    B = 17
    x0s = _scaled_x0(P, B, CONVERGING_SEED)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=4)
    orc = O.OraclePort(prob).load_problem(prob, settings)
    ox, ou, oit, ost, _ = orc.solve_batch(x0s)
    oit, ost = np.asarray(oit), np.asarray(ost)
    conv = ost == 1
    assert np.any(conv & (oit < 60)) and np.any(~conv) and len(np.unique(oit[conv])) >= 2, (oit, ost)
    got = _three(pkg, monkeypatch, prob, B, settings, x0s)
    _assert_equal(got)
    st, sc, it, status, _ = got["start"][0]
    np.testing.assert_array_equal(it, oit)
    np.testing.assert_array_equal(status == 1, conv)
    assert rel_err(st, ox) < TOL
    assert rel_err(sc, ou) < TOL


def test_per_instance_goals_and_bounds_are_bit_identical(pkg, monkeypatch):
    """The goal-form kernel: one goal and one box per instance."""
    P = pkg.problems
    prob = _quadrotor(P)
    batch = 17
    rng = np.random.default_rng(5)
    gx, gu = 0.4 * rng.standard_normal((prob.nx, batch)), 0.05 * rng.standard_normal((prob.nu, batch))
    wx, wu = rng.uniform(0.6, 1.4, (prob.nx, batch)), rng.uniform(0.6, 1.4, (prob.nu, batch))
    xmin, xmax = np.asarray(prob.x_min).reshape(-1, 1), np.asarray(prob.x_max).reshape(-1, 1)
    umin, umax = np.asarray(prob.u_min).reshape(-1, 1), np.asarray(prob.u_max).reshape(-1, 1)

    def configure(s):
        s.set_x_ref_batch(gx)
        s.set_u_ref_batch(gu)
        s.set_bound_constraints_batch(xmin * wx, xmax * wx, umin * wu, umax * wu)

    settings = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=9, check_termination=1)
    got = _three(pkg, monkeypatch, prob, batch, settings, _scaled_x0(P, batch, 6), configure, word="goal")
    _assert_equal(got, "goals and bounds")


@pytest.mark.parametrize("tol", [0.0, 1e-4])
@pytest.mark.parametrize("N,trajectory", [(10, False), (20, False), (20, True)])
def test_cartpole_is_bit_identical(pkg, monkeypatch, N, trajectory, tol):
    """The two cartpole shapes (every slack slot in a register), with constant references and, for N=20, with a reference trajectory
    (the kernels with per-knot tables, which sit behind the table of accumulator starts in LDS)."""
    P = pkg.problems
    prob = _cartpole(P, N)
    batch = 9
    rng = np.random.default_rng(9 + N)
    X = 0.3 * np.sin(0.4 * np.arange(prob.N)[None, :] + np.arange(prob.nx)[:, None])
    U = 0.05 * np.cos(0.3 * np.arange(prob.N - 1)[None, :]) * np.ones((prob.nu, 1))

    def configure(s):
        if trajectory:
            s.set_x_ref(X)
            s.set_u_ref(U)

    x0s = np.asfortranarray(np.asarray(prob.x0).reshape(-1, 1) + 0.2 * rng.standard_normal((prob.nx, batch)))
    settings = dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=7, check_termination=3)
    got = _three(pkg, monkeypatch, prob, batch, settings, x0s, configure, warm_scale=0.8)
    _assert_equal(got, f"N={N} trajectory={trajectory} tol={tol}")

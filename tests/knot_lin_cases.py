"""Cases, inputs and the reference of the per-knot linear constraints' tests (tinympc_set_linear_constraints_knots_batch).

The reference is a STEPPED oracle made of the plain-C oracle's own verbs (oracle/pyoracle.py; nothing under oracle/ knows about rows per
knot): the problem goes into OraclePort, set_linear_constraints with knot 0's rows sizes and enables the family, and every ADMM
iteration is driven from here -- forward_pass, update_slack, then vlnew[:, i] and zlnew[:, i] are overwritten by
pyoracle.project_halfspaces of x_i + gl_i (u_i + yl_i) onto knot i's OWN rows, then update_dual, update_linear_cost, the iteration
count, the termination test, v <- vnew, z <- znew and backward_pass_grad, exactly in orc_solve's order. With rows repeated over the
knots it reproduces orc_solve bit for bit (tests/test_knot_lin_cpu.py). The object keeps its oracle, so warm ticks continue on it.

Inputs (seed 7, drawn in this order): x0_b = x0 + 0.1 randn; Ax, Au random unit rows per knot and instance; bx = a'x0_b +
U(0.5, 2) (1 + |a'x0_b|) with every knot's row taken at x0_b; bu = U(0.2, 0.8)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import pyoracle as O

SEED = 7
TOL = 1e-9
CONV = dict(max_iter=300, abs_pri_tol=1e-4, abs_dua_tol=1e-4)   # the 16-lane cases
FORCED = dict(max_iter=60, abs_pri_tol=0.0, abs_dua_tol=0.0)     # the wide cases: 60 forced iterations


def _wide(P, nx, nu, N):  # (the wide systems of tests/test_instance_bounds_gpu.py, restated so that the CPU tests need no GPU module)
    rng = np.random.default_rng(nx * 100 + nu)
    A = np.eye(nx) + 0.03 * rng.standard_normal((nx, nx))
    B = 0.1 * rng.standard_normal((nx, nu))
    prob = P.Problem("wide", A, B, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(0.5, 2, nu)), N, 2.0, rng.standard_normal(nx))
    prob.u_min, prob.u_max = np.full(nu, -0.3), np.full(nu, 0.3)
    prob.x_min, prob.x_max = np.full(nx, -2.0), np.full(nx, 2.0)
    return prob


CASES = {  # name -> (problem, state rows, input rows, batch, settings); batches are ragged on purpose
    "quadrotor-1+1": (lambda P: P.quadrotor(20), 1, 1, 37, CONV),
    "quadrotor-3+2": (lambda P: P.quadrotor(20), 3, 2, 37, CONV),        # unequal sides, rows beyond the two kept in registers
    "cartpole-2+1": (lambda P: P.cartpole(20, True), 2, 1, 21, CONV),    # lanes beyond the system's rows
    "quadrotor120-1+1": (lambda P: P.quadrotor(120), 1, 1, 6, CONV),     # the long-horizon path (state in HBM)
    "quadrotor-10+3": (lambda P: P.quadrotor(20), 10, 3, 37, CONV),      # rows beyond eight
    "wide32-2+2": (lambda P: _wide(P, 24, 8, 20), 2, 2, 21, FORCED),     # 32 lanes per instance: group sums
    "wide64-1+2": (lambda P: _wide(P, 48, 16, 12), 1, 2, 9, FORCED),     # 64 lanes per instance
}
VERIFIED = ["quadrotor-1+1", "quadrotor-3+2", "cartpole-2+1", "quadrotor120-1+1"]  # the cases whose sample conditions seed 7 meets


def case(pkg, name):
    make, nlx, nlu, batch, settings = CASES[name]
    return make(pkg.problems), nlx, nlu, batch, settings


def rows_knots(prob, nlx, nlu, batch, seed=SEED):
    """-> x0s (nx, batch), Ax (nlx, nx, N, batch), bx (nlx, N, batch), Au (nlu, nu, N-1, batch), bu (nlu, N-1, batch)."""
    rng = np.random.default_rng(seed)
    nx, nu, N = prob.nx, prob.nu, prob.N
    x0s = np.asfortranarray(prob.x0[:, None] + 0.1 * rng.standard_normal((nx, batch)))

    def unit(rows, cols, knots):
        a = rng.standard_normal((rows, cols, knots, batch))
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    Ax, Au = unit(nlx, nx, N), unit(nlu, nu, N - 1)
    ax0 = np.einsum("kcnb,cb->knb", Ax, x0s)
    bx = ax0 + rng.uniform(0.5, 2.0, (nlx, N, batch)) * (1.0 + np.abs(ax0))
    bu = rng.uniform(0.2, 0.8, (nlu, N - 1, batch))
    return x0s, Ax, bx, Au, bu


def sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1}) if batch > 6 else list(range(batch))


def of(rows, b):
    """Instance b's rows of a batch's (Ax, bx, Au, bu)."""
    return tuple(a[..., b] for a in rows)


def held(rows_b, N, knot=0):
    """One knot's rows of an instance repeated over the horizon: (nlx, nx, N), (nlx, N), (nlu, nu, N-1), (nlu, N-1)."""
    Ax, bx, Au, bu = rows_b
    ku = min(knot, N - 2)
    return (np.repeat(Ax[:, :, knot:knot + 1], N, axis=2), np.repeat(bx[:, knot:knot + 1], N, axis=1),
            np.repeat(Au[:, :, ku:ku + 1], N - 1, axis=2), np.repeat(bu[:, ku:ku + 1], N - 1, axis=1))


def repeat_over_knots(rows_const, N):
    """A batch's rows constant over the horizon, (nlx, nx, batch) ..., in the per-knot verb's shapes."""
    Ax, bx, Au, bu = rows_const
    return (np.repeat(Ax[:, :, None, :], N, axis=2), np.repeat(bx[:, None, :], N, axis=1),
            np.repeat(Au[:, :, None, :], N - 1, axis=2), np.repeat(bu[:, None, :], N - 1, axis=1))


class SteppedOracle:
    """The reference of ONE instance (see the module docstring). solve(x0, rows) runs one solve -- cold the first time, warm after -- under
    rows = (Ax (nlx, nx, N), bx (nlx, N), Au (nlu, nu, N-1), bu (nlu, N-1)) and returns (states, controls, iterations, status)."""

    def __init__(self, prob, settings, rows, **flags):
        pb = dataclasses.replace(prob, linear={})
        self.N, self.settings = prob.N, dict(settings)
        self.orc = O.OraclePort(pb).load_problem(pb, settings)
        Ax, bx, Au, bu = rows
        self.orc.set_linear_constraints(Ax[:, :, 0], bx[:, 0], Au[:, :, 0], bu[:, 0])  # sizes and enables the family
        self.state_on = Ax.shape[0] > 0 and bool(flags.get("en_state_linear", 1))
        self.input_on = Au.shape[0] > 0 and bool(flags.get("en_input_linear", 1))
        self.orc.update_settings(**flags)

    def solve(self, x0, rows):
        Ax, bx, Au, bu = rows
        o, N = self.orc, self.N
        o.set_x0(x0)
        o.set_iter(0)
        it, status = 0, 11
        for _ in range(self.settings["max_iter"]):
            o.forward_pass()
            o.update_slack()
            if self.state_on:
                x, gl = o.get("x"), o.get("gl")
                vl = np.zeros_like(x, order="F")
                for i in range(N):
                    vl[:, i] = O.project_halfspaces(x[:, i] + gl[:, i], Ax[:, :, i], bx[:, i])[0]
                o.put("vlnew", vl)
            if self.input_on:
                u, yl = o.get("u"), o.get("yl")
                zl = np.zeros_like(u, order="F")
                for i in range(N - 1):
                    zl[:, i] = O.project_halfspaces(u[:, i] + yl[:, i], Au[:, :, i], bu[:, i])[0]
                o.put("zlnew", zl)
            o.update_dual()
            o.update_linear_cost()
            it += 1
            o.set_iter(it)
            if o.termination_condition():
                status = 1
                break
            o.put("v", o.get("vnew"))
            o.put("z", o.get("znew"))
            o.backward_pass_grad()
        return o.get("vnew"), o.get("znew"), it, status


def whole_solve(prob, settings, x0, rows_one):
    """orc_solve under one set of rows held over the horizon: rows_one = (Ax (nlx, nx), bx (nlx,), Au (nlu, nu), bu (nlu,))."""
    pb = dataclasses.replace(prob, linear={})
    o = O.OraclePort(pb).load_problem(pb, settings)
    o.set_linear_constraints(*rows_one)
    o.set_x0(x0)
    o.solve()
    st = o.stats()
    return o.solution()[0].copy(), o.solution()[1].copy(), st["iter"], st["status"]


@functools.lru_cache(maxsize=None)
def reference(pkg, name):
    """Computed once per case and shared, never modified: for every sampled instance the stepped oracle's cold solve under its own
    per-knot rows (`own`) and orc_solve under knot 0's rows held over the horizon (`held0`)."""
    prob, nlx, nlu, batch, settings = case(pkg, name)
    x0s, *rows = rows_knots(prob, nlx, nlu, batch)
    own, held0 = {}, {}
    for b in sample(batch):
        rb = of(rows, b)
        own[b] = SteppedOracle(prob, settings, rb).solve(x0s[:, b], rb)
        held0[b] = whole_solve(prob, settings, x0s[:, b], (rb[0][:, :, 0], rb[1][:, 0], rb[2][:, :, 0], rb[3][:, 0]))
    return own, held0


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def assert_sample_conditions(name, own, held0, max_iter):
    """On the reference's own results: at least two sampled instances converge, at least one does not, at least half move their controls
    by more than 1e-3 (relative) against knot 0's rows held over the horizon."""
    conv = [own[b][3] == 1 and own[b][2] < max_iter for b in own]
    moved = [rel(own[b][1], held0[b][1]) > 1e-3 for b in own]
    print(name, "reference: converged", sum(conv), "of", len(conv), "moved", sum(moved), "of", len(moved))
    assert sum(conv) >= 2 and sum(not c for c in conv) >= 1, (name, conv)
    assert 2 * sum(moved) >= len(moved), (name, moved)

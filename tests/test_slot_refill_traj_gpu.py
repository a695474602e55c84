"""Slot refill for layout D's per-instance trajectory form and per-knot bounds form (`REFILL && ITRAJ`, `REFILL && IKBND`, both together;
tinympc_solve_d.hip / tinympc_plan.hip): a prepared handle whose instances follow their own trajectories or tracks, and / or have their
own bound schedules, runs a batch beyond one resident set as ONE resident set of wavefronts. A 16-lane row that takes the next instance
takes that instance's lane constants and restages its own column of its wavefront's linref / clamp rows from the new instance's group.
The arithmetic of an instance does not change: everything a solve returns is BIT-IDENTICAL to the plain form's (TINYMPC_REFILL=0), cold
and warm, and a seeded sample matches the oracle with every instance's own trajectory and bound schedule (iterations and solved flags
exact, 1e-9 on the trajectories: the bar of test_slot_refill_gpu.py).

Batches: a refill test needs more than one resident set of the 256-CU device -- 4,096 instances for the forms on one wavefront per SIMD
(trajectories at N=50, per-knot bounds at N=20), 8,192 for those on two (trajectories at N=20 and N=10, and per-knot bounds at N=10,
whose clamp rows still fit the two-wavefront plan: that case runs 8,707 instances, not 4,611, so that it refills at all)."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O
import test_instance_models_gpu as MG
from test_instance_bounds_gpu import _bounds, _refs
from test_instance_lin_gpu import _rows

pytestmark = pytest.mark.gpu

TOL = 1e-9
WHAT = ("states", "controls", "iterations", "status", "residuals")
AMP = 0.1  # the sibling file's trajectories, scaled so that a good part of a batch converges inside max_iter


def _x0s(P, prob, B):
    scale = np.random.default_rng(B + prob.N).uniform(0.02, 1.0, B)
    base = P.quadrotor_batch_x0(B) if prob.nx == 12 else np.repeat(prob.x0[:, None], B, axis=1)
    return np.asfortranarray(base * scale[None, :])


def _trajs(prob, B, seed=1):
    """One trajectory per instance: nx x N x B and nu x (N-1) x B."""
    _, (X, U) = _refs(prob, B, "trajectory", seed=seed)
    return np.asfortranarray(AMP * X), np.asfortranarray(AMP * U)


def _goals(prob, B, seed=3):
    (gx, gu), _ = _refs(prob, B, "goal", seed=seed)
    return np.asfortranarray(AMP * gx), np.asfortranarray(AMP * gu)


def _handle(pkg, prob, B, settings, x0s, X=None, U=None, knots=None, prepare=True):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=B, rho=prob.rho, **settings)
    s.set_bound_constraints(*(a[:, 0] for a in prob.expanded_bounds()))
    if prepare:
        s.prepare()
    if X is not None:
        s.set_x_ref_batch(X)
    if U is not None:
        s.set_u_ref_batch(U)
    if knots is not None:
        s.set_bound_constraints_batch(*knots)
    s.set_x0_batch(x0s)
    return s


def _everything(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


def _same(a, b, tag):
    for x, y, what in zip(a, b, WHAT):
        np.testing.assert_array_equal(x, y, err_msg=f"{tag}: {what}")


def _named(s, refill, words):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert ("slot-refill" in info) == refill and "refused" not in info, info
    for w in words:
        assert w in info, (w, info)


def _both_kernels(pkg, monkeypatch, make, x0s, words, second=None):
    """A first solve, then a second one (from 0.9 x0 unless `second` names the x0s), under TINYMPC_REFILL 0 and 1
    -> {refill: (first, second)}; layout D and the form's words on both sides, `slot-refill` exactly where refill is on (a prepared handle
    settles on the form at its first solve: named from there on)."""
    got = {}
    for refill in (False, True):
        monkeypatch.setenv("TINYMPC_REFILL", "1" if refill else "0")
        s = make()
        s.solve()
        _named(s, refill, words)
        first = _everything(s)
        s.set_x0_batch(np.asfortranarray(0.9 * x0s) if second is None else second)
        s.solve()
        got[refill] = (first, _everything(s), s.jit_info())
        s.reset()
    _same(got[False][0], got[True][0], "first solve")
    _same(got[False][1], got[True][1], "second solve")
    return got


def _oracle_sample(prob, settings, x0s, got, B, n, X=None, U=None, full=None, gx=None, gu=None):
    """A seeded sample of n instances, each with its own trajectory (or goal) and its own bound schedule, against the C restatement (cold solve)."""
    N = prob.N
    for b in np.random.default_rng(1).choice(B, size=n, replace=False):
        orc = O.OraclePort(prob).load_problem(prob, settings)
        if X is not None:
            orc.set_x_ref(X[:, :, b])
        if U is not None:
            orc.set_u_ref(U[:, :, b])
        if gx is not None:
            orc.set_x_ref(np.repeat(gx[:, b:b + 1], N, axis=1))
            orc.set_u_ref(np.repeat(gu[:, b:b + 1], N - 1, axis=1))
        if full is not None:
            orc.set_bound_constraints(*(a[:, :, b] for a in full))
        orc.set_x0(x0s[:, b])
        orc.solve()
        assert got[2][b] == orc.stats()["iter"], b
        assert (got[3][b] == 1) == (orc.stats()["status"] == 1), b
        assert rel_err(got[0][:, :, b], orc.solution()[0]) < TOL, b
        assert rel_err(got[1][:, :, b], orc.solution()[1]) < TOL, b


SHAPES = {  # name -> (problem, batch, check_termination, max_iter, compiled in?)
    "quadrotor50": (lambda P: P.quadrotor(50), 4611, 1, 60, True),    # the compiled-in kernel, one wavefront per SIMD; a ragged last group of three
    "quadrotor20": (lambda P: P.quadrotor(20), 8707, 3, 45, False),   # run-time specialised, two wavefronts per SIMD; a check interval that divides nothing
    "cartpole20": (lambda P: P.cartpole(20), 8500, 1, 30, False),     # one input
}


# ---- 1. + 2. bit identity to the plain trajectory form, and the oracle sample

@pytest.mark.parametrize("shape", list(SHAPES))
def test_trajectory_refill_is_bit_identical_to_the_plain_trajectory_form(pkg, monkeypatch, shape):
    """Cold, then warm from 0.9 x0. (On the parent commit the `slot-refill` assertion fails: the trajectory form has no variant there.)
    Instances that converge after a few iterations next to ones that run max_iter -- the condition below holds for these inputs by the
    algorithm alone: on the oracle the 64-instance sample rng(1).choice(B, 64) runs 8..60 iterations (18 distinct counts, 15 at
    max_iter) for quadrotor50, 9..45 (7 distinct, 19 at max_iter) for quadrotor20 and 4..30 (21 distinct, 10 at max_iter) for cartpole20,
    every instance below max_iter solved."""
    P = pkg.problems
    make, B, ct, max_iter, builtin = SHAPES[shape]
    prob = make(P)
    x0s, (X, U) = _x0s(P, prob, B), _trajs(prob, B)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=max_iter, check_termination=ct)
    got = _both_kernels(pkg, monkeypatch, lambda: _handle(pkg, prob, B, settings, x0s, X, U), x0s, ["per-instance-trajectories"])
    for refill in (False, True):  # (the quadrotor N=50 kernels are found by the options of their plan: a plan that moved would leave them to the run-time compiler)
        assert ("compiled-in" in got[refill][2]) == builtin, got[refill][2]
    it, status = got[True][0][2], got[True][0][3]
    print(shape, "iterations", it.min(), it.max(), "distinct", len(np.unique(it)), "at max_iter", int((it == max_iter).sum()))
    assert it.min() < max_iter and it.max() == max_iter and len(np.unique(it)) > 5  # (a spread worth refilling for)
    assert np.all(status[it < max_iter] == 1)
    _oracle_sample(prob, settings, x0s, got[True][0], B, 16, X=X, U=U)


# ---- 3. per-knot bounds per instance: beside goals, beside trajectories

@pytest.mark.parametrize("N,B,traj", [(20, 4611, False), (20, 4611, True), (10, 8707, False)])
def test_per_knot_bounds_refill_is_bit_identical_to_the_plain_form(pkg, monkeypatch, N, B, traj):
    """Bounds per knot and instance with a goal per instance (IKBND), or with a trajectory per instance (IKBND with ITRAJ: the plain
    kernel is the compiled-in k_builtin_d_quadrotor20_traj_kbnd). N=10 keeps two wavefronts per SIMD with its clamp rows, so its batch
    lies beyond 8,192."""
    P = pkg.problems
    prob = P.quadrotor(N)
    x0s = _x0s(P, prob, B)
    knots, full = _bounds(prob, B, "knot")
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=1)
    if traj:
        X, U = _trajs(prob, B)
        words, ref = ["per-instance-trajectories", "per-knot-bounds"], dict(X=X, U=U)
    else:
        X, U = _goals(prob, B)
        words, ref = ["per-knot-bounds"], dict(gx=X, gu=U)
    got = _both_kernels(pkg, monkeypatch, lambda: _handle(pkg, prob, B, settings, x0s, X, U, knots), x0s, words)
    it = got[True][0][2]
    print(N, B, traj, "iterations", it.min(), it.max(), "distinct", len(np.unique(it)))
    assert it.min() < 60  # (some rows are refilled before the others finish)
    _oracle_sample(prob, settings, x0s, got[True][0], B, 8, full=full, **ref)


# ---- 4. one half per instance

@pytest.mark.parametrize("half", ["x_only", "x_ref_range"])
def test_trajectory_refill_with_only_one_half_per_instance(pkg, monkeypatch, half):
    """State trajectories only, beside a shared constant input reference; trajectories for instances 100..4099 only -- the rest keep the
    shared goal. The trajectory form all the same (the shared values fill the other rows): refill is taken, bit-identical."""
    P = pkg.problems
    prob, B = P.quadrotor(50), 4611
    x0s, (X, U) = _x0s(P, prob, B), _trajs(prob, B)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=60, check_termination=1)

    def make():
        s = _handle(pkg, prob, B, settings, x0s, X if half == "x_only" else None)
        if half == "x_ref_range":
            s.set_x_ref_batch(np.asfortranarray(X[:, :, 100:4100]), first=100)
        return s

    _both_kernels(pkg, monkeypatch, make, x0s, ["per-instance-trajectories"])


# ---- 5. edges

@pytest.mark.parametrize("B,ct,max_iter,tol", [(4097, 1, 30, 1e-3), (4611, 1, 1, 1e-3), (4611, 5, 3, 1e-3), (4611, 1, 25, 1e3)])
def test_trajectory_refill_edges(pkg, monkeypatch, B, ct, max_iter, tol):
    """One instance more than a resident set; max_iter 1; a check interval beyond max_iter (nobody is ever tested); tolerances
    everything meets at the first check. A first solve and a warm one on the same x0: the plain form's bits."""
    P = pkg.problems
    prob = P.quadrotor(50)
    x0s, (X, U) = _x0s(P, prob, B), _trajs(prob, B)
    settings = dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=max_iter, check_termination=ct)
    got = _both_kernels(pkg, monkeypatch, lambda: _handle(pkg, prob, B, settings, x0s, X, U), x0s, ["per-instance-trajectories"], second=x0s)
    if ct > max_iter:
        assert np.all(got[True][0][2] == max_iter) and np.all(got[True][0][3] != 1)
    if tol >= 1e3:
        assert np.all(got[True][0][2] == ct) and np.all(got[True][0][3] == 1)


# ---- 6. policy

def test_trajectory_refill_is_only_taken_where_it_can_pay(pkg, monkeypatch):
    """One resident set, forced iteration counts without TINYMPC_REFILL=1, and TINYMPC_REFILL=0 keep the plain form; forced on with
    tolerances nothing meets, the variant returns the plain form's bits. Without the variable the form follows the measured default
    (profiles/refill_traj_ab.txt): on."""
    P = pkg.problems
    prob = P.quadrotor(50)
    reach = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=12, check_termination=1)
    forced = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=12, check_termination=1)
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    small = _handle(pkg, prob, 4096, reach, _x0s(P, prob, 4096), *_trajs(prob, 4096))
    small.solve()
    _named(small, False, ["per-instance-trajectories"])  # one resident set: nothing to refill with
    small.reset()
    B = 4611
    x0s, (X, U) = _x0s(P, prob, B), _trajs(prob, B)
    monkeypatch.delenv("TINYMPC_REFILL", raising=False)
    s = _handle(pkg, prob, B, forced, x0s, X, U)
    s.solve()
    _named(s, False, ["per-instance-trajectories"])  # nothing converges: nothing to balance
    plain = _everything(s)
    s.update_settings(abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    _named(s, True, ["per-instance-trajectories"])  # on by default: the variant was below the plain form in every round of its A/B
    monkeypatch.setenv("TINYMPC_REFILL", "0")
    _named(s, False, ["per-instance-trajectories"])
    s.reset()
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    s = _handle(pkg, prob, B, forced, x0s, X, U)
    s.solve()
    _named(s, True, ["per-instance-trajectories"])
    _same(plain, _everything(s), "forced iteration counts")
    assert np.all(plain[2] == 12) and np.all(plain[3] == 11)
    s.reset()



def test_what_has_no_variant_keeps_its_kernel(pkg, monkeypatch):
    """Under TINYMPC_REFILL=1 and beyond a resident set: without prepare() the trajectories stay on layout A; per-instance linear rows
    beside the trajectories, and per-instance models, run their own forms -- no `slot-refill` anywhere."""
    P = pkg.problems
    prob, B = P.quadrotor(20), 4611
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=12, check_termination=1)
    x0s, (X, U) = _x0s(P, prob, B), _trajs(prob, B)
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    a = _handle(pkg, prob, 8707, settings, _x0s(P, prob, 8707), *_trajs(prob, 8707), prepare=False)
    a.solve()
    assert a.launch_info()["layout"] == "A" and "slot-refill" not in a.jit_info(), a.jit_info()
    a.reset()
    lin = _handle(pkg, prob, B, settings, x0s, X, U)
    lin.set_linear_constraints_batch(*_rows(prob, 1, 1, B)[1:])
    lin.solve()
    info = lin.jit_info()
    assert "per-instance-linear" in info and "slot-refill" not in info, info
    lin.reset()
    mod = _handle(pkg, prob, B, settings, x0s, X, U)
    MG._set_models(mod, MG._models(prob, B))
    mod.solve()
    assert "per-instance-models" in mod.jit_info() and "slot-refill" not in mod.jit_info(), mod.jit_info()
    mod.reset()


# ---- 7. tracks

def test_tracks_refill_over_closed_loop_ticks(pkg, monkeypatch):
    """Both halves as tracks of T = 40 knots at N = 20, auto-advance on: three mpc_step ticks, every instance's state advanced by the shared
    plant. A twin under TINYMPC_REFILL=0 gets the same calls: first controls, steps and statistics equal bit for bit on every tick."""
    P = pkg.problems
    prob, B, T = P.quadrotor(20), 8707, 40
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40, check_termination=1)
    rng = np.random.default_rng(41)
    tt = np.arange(T)
    Xt = np.asfortranarray(0.03 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (prob.nx, 1, B))))
    Ut = np.asfortranarray(0.003 * np.cos(0.2 * tt[None, :, None] + rng.uniform(0, 6, (prob.nu, 1, B))))
    x = _x0s(P, prob, B)
    pair = []
    for k in range(2):  # [refill, twin]
        monkeypatch.setenv("TINYMPC_REFILL", "1" if k == 0 else "0")
        h = _handle(pkg, prob, B, settings, x)
        h.set_x_ref_track_batch(Xt)
        h.set_u_ref_track_batch(Ut)
        h.set_ref_auto_advance(1)
        pair.append(h)
    for tick in range(3):
        u = []
        for k, h in enumerate(pair):
            monkeypatch.setenv("TINYMPC_REFILL", "1" if k == 0 else "0")
            u.append(h.mpc_step(x).copy())
            _named(h, k == 0, ["per-instance-trajectories", "reference-track"])
        np.testing.assert_array_equal(u[0], u[1], err_msg=f"tick {tick}: first controls")
        np.testing.assert_array_equal(pair[0].get_ref_step_batch(), pair[1].get_ref_step_batch())
        np.testing.assert_array_equal(pair[0].get_ref_step_batch(), np.full(B, tick + 1, dtype=np.int32))
        _same(_everything(pair[1]), _everything(pair[0]), f"tick {tick}")
        it = pair[0].get_stats_batch()["iter"]
        assert len(np.unique(it)) > 1, tick  # (rows finish at different times: something is refilled)
        x = np.asfortranarray(prob.A @ x + prob.B @ u[0])
    for h in pair:
        h.reset()


# ---- 8. mode switches on one handle

def test_trajectory_refill_mode_switches_on_one_handle(pkg, monkeypatch):
    """Trajectories -> per-knot bounds beside them -> constant bounds again -> goals (the goal refill kernel) -> everything shared (the
    shared refill kernel), on the one ADMM state of a prepared handle; a twin under TINYMPC_REFILL=0 receives the same calls and returns
    the same bits."""
    P = pkg.problems
    prob, B = P.quadrotor(20), 8707
    N = prob.N
    x0s, (X, U) = _x0s(P, prob, B), _trajs(prob, B)
    gx, gu = _goals(prob, B)
    knots, _ = _bounds(prob, B, "knot")
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40, check_termination=1)
    monkeypatch.setenv("TINYMPC_REFILL", "1")
    pair = [_handle(pkg, prob, B, settings, x0s, X, U) for _ in range(2)]  # [refill, twin]

    def step(call, tag, words):
        for k, h in enumerate(pair):
            monkeypatch.setenv("TINYMPC_REFILL", "1" if k == 0 else "0")
            call(h)
            h.solve()
            _named(h, k == 0, words)
        _same(_everything(pair[1]), _everything(pair[0]), tag)

    def goals(h):  # (a half that held trajectories stays one until it leaves per-instance mode: through the shared verb)
        h.set_x_ref(np.zeros((prob.nx, N)))
        h.set_u_ref(np.zeros((prob.nu, N - 1)))
        h.set_x_ref_batch(gx)
        h.set_u_ref_batch(gu)

    def shared(h):
        h.set_x_ref(np.zeros((prob.nx, N)))
        h.set_u_ref(np.zeros((prob.nu, N - 1)))

    step(lambda h: None, "trajectories", ["per-instance-trajectories"])
    step(lambda h: h.set_bound_constraints_batch(*knots), "per-knot bounds beside them", ["per-instance-trajectories", "per-knot-bounds"])
    step(lambda h: h.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max), "constant bounds again", ["per-instance-trajectories"])
    step(goals, "goals", [" goal"])
    step(shared, "everything shared", [])
    assert "per-instance" not in pair[0].jit_info(), pair[0].jit_info()
    for h in pair:
        h.reset()

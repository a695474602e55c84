"""Per-instance linear rows together with per-instance trajectories and tracks on layout D (tinympc_set_linear_constraints_batch /
_knots_batch / tinympc_set_cone_slopes_batch with tinympc_set_x_ref_batch / _u_ref_batch / the track verbs on a handle that called
tinympc_prepare): the per-instance families' kernel reading every slot's linref from its wavefront's own LDS copy of the trajectory rows
(ILIN with ITRAJ in tinympc_solve_d.hip). Every instance still solves what a single-instance handle with its own rows and its own
trajectory would -- against the plain-C oracle per sampled instance (the stepped oracle for rows per knot), against the layout A kernel
over the whole batch, bit for bit against the neighbouring forms where the inputs coincide --, one handle moves through the forms with
its ADMM state kept, and what the form does not carry stays on layout A and stays correct.

Shapes are the siblings': 37 instances under TINYMPC_LAYOUT=D (nine full wavefronts and one with a single instance), 70 for sub-ranges;
quadrotor N=20 with 1+1 rows (the compiled-in kernel), cartpole N=20 (KT = 8; run-time specialised), the rocket landing nx=6 nu=3
N=10 with cones, fdyn and its real reference trajectory, quadrotor N=17 and N=12 with one row per knot (N=17: the longest horizon
whose N slots of rows and N + 2 linref rows fit a wavefront's LDS share, tests/test_instance_lin_traj_plan_cpu.py). Rows, seed, TOL and
oracle helpers are the siblings' (test_instance_lin_gpu.py, knot_lin_cases.py, instance_cone_cases.py); trajectories are
test_instance_bounds_gpu._refs(..., "trajectory", seed=TRAJ_SEED)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from conftest import rel_err

import instance_cone_cases as IC
import knot_lin_cases as K
from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs
from test_instance_lin_d_gpu import _d_solver
from test_instance_lin_gpu import CONV, SEED, TOL, _assert_matches, _assert_same_bits, _of, _oracle, _rows, _run, _sample
from test_instance_lin_traj_plan_cpu import lin_traj_plan, longest_knots_horizon
from test_instance_traj_d_gpu import _each_instance_close
from test_instance_traj_plan_cpu import first_fit

pytestmark = pytest.mark.gpu

TRAJ_SEED = 1
BATCH = 37
SHAPES = {"quadrotor20": lambda P: P.quadrotor(20), "cartpole20": lambda P: P.cartpole(20, True)}
SHORT = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)


def _on_d(s, knots=False, track=False):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert ("per-knot-linear" if knots else "per-instance-linear") in info and "per-instance-trajectories" in info and "refused" not in info, info
    assert ("reference-track" in info) == track, info
    return info


def _on_a(s):
    assert s.launch_info()["layout"] == "A", (s.launch_info(), s.jit_info())
    return s.jit_info()


def _traj_oracle(prob, settings, rows_b, Xb, Ub):
    """The oracle of one instance: its own rows (None: no rows) and its own reference trajectory."""
    orc = _oracle(prob, settings, rows_b)
    orc.set_x_ref(Xb)
    orc.set_u_ref(Ub)
    return orc


def _send(handles, rows, vx, vu, knots=False):
    for h in handles:
        (h.set_linear_constraints_knots_batch if knots else h.set_linear_constraints_batch)(*rows)
        h.set_x_ref_batch(vx)
        h.set_u_ref_batch(vu)


def _solve_all(handles, x0s):
    for h in handles:
        h.set_x0_batch(x0s)
        h.solve()


@functools.lru_cache(maxsize=None)
def _parity_reference(pkg, shape):
    """Computed once per shape and shared, never modified: the oracle's cold solve of every sampled instance without rows (`free`), and the
    cold and two warm solves under its own rows (`own`: one list of three results per instance)."""
    prob = SHAPES[shape](pkg.problems)
    x0s, *rows = _rows(prob, 1, 1, BATCH)
    _, (X, U) = _refs(prob, BATCH, "trajectory", seed=TRAJ_SEED)
    own, free = {}, {}
    for b in _sample(BATCH):
        free[b] = _run(_traj_oracle(prob, CONV, None, X[:, :, b], U[:, :, b]), x0s[:, b])
        orc = _traj_oracle(prob, CONV, _of(rows, b), X[:, :, b], U[:, :, b])
        own[b] = [_run(orc, x0s[:, b] * (1.0 - 0.2 * rnd)) for rnd in range(3)]
    return own, free


# ---- 1. parity: the oracle per sampled instance, the layout A twin over the whole batch; cold and two warm solves

@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_instance_matches_the_oracle_and_the_layout_a_twin(pkg, monkeypatch, shape):
    """(On the parent commit the prepared handle stays on layout A: this test fails there.)"""
    prob = SHAPES[shape](pkg.problems)
    x0s, *rows = _rows(prob, 1, 1, BATCH)
    (vx, vu), (X, U) = _refs(prob, BATCH, "trajectory", seed=TRAJ_SEED)
    own, free = _parity_reference(pkg, shape)
    # the oracle alone: the rows act in at least half the sample, and every sampled trajectory is one (it leaves its first column)
    active = [max(rel_err(own[b][0][0], free[b][0]), rel_err(own[b][0][1], free[b][1])) > 1e-6 for b in own]
    print(shape, "oracle iterations", [[r[2] for r in own[b]] for b in own], "rows active", active)
    assert 2 * sum(active) >= len(active), active
    for b in own:
        assert rel_err(X[:, :, b], np.repeat(X[:, :1, b], prob.N, axis=1)) > 1e-3 and rel_err(U[:, :, b], np.repeat(U[:, :1, b], prob.N - 1, axis=1)) > 1e-3, b
    d, a = _d_solver(pkg, monkeypatch, prob, BATCH, CONV), _d_solver(pkg, monkeypatch, prob, BATCH, CONV)
    _send((d, a), rows, vx, vu)
    _on_a(d)
    d.prepare()
    for rnd in range(3):
        _solve_all((d, a), x0s * (1.0 - 0.2 * rnd))
        info = _on_d(d)
        assert "per-instance-linear" in _on_a(a)
        _assert_matches(d, {b: own[b][rnd] for b in own}, (shape, "round", rnd))
        _each_instance_close(d, a, (shape, rnd))
    # (the quadrotor's kernel is found by the options of its plan: a plan that moved would leave it to the run-time compiler)
    assert ("compiled-in" in info) == (shape == "quadrotor20"), info
    assert "per-instance-refs" in info, info
    # the host's plan: the candidate and the bytes the restated arithmetic gives
    (wps, wpg), lds = first_fit(lin_traj_plan(prob.nx, prob.nu, prob.N))
    li = d.launch_info()
    assert (wps, wpg) == (1, 4)
    assert li["lds_bytes"] == lds and li["workgroups"] == -(-((BATCH + 3) // 4) // wpg), (li, wps, wpg, lds)
    d.reset()
    a.reset()


# ---- 2. the rocket landing: cones with per-instance slopes, one row, fdyn, and its real reference trajectory per instance

def test_the_rocket_landing_follows_its_trajectory_on_layout_d(pkg, monkeypatch):
    prob, batch, settings, x0s, cx, cu = IC.data(pkg, "rocket10")  # (problems.rocket(10) as it is: the line from the start to the pad)
    rng = np.random.default_rng(SEED)
    assert rel_err(prob.x_ref, np.repeat(prob.x_ref[:, :1], prob.N, axis=1)) > 1e-3
    X = prob.x_ref[:, :, None] + 0.2 * rng.standard_normal((prob.nx, 1, batch))  # every instance's own offset of the whole line
    Ax = np.repeat(np.asarray(prob.linear["Alin_x"], dtype=np.float64)[:, :, None], batch, axis=2)
    ax0 = np.einsum("kcb,cb->kb", Ax, x0s)
    factor = np.where(np.arange(batch)[None, :] % 3 != 0, rng.uniform(0.0, 0.1, (1, batch)), rng.uniform(0.5, 2.0, (1, batch)))
    bx = ax0 + factor * (1.0 + np.abs(ax0))  # (test_instance_lin_d_gpu._rocket's "binding" ground planes)
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")
    d, a = IC.solver(pkg, prob, batch, settings), IC.solver(pkg, prob, batch, settings)
    for h in (d, a):
        h.set_cone_slopes_batch(cx, cu)
        h.set_linear_constraints_batch(Ax, bx, None, None)
        h.set_x_ref_batch(X)
    d.prepare()
    expect = {}
    for b in IC.sample(batch):
        orc = IC.oracle(prob, settings, cx[:, b], cu[:, b])
        orc.set_linear_constraints(Ax[:, :, b], bx[:, b], np.zeros((0, prob.nu)), np.zeros(0))
        orc.update_settings()
        orc.set_x_ref(X[:, :, b])
        expect[b] = IC.run(orc, x0s[:, b])
    _solve_all((d, a), x0s)
    info = _on_d(d)
    assert "per-instance-cones" in info, info
    _on_a(a)
    IC.assert_matches(d, expect, "rocket on D")
    _each_instance_close(d, a, "rocket")
    (wps, wpg), lds = first_fit(lin_traj_plan(prob.nx, prob.nu, prob.N))
    assert d.launch_info()["lds_bytes"] == lds, (d.launch_info(), lds)
    d.reset()
    a.reset()


# ---- 3. rows per knot + trajectories, at the longest horizon the plan takes and at N=12

@pytest.mark.parametrize("N", [17, 12])
def test_rows_per_knot_on_trajectories(pkg, monkeypatch, N):
    assert longest_knots_horizon(12, 4, 1) == 17
    prob, batch = pkg.problems.quadrotor(N), 21
    x0s, *rows = K.rows_knots(prob, 1, 1, batch)
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=TRAJ_SEED)
    d, a = _d_solver(pkg, monkeypatch, prob, batch, K.CONV), _d_solver(pkg, monkeypatch, prob, batch, K.CONV)
    _send((d, a), rows, vx, vu, knots=True)
    d.prepare()
    expect = {}
    for b in K.sample(batch):
        so = K.SteppedOracle(prob, K.CONV, K.of(rows, b))
        so.orc.set_x_ref(X[:, :, b])
        so.orc.set_u_ref(U[:, :, b])
        expect[b] = so.solve(x0s[:, b], K.of(rows, b))
    _solve_all((d, a), x0s)
    _on_d(d, knots=True)
    assert "per-knot-linear" in _on_a(a)
    _assert_matches(d, expect, ("knots + trajectories", N))
    _each_instance_close(d, a, ("knots", N))
    (wps, wpg), lds = first_fit(lin_traj_plan(prob.nx, prob.nu, N, knots=True))
    assert d.launch_info()["lds_bytes"] == lds, (d.launch_info(), lds)
    d.reset()
    a.reset()


def test_rows_repeated_over_the_knots_are_the_constant_rows_bit_for_bit(pkg, monkeypatch):
    prob, batch = pkg.problems.quadrotor(17), 21
    x0s, *const = _rows(prob, 1, 1, batch)
    (vx, vu), _ = _refs(prob, batch, "trajectory", seed=TRAJ_SEED)
    twin, knots = _d_solver(pkg, monkeypatch, prob, batch, CONV), _d_solver(pkg, monkeypatch, prob, batch, CONV)
    _send((twin,), const, vx, vu)
    _send((knots,), K.repeat_over_knots(const, prob.N), vx, vu, knots=True)
    for h in (twin, knots):
        h.prepare()
    for rnd in range(3):
        _solve_all((twin, knots), x0s * (1.0 - 0.2 * rnd))
        _assert_same_bits(twin, knots)  # states, controls, iterations, status, the four residuals
    _on_d(twin)
    _on_d(knots, knots=True)
    twin.reset()
    knots.reset()


# ---- 4. trajectories of N equal columns == the goal form on the same handle shape

@pytest.mark.parametrize("shape", list(SHAPES))
def test_equal_columns_are_the_goal_form_bit_for_bit(pkg, monkeypatch, shape):
    """One pass builds both stores (k_build_inst_tables: the goal form's row is knot 0's row of the trajectory form's store, the same
    product -(ref * diag)), so equal columns give N equal rows and the two forms the same bits.

    The host verb looks at its data: N equal columns ARE a goal to it. The half becomes a trajectory half -- and stays one, the flag is
    sticky -- through one instance's real trajectory, which the equal columns then replace."""
    prob = SHAPES[shape](pkg.problems)
    x0s, *rows = _rows(prob, 1, 1, BATCH)
    (gx, gu), (Xg, Ug) = _refs(prob, BATCH, "goal", seed=TRAJ_SEED)
    goal, traj = _d_solver(pkg, monkeypatch, prob, BATCH, CONV), _d_solver(pkg, monkeypatch, prob, BATCH, CONV)
    _send((goal,), rows, gx, gu)      # one column per instance: the ILIN goal form
    _send((traj,), rows, Xg, Ug)      # N equal columns per instance: trajectories
    (vx, vu), _ = _refs(prob, BATCH, "trajectory", seed=TRAJ_SEED)
    for verb, real, equal in ((traj.set_x_ref_batch, vx, Xg), (traj.set_u_ref_batch, vu, Ug)):
        verb(real[:, :, :1], first=0)
        verb(equal[:, :, :1], first=0)
    for h in (goal, traj):
        h.prepare()
    for rnd in range(3):
        _solve_all((goal, traj), x0s * (1.0 - 0.2 * rnd))
        _assert_same_bits(goal, traj)
    _on_d(traj)
    info = goal.jit_info()
    assert goal.launch_info()["layout"] == "D" and "goal" in info and "per-instance-trajectories" not in info, info
    goal.reset()
    traj.reset()


# ---- 5. tracks with auto-advance, rows re-sent every tick

def test_tracks_with_rows_re_sent_every_tick(pkg, monkeypatch):
    prob = pkg.problems.quadrotor(20)
    N, T, ticks = prob.N, prob.N + 8, 6
    d, a = _d_solver(pkg, monkeypatch, prob, BATCH, SHORT), _d_solver(pkg, monkeypatch, prob, BATCH, SHORT)
    d.prepare()
    rng = np.random.default_rng(41)
    tt = np.arange(T)
    Xt = np.asfortranarray(0.3 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (prob.nx, 1, BATCH))))
    Ut = np.asfortranarray(0.03 * np.cos(0.2 * tt[None, :, None] + rng.uniform(0, 6, (prob.nu, 1, BATCH))))
    for h in (d, a):
        h.set_x_ref_track_batch(Xt)
        h.set_u_ref_track_batch(Ut)
        h.set_ref_auto_advance(1)
    x = None
    for k in range(ticks):
        x0s, *rows = _rows(prob, 1, 1, BATCH, seed=SEED + k)  # (the obstacle-relinearisation pattern: new rows in front of every tick)
        x = x0s if x is None else x
        for h in (d, a):
            h.set_linear_constraints_batch(*rows)
        ud, ua = d.mpc_step(x), a.mpc_step(x)
        _on_d(d, track=True)
        assert "per-instance-linear" in _on_a(a)
        err = np.max(np.abs(ud - ua), axis=0) / np.maximum(np.max(np.abs(ua), axis=0), 1e-300)
        print("tracks tick %d: worst instance %d rel_err %.2e" % (k, int(np.argmax(err)), float(np.max(err))))
        assert np.all(err < TOL), (k, int(np.argmax(err)), float(np.max(err)))
        _each_instance_close(d, a, ("track tick", k))
        np.testing.assert_array_equal(d.get_ref_step_batch(), np.full(BATCH, k + 1, dtype=np.int32))
        np.testing.assert_array_equal(a.get_ref_step_batch(), d.get_ref_step_batch())
        x = np.asfortranarray(prob.A @ x + prob.B @ ud)
    d.reset()
    a.reset()


def test_a_track_tick_matches_the_oracle_fed_the_windows_by_hand(pkg, monkeypatch):
    prob = pkg.problems.quadrotor(20)
    N, T, ticks = prob.N, prob.N + 8, 3
    d = _d_solver(pkg, monkeypatch, prob, BATCH, SHORT)
    d.prepare()
    rng = np.random.default_rng(43)
    tt = np.arange(T)
    Xt = np.asfortranarray(0.3 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (prob.nx, 1, BATCH))))
    Ut = np.asfortranarray(0.03 * np.cos(0.2 * tt[None, :, None] + rng.uniform(0, 6, (prob.nu, 1, BATCH))))
    x0s, *rows = _rows(prob, 1, 1, BATCH)
    d.set_linear_constraints_batch(*rows)
    d.set_x_ref_track_batch(Xt)
    d.set_u_ref_track_batch(Ut)
    d.set_ref_auto_advance(1)
    orcs = {b: _oracle(prob, SHORT, _of(rows, b)) for b in _sample(BATCH)}
    x = x0s
    for k in range(ticks):
        ud = d.mpc_step(x)
        _on_d(d, track=True)
        cx, cu = np.minimum(k + np.arange(N), T - 1), np.minimum(k + np.arange(N - 1), T - 1)
        expect = {}
        for b, orc in orcs.items():  # (every tick: the oracle is warm-started like the handle)
            orc.set_x_ref(Xt[:, cx, b])
            orc.set_u_ref(Ut[:, cu, b])
            expect[b] = _run(orc, x[:, b])
        _assert_matches(d, expect, ("track tick", k))
        x = np.asfortranarray(prob.A @ x + prob.B @ ud)
    d.reset()


# ---- 6. one handle moves through the forms; the ADMM state, the families' duals included, is shared

def test_one_handle_moves_through_the_forms(pkg, monkeypatch):
    prob = pkg.problems.quadrotor(20)
    N = prob.N
    x0s, Ax, bx, Au, bu = _rows(prob, 1, 1, BATCH)
    (vx, vu), (X, U) = _refs(prob, BATCH, "trajectory", seed=TRAJ_SEED)
    samples = _sample(BATCH)
    rng = np.random.default_rng(3)
    goal = 0.3 * rng.standard_normal(prob.nx)
    shared_traj = goal[:, None] * np.linspace(0.2, 1.0, N)[None, :]
    s = _d_solver(pkg, monkeypatch, prob, BATCH, SHORT)
    s.set_linear_constraints_batch(Ax, bx, Au, bu)
    s.prepare()
    orcs = {b: _oracle(prob, SHORT, _of((Ax, bx, Au, bu), b)) for b in samples}
    off = samples[2]
    stages = [("D", "goal"), ("D", "per-instance-trajectories"), ("A", None), ("D", "goal"), ("D", "goal")]
    for tick, (layout, word) in enumerate(stages):
        if tick == 1:  # per-instance trajectories arrive: the new form
            s.set_x_ref_batch(vx)
            s.set_u_ref_batch(vu)
            for b, orc in orcs.items():
                orc.set_x_ref(X[:, :, b])
                orc.set_u_ref(U[:, :, b])
        if tick == 2:  # a SHARED trajectory through the shared verb: layout A, as pinned by the siblings
            s.set_x_ref(shared_traj)
            s.set_u_ref(prob.u_ref if prob.u_ref is not None else np.zeros((prob.nu, N - 1)))
            for orc in orcs.values():
                orc.set_x_ref(shared_traj)
                orc.set_u_ref(prob.u_ref if prob.u_ref is not None else np.zeros((prob.nu, N - 1)))
        if tick == 3:  # the goal back: the ILIN goal form
            s.set_x_ref(np.repeat(goal[:, None], N, axis=1))
            for orc in orcs.values():
                orc.set_x_ref(np.repeat(goal[:, None], N, axis=1))
        if tick == 4:  # b = +inf for one instance: both of its rows are off
            s.set_linear_constraints_batch(Ax[:, :, off:off + 1], np.full((1, 1), np.inf), Au[:, :, off:off + 1], np.full((1, 1), np.inf), first=off)
            orcs[off].set_linear_constraints(Ax[:, :, off], np.full(1, np.inf), Au[:, :, off], np.full(1, np.inf))
            orcs[off].update_settings()
        x = x0s * (1.0 - 0.15 * tick)
        s.set_x0_batch(x)
        s.solve()
        info = s.jit_info()
        assert s.launch_info()["layout"] == layout and "per-instance-linear" in info, (tick, s.launch_info(), info)
        assert ("per-instance-trajectories" in info) == (tick == 1), (tick, info)
        assert word is None or (word in info and "refused" not in info), (tick, info)
        _assert_matches(s, {b: _run(orcs[b], x[:, b]) for b in samples}, ("form tick", tick, layout))
    s.reset()


# ---- 7. what the form does not carry stays on layout A and stays correct

@pytest.mark.parametrize("name", ["no-prepare", "knots-n20", "per-knot-bounds", "nojit-cartpole"])
def test_what_the_form_does_not_carry_stays_on_layout_a(pkg, monkeypatch, name):
    P = pkg.problems
    prob = P.cartpole(20, True) if name == "nojit-cartpole" else P.quadrotor(20)
    if name == "nojit-cartpole":  # a shape that is not compiled in, the specialiser switched off
        monkeypatch.setenv("TINYMPC_JIT", "0")
    (vx, vu), (X, U) = _refs(prob, BATCH, "trajectory", seed=TRAJ_SEED)
    s = _d_solver(pkg, monkeypatch, prob, BATCH, SHORT)
    samples = _sample(BATCH)
    full = None
    if name == "knots-n20":  # 20 slots of rows and 22 linref rows: 304 + 3,840 + 1,408 doubles of a wavefront's 4,992
        x0s, *rows = K.rows_knots(prob, 1, 1, BATCH)
        _send((s,), rows, vx, vu, knots=True)
    else:
        x0s, *rows = _rows(prob, 1, 1, BATCH)
        _send((s,), rows, vx, vu)
    if name == "per-knot-bounds":
        knots, full = _bounds(prob, BATCH, "knot", seed=33)
        s.set_bound_constraints_batch(*knots)
    if name != "no-prepare":
        s.prepare()
    s.set_x0_batch(x0s)
    s.solve()
    info = _on_a(s)
    if name == "knots-n20":
        assert "refused(" in info and "per-knot-linear" in info and "per-instance-trajectories" in info, info
        assert first_fit(lin_traj_plan(12, 4, 20, knots=True))[0] is None
    if name == "nojit-cartpole":
        assert "refused(TINYMPC_JIT=0)" in info and "per-instance-linear" in info, info
    expect = {}
    for b in samples:
        if name == "knots-n20":
            so = K.SteppedOracle(prob, SHORT, K.of(rows, b))
            so.orc.set_x_ref(X[:, :, b])
            so.orc.set_u_ref(U[:, :, b])
            expect[b] = so.solve(x0s[:, b], K.of(rows, b))
        else:
            orc = _traj_oracle(prob, SHORT, _of(rows, b), X[:, :, b], U[:, :, b])
            if full is not None:
                orc.set_bound_constraints(*(f[:, :, b] for f in full))
            expect[b] = _run(orc, x0s[:, b])
    _assert_matches(s, expect, name)
    s.reset()


def test_cones_in_rounds_stay_on_layout_a_with_trajectories(pkg, monkeypatch):
    name = "rocket20-held-two-rounds"
    prob, batch, settings, x0s, cx, cu = IC.data(pkg, name)
    settings = dict(settings, max_iter=40)
    rng = np.random.default_rng(SEED)
    X = prob.x_ref[:, :, None] * (1.0 + 0.1 * np.linspace(0.0, 1.0, prob.N)[None, :, None] * rng.standard_normal((prob.nx, 1, batch)))
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")
    s = IC.solver(pkg, prob, batch, settings)
    s.set_cone_slopes_batch(cx, cu)
    s.set_x_ref_batch(X)
    s.prepare()
    info = _on_a(s)
    assert "refused(" in info and "rounds" in info, info
    s.set_x0_batch(x0s)
    s.solve()
    _on_a(s)
    expect = {}
    for b in IC.sample(batch):
        orc = IC.oracle(prob, settings, cx[:, b], cu[:, b])
        orc.set_x_ref(X[:, :, b])
        expect[b] = IC.run(orc, x0s[:, b])
    IC.assert_matches(s, expect, name)
    s.reset()


# ---- 8. sub-ranges and device input

def test_sub_ranges_and_device_input(pkg, monkeypatch):
    prob, batch, lo, hi = pkg.problems.quadrotor(20), 70, 10, 60
    x0s, *rows = _rows(prob, 1, 1, batch)
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=TRAJ_SEED)
    shared_rows = _of(rows, batch - 1)
    host, devh, shared = (_d_solver(pkg, monkeypatch, prob, batch, SHORT) for _ in range(3))
    for h in (host, devh, shared):
        h.set_linear_constraints(*shared_rows)  # the shared rows every instance outside the range keeps
    sub = tuple(a[..., lo:hi] for a in rows)
    host.set_linear_constraints_batch(*sub, first=lo)
    host.set_x_ref_batch(vx[:, :, lo:hi], first=lo)
    host.set_u_ref_batch(vu[:, :, lo:hi], first=lo)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    n = hi - lo
    assert L.tinympc_set_linear_constraints_batch_device(devh._h, dev.put(sub[0]), dev.put(sub[1]), 1, dev.put(sub[2]), dev.put(sub[3]), 1, lo, n) == 0, pkg._lib.last_error()
    assert L.tinympc_set_x_ref_batch_device(devh._h, dev.put(vx[:, :, lo:hi]), prob.nx, prob.N, lo, n) == 0, pkg._lib.last_error()
    assert L.tinympc_set_u_ref_batch_device(devh._h, dev.put(vu[:, :, lo:hi]), prob.nu, prob.N - 1, lo, n) == 0, pkg._lib.last_error()
    dev.free()  # (the input has been copied when the verbs return)
    devh.settings["en_state_linear"] = devh.settings["en_input_linear"] = True  # (as the Python verb does after the C call)
    for h in (host, devh):
        h.prepare()
    _solve_all((host, devh, shared), x0s)
    _on_d(host)
    _on_d(devh)
    _assert_same_bits(host, devh)
    assert shared.launch_info()["layout"] == "D" and "per-instance" not in shared.jit_info(), shared.jit_info()
    _each_instance_close(host, shared, "below the range", 0, lo)
    _each_instance_close(host, shared, "above the range", hi, batch)
    samples = [lo, (lo + hi) // 2, hi - 1]
    expect = {b: _run(_traj_oracle(prob, SHORT, _of(rows, b), X[:, :, b], U[:, :, b]), x0s[:, b]) for b in samples}
    _assert_matches(host, expect, "inside the range")
    for h in (host, devh, shared):
        h.reset()

"""Per-instance reference trajectories and tracks on layout D (tinympc_set_x_ref_batch / _u_ref_batch / the track verbs on a handle that
called tinympc_prepare): the goal kernel with every wavefront's own linref rows staged into its LDS region (ITRAJ in
tinympc_solve_d.hip). Every instance still solves what a single-instance handle with its own trajectory would -- against the oracle per
instance, against the layout A kernel over the whole batch, bit for bit against the shared per-knot form of layout D where the
trajectories coincide --, a handle moves between layout A, the goal form and this form with its ADMM state kept, and everything the
form does not carry (a horizon whose rows fit no wavefront's LDS share, wide systems, a switched-off specialiser, per-instance models)
stays on layout A and stays correct.

Shapes, the smallest that reach every path (the sibling layout D tests use the same ones): quadrotor N=50 x 773 in the default
environment (773 > 768: layout D without a switch; the compiled-in kernel, one wavefront per SIMD; 193 full wavefronts + one instance: a
ragged last wavefront in a partial last workgroup), and quadrotor N=20 / cartpole N=20 (KT = 8) x 37 under TINYMPC_LAYOUT=D (run-time
specialised, two wavefronts per SIMD; the last wavefront holds one instance). Helpers, TOL and the sample are the sibling file's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
from conftest import rel_err

import test_instance_models_gpu as MG
from test_instance_bounds_gpu import _bounds
from test_instance_traj_plan_cpu import first_fit, traj_plan
from test_instance_refs_gpu import SETTINGS, TOL, _check, _oracle, _refs, _sample, _solver, _wide, _x0s

pytestmark = pytest.mark.gpu

SHAPES = {  # name -> (problem, batch, TINYMPC_LAYOUT at setup)
    "quadrotor50": (lambda P: P.quadrotor(50), 773, None),
    "quadrotor20": (lambda P: P.quadrotor(20), 37, "D"),
    "cartpole20": (lambda P: P.cartpole(20, True), 37, "D"),
}


def _handle(pkg, monkeypatch, prob, batch, layout, settings=SETTINGS):
    if layout:
        monkeypatch.setenv("TINYMPC_LAYOUT", layout)
    s = _solver(pkg, prob, batch, settings)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    return s


def _shape(pkg, shape):
    make, batch, layout = SHAPES[shape]
    return make(pkg.problems), batch, layout


def _on_d(s):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert "per-instance-trajectories" in info and "refused" not in info, info


def _on_a(s):
    assert s.launch_info()["layout"] == "A", (s.launch_info(), s.jit_info())
    assert "per-instance-refs" in s.jit_info(), s.jit_info()


def _each_instance_close(d, a, tag, lo=0, hi=None):
    """Iterations and status equal, states and controls within TOL, for EVERY instance of [lo, hi)."""
    sd, sa, td, ta = d.get_solution_batch(), a.get_solution_batch(), d.get_stats_batch(), a.get_stats_batch()
    sl = slice(lo, hi)
    np.testing.assert_array_equal(td["iter"][sl], ta["iter"][sl], err_msg=str(tag))
    np.testing.assert_array_equal(td["status"][sl], ta["status"][sl], err_msg=str(tag))
    for n in ("states", "controls"):
        x, y = sd[n][:, :, sl], sa[n][:, :, sl]
        err = np.max(np.abs(x - y), axis=(0, 1)) / np.maximum(np.max(np.abs(y), axis=(0, 1)), 1e-300)
        print("trajectories D against A %s %s: worst instance %d rel_err %.2e" % (tag, n, lo + int(np.argmax(err)), float(np.max(err))))
        assert np.all(err < TOL), (tag, n, lo + int(np.argmax(err)), float(np.max(err)))


def _same(a, b, tag=""):
    sa, sb = a.get_solution_batch(), b.get_solution_batch()
    np.testing.assert_array_equal(sa["states"], sb["states"], err_msg=str(tag))
    np.testing.assert_array_equal(sa["controls"], sb["controls"], err_msg=str(tag))
    ta, tb = a.get_stats_batch(), b.get_stats_batch()
    for k in ta:  # iterations, status, the four residuals
        np.testing.assert_array_equal(ta[k], tb[k], err_msg=str((tag, k)))


def _solve_all(handles, x0s):
    for h in handles:
        h.set_x0_batch(x0s)
        h.solve()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_instance_matches_the_oracle_and_layout_a(pkg, monkeypatch, shape):
    """One prepared handle and one unprepared twin with the same trajectories: the sample against the oracle, the whole batch against the
    twin; cold, then two warm starts. (On the parent commit the prepared handle stays on layout A: this test fails there.)"""
    prob, batch, layout = _shape(pkg, shape)
    d, a = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    d.prepare()
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory")
    for h in (d, a):
        h.set_x_ref_batch(vx)
        h.set_u_ref_batch(vu)
    orcs = {b: _oracle(prob, X[:, :, b], U[:, :, b]) for b in _sample(batch)}
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        _solve_all((d, a), x0s)
        _on_d(d)
        _on_a(a)
        _check(d, orcs, x0s, (shape, rnd))
        _each_instance_close(d, a, (shape, rnd))
    info = d.jit_info()
    assert ("compiled-in" in info) == (shape == "quadrotor50"), info
    assert "per-instance-refs" in info, info
    # the host's plan: the candidate and the bytes the restated arithmetic gives (two wavefronts per SIMD at N=20, one at N=50)
    (wps, wpg), lds = first_fit(traj_plan(prob.nx, prob.nu, prob.N))
    li = d.launch_info()
    assert wps == (1 if shape == "quadrotor50" else 2)
    assert li["lds_bytes"] == lds and li["workgroups"] == -(-((batch + 3) // 4) // wpg), (li, wps, wpg, lds)
    d.reset()
    a.reset()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_only_one_half_per_instance(pkg, monkeypatch, shape):
    """x trajectories with the shared u reference, then u trajectories with the shared x reference: both on layout D, within TOL of A."""
    prob, batch, layout = _shape(pkg, shape)
    (_, _), (Xs, Us) = _refs(prob, 1, "goal", seed=21)
    prob.x_ref, prob.u_ref = Xs[:, :, 0], Us[:, :, 0]  # a non-zero shared goal
    d, a = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    d.prepare()
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=22)
    x0s = _x0s(prob, batch)
    for h in (d, a):
        h.set_x_ref_batch(vx)
    _solve_all((d, a), x0s)
    _on_d(d)
    _on_a(a)
    _each_instance_close(d, a, (shape, "x only"))
    _check(d, {b: _oracle(prob, X[:, :, b], None) for b in (0, batch - 1)}, x0s, (shape, "x only"))
    for h in (d, a):
        h.set_x_ref(prob.x_ref)
        h.set_u_ref_batch(vu)
        h.reset_workspace()
    _solve_all((d, a), x0s)
    _on_d(d)
    _on_a(a)
    _each_instance_close(d, a, (shape, "u only"))
    _check(d, {b: _oracle(prob, None, U[:, :, b]) for b in (0, batch - 1)}, x0s, (shape, "u only"))
    d.reset()
    a.reset()


@pytest.mark.parametrize("shape", ["quadrotor20", "cartpole20"])
def test_equal_trajectories_are_bit_identical_to_the_shared_per_knot_form_of_layout_d(pkg, monkeypatch, shape):
    """Every instance given the shared trajectory: solutions, iterations, status and the four residuals of the handle that sent it through
    set_x_ref / set_u_ref, which runs layout D's shared per-knot form (the same sweeps reading the workgroup's table)."""
    prob, batch, layout = _shape(pkg, shape)
    (_, _), (X, U) = _refs(prob, 1, "trajectory", seed=5)
    prob.x_ref, prob.u_ref = X[:, :, 0], U[:, :, 0]
    shared, inst = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    inst.prepare()
    inst.set_x_ref_batch(np.repeat(prob.x_ref[:, :, None], batch, axis=2))
    inst.set_u_ref_batch(np.repeat(prob.u_ref[:, :, None], batch, axis=2))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        _solve_all((shared, inst), x0s)
        _same(shared, inst, (shape, rnd))
    _on_d(inst)
    assert shared.launch_info()["layout"] == "D" and "per-instance-refs" not in shared.jit_info(), shared.jit_info()
    shared.reset()
    inst.reset()


def test_partial_ranges_second_call_and_return_to_shared(pkg, monkeypatch):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 70
    (_, _), (Xs, Us) = _refs(prob, 1, "trajectory", seed=7)
    prob.x_ref, prob.u_ref = Xs[:, :, 0], Us[:, :, 0]  # a non-zero shared trajectory
    s, shared = _handle(pkg, monkeypatch, prob, batch, "D"), _handle(pkg, monkeypatch, prob, batch, "D")
    s.prepare()
    (tx, tu), (X, U) = _refs(prob, batch, "trajectory", seed=9)
    (t2x, t2u), (X2, U2) = _refs(prob, batch, "trajectory", seed=10)
    s.set_x_ref_batch(tx[:, :, 10:60], first=10)
    s.set_u_ref_batch(tu[:, :, 10:60], first=10)
    s.set_x_ref_batch(t2x[:, :, 55:57], first=55)  # a later call overrides a part of the earlier range
    s.set_u_ref_batch(t2u[:, :, 55:57], first=55)
    wx = {b: prob.x_ref for b in range(batch)}
    wu = {b: prob.u_ref for b in range(batch)}
    wx.update({b: X[:, :, b] for b in range(10, 60)})
    wu.update({b: U[:, :, b] for b in range(10, 60)})
    wx.update({b: X2[:, :, b] for b in (55, 56)})
    wu.update({b: U2[:, :, b] for b in (55, 56)})
    samples = [0, 9, 10, 54, 55, 56, 57, 59, 60, 69]
    orcs = {b: _oracle(prob, wx[b], wu[b]) for b in samples}
    x0s = _x0s(prob, batch)
    _solve_all((s, shared), x0s)
    _on_d(s)
    _check(s, orcs, x0s, "partial")
    # the instances no call named hold the shared trajectory: what the shared handle computes
    _each_instance_close(s, shared, "below the range", 0, 10)
    _each_instance_close(s, shared, "above the range", 60, batch)
    # set_x_ref / set_u_ref: every instance on the shared references, the handle on the shared plan again
    s.set_x_ref(prob.x_ref)
    s.set_u_ref(prob.u_ref)
    assert "per-instance" not in s.jit_info() and s.launch_info() == shared.launch_info(), (s.jit_info(), s.launch_info())
    for h in (s, shared):
        h.reset_workspace()
    _solve_all((s, shared), x0s)
    _same(s, shared, "shared again")
    s.reset()
    shared.reset()


def test_switching_forms_keeps_the_admm_state(pkg, monkeypatch):
    """goals (the goal form, D) -> trajectories (this form, D) -> per-knot per-instance bounds (layout A) -> constant bounds (D): one
    solve at each stage, every one a warm start of the last, against oracles that went the same way."""
    prob, batch, layout = _shape(pkg, "quadrotor50")
    s = _handle(pkg, monkeypatch, prob, batch, layout)
    s.prepare()
    (gx, gu), (Xg, Ug) = _refs(prob, batch, "goal", seed=31)
    (tx, tu), (Xt, Ut) = _refs(prob, batch, "trajectory", seed=32)
    knots, full = _bounds(prob, batch, "knot", seed=33)
    samples = _sample(batch)
    orcs = {b: _oracle(prob, Xg[:, :, b], Ug[:, :, b]) for b in samples}
    shared_bounds = prob.expanded_bounds()

    def stage(tag, layout_, word, scale, seed):
        x0s = _x0s(prob, batch, scale, seed=seed)
        s.set_x0_batch(x0s)
        s.solve()
        info = s.jit_info()
        assert s.launch_info()["layout"] == layout_ and word in info and "refused" not in info, (tag, s.launch_info(), info)
        _check(s, orcs, x0s, tag)

    s.set_x_ref_batch(gx)
    s.set_u_ref_batch(gu)
    stage("goals", "D", "goal", 1.0, 0)
    s.set_x_ref_batch(tx)
    s.set_u_ref_batch(tu)
    for b, orc in orcs.items():
        orc.set_x_ref(Xt[:, :, b])
        orc.set_u_ref(Ut[:, :, b])
    stage("trajectories", "D", "per-instance-trajectories", 0.8, 1)
    s.set_bound_constraints_batch(*knots)
    for b, orc in orcs.items():
        orc.set_bound_constraints(*(a[:, :, b] for a in full))
    stage("per-knot bounds", "A", "per-instance-bounds", 0.6, 2)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    for b, orc in orcs.items():
        orc.set_bound_constraints(*shared_bounds)
    stage("constant bounds", "D", "per-instance-trajectories", 0.5, 3)
    s.reset()


@pytest.mark.parametrize("shape", ["quadrotor50", "cartpole20"])
def test_tracks_with_auto_advance(pkg, monkeypatch, shape):
    """Both halves as tracks of T = N + 8 knots, auto-advance on: six closed-loop ticks on layout D, first controls within TOL of an
    unprepared twin's (layout A), equal steps, and the sixth tick's solution against an oracle fed the windows by hand."""
    prob, batch, layout = _shape(pkg, shape)
    N, T, ticks = prob.N, prob.N + 8, 6
    settings = dict(SETTINGS, max_iter=50)
    d, a = _handle(pkg, monkeypatch, prob, batch, layout, settings), _handle(pkg, monkeypatch, prob, batch, layout, settings)
    d.prepare()
    rng = np.random.default_rng(41)
    tt = np.arange(T)
    Xt = np.asfortranarray(0.3 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (prob.nx, 1, batch))))
    Ut = np.asfortranarray(0.03 * np.cos(0.2 * tt[None, :, None] + rng.uniform(0, 6, (prob.nu, 1, batch))))
    for h in (d, a):
        h.set_x_ref_track_batch(Xt)
        h.set_u_ref_track_batch(Ut)
        h.set_ref_auto_advance(1)
    samples = _sample(batch)
    orcs = {b: _oracle(prob, None, None, settings) for b in samples}
    x = _x0s(prob, batch)
    f = 0.0 if prob.fdyn is None else np.asarray(prob.fdyn, dtype=np.float64).reshape(prob.nx, 1)
    for k in range(ticks):
        ud, ua = d.mpc_step(x), a.mpc_step(x)
        info = d.jit_info()
        assert d.launch_info()["layout"] == "D" and "per-instance-trajectories" in info and "reference-track" in info and "refused" not in info, (k, info)
        assert a.launch_info()["layout"] == "A", (k, a.jit_info())
        err = np.max(np.abs(ud - ua), axis=0) / np.maximum(np.max(np.abs(ua), axis=0), 1e-300)
        print("tracks %s tick %d: worst instance %d rel_err %.2e" % (shape, k, int(np.argmax(err)), float(np.max(err))))
        assert np.all(err < TOL), (k, int(np.argmax(err)), float(np.max(err)))
        np.testing.assert_array_equal(d.get_ref_step_batch(), a.get_ref_step_batch())
        np.testing.assert_array_equal(d.get_ref_step_batch(), np.full(batch, k + 1, dtype=np.int32))
        np.testing.assert_array_equal(d.get_stats_batch()["iter"], a.get_stats_batch()["iter"])
        cx, cu = np.minimum(k + np.arange(N), T - 1), np.minimum(k + np.arange(N - 1), T - 1)
        sol, st = d.get_solution_batch(), d.get_stats_batch()
        for b, orc in orcs.items():  # (every tick: the oracle is warm-started like the handle)
            orc.set_x_ref(Xt[:, cx, b])
            orc.set_u_ref(Ut[:, cu, b])
            orc.set_x0(x[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (k, b)
            if k == ticks - 1:
                assert st["status"][b] == orc.stats()["status"], (k, b)
                assert rel_err(sol["states"][:, :, b], orc.solution()[0]) < TOL, (k, b)
                assert rel_err(sol["controls"][:, :, b], orc.solution()[1]) < TOL, (k, b)
        x = np.asfortranarray(prob.A @ x + prob.B @ ud + f)
    d.reset()
    a.reset()


def _refused_case(pkg, monkeypatch, name):
    P = pkg.problems
    if name == "quadrotor100":  # 102 rows of 512 B: more than a wavefront's LDS share under either plan
        prob = P.quadrotor(100)
        return prob, _handle(pkg, monkeypatch, prob, 37, "D"), None
    if name == "wide32":  # 32 lanes per instance
        prob = _wide(P, 24, 8, 20)
        return prob, _handle(pkg, monkeypatch, prob, 37, None), None
    if name == "nojit":  # a shape that is not compiled in, the specialiser switched off
        monkeypatch.setenv("TINYMPC_JIT", "0")
        prob = P.quadrotor(20)
        return prob, _handle(pkg, monkeypatch, prob, 37, "D"), None
    prob = P.quadrotor(20)  # trajectories together with per-instance models
    s = _handle(pkg, monkeypatch, prob, 37, "D")
    M = MG._models(prob, 37)
    MG._set_models(s, M)
    return prob, s, M


@pytest.mark.parametrize("name", ["quadrotor100", "wide32", "nojit", "models"])
def test_what_the_form_does_not_carry_stays_on_layout_a_and_correct(pkg, monkeypatch, name):
    prob, s, M = _refused_case(pkg, monkeypatch, name)
    batch = 37
    s.prepare()
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=51)
    s.set_x_ref_batch(vx)
    s.set_u_ref_batch(vu)
    orcs = {}
    for b in _sample(batch):
        orcs[b] = _oracle(prob if M is None else M.problem(prob, b), X[:, :, b], U[:, :, b])
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _on_a(s)
        _check(s, orcs, x0s, (name, rnd))
    if name == "quadrotor100":
        assert "refused" in s.jit_info() and "per-instance-trajectories" in s.jit_info(), s.jit_info()
    s.reset()


def test_device_input_matches_host_input(pkg, monkeypatch):
    """Trajectories from device memory (another handle's device solution: nx x N x batch and nu x (N-1) x batch, the verbs' layout)
    through the _device verbs: the solve of the same trajectories from numpy, bit for bit, both on layout D."""
    prob, batch, layout = _shape(pkg, "quadrotor50")
    src = _handle(pkg, monkeypatch, prob, batch, layout)
    src.set_x0_batch(_x0s(prob, batch, 0.5, seed=4))
    src.solve()
    d_x, d_u = C.c_void_p(), C.c_void_p()
    L = pkg.load_library()
    assert L.tinympc_get_solution_device_ptrs(src._h, C.byref(d_x), C.byref(d_u)) == 0
    sol = src.get_solution_batch()
    h, d = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    for q in (h, d):
        q.prepare()
    h.set_x_ref_batch(sol["states"])
    h.set_u_ref_batch(sol["controls"])
    assert L.tinympc_set_x_ref_batch_device(d._h, d_x, prob.nx, prob.N, 0, batch) == 0, pkg._lib.last_error()
    assert L.tinympc_set_u_ref_batch_device(d._h, d_u, prob.nu, prob.N - 1, 0, batch) == 0, pkg._lib.last_error()
    x0s = _x0s(prob, batch)
    _solve_all((h, d), x0s)
    _on_d(h)
    _on_d(d)
    _same(h, d, "device input")
    for q in (h, d, src):
        q.reset()

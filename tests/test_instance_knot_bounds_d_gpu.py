"""Box bounds per knot AND per instance on layout D (tinympc_set_bound_constraints_batch with a column per knot on a handle that called
tinympc_prepare, or shared per-knot bounds beside per-instance trajectories): the goal kernel with every wavefront's own clamp rows --
and, beside trajectories, its linref rows -- staged into its LDS region (IKBND, with or without ITRAJ, in tinympc_solve_d.hip). Every
instance still solves what a single-instance handle with its own bounds would -- against the oracle per instance, against the layout A
kernel over the whole batch, bit for bit against the shared per-knot form of layout D where the bounds coincide --, a handle moves
between layout A, the goal form, the trajectory form and this form with its ADMM state kept, and everything the form does not carry (a
horizon whose rows fit no wavefront's LDS share, wide systems, a switched-off specialiser, per-instance models or linear rows) stays
on layout A and stays correct.

Shapes, the smallest that reach every path: quadrotor N=20 x 773 in the default environment (773 > 768: layout D without a switch; one
wavefront per SIMD; the compiled-in kernel with trajectories, the run-time specialised one without; 193 full wavefronts + one
instance: a ragged last wavefront in a partial last workgroup), quadrotor N=10 x 37 under TINYMPC_LAYOUT=D (two wavefronts per SIMD, in
workgroups of four without and of eight with trajectories) and cartpole N=20 x 37 under TINYMPC_LAYOUT=D (nu = 1, KT = 8). Helpers, TOL,
SETTINGS and the sample are the sibling files'.

Seeds: the siblings' defaults (bounds seed 1, references seed 1, x0 seeds 0 / 1 / 2 per round). No sampled instance of any shape
terminates on a knife edge against the oracle with them."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
from conftest import rel_err

import test_instance_lin_gpu as LG
import test_instance_models_gpu as MG
from test_instance_bounds_gpu import _binds, _bounds, _DeviceArrays
from test_instance_bounds_gpu import _oracle as _oracle_b
from test_instance_knot_bounds_plan_cpu import first_fit, kbnd_plan
from test_instance_refs_gpu import SETTINGS, TOL, _check, _oracle, _refs, _sample, _wide, _x0s
from test_instance_traj_d_gpu import _each_instance_close, _handle, _same, _solve_all

pytestmark = pytest.mark.gpu

SHAPES = {  # name -> (problem, batch, TINYMPC_LAYOUT at setup)
    "quadrotor20": (lambda P: P.quadrotor(20), 773, None),
    "quadrotor10": (lambda P: P.quadrotor(10), 37, "D"),
    "cartpole20": (lambda P: P.cartpole(20, True), 37, "D"),
}


def _shape(pkg, shape):
    make, batch, layout = SHAPES[shape]
    return make(pkg.problems), batch, layout


def _on_d(s, traj, inst_bounds=True):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert " per-knot-bounds" in info and "(no plan)" not in info and "refused" not in info, info
    assert ("per-instance-bounds" in info) == inst_bounds and ("per-instance-trajectories" in info) == traj, info


def _on_a(s, word="per-instance-bounds"):
    assert s.launch_info()["layout"] == "A", (s.launch_info(), s.jit_info())
    assert word in s.jit_info(), s.jit_info()


def _plan_holds(s, prob, batch, traj):
    """The host's plan: the candidate and the bytes the restated arithmetic gives."""
    (wps, wpg), lds = first_fit(kbnd_plan(prob.nx, prob.nu, prob.N, itraj=traj))
    li = s.launch_info()
    assert li["lds_bytes"] == lds and li["workgroups"] == -(-((batch + 3) // 4) // wpg), (li, wps, wpg, lds)
    return wps, wpg


@pytest.mark.parametrize("refs", ["goal", "trajectory"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_instance_matches_the_oracle_and_layout_a(pkg, monkeypatch, shape, refs):
    """One prepared handle and one unprepared twin with the same per-knot bounds and references per instance: the sample against the
    oracle, EVERY instance against the twin; cold, then two warm starts. (On the parent commit the prepared handle stays on layout A:
    this test fails there.)"""
    prob, batch, layout = _shape(pkg, shape)
    traj = refs == "trajectory"
    d, a = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    d.prepare()
    (vx, vu), (X, U) = _refs(prob, batch, refs)
    verb, full = _bounds(prob, batch, "knot")
    for h in (d, a):
        h.set_x_ref_batch(vx)
        h.set_bound_constraints_batch(*verb)
        h.set_u_ref_batch(vu)
    orcs = {b: _oracle_b(prob, full, b, X[:, :, b], U[:, :, b]) for b in _sample(batch)}
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        _solve_all((d, a), x0s)
        _on_d(d, traj)
        _on_a(a)
        _check(d, orcs, x0s, (shape, refs, rnd))
        _each_instance_close(d, a, (shape, refs, rnd))
    info = d.jit_info()
    assert ("compiled-in" in info) == (shape == "quadrotor20" and traj), info
    assert "per-instance-refs" in info, info
    wps, wpg = _plan_holds(d, prob, batch, traj)
    assert (wps, wpg) == {"quadrotor20": (1, 4), "cartpole20": (1, 4), "quadrotor10": (2, 8) if traj else (2, 4)}[shape]
    d.reset()
    a.reset()


@pytest.mark.parametrize("refs", ["shared", "trajectory"])
def test_the_solve_ran_on_each_instances_own_bounds_of_each_knot(pkg, monkeypatch, refs):
    """The sampled instances' controls respect their own per-knot bounds, at least one touches its own bound at some knot, at least one
    would break another sampled instance's bound (_binds compares every knot), and a touched bound lies at a knot whose limit differs
    from the instance's knot-0 limit: the clamp rows are the knots' own."""
    prob, batch, layout = _shape(pkg, "quadrotor10")
    s = _handle(pkg, monkeypatch, prob, batch, layout)
    s.prepare()
    verb, full = _bounds(prob, batch, "knot")
    s.set_bound_constraints_batch(*verb)
    if refs == "trajectory":
        (vx, vu), _ = _refs(prob, batch, "trajectory")
        s.set_x_ref_batch(vx)
        s.set_u_ref_batch(vu)
    x0s = _x0s(prob, batch, seed=0)
    _solve_all((s,), x0s)
    _on_d(s, refs == "trajectory")
    samples = _sample(batch)
    _binds(s, full, samples, refs)
    u = s.get_solution_batch()["controls"]
    later = False
    for b in samples:
        for lim in (full[2][:, :, b], full[3][:, :, b]):
            hit = np.abs(u[:, :, b] - lim) < 1e-12
            later |= bool(np.any(hit[:, 1:] & (np.abs(lim[:, 1:] - lim[:, :1]) > 1e-3 * np.abs(lim[:, :1]))))
    assert later, refs
    s.reset()


@pytest.mark.parametrize("refs", ["constant", "trajectory"])
@pytest.mark.parametrize("shape", ["quadrotor10", "cartpole20"])
def test_equal_bounds_are_bit_identical_to_the_shared_per_knot_form_of_layout_d(pkg, monkeypatch, shape, refs):
    """Every instance given the shared per-knot bounds through the batch verb: solutions, iterations, status and the four residuals of
    the handle that sent them through set_bound_constraints, which runs layout D's shared per-knot form (the same sweeps reading the
    workgroup's table) -- with references constant over the horizon, and with the shared trajectory given to every instance."""
    prob, batch, layout = _shape(pkg, shape)
    _, full = _bounds(prob, 1, "knot", seed=5)
    prob.x_min, prob.x_max, prob.u_min, prob.u_max = (f[:, :, 0] for f in full)
    if refs == "trajectory":
        (_, _), (X, U) = _refs(prob, 1, "trajectory", seed=5)
        prob.x_ref, prob.u_ref = X[:, :, 0], U[:, :, 0]
    shared, inst = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    inst.prepare()
    inst.set_bound_constraints_batch(*(np.repeat(f, batch, axis=2) for f in full))
    if refs == "trajectory":
        inst.set_x_ref_batch(np.repeat(prob.x_ref[:, :, None], batch, axis=2))
        inst.set_u_ref_batch(np.repeat(prob.u_ref[:, :, None], batch, axis=2))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        _solve_all((shared, inst), x0s)
        _same(shared, inst, (shape, refs, rnd))
    _on_d(inst, refs == "trajectory")
    assert shared.launch_info()["layout"] == "D" and "per-instance" not in shared.jit_info(), shared.jit_info()
    shared.reset()
    inst.reset()


def test_partial_ranges_a_later_call_and_return_to_shared(pkg, monkeypatch):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 200
    s, shared = _handle(pkg, monkeypatch, prob, batch, "D"), _handle(pkg, monkeypatch, prob, batch, "D")
    s.prepare()
    (bl, bh, cl, ch), fb = _bounds(prob, batch, "box", seed=7)
    kn, fk = _bounds(prob, batch, "knot", seed=8)
    s.set_bound_constraints_batch(bl[:, 10:60], bh[:, 10:60], cl[:, 10:60], ch[:, 10:60], first=10)
    s.set_bound_constraints_batch(*(a[:, :, 100:130] for a in kn), first=100)
    s.set_bound_constraints_batch(bl[:, 55:57], bh[:, 55:57], cl[:, 55:57], ch[:, 55:57], first=55)  # overrides a part of the first range
    want = tuple(np.repeat(a[:, :, None], batch, axis=2) for a in prob.expanded_bounds())
    for w, a, k in zip(want, fb, fk):
        w[:, :, 10:60] = a[:, :, 10:60]
        w[:, :, 100:130] = k[:, :, 100:130]
    samples = [0, 9, 10, 30, 55, 56, 59, 60, 99, 100, 129, 130, 199]
    orcs = {b: _oracle_b(prob, want, b) for b in samples}
    x0s = _x0s(prob, batch)
    _solve_all((s, shared), x0s)
    _on_d(s, False)
    _check(s, orcs, x0s, "partial")
    # the instances no call named hold the shared bounds: what the shared handle computes
    for lo, hi in ((0, 10), (60, 100), (130, batch)):
        _each_instance_close(s, shared, "outside the ranges", lo, hi)
    # set_bound_constraints: every instance on the shared bounds, the handle on the shared plan again
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    assert "per-instance" not in s.jit_info() and "per-knot-bounds" not in s.jit_info() and s.launch_info() == shared.launch_info(), (s.jit_info(), s.launch_info())
    for h in (s, shared):
        h.reset_workspace()
    _solve_all((s, shared), x0s)
    _same(s, shared, "shared again")
    s.reset()
    shared.reset()


def test_shared_per_knot_bounds_with_per_instance_trajectories(pkg, monkeypatch):
    """The bounds vary over the horizon but not between instances; the references are a trajectory per instance: the form with ITRAJ, its
    clamp rows built from the shared bounds -- the compiled-in kernel -- against the oracle and the unprepared twin."""
    prob, batch, layout = _shape(pkg, "quadrotor20")
    batch = 37
    _, full = _bounds(prob, 1, "knot", seed=5)
    prob.x_min, prob.x_max, prob.u_min, prob.u_max = (f[:, :, 0] for f in full)
    d, a = _handle(pkg, monkeypatch, prob, batch, "D"), _handle(pkg, monkeypatch, prob, batch, "D")
    d.prepare()
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=3)
    for h in (d, a):
        h.set_x_ref_batch(vx)
        h.set_u_ref_batch(vu)
    orcs = {b: _oracle(prob, X[:, :, b], U[:, :, b]) for b in _sample(batch)}
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        _solve_all((d, a), x0s)
        _on_d(d, True, inst_bounds=False)
        _on_a(a, "per-instance-refs")
        _check(d, orcs, x0s, ("shared bounds", rnd))
        _each_instance_close(d, a, ("shared bounds", rnd))
    assert "compiled-in" in d.jit_info(), d.jit_info()
    _plan_holds(d, prob, batch, True)
    # new shared per-knot bounds reach the staged rows
    _, full2 = _bounds(prob, 1, "knot", seed=6)
    for h in (d, a):
        h.set_bound_constraints(*(f[:, :, 0] for f in full2))
    for orc in orcs.values():
        orc.set_bound_constraints(*(f[:, :, 0] for f in full2))
    x0s = _x0s(prob, batch, 0.5, seed=2)
    _solve_all((d, a), x0s)
    _on_d(d, True, inst_bounds=False)
    _check(d, orcs, x0s, "new shared bounds")
    _each_instance_close(d, a, "new shared bounds")
    d.reset()
    a.reset()


def test_switching_forms_keeps_the_admm_state(pkg, monkeypatch):
    """A box per instance (the goal form, D) -> bounds per knot (this form) -> trajectories added (this form with ITRAJ) -> a shared
    trajectory through set_x_ref (layout A) -> the per-instance trajectories again (this form with ITRAJ) -> boxes again (the
    trajectory form): one solve at each stage, every one a warm start of the last, against oracles that went the same way."""
    prob, batch = pkg.problems.quadrotor(20), 37
    s = _handle(pkg, monkeypatch, prob, batch, "D")
    s.prepare()
    box, full_box = _bounds(prob, batch, "box", seed=31)
    knots, full = _bounds(prob, batch, "knot", seed=33)
    (tx, tu), (Xt, Ut) = _refs(prob, batch, "trajectory", seed=32)
    (_, _), (Xs, _) = _refs(prob, 1, "trajectory", seed=34)
    samples = _sample(batch)
    orcs = {b: _oracle_b(prob, full_box, b) for b in samples}

    def stage(tag, layout_, words, scale, seed):
        x0s = _x0s(prob, batch, scale, seed=seed)
        s.set_x0_batch(x0s)
        s.solve()
        info = s.jit_info()
        assert s.launch_info()["layout"] == layout_ and all(w in info for w in words) and "refused" not in info, (tag, s.launch_info(), info)
        _check(s, orcs, x0s, tag)
        return info

    s.set_bound_constraints_batch(*box)
    stage("boxes", "D", ["goal", "per-instance-bounds"], 1.0, 0)
    s.set_bound_constraints_batch(*knots)
    for b, orc in orcs.items():
        orc.set_bound_constraints(*(f[:, :, b] for f in full))
    info = stage("bounds per knot", "D", [" per-knot-bounds", "per-instance-bounds"], 0.8, 1)
    assert "per-instance-trajectories" not in info and "compiled-in" not in info, info
    s.set_x_ref_batch(tx)
    s.set_u_ref_batch(tu)
    for b, orc in orcs.items():
        orc.set_x_ref(Xt[:, :, b])
        orc.set_u_ref(Ut[:, :, b])
    info = stage("trajectories added", "D", [" per-knot-bounds", "per-instance-trajectories", "compiled-in"], 0.7, 2)
    s.set_x_ref(Xs[:, :, 0])
    for orc in orcs.values():
        orc.set_x_ref(Xs[:, :, 0])
    info = stage("a shared trajectory", "A", ["per-instance-bounds", "per-instance-refs"], 0.6, 3)
    assert "per-knot-bounds" not in info, info
    s.set_x_ref_batch(tx)
    for b, orc in orcs.items():
        orc.set_x_ref(Xt[:, :, b])
    stage("back", "D", [" per-knot-bounds", "per-instance-trajectories"], 0.5, 4)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    for orc in orcs.values():
        orc.set_bound_constraints(*prob.expanded_bounds())
    info = stage("shared boxes", "D", ["per-instance-trajectories"], 0.4, 5)
    assert "per-knot-bounds" not in info, info
    s.reset()


@pytest.mark.parametrize("shape", ["quadrotor20", "cartpole20"])
def test_tracks_with_auto_advance_and_bounds_per_knot(pkg, monkeypatch, shape):
    """Both halves as tracks of T = N + 8 knots, auto-advance on, bounds per knot and instance: six closed-loop ticks on layout D, first
    controls within TOL of an unprepared twin's (layout A), equal steps and iterations, and the sixth tick's solution against an oracle
    fed the windows by hand."""
    prob, _, _ = _shape(pkg, shape)
    batch = 37
    N, T, ticks = prob.N, prob.N + 8, 6
    settings = dict(SETTINGS, max_iter=50)
    d, a = _handle(pkg, monkeypatch, prob, batch, "D", settings), _handle(pkg, monkeypatch, prob, batch, "D", settings)
    d.prepare()
    rng = np.random.default_rng(41)
    tt = np.arange(T)
    Xt = np.asfortranarray(0.3 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (prob.nx, 1, batch))))
    Ut = np.asfortranarray(0.03 * np.cos(0.2 * tt[None, :, None] + rng.uniform(0, 6, (prob.nu, 1, batch))))
    verb, full = _bounds(prob, batch, "knot", seed=42)
    for h in (d, a):
        h.set_x_ref_track_batch(Xt)
        h.set_u_ref_track_batch(Ut)
        h.set_ref_auto_advance(1)
        h.set_bound_constraints_batch(*verb)
    samples = _sample(batch)
    orcs = {b: _oracle_b(prob, full, b, settings=settings) for b in samples}
    x = _x0s(prob, batch)
    f = 0.0 if prob.fdyn is None else np.asarray(prob.fdyn, dtype=np.float64).reshape(prob.nx, 1)
    for k in range(ticks):
        ud, ua = d.mpc_step(x), a.mpc_step(x)
        info = d.jit_info()
        _on_d(d, True)
        assert "reference-track" in info and ("compiled-in" in info) == (shape == "quadrotor20"), (k, info)
        _on_a(a)
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


NOT_CARRIED = ["quadrotor34", "quadrotor23-trajectories", "quadrotor50", "wide32", "nojit", "models", "linear-rows"]


@pytest.mark.parametrize("name", NOT_CARRIED)
def test_what_the_form_does_not_carry_stays_on_layout_a_and_correct(pkg, monkeypatch, name):
    P = pkg.problems
    batch, M, rows, settings, x0l = 37, None, None, SETTINGS, None
    traj = name == "quadrotor23-trajectories"
    if name == "wide32":  # 32 lanes per instance
        prob = _wide(P, 24, 8, 20)
        s = _handle(pkg, monkeypatch, prob, batch, None)
    elif name == "nojit":  # the specialiser switched off, a shape whose box kernel is compiled in and whose per-knot bounds kernel is not
        monkeypatch.setenv("TINYMPC_JIT", "0")
        prob = P.cartpole(20, True)
        s = _handle(pkg, monkeypatch, prob, batch, "D")
    elif name == "linear-rows":  # per-instance linear rows: their form takes bounds constant over the horizon
        prob, nlx, nlu, _, settings = LG._case(pkg, "quadrotor-1+1")
        x0l, *rows = LG._rows(prob, nlx, nlu, batch)  # (the rows are placed relative to these initial states)
        s = _handle(pkg, monkeypatch, prob, batch, "D", settings)
        s.set_linear_constraints_batch(*rows)
    else:  # horizons without a plan (34 with constant references, 23 with trajectories, 50 with either), and per-instance models
        prob = P.quadrotor({"quadrotor34": 34, "quadrotor23-trajectories": 23, "quadrotor50": 50, "models": 10}[name])
        s = _handle(pkg, monkeypatch, prob, batch, "D")
        if name == "models":
            M = MG._models(prob, batch)
            MG._set_models(s, M)
    s.prepare()
    verb, full = _bounds(prob, batch, "knot", seed=51)
    s.set_bound_constraints_batch(*verb)
    X = U = None
    if traj:
        (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=52)
        s.set_x_ref_batch(vx)
        s.set_u_ref_batch(vu)
    orcs = {}
    for b in _sample(batch):
        pb = prob if M is None else M.problem(prob, b)
        pb = dataclasses.replace(pb, x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
        if rows is not None:
            orcs[b] = LG._oracle(pb, settings, LG._of(rows, b))
        else:
            orcs[b] = _oracle(pb, None if X is None else X[:, :, b], None if U is None else U[:, :, b], settings)
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd) if x0l is None else np.asfortranarray(x0l * (1.0 - 0.3 * rnd))
        s.set_x0_batch(x0s)
        s.solve()
        _on_a(s)
        _check(s, orcs, x0s, (name, rnd))
    info = s.jit_info()
    if name.startswith("quadrotor"):
        assert " per-knot-bounds(no plan)" in info and "refused" not in info, info
    else:
        assert "(no plan)" not in info, info
        assert ("refused(TINYMPC_JIT=0)" in info and " per-knot-bounds" in info) == (name == "nojit"), info
    s.reset()


def test_device_input_matches_host_input(pkg, monkeypatch):
    """tinympc_set_bound_constraints_batch_device with a column per knot: the solve of the same bounds from numpy, bit for bit, both on
    layout D."""
    prob, batch, layout = _shape(pkg, "quadrotor10")
    verb, _ = _bounds(prob, batch, "knot", seed=6)
    h, d = _handle(pkg, monkeypatch, prob, batch, layout), _handle(pkg, monkeypatch, prob, batch, layout)
    for q in (h, d):
        q.prepare()
    L = pkg.load_library()
    dev = _DeviceArrays(pkg)
    h.set_bound_constraints_batch(*verb)
    assert L.tinympc_set_bound_constraints_batch_device(d._h, *(dev.put(a) for a in verb), prob.N, 0, batch) == 0, pkg._lib.last_error()
    dev.free()
    x0s = _x0s(prob, batch)
    _solve_all((h, d), x0s)
    _on_d(h, False)
    _on_d(d, False)
    _same(h, d, "device input")
    for q in (h, d):
        q.reset()

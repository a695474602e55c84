"""Per-instance linear rows on layout D (tinympc_set_linear_constraints_batch on a handle that called tinympc_prepare): the families'
kernel reading every lane's own instance's rows from its wavefront's LDS region (ILIN in tinympc_solve_d.hip), in the goal form. Every
instance still solves what a single-instance handle with its own rows would -- against the plain-C oracle per sampled instance, bit for
bit against a shared-row handle on layout D where the rows coincide, across the host and device forms of the verb, sub-range updates
between warm ticks, per-instance goals and boxes, and switches between layouts A and D on one handle --, and everything the form does
not carry (no prepare(), trajectories, a row count without a plan) stays on layout A and stays correct.

Shapes, the smallest that reach every path, all under TINYMPC_LAYOUT=D (layout D at any batch size): quadrotor N=20 with 1+1 rows x 37
(the compiled-in kernel; nine full wavefronts and one with a single instance), cartpole N=20 with 2+1 rows x 21 (the generic row loop,
run-time specialised), rocket N=10 with shared cones and fdyn and one state row x 21 (the fused cone + one-row block, run-time
specialised; its reference held constant over the horizon, see _rocket), and a batch of 3 (one partial wavefront). Recipes, seed, tolerance and oracle helpers are the sibling file's
(test_instance_lin_gpu.py); seed 7 meets its sample conditions on the oracle alone, asserted again here."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
from conftest import rel_err

from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs
from test_instance_lin_gpu import (CONV, SEED, _assert_matches, _assert_same_bits, _case, _of, _oracle, _reference, _rows, _run, _sample,
                                   _solver)

pytestmark = pytest.mark.gpu


def _d_solver(pkg, monkeypatch, prob, batch, settings):
    """A handle that runs layout D whatever its batch size (the switch stays set: a shared-row handle then keeps layout D's families
    kernel at every launch too)."""
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")
    return _solver(pkg, prob, batch, settings)


def _on_d(s):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert "per-instance-linear" in info and "refused" not in info, info


def _on_a(s):
    assert s.launch_info()["layout"] == "A", (s.launch_info(), s.jit_info())
    assert "per-instance-linear" in s.jit_info(), s.jit_info()


def _rocket(pkg, batch=21):
    """problems.rocket(10) with the sibling file's "binding" offsets: shared cones and fdyn, the ground-plane row with every instance's
    own b -- two instances in three get the plane 0 to 2.3 m below their start, which the descent reaches.

    One thing differs from the sibling's case: problems.rocket() follows a reference TRAJECTORY (the straight line from the start to the
    pad), and a trajectory is what keeps a handle on layout A; layout D's form takes references that are constant over the horizon. The
    reference is therefore held at the trajectory's first column (over ten knots the line moves a tenth of the way). Shape, cones, fdyn,
    rows, offsets, batch, seed and tolerance are the sibling's; on the oracle alone seed 7 still meets the sample conditions with it
    (iterations 27 / 300 / 300 / 300 / 300, three of five move by more than 1e-3 against no rows, all five against the neighbour's b)."""
    prob = pkg.problems.rocket(10)
    prob = dataclasses.replace(prob, x_ref=np.repeat(prob.x_ref[:, :1], prob.N, axis=1))
    rng = np.random.default_rng(SEED)
    x0s = np.asfortranarray(prob.x0[:, None] + 0.1 * rng.standard_normal((prob.nx, batch)))
    Ax = np.repeat(np.asarray(prob.linear["Alin_x"])[:, :, None], batch, axis=2)
    ax0 = np.einsum("kcb,cb->kb", Ax, x0s)
    factor = rng.uniform(0.5, 2.0, (1, batch))
    factor = np.where(np.arange(batch)[None, :] % 3 != 0, rng.uniform(0.0, 0.1, (1, batch)), factor)
    bx = ax0 + factor * (1.0 + np.abs(ax0))
    return prob, x0s, (Ax, bx, np.zeros((0, prob.nu, batch)), np.zeros((0, batch)))


# ---- 1. parity with the oracle per sampled instance, after the verb + prepare()

@pytest.mark.parametrize("name", ["quadrotor-1+1", "cartpole-2+1", "rocket-binding"])
def test_each_instance_matches_the_oracle_on_layout_d(pkg, monkeypatch, name):
    if name == "rocket-binding":
        batch, settings = 21, CONV
        prob, x0s, rows = _rocket(pkg, batch)
        samples = _sample(batch)
        own = {b: _run(_oracle(prob, settings, _of(rows, b)), x0s[:, b]) for b in samples}
        free = {b: _run(_oracle(prob, settings), x0s[:, b]) for b in samples}
        other = {b: _run(_oracle(prob, settings, _of(rows, samples[(i + 1) % len(samples)])), x0s[:, b]) for i, b in enumerate(samples)}
        converged_min = 1
    else:
        prob, nlx, nlu, batch, settings = _case(pkg, name)
        x0s, *rows = _rows(prob, nlx, nlu, batch)
        own, free, other = _reference(pkg, name)
        converged_min = 2
    # the oracle alone: the sample is neither all converged nor all stuck, and the rows matter per instance -- a kernel that read another
    # lane row's or another wavefront's rows fails the parity below
    its = [own[b][2] for b in own]
    moved = [rel_err(own[b][1], free[b][1]) > 1e-3 for b in own]
    differ = [rel_err(own[b][1], other[b][1]) > 1e-3 for b in own]
    print(name, "oracle iterations", its, "moved", moved, "differ", differ)
    assert sum(i < settings["max_iter"] for i in its) >= converged_min and sum(i >= settings["max_iter"] for i in its) >= 1
    assert 2 * sum(moved) >= len(moved) and 2 * sum(differ) >= len(differ)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    _on_a(s)  # (without prepare(): the parent's kernel)
    s.prepare()
    _on_d(s)
    # (the quadrotor's kernel is found by the options of its plan: a plan that moved would leave it to the run-time compiler)
    assert ("compiled-in" in s.jit_info()) == (name == "quadrotor-1+1"), s.jit_info()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    _assert_matches(s, own, name + " on D")
    s.reset()


# ---- 2. identical rows on every instance == the shared rows of a twin on layout D, bit for bit, cold and over two warm ticks

@pytest.mark.parametrize("name", ["quadrotor-1+1", "rocket-binding"])
def test_identical_rows_are_the_shared_rows_on_layout_d_bit_for_bit(pkg, monkeypatch, name):
    if name == "rocket-binding":
        batch, settings = 21, CONV
        prob, x0s, rows = _rocket(pkg, batch)
    else:
        prob, nlx, nlu, batch, settings = _case(pkg, name)
        x0s, *rows = _rows(prob, nlx, nlu, batch)
    one = _of(rows, batch - 1)
    inst, twin = _d_solver(pkg, monkeypatch, prob, batch, settings), _d_solver(pkg, monkeypatch, prob, batch, settings)
    twin.set_linear_constraints(*one)
    inst.prepare()  # (before the verb: either order)
    inst.set_linear_constraints_batch(*(np.repeat(a[..., None], batch, axis=-1) for a in one))
    for rnd in range(3):
        for h in (twin, inst):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        _assert_same_bits(twin, inst)  # states, controls, iterations, status, the four residuals
    _on_d(inst)
    assert twin.launch_info()["layout"] == "D" and "per-instance-linear" not in twin.jit_info(), twin.jit_info()
    twin.reset()
    inst.reset()


# ---- 3. the _device form is the host form on layout D, bit for bit

def test_device_form_is_the_host_form_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, Ax, bx, Au, bu = _rows(prob, nlx, nlu, batch)
    host, devh = _d_solver(pkg, monkeypatch, prob, batch, settings), _d_solver(pkg, monkeypatch, prob, batch, settings)
    host.set_linear_constraints_batch(Ax, bx, Au, bu)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    assert L.tinympc_set_linear_constraints_batch_device(devh._h, dev.put(Ax), dev.put(bx), nlx, dev.put(Au), dev.put(bu), nlu, 0, batch) == 0
    dev.free()  # (the input has been copied when the verb returns)
    # (the C verb switched both sides on; the Python object mirrors the settings and pushes its copy in prepare(): told here, as its own
    # method does after the call)
    devh.settings["en_state_linear"] = devh.settings["en_input_linear"] = True
    for h in (host, devh):
        h.prepare()
        h.set_x0_batch(x0s)
        h.solve()
        _on_d(h)
    _assert_same_bits(host, devh)
    host.reset()
    devh.reset()


# ---- 4. between two warm ticks the rows of a sub-range that straddles a wavefront boundary are re-sent

def test_a_sub_range_update_between_warm_ticks(pkg, monkeypatch):
    prob, nlx, nlu, batch, _ = _case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    _, *rows2 = _rows(prob, nlx, nlu, batch, seed=SEED + 1)
    lo, hi = 2, 7  # (instances 0-3 are the first wavefront, 4-7 the second)
    s, ref = _d_solver(pkg, monkeypatch, prob, batch, settings), _d_solver(pkg, monkeypatch, prob, batch, settings)
    orcs = {b: _oracle(prob, settings, _of(rows, b)) for b in range(lo, hi)}
    for h in (s, ref):
        h.set_linear_constraints_batch(*rows)
        h.prepare()
    for tick in range(3):
        x = x0s * (1.0 - 0.2 * tick)
        if tick == 2:  # between the two warm ticks
            s.set_linear_constraints_batch(*(a[..., lo:hi] for a in rows2), first=lo)
            for b, orc in orcs.items():
                orc.set_linear_constraints(*_of(rows2, b))  # (keeps the workspace, the linear family's duals included)
                orc.update_settings()
        for h in (s, ref):
            h.set_x0_batch(x)
            h.solve()
            _on_d(h)
        expect = {b: _run(orc, x[:, b]) for b, orc in orcs.items()}
        _assert_matches(s, expect, ("sub-range tick", tick))
    outside = [b for b in range(batch) if not lo <= b < hi]
    a, r = s.get_solution_batch(), ref.get_solution_batch()
    np.testing.assert_array_equal(a["states"][:, :, outside], r["states"][:, :, outside])
    np.testing.assert_array_equal(a["controls"][:, :, outside], r["controls"][:, :, outside])
    ta, tr = s.get_stats_batch(), ref.get_stats_batch()
    for k in ta:
        np.testing.assert_array_equal(np.asarray(ta[k])[..., outside], np.asarray(tr[k])[..., outside])  # (the instance is the last axis)
    assert rel_err(a["controls"][:, :, lo:hi], r["controls"][:, :, lo:hi]) > 1e-6  # (the new rows act)
    s.reset()
    ref.reset()


# ---- 5. per-instance goals and boxes inside the mode

def test_per_instance_goals_and_boxes_inside_the_mode_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    verb, (X, U) = _refs(prob, batch, "goal")
    s.set_x_ref_batch(verb[0])  # one column per instance
    s.set_u_ref_batch(verb[1])
    bverb, full = _bounds(prob, batch, "box")
    s.set_bound_constraints_batch(*bverb)  # cols = 1
    s.prepare()
    s.set_x0_batch(x0s)
    s.solve()
    expect = {}
    for b in _sample(batch):
        pb = dataclasses.replace(prob, x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
        orc = _oracle(pb, settings, _of(rows, b))
        orc.set_x_ref(X[:, :, b])
        orc.set_u_ref(U[:, :, b])
        expect[b] = _run(orc, x0s[:, b])
    _assert_matches(s, expect, "goals+box on D")
    _on_d(s)
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info, info
    s.reset()


# ---- 6. one handle moves between the layouts; the ADMM state, the families' duals included, is shared

def test_switching_between_layouts_keeps_a_valid_warm_start(pkg, monkeypatch):
    prob, nlx, nlu, batch, _ = _case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, Ax, bx, Au, bu = _rows(prob, nlx, nlu, batch)
    samples = _sample(batch)
    N = prob.N
    rng = np.random.default_rng(3)
    goal = 0.3 * rng.standard_normal(prob.nx)
    traj = goal[:, None] * np.linspace(0.2, 1.0, N)[None, :]
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(Ax, bx, Au, bu)
    s.prepare()
    orcs = {b: _oracle(prob, settings, _of((Ax, bx, Au, bu), b)) for b in samples}
    off = samples[2]
    layouts = ["D", "D", "A", "D", "D"]  # a cold solve, then the four warm ticks
    for tick, layout in enumerate(layouts):
        if tick == 2:  # a trajectory reference arrives: layout A
            s.set_x_ref(traj)
            for orc in orcs.values():
                orc.set_x_ref(traj)
        if tick == 3:  # the goals come back: layout D
            s.set_x_ref(np.repeat(goal[:, None], N, axis=1))
            for orc in orcs.values():
                orc.set_x_ref(np.repeat(goal[:, None], N, axis=1))
        if tick == 4:  # b = +inf for one instance: both of its rows are off
            s.set_linear_constraints_batch(Ax[:, :, off:off + 1], np.full((nlx, 1), np.inf), Au[:, :, off:off + 1], np.full((nlu, 1), np.inf), first=off)
            orcs[off].set_linear_constraints(Ax[:, :, off], np.full(nlx, np.inf), Au[:, :, off], np.full(nlu, np.inf))
            orcs[off].update_settings()
        x = x0s * (1.0 - 0.15 * tick)
        s.set_x0_batch(x)
        s.solve()
        assert s.launch_info()["layout"] == layout, (tick, s.launch_info(), s.jit_info())
        assert "per-instance-linear" in s.jit_info()
        _assert_matches(s, {b: _run(orcs[b], x[:, b]) for b in samples}, ("switch tick", tick, layout))
    s.reset()


# ---- 7. fallbacks and refusals

def test_without_prepare_the_mode_stays_on_layout_a(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    d = _d_solver(pkg, monkeypatch, prob, batch, settings)  # layout D is the handle's, prepare() is not called
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    a = _solver(pkg, prob, batch, settings)
    for h in (d, a):
        h.set_linear_constraints_batch(*rows)
        for rnd in range(2):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        _on_a(h)
    _assert_same_bits(a, d)
    d.reset()
    a.reset()


def test_a_row_count_without_a_plan_is_refused_and_runs_on_layout_a(pkg, monkeypatch):
    prob, _, _, batch, _ = _case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=30, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, *rows = _rows(prob, 32, 1, batch)  # 3 x 32 vectors of 64 doubles per wavefront: beyond its LDS share
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    s.prepare()
    info = s.jit_info()
    assert "refused(" in info and "per-instance-linear" in info, info
    _on_a(s)
    s.set_x0_batch(x0s)
    s.solve()
    b = batch // 2
    _assert_matches(s, {b: _run(_oracle(prob, settings, _of(rows, b)), x0s[:, b])}, "32 rows")
    # ... and a whole-batch call with a count the form holds is asked again
    x0s, *rows = _rows(prob, 1, 1, batch)
    s.set_linear_constraints_batch(*rows)
    s.reset_workspace()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    s.reset()


def test_models_stay_refused_and_the_enable_flags_are_honoured_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    s.prepare()
    s.set_x0_batch(x0s)
    s.set_model_batch(*(np.repeat(m[:, :, None], batch, axis=2) for m in (prob.A, prob.B, prob.Q, prob.R)))
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED and "set_linear_constraints_batch" in str(ei.value), ei.value
    s.clear_model_batch()
    s.update_settings(en_state_linear=False)
    s.solve()
    _on_d(s)
    _assert_matches(s, {b: _run(_oracle(prob, settings, _of(rows, b), en_state_linear=0), x0s[:, b]) for b in _sample(batch)}, "flag off on D")
    s.reset()


def test_one_partial_wavefront(pkg, monkeypatch):
    prob, nlx, nlu, _, settings = _case(pkg, "quadrotor-1+1")
    batch = 3
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    s.prepare()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    _assert_matches(s, {b: _run(_oracle(prob, settings, _of(rows, b)), x0s[:, b]) for b in range(batch)}, "batch of 3")
    s.reset()

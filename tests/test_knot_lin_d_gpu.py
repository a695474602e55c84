"""Per-knot linear rows on layout D (tinympc_set_linear_constraints_knots_batch on a handle that called tinympc_prepare): the per-knot
variant of the families' ILIN form in tinympc_solve_d.hip -- every wavefront stages its group's N slots of rows into its own LDS region
and a step reads the slot of its knot. Every instance still solves the problem whose linear slack at knot i is the projection onto knot
i's OWN rows: checked per sampled instance against the stepped oracle of tests/knot_lin_cases.py (seed 7, TOL = 1e-9 on states and
controls, iterations and status exact), bit for bit against a twin on the constant-row form where the rows repeat over the knots, across
the host and device forms of the verb, warm ticks with shifted rows, sub-range updates, rows switched off at single knots, per-instance
goals and boxes, switches between layouts A and D and between the two forms on one handle; what the plan does not hold is refused and
stays on layout A, and stays correct.

Every handle runs under TINYMPC_LAYOUT=D (layout D at any batch size). Cases, the smallest that reach each path -- their sample
conditions (K.assert_sample_conditions) hold on the oracle alone and are asserted again before the GPU is asked:
  quadrotor-1+1     quadrotor(20), 1+1 rows x 37   the compiled-in kernel, the fused one-row block; nine full wavefronts and one with
                                                   a single instance
  quadrotor20-1+0   quadrotor(20), 1+0 rows x 37   state rows only (the moving-obstacle example's shape): the input side is absent
  cartpole10-2+1    cartpole(10), 2+1 rows x 21    the generic row loop, unequal sides, lanes beyond the system's rows; specialised at run time
  quadrotor8-3+2    quadrotor(8), 3+2 rows x 21    three rows at the edge of the LDS plan, 4,608 + 112 of 4,992 doubles; max_iter = 100
                                                   (with K.CONV all five sampled instances converge, in 45 to 118 iterations)"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest
from conftest import rel_err

import knot_lin_cases as K
from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs
from test_instance_lin_d_gpu import _d_solver, _rocket
from test_instance_lin_gpu import _assert_matches, _assert_same_bits, _of, _oracle, _rows, _run, _solver

pytestmark = pytest.mark.gpu

CAP100 = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
CASES = {  # name -> (problem, state rows, input rows, batch, settings)
    "quadrotor-1+1": K.CASES["quadrotor-1+1"],
    "quadrotor20-1+0": (lambda P: P.quadrotor(20), 1, 0, 37, K.CONV),
    "cartpole10-2+1": (lambda P: P.cartpole(10, True), 2, 1, 21, K.CONV),
    "quadrotor8-3+2": (lambda P: P.quadrotor(8), 3, 2, 21, CAP100),
}


def _case(pkg, name):
    make, nlx, nlu, batch, settings = CASES[name]
    return make(pkg.problems), nlx, nlu, batch, settings


@functools.lru_cache(maxsize=None)
def _reference(pkg, name):
    """(own, held0) of K.reference for this file's cases: computed once per case, shared, never modified."""
    if name in K.CASES:
        return K.reference(pkg, name)
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    own, held0 = {}, {}
    for b in K.sample(batch):
        rb = K.of(rows, b)
        own[b] = K.SteppedOracle(prob, settings, rb).solve(x0s[:, b], rb)
        held0[b] = K.whole_solve(prob, settings, x0s[:, b], (rb[0][:, :, 0], rb[1][:, 0], rb[2][:, :, 0], rb[3][:, 0]))
    return own, held0


def _stepped(prob, settings, rows, x0s, samples, **flags):
    """The stepped oracle's cold solve of the given instances under their own rows."""
    return {b: K.SteppedOracle(prob, settings, K.of(rows, b), **flags).solve(x0s[:, b], K.of(rows, b)) for b in samples}


def _on_d(s):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert "per-knot-linear" in info and "refused" not in info, info


def _on_a(s):
    assert s.launch_info()["layout"] == "A", (s.launch_info(), s.jit_info())
    assert "per-knot-linear" in s.jit_info(), s.jit_info()


# ---- 1. parity with the stepped oracle per sampled instance, after the verb + prepare()

@pytest.mark.parametrize("name", list(CASES))
def test_each_instance_matches_the_stepped_oracle_on_layout_d(pkg, monkeypatch, name):
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    own, held0 = _reference(pkg, name)
    print(name, "oracle iterations", [own[b][2] for b in own])
    K.assert_sample_conditions(name, own, held0, settings["max_iter"])
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    _on_a(s)  # (without prepare(): layout A's per-knot kernel)
    s.prepare()
    _on_d(s)
    # (the quadrotor's kernel is found by the options of its plan: a plan that moved would leave it to the run-time compiler. The form is
    # specialised on the larger of the two sides' counts, so quadrotor(20) with 1+0 rows is the same compiled-in kernel as with 1+1;
    # the other shapes are specialised at run time)
    assert ("compiled-in" in s.jit_info()) == (name in ("quadrotor-1+1", "quadrotor20-1+0")), s.jit_info()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    _assert_matches(s, own, name + " on D")
    s.reset()


# ---- 2. rows repeated over the knots == the constant rows of a twin on layout D's ILIN form, bit for bit, cold and over two warm ticks

@pytest.mark.parametrize("name", ["quadrotor-1+1", "rocket", "rocket-slopes"])
def test_repeated_rows_are_the_constant_rows_on_layout_d_bit_for_bit(pkg, monkeypatch, name):
    if name == "quadrotor-1+1":
        prob, nlx, nlu, batch, settings = _case(pkg, name)
        x0s, *const = _rows(prob, nlx, nlu, batch)  # (per instance, constant over the horizon)
    else:  # shared cones and fdyn: the fused cone + one-row block, every instance's own b
        batch, settings = 21, K.CONV
        prob, x0s, const = _rocket(pkg, batch)
    twin, knots = _d_solver(pkg, monkeypatch, prob, batch, settings), _d_solver(pkg, monkeypatch, prob, batch, settings)
    if name == "rocket-slopes":  # ... and every instance's own glide and thrust cone on both handles (ICONE)
        rng = np.random.default_rng(K.SEED)
        cx = np.repeat(np.asarray(prob.cones["cx"], dtype=float)[:, None], batch, axis=1) * rng.uniform(0.7, 1.3, (len(prob.cones["cx"]), batch))
        cu = np.repeat(np.asarray(prob.cones["cu"], dtype=float)[:, None], batch, axis=1) * rng.uniform(0.7, 1.3, (len(prob.cones["cu"]), batch))
        for h in (twin, knots):
            h.set_cone_slopes_batch(cx, cu)
    twin.set_linear_constraints_batch(*const)
    knots.prepare()  # (before the verb: either order)
    knots.set_linear_constraints_knots_batch(*K.repeat_over_knots(const, prob.N))
    twin.prepare()
    for rnd in range(3):
        for h in (twin, knots):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        _assert_same_bits(twin, knots)  # states, controls, iterations, status, the four residuals
    _on_d(knots)
    info = twin.jit_info()
    assert twin.launch_info()["layout"] == "D" and "per-instance-linear" in info and "per-knot-linear" not in info and "refused" not in info, info
    assert ("per-instance-cones" in knots.jit_info()) == ("per-instance-cones" in info) == (name == "rocket-slopes"), (knots.jit_info(), info)
    twin.reset()
    knots.reset()


# ---- 3. the _device form is the host form on layout D, bit for bit

def test_device_form_is_the_host_form_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, Ax, bx, Au, bu = K.rows_knots(prob, nlx, nlu, batch)
    host, devh = _d_solver(pkg, monkeypatch, prob, batch, settings), _d_solver(pkg, monkeypatch, prob, batch, settings)
    host.set_linear_constraints_knots_batch(Ax, bx, Au, bu)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    assert L.tinympc_set_linear_constraints_knots_batch_device(devh._h, dev.put(Ax), dev.put(bx), nlx, dev.put(Au), dev.put(bu), nlu, 0, batch) == 0
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


# ---- 4. warm ticks: the rows shifted by one knot and re-sent before every tick, the duals kept (test 9 of test_knot_lin_gpu.py on layout D)

def test_rows_shifted_every_tick_keep_the_duals_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, _ = _case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    samples = K.sample(batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.prepare()
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    orcs = {b: K.SteppedOracle(prob, settings, K.of(rows, b)) for b in samples}
    for tick in range(4):
        # the horizon recedes: knot i takes what knot i+1 had, the last knot keeps its rows
        Ax, bx, Au, bu = (np.concatenate([a[..., tick:, :]] + [a[..., -1:, :]] * tick, axis=-2) for a in rows)
        if tick % 2:  # the host form and the _device form in turns
            assert L.tinympc_set_linear_constraints_knots_batch_device(s._h, dev.put(Ax), dev.put(bx), nlx, dev.put(Au), dev.put(bu), nlu, 0, batch) == 0
            dev.free()
        else:
            s.set_linear_constraints_knots_batch(Ax, bx, Au, bu)
        x0t = x0s * (1.0 - 0.1 * tick)
        s.mpc_step(x0t)
        _on_d(s)
        expect = {b: orcs[b].solve(x0t[:, b], K.of((Ax, bx, Au, bu), b)) for b in samples}  # (the oracle object keeps its workspace)
        _assert_matches(s, expect, ("tick on D", tick))
    s.reset()


# ---- 5. between two warm ticks the rows of a sub-range that straddles a wavefront boundary are re-sent

def test_a_sub_range_update_between_warm_ticks_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, _ = _case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    _, *rows2 = K.rows_knots(prob, nlx, nlu, batch, seed=K.SEED + 1)
    lo, hi = 2, 7  # instances 2..6 (instances 0-3 are the first wavefront, 4-7 the second)
    s, ref = _d_solver(pkg, monkeypatch, prob, batch, settings), _d_solver(pkg, monkeypatch, prob, batch, settings)
    orcs = {b: K.SteppedOracle(prob, settings, K.of(rows, b)) for b in range(lo, hi)}
    for h in (s, ref):
        h.set_linear_constraints_knots_batch(*rows)
        h.prepare()
    now = rows
    for tick in range(3):
        x = x0s * (1.0 - 0.2 * tick)
        if tick == 2:  # between the two warm ticks
            s.set_linear_constraints_knots_batch(*(a[..., lo:hi] for a in rows2), first=lo)
            now = rows2
        for h in (s, ref):
            h.set_x0_batch(x)
            h.solve()
            _on_d(h)
        expect = {b: orc.solve(x[:, b], K.of(now, b)) for b, orc in orcs.items()}  # (the oracle object keeps its workspace)
        _assert_matches(s, expect, ("sub-range tick on D", tick))
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


# ---- 6. b = +inf switches one row off at one knot: knot 0, an interior knot and the last knot of each side, one instance per wavefront

def test_infinite_b_switches_a_row_off_at_single_knots_on_layout_d(pkg, monkeypatch):
    """The interior knot is, per instance and side, the one where the oracle's solution under the full rows presses hardest against its
    row (the largest a'x - b over the knots inside the horizon), so that switching it off moves the solution: on the oracle alone eight of
    the ten instances move their controls by 3e-6 to 0.57 (relative), far above TOL -- a kernel that read another knot's b fails."""
    name = "quadrotor-1+1"
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, Ax, bx, Au, bu = K.rows_knots(prob, nlx, nlu, batch)
    N = prob.N
    picks = [0, 5, 10, 15, 18, 21, 26, 31, 32, 36]  # one instance of every wavefront, on every 16-lane row of one
    assert sorted(b // 4 for b in picks) == list(range((batch + 3) // 4)) and {b % 4 for b in picks} == {0, 1, 2, 3}
    full = _stepped(prob, settings, (Ax, bx, Au, bu), x0s, picks)
    bx, bu = bx.copy(), bu.copy()
    for b in picks:
        X, U = full[b][0], full[b][1]
        kx = 1 + int(np.argmax((np.einsum("cn,cn->n", Ax[0, :, :, b], X) - bx[0, :, b])[1:N - 1]))
        ku = 1 + int(np.argmax((np.einsum("cn,cn->n", Au[0, :, :, b], U) - bu[0, :, b])[1:N - 2]))
        for knot in (0, kx, N - 1):  # slot 0 (the call in front of the sweep), a step inside the sweep, the last step's slot
            bx[0, knot, b] = np.inf
        for knot in (0, ku, N - 2):  # slot 1 (forward step 0's input lanes), inside, the last step's slot
            bu[0, knot, b] = np.inf
    rows = (Ax, bx, Au, bu)
    expect = _stepped(prob, settings, rows, x0s, picks)
    moved = [rel_err(expect[b][1], full[b][1]) for b in picks]
    print("rows off at knots: moved against the full rows", moved)
    assert 2 * sum(m > 1e-6 for m in moved) >= len(moved)  # (the switched-off rows mattered)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.prepare()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    _assert_matches(s, expect, "rows off at knots on D")
    s.reset()


# ---- 7. per-instance goals and boxes inside the mode

def test_per_instance_goals_and_boxes_inside_the_mode_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    verb, (X, U) = _refs(prob, batch, "goal")
    s.set_x_ref_batch(verb[0])  # one column per instance
    s.set_u_ref_batch(verb[1])
    bverb, full = _bounds(prob, batch, "box")
    s.set_bound_constraints_batch(*bverb)  # cols = 1
    s.prepare()
    s.set_x0_batch(x0s)
    s.solve()
    expect = {}
    for b in K.sample(batch):
        pb = dataclasses.replace(prob, x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
        orc = K.SteppedOracle(pb, settings, K.of(rows, b))
        orc.orc.set_x_ref(X[:, :, b])
        orc.orc.set_u_ref(U[:, :, b])
        expect[b] = orc.solve(x0s[:, b], K.of(rows, b))
    _assert_matches(s, expect, "goals+box on D")
    _on_d(s)
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info, info
    s.reset()


# ---- 8. one handle moves between the layouts; the ADMM state, the rows' duals included, is shared

def test_switching_between_layouts_keeps_a_valid_warm_start(pkg, monkeypatch):
    prob, nlx, nlu, batch, _ = _case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    samples = K.sample(batch)
    N = prob.N
    rng = np.random.default_rng(3)
    goal = 0.3 * rng.standard_normal(prob.nx)
    traj = goal[:, None] * np.linspace(0.2, 1.0, N)[None, :]
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.prepare()
    orcs = {b: K.SteppedOracle(prob, settings, K.of(rows, b)) for b in samples}
    layouts = ["D", "D", "A", "D", "D"]  # a cold solve, then the four warm ticks
    for tick, layout in enumerate(layouts):
        if tick == 2:  # a trajectory reference arrives: layout A's per-knot kernel
            s.set_x_ref(traj)
            for o in orcs.values():
                o.orc.set_x_ref(traj)
        if tick == 3:  # a goal returns: layout D
            s.set_x_ref(np.repeat(goal[:, None], N, axis=1))
            for o in orcs.values():
                o.orc.set_x_ref(np.repeat(goal[:, None], N, axis=1))
        x = x0s * (1.0 - 0.15 * tick)
        s.set_x0_batch(x)
        s.solve()
        assert s.launch_info()["layout"] == layout, (tick, s.launch_info(), s.jit_info())
        assert "per-knot-linear" in s.jit_info() and (layout == "A" or "refused" not in s.jit_info()), s.jit_info()
        _assert_matches(s, {b: orcs[b].solve(x[:, b], K.of(rows, b)) for b in samples}, ("switch tick", tick, layout))
    s.reset()


# ---- 9. leaving the per-knot form for rows constant over the horizon, and re-entering it, on one prepared handle

def test_leaving_and_re_entering_the_mode_on_one_prepared_handle(pkg, monkeypatch):
    name = "quadrotor-1+1"
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    _, *const = _rows(prob, nlx, nlu, batch)
    samples = K.sample(batch)
    own, _ = _reference(pkg, name)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.prepare()
    for rnd in range(2):
        s.set_linear_constraints_knots_batch(*rows)  # rows per knot: the per-knot form
        s.reset_workspace()
        s.set_x0_batch(x0s)
        s.solve()
        _on_d(s)
        _assert_matches(s, own, ("per knot", rnd))
        if rnd:
            break
        s.set_linear_constraints_batch(*const)  # a whole-batch call of the constant verb: the ILIN form
        s.reset_workspace()
        s.set_x0_batch(x0s)
        s.solve()
        info = s.jit_info()
        assert s.launch_info()["layout"] == "D" and "per-instance-linear" in info and "per-knot-linear" not in info and "refused" not in info, info
        _assert_matches(s, {b: _run(_oracle(prob, settings, _of(const, b)), x0s[:, b]) for b in samples}, "constant rows in between")
    s.reset()


# ---- 10. a plan that does not fit

def test_a_plan_that_does_not_fit_is_refused_and_runs_on_layout_a(pkg, monkeypatch):
    name = "cartpole-2+1"  # of K.CASES: N = 20, two rows -- 3 x 2 x 20 x 64 = 7,680 doubles per wavefront, beyond its 4,992
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    own, _ = K.reference(pkg, name)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.prepare()
    info = s.jit_info()
    assert "refused(" in info and "per-knot-linear" in info, info
    _on_a(s)
    s.set_x0_batch(x0s)
    s.solve()
    _on_a(s)
    _assert_matches(s, own, name + " refused, on A")
    # ... and a whole-batch call with a count the plan holds is asked again: one row per side, 3,840 + 76 doubles
    x0s, *rows = K.rows_knots(prob, 1, 1, batch)
    s.set_linear_constraints_knots_batch(*rows)
    s.reset_workspace()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    b = batch // 2
    _assert_matches(s, _stepped(prob, settings, rows, x0s, [b]), "one row per side, on D")
    s.reset()


# ---- 11. fallbacks and refusals

def test_without_prepare_layout_a_and_with_it_refusals_and_enable_flags_on_layout_d(pkg, monkeypatch):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    d = _d_solver(pkg, monkeypatch, prob, batch, settings)  # layout D is the handle's, prepare() is not called
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    a = _solver(pkg, prob, batch, settings)
    for h in (d, a):
        h.set_linear_constraints_knots_batch(*rows)
        for rnd in range(2):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        _on_a(h)
        assert "refused" not in h.jit_info(), h.jit_info()
    _assert_same_bits(a, d)
    d.reset()
    a.reset()
    # ... with prepare(): models stay refused, by the verb's name, and the enable flags are honoured on layout D
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.prepare()
    s.set_x0_batch(x0s)
    s.set_model_batch(*(np.repeat(m[:, :, None], batch, axis=2) for m in (prob.A, prob.B, prob.Q, prob.R)))
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED and "set_linear_constraints_knots_batch" in str(ei.value), ei.value
    s.clear_model_batch()
    s.update_settings(en_state_linear=False)
    s.solve()
    _on_d(s)
    _assert_matches(s, _stepped(prob, settings, rows, x0s, K.sample(batch), en_state_linear=0), "flag off on D")
    s.reset()


# ---- 12. a batch of 3: one partial wavefront

def test_one_partial_wavefront(pkg, monkeypatch):
    prob, nlx, nlu, _, settings = _case(pkg, "quadrotor-1+1")
    batch = 3
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.prepare()
    s.set_x0_batch(x0s)
    s.solve()
    _on_d(s)
    _assert_matches(s, _stepped(prob, settings, rows, x0s, range(batch)), "batch of 3")
    s.reset()

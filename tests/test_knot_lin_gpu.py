"""Per-knot linear (half-space) constraints of batched handles (tinympc_set_linear_constraints_knots_batch and its _device form): every
instance solves the ADMM problem whose linear slack at knot i is the projection onto knot i's OWN rows -- checked per instance against
the stepped oracle of tests/knot_lin_cases.py (TOL = 1e-9 on states and controls, equal iteration counts and status); bit for bit against
a twin with the same rows constant over the horizon (tinympc_set_linear_constraints_batch on layout A) where the rows repeat over the
knots, at 16, 32 and 64 lanes per instance; through the registers path, the per-use path, the group-sum path and the long-horizon
path; at the horizon's edges; across sub-ranges, the ways out of the mode, the enable flags, prepare(), warm ticks with shifted rows
and device input; together with cones, fdyn and every other per-instance family. What no kernel carries is refused, and invalid
input changes nothing. Inputs and sample conditions: tests/knot_lin_cases.py."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest
from conftest import rel_err

import knot_lin_cases as K
from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs, _torch_gpu
from test_instance_lin_gpu import _assert_same_bits, _rows, _solver

pytestmark = pytest.mark.gpu

TOL = K.TOL


def _assert_matches(s, expect, tag):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, (ox, ou, it, status) in expect.items():
        ex, eu = rel_err(sol["states"][:, :, b], ox), rel_err(sol["controls"][:, :, b], ou)
        print(tag, "instance", b, "iter", st["iter"][b], it, "status", st["status"][b], status, "rel_err x %.2e u %.2e" % (ex, eu))
        assert st["iter"][b] == it and st["status"][b] == status, (tag, b)
        assert ex < TOL and eu < TOL, (tag, b, ex, eu)


def _stepped(prob, settings, rows, x0s, samples, **flags):
    """The stepped oracle's cold solve of the sampled instances under their own rows."""
    return {b: K.SteppedOracle(prob, settings, K.of(rows, b), **flags).solve(x0s[:, b], K.of(rows, b)) for b in samples}


# ---- 1. parity with the stepped oracle

@pytest.mark.parametrize("name", list(K.CASES))
def test_each_instance_matches_the_stepped_oracle(pkg, name):
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    own, held0 = K.reference(pkg, name)
    if name in K.VERIFIED:
        K.assert_sample_conditions(name, own, held0, settings["max_iter"])
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    assert s.launch_info()["layout"] == "A" and "per-knot-linear" in s.jit_info()
    s.set_x0_batch(x0s)
    s.solve()
    _assert_matches(s, own, name)
    s.reset()


# ---- 2. rows repeated over the knots == the same rows through the constant verb on layout A, bit for bit

@pytest.mark.parametrize("name", ["quadrotor-1+1", "quadrotor-10+3", "wide32-2+2", "wide64-1+2", "quadrotor120-1+1"])
def test_repeated_rows_are_the_constant_rows_bit_for_bit(pkg, name):
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *const = _rows(prob, nlx, nlu, batch)  # (per instance, constant over the horizon)
    twin, knots = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)
    twin.set_linear_constraints_batch(*const)
    knots.set_linear_constraints_knots_batch(*K.repeat_over_knots(const, prob.N))
    for rnd in range(2):  # a cold start, then a warm start
        for h in (twin, knots):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        _assert_same_bits(twin, knots)  # states, controls, iterations, status, the four residuals
    assert twin.launch_info()["layout"] == knots.launch_info()["layout"] == "A"
    assert "per-knot-linear" in knots.jit_info() and "per-knot-linear" not in twin.jit_info()
    for h in (twin, knots):
        h.reset()


# ---- 3. the _device form is the host form, bit for bit

@pytest.mark.parametrize("name", ["quadrotor-3+2", "wide32-2+2"])
def test_device_form_is_the_host_form_bit_for_bit(pkg, name):
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    host, devh = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)
    host.set_linear_constraints_knots_batch(*rows)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    Ax, bx, Au, bu = rows
    assert L.tinympc_set_linear_constraints_knots_batch_device(devh._h, dev.put(Ax), dev.put(bx), nlx, dev.put(Au), dev.put(bu), nlu, 0, batch) == 0
    dev.free()  # (the input has been copied when the verb returns)
    handles = [host, devh]
    torch = _torch_gpu()
    if torch is not None:  # the Python method routes CUDA tensors to the _device form: (count, knots, cols, rows) / (count, knots, rows)
        th = _solver(pkg, prob, batch, settings)
        th.set_linear_constraints_knots_batch(*(torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in rows))
        handles.append(th)
    for h in handles:
        h.set_x0_batch(x0s)
        h.solve()
    for h in handles[1:]:
        _assert_same_bits(host, h)
    for h in handles:
        h.reset()


# ---- 4. b = +inf switches one row off at one knot

def test_infinite_b_switches_a_row_off_at_single_knots(pkg):
    name = "quadrotor-3+2"
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, Ax, bx, Au, bu = K.rows_knots(prob, nlx, nlu, batch)
    bx, bu = bx.copy(), bu.copy()
    N, samples = prob.N, K.sample(batch)
    for i, b in enumerate(samples):  # other rows and knots per sampled instance: registers and per-use path, both edges of the horizon
        bx[i % nlx, (3 * i) % N, b] = np.inf
        bx[nlx - 1, N - 1 - i, b] = np.inf
        bu[i % nlu, (5 * i) % (N - 1), b] = np.inf
        bu[:, 0, b] = np.inf  # (a knot without any input row)
    rows = (Ax, bx, Au, bu)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.set_x0_batch(x0s)
    s.solve()
    expect = _stepped(prob, settings, rows, x0s, samples)
    own, _ = K.reference(pkg, name)
    assert any(rel_err(expect[b][1], own[b][1]) > 1e-6 for b in samples)  # (the switched-off rows mattered)
    _assert_matches(s, expect, "rows off at knots")
    s.reset()


# ---- 5. the horizon's edges: rows that act only at knot 0 (the state lanes' call in front of the sweep) / only at the last knot

@pytest.mark.parametrize("edge", ["first", "last"])
def test_rows_active_only_at_one_edge_of_the_horizon(pkg, edge):
    prob, nlx, nlu, batch, settings = K.case(pkg, "quadrotor-1+1")
    x0s, Ax, bx, Au, bu = K.rows_knots(prob, nlx, nlu, batch)
    N = prob.N
    kx, ku = (0, 0) if edge == "first" else (N - 1, N - 2)
    samples = K.sample(batch)
    off = (Ax, np.full_like(bx, np.inf), Au, np.full_like(bu, np.inf))
    free = _stepped(prob, settings, off, x0s, samples)  # the reference with every row off: where the edge's rows have to cut
    tight_x = np.einsum("kcb,cb->kb", Ax[:, :, kx, :], x0s) - 0.05  # violated by x0 itself (knot 0) / close to the trajectory (last knot)
    tight_u = np.full((nlu, batch), -0.05)
    for b in samples:  # 0.1 inside what the instance does without rows at that knot, so that the row binds
        tight_u[:, b] = Au[:, :, ku, b] @ free[b][1][:, ku] - 0.1
    bx, bu = off[1].copy(), off[3].copy()
    bx[:, kx, :], bu[:, ku, :] = tight_x, tight_u
    rows = (Ax, bx, Au, bu)
    expect = _stepped(prob, settings, rows, x0s, samples)
    moved = [rel_err(expect[b][1], free[b][1]) for b in samples]
    print(edge, "moved against rows that are off everywhere", moved)
    assert 2 * sum(m > 1e-3 for m in moved) >= len(moved)  # (the edge's rows act)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.set_x0_batch(x0s)
    s.solve()
    _assert_matches(s, expect, "edge " + edge)
    s.reset()


# ---- 6. a sub-range replaces rows after a whole-batch call

@pytest.mark.parametrize("name", ["quadrotor-1+1", "wide32-2+2"])
def test_a_sub_range_replaces_rows_after_a_whole_batch_call(pkg, name):
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    _, *other = K.rows_knots(prob, nlx, nlu, batch, seed=K.SEED + 1)
    lo, hi = batch // 2, batch - 1  # (the last instance keeps its rows)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.set_linear_constraints_knots_batch(*(a[..., lo:hi] for a in other), first=lo)
    s.set_x0_batch(x0s)
    s.solve()
    mixed = tuple(np.concatenate([r[..., :lo], o[..., lo:hi], r[..., hi:]], axis=-1) for r, o in zip(rows, other))
    picks = sorted({0, lo - 1, lo, hi - 1, hi})
    _assert_matches(s, _stepped(prob, settings, mixed, x0s, picks), name + " sub-range")
    with pytest.raises(pkg.TinyMPCError) as ei:  # a sub-range may not change the counts
        s.set_linear_constraints_knots_batch(other[0][..., 0:2], other[1][..., 0:2], None, None, first=0)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    s.reset()


# ---- 7. the ways back

def test_the_ways_back(pkg):
    prob, nlx, nlu, batch, settings = K.case(pkg, "quadrotor-1+1")
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    _, *const = _rows(prob, nlx, nlu, batch)
    E = pkg._lib.ERR_INVALID_INPUT
    own, _ = K.reference(pkg, "quadrotor-1+1")
    # a sub-range of the constant verb inside the mode: refused, nothing changed
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.set_x0_batch(x0s)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_linear_constraints_batch(*(a[..., 3:9] for a in const), first=3)
    assert ei.value.code == E and "name the whole batch" in str(ei.value)
    assert "per-knot-linear" in s.jit_info()
    s.solve()
    _assert_matches(s, own, "after the refused sub-range")
    # the whole-batch constant verb: rows constant over the horizon again, the bits of a handle that never was per knot
    twin = _solver(pkg, prob, batch, settings)
    for h in (s, twin):
        h.set_linear_constraints_batch(*const)
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    info = s.jit_info()
    assert "per-instance-linear" in info and "per-knot-linear" not in info and s.launch_info()["layout"] == "A"
    _assert_same_bits(twin, s)
    s.set_linear_constraints_batch(*(a[..., 3:9] for a in const), first=3)  # (outside the mode a sub-range is welcome again)
    # ... and back in, then the shared verb: every instance on shared rows
    s.set_linear_constraints_knots_batch(*rows)
    assert "per-knot-linear" in s.jit_info()
    shared = tuple(a[..., 0] for a in const)
    for h in (s, twin):
        h.set_linear_constraints(*shared)
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    info = s.jit_info()
    assert "per-knot-linear" not in info and "per-instance-linear" not in info
    _assert_same_bits(twin, s)
    for h in (s, twin):
        h.reset()


# ---- 8. together with cones and fdyn, per-instance cone slopes, references, tracks and bounds

@pytest.mark.parametrize("slopes", ["shared", "per-instance"])
def test_rocket_keeps_its_cones_and_fdyn(pkg, slopes):
    """problems.rocket(10): the state and input cones and fdyn stay; the ground-plane row -z <= b gets a b per knot and instance, some of
    them inside the descent so that the row binds. With per-instance slopes (the other half of the same mode, the same store) every
    instance has its own glide and thrust cone as well."""
    prob = pkg.problems.rocket(10)
    batch, settings, N = 21, K.CONV, 10
    rng = np.random.default_rng(K.SEED)
    x0s = np.asfortranarray(prob.x0[:, None] + 0.1 * rng.standard_normal((prob.nx, batch)))
    Ax = np.repeat(np.repeat(np.asarray(prob.linear["Alin_x"])[:, :, None, None], N, axis=2), batch, axis=3)
    ax0 = np.einsum("kcnb,cb->knb", Ax, x0s)
    bx = ax0 + rng.uniform(0.0, 0.15, (1, N, batch)) * (1.0 + np.abs(ax0))  # 0 to 3.5 m below the start, another depth at every knot
    rows = (Ax, bx, np.zeros((0, prob.nu, N - 1, batch)), np.zeros((0, N - 1, batch)))
    samples = K.sample(batch)
    s = _solver(pkg, prob, batch, settings)
    cx = np.repeat(np.asarray(prob.cones["cx"], dtype=float)[:, None], batch, axis=1)
    cu = np.repeat(np.asarray(prob.cones["cu"], dtype=float)[:, None], batch, axis=1)
    if slopes == "per-instance":
        cx, cu = cx * rng.uniform(0.7, 1.3, cx.shape), cu * rng.uniform(0.7, 1.3, cu.shape)
        s.set_cone_slopes_batch(cx, cu)
    s.set_linear_constraints_knots_batch(Ax, bx, None, None)
    s.set_x0_batch(x0s)
    s.solve()
    info = s.jit_info()
    assert s.launch_info()["layout"] == "A" and "per-knot-linear" in info and ("per-instance-cones" in info) == (slopes == "per-instance"), info
    expect, moved = {}, []
    for b in samples:
        pb = dataclasses.replace(prob, cones=dict(prob.cones, cx=list(cx[:, b]), cu=list(cu[:, b])))
        expect[b] = K.SteppedOracle(pb, settings, K.of(rows, b)).solve(x0s[:, b], K.of(rows, b))
        off = (Ax[..., b], np.full_like(bx[..., b], np.inf), rows[2][..., b], rows[3][..., b])
        moved.append(rel_err(expect[b][1], K.SteppedOracle(pb, settings, off).solve(x0s[:, b], off)[1]))
    print("rocket", slopes, "moved by the rows", moved)
    assert 2 * sum(m > 1e-3 for m in moved) >= len(moved)
    _assert_matches(s, expect, "rocket " + slopes)
    s.reset()


@pytest.mark.parametrize("with_what", ["goals+box", "trajectories+knot", "track"])
def test_per_instance_references_and_bounds_inside_the_mode(pkg, with_what):
    name = "quadrotor-3+2"
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    samples, N = K.sample(batch), prob.N
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    full = None
    if with_what == "track":
        T, rng = N + 6, np.random.default_rng(3)
        track = 0.3 * rng.standard_normal((prob.nx, 1, batch)) * np.linspace(0.0, 1.0, T)[None, :, None]
        s.set_x_ref_track_batch(track)
        steps = (np.arange(batch) % 3).astype(np.int32)
        s.set_ref_step_batch(steps)
        s.set_ref_auto_advance(1)
    else:
        verb, (X, U) = _refs(prob, batch, "goal" if with_what.startswith("goals") else "traj")
        s.set_x_ref_batch(verb[0])
        s.set_u_ref_batch(verb[1])
        bverb, full = _bounds(prob, batch, "box" if with_what.endswith("box") else "knot")
        s.set_bound_constraints_batch(*bverb)
    orcs = {}
    for b in samples:
        pb = prob if full is None else dataclasses.replace(prob, x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
        orcs[b] = K.SteppedOracle(pb, settings, K.of(rows, b))
    for tick in range(2 if with_what == "track" else 1):
        expect = {}
        for b in samples:
            if with_what == "track":
                cols = np.minimum(steps[b] + tick + np.arange(N), T - 1)
                orcs[b].orc.set_x_ref(track[:, cols, b])
            else:
                orcs[b].orc.set_x_ref(X[:, :, b])
                orcs[b].orc.set_u_ref(U[:, :, b])
            expect[b] = orcs[b].solve(x0s[:, b], K.of(rows, b))
        if with_what == "track":
            s.mpc_step(x0s)  # (the steps advance after the solve)
        else:
            s.set_x0_batch(x0s)
            s.solve()
        _assert_matches(s, expect, (with_what, tick))
    info = s.jit_info()
    assert "per-knot-linear" in info and "per-instance-refs" in info and s.launch_info()["layout"] == "A", info
    assert ("per-instance-bounds" in info) == (with_what != "track") and ("reference-track" in info) == (with_what == "track"), info
    s.reset()


# ---- 9. warm ticks: the rows shifted by one knot and re-sent before every tick, the duals kept

def test_rows_shifted_every_tick_keep_the_duals(pkg):
    prob, nlx, nlu, batch, _ = K.case(pkg, "quadrotor-1+1")
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    samples = K.sample(batch)
    s = _solver(pkg, prob, batch, settings)
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
        expect = {b: orcs[b].solve(x0t[:, b], K.of((Ax, bx, Au, bu), b)) for b in samples}  # (the oracle object keeps its workspace)
        _assert_matches(s, expect, ("tick", tick))
    s.reset()


# ---- 10. the enable flags act on every instance

def test_state_side_switched_off_after_the_verb(pkg):
    name = "quadrotor-3+2"
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.update_settings(en_state_linear=False)
    s.set_x0_batch(x0s)
    s.solve()
    assert "per-knot-linear" in s.jit_info()
    _assert_matches(s, _stepped(prob, settings, rows, x0s, K.sample(batch), en_state_linear=0), "flag off")
    s.reset()


# ---- 11. prepare(), before and after the verb: still layout A, the same bits

def test_prepare_keeps_the_mode_on_layout_a(pkg):
    prob, nlx, nlu, batch, settings = K.case(pkg, "quadrotor-1+1")
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    plain, before, after = (_solver(pkg, prob, batch, settings) for _ in range(3))
    before.prepare()
    for h in (plain, before, after):
        h.set_linear_constraints_knots_batch(*rows)
    after.prepare()
    for h in (plain, before, after):
        h.set_x0_batch(x0s)
        h.solve()
        info = h.jit_info()
        assert h.launch_info()["layout"] == "A" and "per-knot-linear" in info and "refused" not in info, info
    _assert_same_bits(plain, before)
    _assert_same_bits(plain, after)
    for h in (plain, before, after):
        h.reset()


# ---- 12. refusals: TINYMPC_ERR_UNSUPPORTED, a message that names the verb and the way back, and the way back works

def _refused(pkg, call):
    with pytest.raises(pkg.TinyMPCError) as ei:
        call()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED, ei.value
    assert "set_linear_constraints_knots_batch" in str(ei.value) and "tinympc_set_linear_constraints returns to shared rows" in str(ei.value), ei.value


def test_refusals_and_the_way_back(pkg):
    prob, nlx, nlu, batch, settings = K.case(pkg, "quadrotor-1+1")
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    own, _ = K.reference(pkg, "quadrotor-1+1")
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_knots_batch(*rows)
    s.set_x0_batch(x0s)
    s.set_rho_batch(np.full(batch, prob.rho * 1.5))   # per-instance rho (the model mode) ...
    _refused(pkg, s.solve)
    s.clear_model_batch()
    s.set_model_batch(*(np.repeat(m[:, :, None], batch, axis=2) for m in (prob.A, prob.B, prob.Q, prob.R)))  # ... models ...
    _refused(pkg, s.solve)
    s.clear_model_batch()
    s.update_settings(adaptive_rho=True)              # ... adaptive rho ...
    _refused(pkg, s.solve)
    s.update_settings(adaptive_rho=False)
    L = pkg.load_library()                            # ... and the resident session
    assert L.tinympc_session_begin(s._h) == pkg._lib.ERR_UNSUPPORTED
    s.reset_workspace()
    s.solve()                                         # every way back taken: the mode solves, with its own rows
    _assert_matches(s, own, "after the refusals")
    big = K.rows_knots(prob, 33, 1, batch)            # more than 32 rows on a side: refused at the verb
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_linear_constraints_knots_batch(*big[1:])
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    s.reset()


def test_large_systems_and_single_instances_are_refused(pkg):
    P = pkg.problems
    rng = np.random.default_rng(5)
    nx, nu, batch = 60, 12, 3
    prob = P.Problem("large", np.eye(nx) + 0.02 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), 8, 1.0,
                     rng.standard_normal(nx))
    s = _solver(pkg, prob, batch, K.FORCED)
    x0s, *rows = K.rows_knots(prob, 1, 1, batch)
    s.set_linear_constraints_knots_batch(*rows)       # nx+nu > 64: no kernel carries the mode, the solve refuses
    s.set_x0_batch(x0s)
    _refused(pkg, s.solve)
    s.set_linear_constraints(*(a[..., 0, 0] for a in rows))
    s.solve()
    s.reset()
    prob, nlx, nlu, _, settings = K.case(pkg, "quadrotor-1+1")  # batch == 1: the verb itself refuses and changes nothing
    x0s, *rows = K.rows_knots(prob, nlx, nlu, 1)
    one = _solver(pkg, prob, 1, settings)
    one.set_x0(x0s[:, 0])
    one.solve()
    before = one.get_solution()
    with pytest.raises(pkg.TinyMPCError) as ei:
        one.set_linear_constraints_knots_batch(*rows)
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED and "per-knot-linear" not in one.jit_info()
    one.reset_workspace()
    one.solve()
    np.testing.assert_array_equal(before["controls"], one.get_solution()["controls"])
    one.reset()


# ---- 13. invalid arguments change nothing

def _raise(pkg, code):
    pkg._lib.check(code)


def test_invalid_arguments_change_nothing(pkg):
    prob, nlx, nlu, batch, settings = K.case(pkg, "quadrotor-1+1")
    x0s, Ax, bx, Au, bu = K.rows_knots(prob, nlx, nlu, batch)
    N = prob.N
    L, lib, dev = pkg.load_library(), pkg._lib, _DeviceArrays(pkg)
    E = lib.ERR_INVALID_INPUT
    s, twin = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)  # (the twin: the same history without the bad calls)
    with pytest.raises(pkg.TinyMPCError) as ei:  # a first call on a sub-range, before the mode exists
        s.set_linear_constraints_knots_batch(*(a[..., 3:9] for a in (Ax, bx, Au, bu)), first=3)
    assert ei.value.code == E and "per-knot-linear" not in s.jit_info() and not s.settings.get("en_state_linear")
    for h in (s, twin):
        h.set_linear_constraints_knots_batch(Ax, bx, Au, bu)
        h.set_x0_batch(x0s)
        h.solve()
        h.solve()  # (a warm start: the state a bad call must not touch)

    def bad(which, value, knot):
        a = [Ax.copy(), bx.copy(), Au.copy(), bu.copy()]
        if which == 0 or which == 2:
            a[which][0, :, knot, batch - 1] = value
        else:
            a[which][0, knot, batch - 1] = value
        return a

    host = [np.asfortranarray(a) for a in (Ax, bx, Au, bu)]
    calls = []
    for which, value, knot in ((0, 0.0, 0), (0, np.nan, N - 1), (0, np.inf, 7), (2, 0.0, N - 2), (2, np.nan, 0), (1, np.nan, N - 1), (1, -np.inf, 0),
                               (3, np.nan, 5), (3, -np.inf, N - 2)):
        arrays = bad(which, value, knot)
        calls.append(lambda arrays=arrays: s.set_linear_constraints_knots_batch(*arrays))                          # the host form
        calls.append(lambda arrays=arrays: _raise(pkg, L.tinympc_set_linear_constraints_knots_batch_device(       # the _device form
            s._h, dev.put(arrays[0]), dev.put(arrays[1]), nlx, dev.put(arrays[2]), dev.put(arrays[3]), nlu, 0, batch)))
    p = [a.ctypes.data_as(lib.c_double_p) for a in host]
    raw = L.tinympc_set_linear_constraints_knots_batch
    calls += [
        lambda: _raise(pkg, raw(s._h, None, p[1], nlx, p[2], p[3], nlu, 0, batch)),        # NULL for a non-empty side
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], None, nlu, 0, batch)),
        lambda: _raise(pkg, raw(s._h, p[0], p[1], -1, p[2], p[3], nlu, 0, batch)),         # negative counts
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], -2, 0, batch)),
        lambda: _raise(pkg, raw(s._h, None, None, 0, None, None, 0, 0, batch)),            # no row on either side
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], nlu, 0, 0)),            # an empty range
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], nlu, -1, 2)),           # ranges beyond the batch
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], nlu, batch - 1, 2)),
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, None, None, 0, 2, 3)),              # a sub-range with other counts
        lambda: _raise(pkg, L.tinympc_set_linear_constraints_knots_batch_device(           # host memory handed to the _device form
            s._h, C.c_void_p(host[0].ctypes.data), C.c_void_p(host[1].ctypes.data), nlx, C.c_void_p(host[2].ctypes.data),
            C.c_void_p(host[3].ctypes.data), nlu, 0, batch)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == E, (i, ei.value)
        for h in (s, twin):  # each bad call leaves the following solve bit-identical
            h.solve()
        _assert_same_bits(twin, s)
    dev.free()
    assert "per-knot-linear" in s.jit_info() and s.settings["en_state_linear"] and s.settings["en_input_linear"]
    s.reset()
    twin.reset()

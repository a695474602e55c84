"""Per-instance linear (half-space) constraints of batched handles (tinympc_set_linear_constraints_batch and its _device form): every
instance solves what a single-instance handle would solve after set_linear_constraints with its own rows -- checked against the plain-C
oracle per instance (TOL on states and controls, equal iteration counts and status), bit for bit against a shared-row twin on layout A
where the rows coincide, through the registers path (up to 8 rows), the per-use path (rows beyond 8), the group-sum path (32 / 64 lanes
per instance) and the long-horizon path, together with shared cones and fdyn, per-instance references, tracks and bounds, across
sub-ranges, mode switches, the enable flags, warm-started ticks with re-sent rows and device input; what no kernel carries is refused,
never solved with shared rows, and invalid input changes nothing.

Inputs (seed SEED = 7, chosen so that the ORACLE ALONE meets the sample conditions below -- tools are not involved): x0_b = x0 + 0.1 randn,
rows of A random unit vectors, state side b = a'x0_b + U(0.5, 2) (1 + |a'x0_b|) (feasible at knot 0), input side b = U(0.2, 0.8).
Sample conditions of the 16-lane parity cases, asserted on the oracle's own results for the sampled instances: at least two converge
before max_iter, at least one does not, at least half move their controls by more than 1e-3 (relative) against no rows and against
the same instance under another instance's rows."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O
from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs, _torch_gpu, _wide

pytestmark = pytest.mark.gpu

TOL = 1e-9
SEED = 7
CONV = dict(max_iter=300, abs_pri_tol=1e-4, abs_dua_tol=1e-4)   # the 16-lane cases
FORCED = dict(max_iter=60, abs_pri_tol=0.0, abs_dua_tol=0.0)     # the wide cases do not converge: 60 forced iterations

CASES = {  # name -> (problem, state rows, input rows, batch, settings); batches are ragged on purpose
    "quadrotor-1+1": (lambda P: P.quadrotor(20), 1, 1, 37, CONV),
    "quadrotor-10+3": (lambda P: P.quadrotor(20), 10, 3, 37, CONV),      # rows beyond the eight kept in registers
    "cartpole-2+1": (lambda P: P.cartpole(20, True), 2, 1, 21, CONV),
    "wide32-2+2": (lambda P: _wide(P, 24, 8, 20), 2, 2, 21, FORCED),     # 32 lanes per instance: group sums
    "wide64-1+2": (lambda P: _wide(P, 48, 16, 12), 1, 2, 9, FORCED),     # 64 lanes per instance
    "quadrotor120-1+1": (lambda P: P.quadrotor(120), 1, 1, 6, CONV),     # the long-horizon path (state in HBM)
}
CONDITIONED = ["quadrotor-1+1", "quadrotor-10+3", "cartpole-2+1", "quadrotor120-1+1"]  # the 16-lane cases: SEED meets the sample conditions


def _case(pkg, name):
    make, nlx, nlu, batch, settings = CASES[name]
    return make(pkg.problems), nlx, nlu, batch, settings


def _rows(prob, nlx, nlu, batch, seed=SEED):
    """-> x0s (nx, batch), Ax (nlx, nx, batch), bx (nlx, batch), Au (nlu, nu, batch), bu (nlu, batch): the recipe of the module docstring."""
    rng = np.random.default_rng(seed)
    nx, nu = prob.nx, prob.nu
    x0s = np.asfortranarray(prob.x0[:, None] + 0.1 * rng.standard_normal((nx, batch)))

    def unit(rows, cols):
        a = rng.standard_normal((rows, cols, batch))
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    Ax, Au = unit(nlx, nx), unit(nlu, nu)
    ax0 = np.einsum("kcb,cb->kb", Ax, x0s)
    bx = ax0 + rng.uniform(0.5, 2.0, (nlx, batch)) * (1.0 + np.abs(ax0))
    bu = rng.uniform(0.2, 0.8, (nlu, batch))
    return x0s, Ax, bx, Au, bu


def _sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1}) if batch > 6 else list(range(batch))


def _solver(pkg, prob, batch, settings):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if prob.x_ref is not None:
        s.set_x_ref(prob.x_ref)
    if prob.u_ref is not None:
        s.set_u_ref(prob.u_ref)
    if prob.cones:
        s.set_cone_constraints(**prob.cones)
    return s


def _oracle(prob, settings, rows=None, **flags):
    """The oracle of one instance: the problem (its cones and fdyn included) with `rows` = (Ax_b, bx_b, Au_b, bu_b), or without rows."""
    pb = dataclasses.replace(prob, linear={})
    orc = O.OraclePort(pb).load_problem(pb, settings)
    if rows is not None:
        orc.set_linear_constraints(*rows)
    orc.update_settings(**flags)
    return orc


def _of(rows, b):
    Ax, bx, Au, bu = rows
    return Ax[:, :, b], bx[:, b], Au[:, :, b], bu[:, b]


def _run(orc, x0):
    orc.set_x0(x0)
    orc.solve()
    return orc.solution()[0].copy(), orc.solution()[1].copy(), orc.stats()["iter"], orc.stats()["status"]


@functools.lru_cache(maxsize=None)
def _reference(pkg, name):
    """Computed once per case and shared: the oracle's cold solve of every sampled instance under its own rows, under no rows and under
    its neighbour's rows."""
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    samples = _sample(batch)
    own, free, other = {}, {}, {}
    for i, b in enumerate(samples):
        own[b] = _run(_oracle(prob, settings, _of(rows, b)), x0s[:, b])
        free[b] = _run(_oracle(prob, settings), x0s[:, b])
        other[b] = _run(_oracle(prob, settings, _of(rows, samples[(i + 1) % len(samples)])), x0s[:, b])
    return own, free, other


def _assert_matches(s, expect, tag):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, (ox, ou, it, status) in expect.items():
        ex, eu = rel_err(sol["states"][:, :, b], ox), rel_err(sol["controls"][:, :, b], ou)
        print(tag, "instance", b, "iter", st["iter"][b], it, "status", st["status"][b], status, "rel_err x %.2e u %.2e" % (ex, eu))
        assert st["iter"][b] == it and st["status"][b] == status, (tag, b)
        assert ex < TOL and eu < TOL, (tag, b, ex, eu)


def _assert_same_bits(a, b):
    sa, sb = a.get_solution_batch(), b.get_solution_batch()
    np.testing.assert_array_equal(sa["states"], sb["states"])
    np.testing.assert_array_equal(sa["controls"], sb["controls"])
    ta, tb = a.get_stats_batch(), b.get_stats_batch()
    for k in ta:  # iterations, status, the four residuals
        np.testing.assert_array_equal(ta[k], tb[k])


# ---- 1. parity with the oracle

@pytest.mark.parametrize("name", list(CASES))
def test_each_instance_matches_the_oracle_with_its_own_rows(pkg, name):
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    own, free, other = _reference(pkg, name)
    if name in CONDITIONED:  # the oracle alone: the sample is neither all converged nor all stuck, and the rows matter per instance
        its = [own[b][2] for b in own]
        moved = [rel_err(own[b][1], free[b][1]) > 1e-3 for b in own]
        differ = [rel_err(own[b][1], other[b][1]) > 1e-3 for b in own]
        print(name, "oracle iterations", its, "moved", moved, "differ", differ)
        assert sum(i < settings["max_iter"] for i in its) >= 2 and sum(i >= settings["max_iter"] for i in its) >= 1
        assert 2 * sum(moved) >= len(moved) and 2 * sum(differ) >= len(differ)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    assert s.launch_info()["layout"] == "A" and "per-instance-linear" in s.jit_info()
    s.prepare()  # (nothing to specialise)
    s.set_x0_batch(x0s)
    s.solve()
    _assert_matches(s, own, name)
    s.reset()


@pytest.mark.parametrize("offsets", ["recipe", "binding"])
def test_rocket_keeps_its_cones_and_fdyn(pkg, offsets):
    """problems.rocket(10): the shared state and input cones and fdyn stay, the ground-plane row -z <= b gets every instance's own b.

    "recipe": the issue's b = a'x0_b + U(0.5, 2) (1 + |a'x0_b|). The vehicle starts at z = 22 m and descends 2.5 m in its ten knots; the
    recipe puts the plane 11.5 to 46 m below it, so the row is never active. On the oracle alone, for every seed from 0 to 399: no
    sampled instance reaches max_iter (seed 7: 41 to 62 iterations) and fewer than three of the five move by 1e-3 against no rows
    (seed 7: 4.6e-4 to 9.8e-4, the effect of switching the family on); for the seeds looked at in full (0 to 4 and 7) an instance under
    its NEIGHBOUR's b gives exactly the controls it gives under its own, relative difference 0.0. No seed meets the sample conditions
    here: this case asserts parity (and that the family acts), nothing about b.
    "binding" (this file's addition, so that a kernel that read another instance's b fails on the rocket too): two instances in three
    get the plane 0 to 2.3 m below their start, b = a'x0_b + U(0, 0.1) (1 + |a'x0_b|), which the descent reaches; every third keeps
    the recipe's. Asserted on the oracle alone, for the sampled instances: at least one converges before max_iter and at least one
    does not, at least half move their controls by more than 1e-3 against no rows, and at least half against their neighbour's b."""
    prob = pkg.problems.rocket(10)
    batch, settings = 21, CONV
    rng = np.random.default_rng(SEED)
    x0s = np.asfortranarray(prob.x0[:, None] + 0.1 * rng.standard_normal((prob.nx, batch)))
    Ax = np.repeat(np.asarray(prob.linear["Alin_x"])[:, :, None], batch, axis=2)
    ax0 = np.einsum("kcb,cb->kb", Ax, x0s)
    factor = rng.uniform(0.5, 2.0, (1, batch))
    if offsets == "binding":
        factor = np.where(np.arange(batch)[None, :] % 3 != 0, rng.uniform(0.0, 0.1, (1, batch)), factor)
    bx = ax0 + factor * (1.0 + np.abs(ax0))
    rows = (Ax, bx, np.zeros((0, prob.nu, batch)), np.zeros((0, batch)))
    samples = _sample(batch)
    expect = {b: _run(_oracle(prob, settings, _of(rows, b)), x0s[:, b]) for b in samples}
    moved = [rel_err(expect[b][1], _run(_oracle(prob, settings), x0s[:, b])[1]) for b in samples]
    differ = [rel_err(expect[b][1], _run(_oracle(prob, settings, _of(rows, samples[(i + 1) % len(samples)])), x0s[:, b])[1])
              for i, b in enumerate(samples)]
    its = [expect[b][2] for b in samples]
    print("rocket", offsets, "oracle iterations", its, "moved", moved, "differ", differ)
    assert all(m > 1e-6 for m in moved)  # (the family acts on every sampled instance, far above TOL)
    if offsets == "binding":
        assert sum(i < settings["max_iter"] for i in its) >= 1 and sum(i >= settings["max_iter"] for i in its) >= 1
        assert 2 * sum(m > 1e-3 for m in moved) >= len(samples) and 2 * sum(d > 1e-3 for d in differ) >= len(samples)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(Ax, bx, None, None)
    s.set_x0_batch(x0s)
    s.solve()
    assert s.launch_info()["layout"] == "A"
    _assert_matches(s, expect, "rocket " + offsets)
    s.reset()


# ---- 2. identical rows on every instance == the shared rows of a twin on layout A, bit for bit; 7. the shared verb returns the mode

@pytest.mark.parametrize("name", ["quadrotor-1+1", "quadrotor-10+3", "wide32-2+2", "wide64-1+2", "quadrotor120-1+1"])
def test_identical_rows_are_the_shared_rows_bit_for_bit(pkg, monkeypatch, name):
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    one = _of(rows, batch - 1)
    inst = _solver(pkg, prob, batch, settings)  # (a handle as setup makes it: the mode puts it on layout A)
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")   # the twins: shared rows on layout A, at setup and at every launch
    twin = _solver(pkg, prob, batch, settings)
    twin.set_linear_constraints(*one)
    inst.set_linear_constraints_batch(*(np.repeat(a[..., None], batch, axis=-1) for a in one))
    for rnd in range(2):  # a cold start, then a warm start
        for h in (twin, inst):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        _assert_same_bits(twin, inst)
    assert twin.launch_info()["layout"] == inst.launch_info()["layout"] == "A"
    assert "per-instance-linear" in inst.jit_info() and "per-instance-linear" not in twin.jit_info()
    # the shared verb returns every instance to shared rows (other ones, after per-instance ones), and the word is gone
    other = _of(rows, 0)
    back, twin2 = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)
    back.set_linear_constraints_batch(*rows)
    for h in (back, twin2):
        h.set_linear_constraints(*other)
        h.set_x0_batch(x0s)
        h.solve()
    assert "per-instance-linear" not in back.jit_info() and back.launch_info()["layout"] == "A"
    _assert_same_bits(twin2, back)
    for h in (twin, twin2, inst, back):
        h.reset()


# ---- 3. the _device form is the host form, bit for bit

@pytest.mark.parametrize("name", ["quadrotor-10+3", "wide32-2+2"])
def test_device_form_is_the_host_form_bit_for_bit(pkg, name):
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    host, devh = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)
    host.set_linear_constraints_batch(*rows)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    Ax, bx, Au, bu = rows
    assert L.tinympc_set_linear_constraints_batch_device(devh._h, dev.put(Ax), dev.put(bx), nlx, dev.put(Au), dev.put(bu), nlu, 0, batch) == 0
    dev.free()  # (the input has been copied when the verb returns)
    handles = [host, devh]
    torch = _torch_gpu()
    if torch is not None:  # the Python method routes CUDA tensors to the _device form: (count, cols, rows) / (count, rows)
        th = _solver(pkg, prob, batch, settings)
        th.set_linear_constraints_batch(*(torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in rows))
        handles.append(th)
    for h in handles:
        h.set_x0_batch(x0s)
        h.solve()
    for h in handles[1:]:
        _assert_same_bits(host, h)
    for h in handles:
        h.reset()


# ---- 4. b = +inf switches one row off for one instance

def test_infinite_b_switches_a_row_off(pkg):
    name = "quadrotor-10+3"
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, Ax, bx, Au, bu = _rows(prob, nlx, nlu, batch)
    samples = _sample(batch)
    bx, bu = bx.copy(), bu.copy()
    off = {b: (i % nlx, i % nlu) for i, b in enumerate(samples)}  # a different row per sampled instance (registers and per-use path)
    off[samples[-1]] = (nlx - 1, nlu - 1)
    for b, (kx, ku) in off.items():
        bx[kx, b] = np.inf
        bu[ku, b] = np.inf
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(Ax, bx, Au, bu)
    s.set_x0_batch(x0s)
    s.solve()
    expect = {}
    for b, (kx, ku) in off.items():
        keep_x, keep_u = [k for k in range(nlx) if k != kx], [k for k in range(nlu) if k != ku]
        expect[b] = _run(_oracle(prob, settings, (Ax[keep_x, :, b], bx[keep_x, b], Au[keep_u, :, b], bu[keep_u, b])), x0s[:, b])
    _assert_matches(s, expect, "row off")
    s.reset()


# ---- 5. / 6. sub-ranges

@pytest.mark.parametrize("name", ["quadrotor-1+1", "wide32-2+2"])
def test_a_sub_range_over_shared_rows_leaves_the_others_on_them(pkg, name):
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    shared = _of(rows, 1)
    lo, hi = batch // 2, batch - 1  # (the last instance stays on the shared rows)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints(*shared)
    s.set_linear_constraints_batch(*(a[..., lo:hi] for a in rows), first=lo)
    s.set_x0_batch(x0s)
    s.solve()
    assert "per-instance-linear" in s.jit_info()
    expect = {b: _run(_oracle(prob, settings, _of(rows, b) if lo <= b < hi else shared), x0s[:, b]) for b in sorted({0, lo - 1, lo, hi - 1, hi})}
    _assert_matches(s, expect, name + " sub-range")
    # a later sub-range call keeps the mode's counts ...
    s.set_linear_constraints_batch(*(a[..., 0:2] for a in rows), first=0)
    E = pkg._lib.ERR_INVALID_INPUT
    with pytest.raises(pkg.TinyMPCError) as ei:  # ... and may not change them
        s.set_linear_constraints_batch(rows[0][:, :, 0:2], rows[1][:, 0:2], None, None, first=0)
    assert ei.value.code == E
    s.reset_workspace()
    s.solve()
    expect = {b: _run(_oracle(prob, settings, _of(rows, b) if (lo <= b < hi or b < 2) else shared), x0s[:, b]) for b in sorted({0, 1, 2, hi})}
    _assert_matches(s, expect, name + " second sub-range")
    s.reset()


def test_a_first_sub_range_call_without_matching_shared_rows_is_invalid(pkg):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    E = pkg._lib.ERR_INVALID_INPUT
    s = _solver(pkg, prob, batch, settings)
    s.set_x0_batch(x0s)
    for shared in (None, (rows[0][:, :, 0], rows[1][:, 0], np.zeros((0, prob.nu)), np.zeros(0))):  # no shared rows; other counts
        if shared is not None:
            s.set_linear_constraints(*shared)
        s.solve()
        before = s.get_solution_batch()
        with pytest.raises(pkg.TinyMPCError) as ei:
            s.set_linear_constraints_batch(*(a[..., 3:9] for a in rows), first=3)
        assert ei.value.code == E and "per-instance-linear" not in s.jit_info()
        s.reset_workspace()
        s.solve()
        np.testing.assert_array_equal(before["controls"], s.get_solution_batch()["controls"])
        s.reset_workspace()
    s.set_linear_constraints_batch(*rows)  # the whole batch may begin the mode with counts of its own
    assert "per-instance-linear" in s.jit_info()
    s.reset()


# ---- 8. inside the mode: per-instance references, bounds and tracks

@pytest.mark.parametrize("with_what", ["goals+box", "trajectories+knot", "track"])
def test_per_instance_references_and_bounds_inside_the_mode(pkg, with_what):
    name = "quadrotor-10+3"
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    samples = _sample(batch)
    N = prob.N
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
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
        orcs[b] = _oracle(pb, settings, _of(rows, b))
    for tick in range(2 if with_what == "track" else 1):
        expect = {}
        for b in samples:
            if with_what == "track":
                cols = np.minimum(steps[b] + tick + np.arange(N), T - 1)
                orcs[b].set_x_ref(track[:, cols, b])
            else:
                orcs[b].set_x_ref(X[:, :, b])
                orcs[b].set_u_ref(U[:, :, b])
            expect[b] = _run(orcs[b], x0s[:, b])
        if with_what == "track":
            s.mpc_step(x0s)  # (the steps advance after the solve)
        else:
            s.set_x0_batch(x0s)
            s.solve()
        _assert_matches(s, expect, (with_what, tick))
    info = s.jit_info()
    assert "per-instance-linear" in info and "per-instance-refs" in info and s.launch_info()["layout"] == "A", info
    assert ("per-instance-bounds" in info) == (with_what != "track") and ("reference-track" in info) == (with_what == "track"), info
    s.reset()


# ---- 9. warm-started ticks with the rows replaced before every tick through the _device form: the duals are kept

def test_rows_replaced_every_tick_keep_the_duals(pkg):
    name = "quadrotor-1+1"
    prob, nlx, nlu, batch, _ = _case(pkg, name)
    settings = dict(max_iter=40, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    samples = _sample(batch)
    s = _solver(pkg, prob, batch, settings)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    orcs = {b: _oracle(prob, settings) for b in samples}
    for tick in range(4):
        x0s, Ax, bx, Au, bu = _rows(prob, nlx, nlu, batch, seed=SEED + tick)
        assert L.tinympc_set_linear_constraints_batch_device(s._h, dev.put(Ax), dev.put(bx), nlx, dev.put(Au), dev.put(bu), nlu, 0, batch) == 0
        dev.free()
        s.mpc_step(x0s)
        expect = {}
        for b in samples:
            orcs[b].set_linear_constraints(*_of((Ax, bx, Au, bu), b))  # (keeps the workspace, the linear family's duals included)
            orcs[b].update_settings()
            expect[b] = _run(orcs[b], x0s[:, b])
        _assert_matches(s, expect, ("tick", tick))
    s.reset()


# ---- 10. the enable flags act on every instance

def test_state_side_switched_off_after_the_verb(pkg):
    name = "quadrotor-10+3"
    prob, nlx, nlu, batch, settings = _case(pkg, name)
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    s.update_settings(en_state_linear=False)
    s.set_x0_batch(x0s)
    s.solve()
    assert "per-instance-linear" in s.jit_info()
    _assert_matches(s, {b: _run(_oracle(prob, settings, _of(rows, b), en_state_linear=0), x0s[:, b]) for b in _sample(batch)}, "flag off")
    s.reset()


# ---- 11. refusals: TINYMPC_ERR_UNSUPPORTED at solve, a message that names the verb and the way back, and the way back works

def _refused(pkg, call):
    with pytest.raises(pkg.TinyMPCError) as ei:
        call()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED, ei.value
    assert "set_linear_constraints_batch" in str(ei.value) and "tinympc_set_linear_constraints returns to shared rows" in str(ei.value), ei.value


def test_refusals_and_the_way_back(pkg):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, *rows = _rows(prob, nlx, nlu, batch)
    own, _, _ = _reference(pkg, "quadrotor-1+1")
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(*rows)
    s.set_x0_batch(x0s)
    # per-instance rho (the model mode) ...
    s.set_rho_batch(np.full(batch, prob.rho * 1.5))
    _refused(pkg, s.solve)
    s.clear_model_batch()
    # ... per-instance models ...
    s.set_model_batch(*(np.repeat(m[:, :, None], batch, axis=2) for m in (prob.A, prob.B, prob.Q, prob.R)))
    _refused(pkg, s.solve)
    s.clear_model_batch()
    # ... adaptive rho ...
    s.update_settings(adaptive_rho=True)
    _refused(pkg, s.solve)
    s.update_settings(adaptive_rho=False)
    # ... more rounds of overlapping cones than the generic kernel holds (five cones that all share a row: five rounds)
    s.set_cone_constraints([0, 1, 2, 3, 4], [3, 3, 3, 3, 3], [0.5] * 5, [], [], [])
    _refused(pkg, s.solve)
    s.set_cone_constraints([], [], [], [], [], [])
    s.update_settings(en_state_soc=False)
    # ... and the resident session
    L = pkg.load_library()
    assert L.tinympc_session_begin(s._h) == pkg._lib.ERR_UNSUPPORTED
    # every documented way back taken: the mode solves, with its own rows
    s.reset_workspace()
    s.solve()
    _assert_matches(s, own, "after the refusals")
    # more than 32 rows on a side: refused at the verb
    big = _rows(prob, 33, 1, batch)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_linear_constraints_batch(*big[1:])
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    # the way back out of the mode itself
    s.set_linear_constraints(*_of(rows, 0))
    s.set_rho_batch(np.full(batch, prob.rho))
    with pytest.raises(pkg.TinyMPCError) as ei:  # (outside the mode: the pinned refusal of models with a family, unchanged)
        s.solve()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED and "set_linear_constraints_batch" not in str(ei.value)
    s.reset()


def test_large_systems_are_refused(pkg):
    P = pkg.problems
    rng = np.random.default_rng(5)
    nx, nu, batch = 60, 12, 3
    prob = P.Problem("large", np.eye(nx) + 0.02 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), 8, 1.0,
                     rng.standard_normal(nx))
    s = _solver(pkg, prob, batch, FORCED)
    x0s, *rows = _rows(prob, 1, 1, batch)
    s.set_linear_constraints_batch(*rows)
    s.set_x0_batch(x0s)
    _refused(pkg, s.solve)
    s.set_linear_constraints(*_of(rows, 0))
    s.solve()
    s.reset()


def test_single_instance_handle_takes_the_shared_verb(pkg):
    """batch = 1: the call is tinympc_set_linear_constraints with count 1 -- the same bits, no mode, and the verb's own checks of the values."""
    prob, nlx, nlu, _, settings = _case(pkg, "quadrotor-10+3")
    x0s, *rows = _rows(prob, nlx, nlu, 3)
    a, b = _solver(pkg, prob, 1, settings), _solver(pkg, prob, 1, settings)
    a.set_linear_constraints(*_of(rows, 2))
    b.set_linear_constraints_batch(*_of(rows, 2))  # (the arrays may lack the count axis)
    for h in (a, b):
        h.set_x0(x0s[:, 2])
        h.solve()
    _assert_same_bits(a, b)
    assert "per-instance-linear" not in b.jit_info()
    bad = [m.copy() for m in _of(rows, 2)]
    bad[1][0] = np.nan
    with pytest.raises(pkg.TinyMPCError) as ei:
        b.set_linear_constraints_batch(*bad)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    with pytest.raises(pkg.TinyMPCError) as ei:
        b.set_linear_constraints_batch(*_of(rows, 2), first=1)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    b.solve()
    a.solve()
    _assert_same_bits(a, b)
    a.reset()
    b.reset()


# ---- 12. invalid arguments change nothing

def test_invalid_arguments_change_nothing(pkg):
    prob, nlx, nlu, batch, settings = _case(pkg, "quadrotor-1+1")
    x0s, Ax, bx, Au, bu = _rows(prob, nlx, nlu, batch)
    s = _solver(pkg, prob, batch, settings)
    s.set_linear_constraints_batch(Ax, bx, Au, bu)
    s.set_x0_batch(x0s)
    s.solve()
    s.solve()  # (a warm start: the state a bad call must not touch)
    L, lib, dev = pkg.load_library(), pkg._lib, _DeviceArrays(pkg)
    E = lib.ERR_INVALID_INPUT
    twin = _solver(pkg, prob, batch, settings)  # the same history without the bad calls
    twin.set_linear_constraints_batch(Ax, bx, Au, bu)
    twin.set_x0_batch(x0s)
    twin.solve()
    twin.solve()

    def bad(which, value):
        a = [Ax.copy(), bx.copy(), Au.copy(), bu.copy()]
        if which == 0 or which == 2:
            a[which][0, :, batch - 1] = value
        else:
            a[which][0, batch - 1] = value
        return a

    host = [np.asfortranarray(a) for a in (Ax, bx, Au, bu)]
    calls = []
    for which, value in ((0, 0.0), (0, np.nan), (0, np.inf), (2, 0.0), (2, np.nan), (1, np.nan), (1, -np.inf), (3, np.nan), (3, -np.inf)):
        arrays = bad(which, value)
        calls.append(lambda arrays=arrays: s.set_linear_constraints_batch(*arrays))                         # the host form
        calls.append(lambda arrays=arrays: _raise(pkg, L.tinympc_set_linear_constraints_batch_device(      # the _device form
            s._h, dev.put(arrays[0]), dev.put(arrays[1]), nlx, dev.put(arrays[2]), dev.put(arrays[3]), nlu, 0, batch)))
    p = [a.ctypes.data_as(lib.c_double_p) for a in host]
    raw = L.tinympc_set_linear_constraints_batch
    calls += [
        lambda: _raise(pkg, raw(s._h, None, p[1], nlx, p[2], p[3], nlu, 0, batch)),        # NULL for a non-empty side
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], None, nlu, 0, batch)),
        lambda: _raise(pkg, raw(s._h, p[0], p[1], -1, p[2], p[3], nlu, 0, batch)),         # negative counts
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], -2, 0, batch)),
        lambda: _raise(pkg, raw(s._h, None, None, 0, None, None, 0, 0, batch)),            # no row on either side (the header says so)
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], nlu, 0, 0)),            # an empty range
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], nlu, -1, 2)),           # ranges beyond the batch
        lambda: _raise(pkg, raw(s._h, p[0], p[1], nlx, p[2], p[3], nlu, batch - 1, 2)),
        lambda: _raise(pkg, L.tinympc_set_linear_constraints_batch_device(                 # host memory handed to the _device form
            s._h, C.c_void_p(host[0].ctypes.data), C.c_void_p(host[1].ctypes.data), nlx, C.c_void_p(host[2].ctypes.data),
            C.c_void_p(host[3].ctypes.data), nlu, 0, batch)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == E, (i, ei.value)
    dev.free()
    assert "per-instance-linear" in s.jit_info() and s.settings["en_state_linear"] and s.settings["en_input_linear"]
    for h in (s, twin):
        h.solve()
    _assert_same_bits(twin, s)
    s.reset()
    twin.reset()


def _raise(pkg, code):
    pkg._lib.check(code)

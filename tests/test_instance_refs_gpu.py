"""Per-instance references of batched handles (tinympc_set_x_ref_batch / _u_ref_batch and their _device forms): every instance solves
what it would solve alone after set_x_ref / set_u_ref with its own references -- checked against the oracle per instance, bit for bit
against the shared-reference handle where the references coincide, across partial ranges, mode switches, closed-loop ticks, device
input and sharding; and the configurations no kernel carries are refused, never solved with the shared reference."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
SETTINGS = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)


def _wide(P, nx, nu, N):
    rng = np.random.default_rng(nx * 100 + nu)
    A = np.eye(nx) + 0.03 * rng.standard_normal((nx, nx))
    B = 0.1 * rng.standard_normal((nx, nu))
    prob = P.Problem("wide", A, B, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(0.5, 2, nu)), N, 2.0, rng.standard_normal(nx))
    prob.u_min, prob.u_max = np.full(nu, -0.3), np.full(nu, 0.3)
    prob.x_min, prob.x_max = np.full(nx, -2.0), np.full(nx, 2.0)
    return prob


CASES = {  # name -> (problem, batch)
    "quadrotor50": (lambda P: P.quadrotor(50), 1301),
    "quadrotor30": (lambda P: P.quadrotor(30), 1301),
    "cartpole20": (lambda P: P.cartpole(20, True), 37),
    "wide32": (lambda P: _wide(P, 24, 8, 20), 37),
    "wide64": (lambda P: _wide(P, 48, 16, 12), 21),
    "quadrotor120": (lambda P: P.quadrotor(120), 70),
}
# goals on layout D: compiled in (quadrotor N=50), or run-time specialised (the others; not with TINYMPC_JIT=0)
GOAL_ON_D = {"1": {"quadrotor50", "quadrotor30", "wide32", "wide64"}, "0": {"quadrotor50"}}


def _solver(pkg, prob, batch, settings=SETTINGS):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if prob.x_ref is not None:
        s.set_x_ref(prob.x_ref)
    if prob.u_ref is not None:
        s.set_u_ref(prob.u_ref)
    return s


def _refs(prob, batch, form, seed=1):
    """-> (what the verbs take, the per-instance nx x N / nu x (N-1) references)."""
    rng = np.random.default_rng(seed)
    nx, nu, N = prob.nx, prob.nu, prob.N
    gx, gu = 0.4 * rng.standard_normal((nx, batch)), 0.05 * rng.standard_normal((nu, batch))
    if form == "goal":
        return (gx, gu), (np.repeat(gx[:, None, :], N, axis=1), np.repeat(gu[:, None, :], N - 1, axis=1))
    t = np.linspace(0.0, 1.0, N)
    X = gx[:, None, :] * (1.0 + 0.5 * np.sin(3.0 * t + np.arange(nx)[:, None]))[:, :, None]
    U = gu[:, None, :] * np.cos(2.0 * t[: N - 1])[None, :, None]
    return (X, U), (X, U)


def _x0s(prob, batch, scale=1.0, seed=2):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(prob.x0[:, None] * scale + 0.2 * rng.standard_normal((prob.nx, batch)))


def _oracle(prob, Xb, Ub, settings=SETTINGS):
    orc = O.OraclePort(prob).load_problem(prob, settings)
    if Xb is not None:
        orc.set_x_ref(Xb)
    if Ub is not None:
        orc.set_u_ref(Ub)
    return orc


def _check(s, orcs, x0s, tag):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, orc in orcs.items():
        orc.set_x0(x0s[:, b])
        orc.solve()
        assert st["iter"][b] == orc.stats()["iter"], (tag, b)
        assert st["status"][b] == orc.stats()["status"], (tag, b)
        assert rel_err(sol["states"][:, :, b], orc.solution()[0]) < TOL, (tag, b)
        assert rel_err(sol["controls"][:, :, b], orc.solution()[1]) < TOL, (tag, b)


def _sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1})


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("form", ["goal", "trajectory"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_instance_matches_the_oracle_with_its_own_references(pkg, monkeypatch, case, form, jit):
    monkeypatch.setenv("TINYMPC_JIT", jit)
    prob, batch = CASES[case][0](pkg.problems), CASES[case][1]
    s = _solver(pkg, prob, batch)
    (vx, vu), (X, U) = _refs(prob, batch, form)
    s.set_x_ref_batch(vx)
    s.set_u_ref_batch(vu)
    orcs = {b: _oracle(prob, X[:, :, b], U[:, :, b]) for b in _sample(batch)}
    for rnd in range(3):  # a cold start, then two warm starts
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (case, form, rnd))
    # the kernel that ran (decided -- and specialised where needed -- by the first solve)
    info = s.jit_info()
    assert "per-instance-refs" in info
    if form == "trajectory":
        assert s.launch_info()["layout"] == "A"
    elif case in GOAL_ON_D[jit]:  # a batch layout D serves: the goal form runs there
        assert s.launch_info()["layout"] == "D" and "goal" in info and "refused" not in info, info
        assert ("compiled-in" in info) == (case == "quadrotor50"), info
    s.reset()


@pytest.mark.parametrize("case", ["quadrotor50", "cartpole20", "wide32", "wide64", "quadrotor120", "quadrotor50-goal", "wide32-goal", "quadrotor30-goal"])
def test_per_instance_equal_to_shared_is_bit_identical(pkg, monkeypatch, case):
    """Every instance given the shared reference: the same numbers as the shared-reference handle on the same layout -- A for
    trajectories, D (the compiled-in constant-table kernel) for goals."""
    P = pkg.problems
    goal = case.endswith("-goal")
    prob, batch = CASES[case.replace("-goal", "")][0](P), CASES[case.replace("-goal", "")][1] if goal else min(CASES[case][1], 300)
    (gx, gu), (X, U) = _refs(prob, 1, "goal" if goal else "trajectory", seed=5)
    prob.x_ref, prob.u_ref = X[:, :, 0], U[:, :, 0]
    if not goal:
        monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    shared = _solver(pkg, prob, batch)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    inst = _solver(pkg, prob, batch)
    if goal:
        inst.set_x_ref_batch(np.repeat(gx, batch, axis=1))
        inst.set_u_ref_batch(np.repeat(gu, batch, axis=1))
    else:
        inst.set_x_ref_batch(np.repeat(prob.x_ref[:, :, None], batch, axis=2))
        inst.set_u_ref_batch(np.repeat(prob.u_ref[:, :, None], batch, axis=2))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, inst):
            h.set_x0_batch(x0s)
            h.solve()
        a, b = shared.get_solution_batch(), inst.get_solution_batch()
        sa, sb = shared.get_stats_batch(), inst.get_stats_batch()
        np.testing.assert_array_equal(a["states"], b["states"])
        np.testing.assert_array_equal(a["controls"], b["controls"])
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k])
    assert shared.launch_info()["layout"] == inst.launch_info()["layout"] == ("D" if goal else "A")
    assert "per-instance-refs" not in shared.jit_info() and "per-instance-refs" in inst.jit_info()
    shared.reset()
    inst.reset()


def test_partial_ranges_x_only_and_return_to_shared(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 200
    (_, _), (X, U) = _refs(prob, 1, "trajectory", seed=7)
    prob.x_ref, prob.u_ref = X[:, :, 0], U[:, :, 0]  # a non-zero shared reference
    s = _solver(pkg, prob, batch)
    (gx, _), (Xg, _) = _refs(prob, batch, "goal", seed=8)
    (tx, _), (Xt, _) = _refs(prob, batch, "trajectory", seed=9)
    # x only, two ranges of two forms; u stays shared for everyone
    s.set_x_ref_batch(gx[:, 10:60], first=10)
    s.set_x_ref_batch(tx[:, :, 100:130], first=100)
    s.set_x_ref_batch(gx[:, 55:57], first=55)  # a later call overrides a part of an earlier range
    want = {b: prob.x_ref for b in range(batch)}
    want.update({b: Xg[:, :, b] for b in range(10, 60)})
    want.update({b: Xt[:, :, b] for b in range(100, 130)})
    samples = [0, 9, 10, 30, 55, 56, 59, 60, 99, 100, 129, 130, 199]
    orcs = {b: _oracle(prob, want[b], None) for b in samples}
    x0s = _x0s(prob, batch)
    s.set_x0_batch(x0s)
    s.solve()
    _check(s, orcs, x0s, "partial")
    # kept across reset_workspace and update_settings (cold start on both sides)
    s.reset_workspace()
    s.update_settings(max_iter=80)
    settings = dict(SETTINGS, max_iter=80)
    orcs = {b: _oracle(prob, want[b], None, settings) for b in samples}
    s.solve()
    _check(s, orcs, x0s, "after reset")
    # set_x_ref returns x to shared mode for every instance
    s.set_x_ref(prob.x_ref)
    assert "per-instance-refs" not in s.jit_info()
    ref = _solver(pkg, prob, batch, dict(SETTINGS, max_iter=80))
    for h in (s, ref):
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    np.testing.assert_array_equal(s.get_solution_batch()["controls"], ref.get_solution_batch()["controls"])
    # u per instance on its own, x shared
    (_, gu), (_, Ug) = _refs(prob, batch, "goal", seed=10)
    s.set_u_ref_batch(gu[:, 20:40], first=20)
    s.reset_workspace()
    s.solve()
    orcs = {b: _oracle(prob, prob.x_ref, Ug[:, :, b] if 20 <= b < 40 else prob.u_ref, settings) for b in (0, 19, 20, 39, 40)}
    _check(s, orcs, x0s, "u only")
    s.reset()
    ref.reset()


@pytest.mark.parametrize("batch", [256, 4096])
def test_closed_loop_with_shifting_windows(pkg, batch):
    P = pkg.problems
    prob = P.quadrotor(50)
    N, T = prob.N, 8
    settings = dict(max_iter=50, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    rng = np.random.default_rng(11)
    tt = np.arange(N + T)
    long_x = 0.3 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (prob.nx, 1, batch)))  # nx x (N+T) x batch
    s = _solver(pkg, prob, batch, settings)
    r = _solver(pkg, prob, batch, settings)
    samples = [0, batch // 3, batch - 1]
    orcs = {b: _oracle(prob, None, None, settings) for b in samples}
    x = _x0s(prob, batch)
    for k in range(T):
        win = np.ascontiguousarray(long_x[:, k:k + N, :])
        s.set_x_ref_batch(win)
        r.set_x_ref_batch(win)
        u = s.mpc_step(x)
        r.set_x0_batch(x)
        r.solve()
        np.testing.assert_array_equal(u, r.get_first_controls_batch())
        st = s.get_stats_batch()
        for b, orc in orcs.items():
            orc.set_x_ref(win[:, :, b])
            orc.set_x0(x[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (k, b)
            assert rel_err(u[:, b], orc.solution()[1][:, 0]) < TOL, (k, b)
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
    s.reset()
    r.reset()


def test_device_input_matches_host_input(pkg):
    """References from device memory: another handle's device solution (nx x N x batch, the trajectory layout) through the _device
    verb, and -- where torch sees the GPU -- CUDA tensors in both forms; the same results as the same references from numpy."""
    import ctypes as C
    P = pkg.problems
    prob, batch = P.quadrotor(50), 300
    x0s = _x0s(prob, batch)
    src = _solver(pkg, prob, batch)  # its solution's states are the trajectories
    src.set_x0_batch(_x0s(prob, batch, 0.5, seed=4))
    src.solve()
    d_x, d_u = C.c_void_p(), C.c_void_p()
    L = pkg.load_library()
    assert L.tinympc_get_solution_device_ptrs(src._h, C.byref(d_x), C.byref(d_u)) == 0
    X = src.get_solution_batch()["states"]
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    h.set_x_ref_batch(X)
    assert L.tinympc_set_x_ref_batch_device(d._h, d_x, prob.nx, prob.N, 0, batch) == 0
    for q in (h, d):
        q.set_x0_batch(x0s)
        q.solve()
    np.testing.assert_array_equal(h.get_solution_batch()["states"], d.get_solution_batch()["states"])
    np.testing.assert_array_equal(h.get_stats_batch()["iter"], d.get_stats_batch()["iter"])
    for q in (h, d, src):
        q.reset()


def test_torch_tensor_input_matches_host_input(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the GPU")
    P = pkg.problems
    prob, batch = P.quadrotor(50), 300
    x0s = _x0s(prob, batch)
    out = []
    for form in ("goal", "trajectory"):
        (vx, vu), _ = _refs(prob, batch, form)
        h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
        h.set_x_ref_batch(vx)
        h.set_u_ref_batch(vu)
        d.set_x_ref_batch(torch.from_numpy(np.ascontiguousarray(vx.T)).cuda())  # (count, nx) / (count, N, nx)
        d.set_u_ref_batch(torch.from_numpy(np.ascontiguousarray(vu.T)).cuda())
        for q in (h, d):
            q.set_x0_batch(x0s)
            q.solve()
        np.testing.assert_array_equal(h.get_solution_batch()["states"], d.get_solution_batch()["states"])
        np.testing.assert_array_equal(h.get_stats_batch()["iter"], d.get_stats_batch()["iter"])
        out.append(h.get_solution_batch()["controls"])
        h.reset()
        d.reset()
    assert not np.array_equal(out[0], out[1])
    # what the library cannot read correctly is refused, not reinterpreted
    s = _solver(pkg, prob, batch)
    for bad in (torch.zeros((batch, prob.nx), dtype=torch.int64).cuda(), torch.zeros((prob.nx, batch), dtype=torch.float64).cuda(),
                torch.zeros((batch, 2 * prob.nx), dtype=torch.float64).cuda()[:, ::2]):
        with pytest.raises(pkg.TinyMPCError) as ei:
            s.set_x_ref_batch(bad)
        assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    s.reset()


def test_two_shards_equal_one_handle(pkg):
    P = pkg.problems
    prob, n = P.quadrotor(50), 402
    (vx, vu), _ = _refs(prob, n, "trajectory")
    x0s = _x0s(prob, n)
    whole = _solver(pkg, prob, n)
    whole.set_x_ref_batch(vx)
    whole.set_u_ref_batch(vu)
    whole.set_x0_batch(x0s)
    whole.solve()
    h = n // 2
    for lo, hi in ((0, h), (h, n)):
        part = _solver(pkg, prob, hi - lo)
        part.set_x_ref_batch(np.ascontiguousarray(vx[:, :, lo:hi]))
        part.set_u_ref_batch(np.ascontiguousarray(vu[:, :, lo:hi]))
        part.set_x0_batch(np.asfortranarray(x0s[:, lo:hi]))
        part.solve()
        np.testing.assert_array_equal(part.get_solution_batch()["controls"], whole.get_solution_batch(lo, hi - lo)["controls"])
        np.testing.assert_array_equal(part.get_stats_batch()["iter"], whole.get_stats_batch()["iter"][lo:hi])
        part.reset()
    whole.reset()


def test_batch_one_is_the_shared_verb(pkg):
    P = pkg.problems
    prob = P.quadrotor(50)
    (vx, vu), (X, U) = _refs(prob, 1, "goal")
    a, b = _solver(pkg, prob, 1), _solver(pkg, prob, 1)
    a.set_x_ref_batch(vx)
    a.set_u_ref_batch(vu)
    b.set_x_ref(X[:, :, 0])
    b.set_u_ref(U[:, :, 0])
    for q in (a, b):
        q.set_x0(prob.x0)
        q.solve()
    np.testing.assert_array_equal(a.get_solution()["controls"], b.get_solution()["controls"])
    assert "per-instance-refs" not in a.jit_info()
    a.reset()
    b.reset()


def _expect_unsupported(pkg, s):
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    assert "per-instance references" in str(ei.value)


def test_refusals_and_recovery(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    (vx, vu), _ = _refs(prob, batch, "goal")
    # adaptive rho, set after the references
    s = _solver(pkg, prob, batch)
    s.set_x_ref_batch(vx)
    s.set_x0_batch(_x0s(prob, batch))
    s.solve()
    s.update_settings(adaptive_rho=1)
    _expect_unsupported(pkg, s)
    s.set_x_ref(np.zeros((prob.nx, prob.N)))  # shared again: the adaptive-rho kernel may run
    s.solve()
    s.reset()
    # cone constraints set after the references, then cleared with the shared verbs
    s = _solver(pkg, prob, batch)
    s.set_u_ref_batch(vu)
    s.set_x0_batch(_x0s(prob, batch))
    s.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    s.update_settings(en_state_soc=1)
    _expect_unsupported(pkg, s)
    s.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    s.solve()
    s.reset()
    # nx + nu > 64 (layout M)
    rng = np.random.default_rng(3)
    nx, nu, N = 60, 8, 6
    big = P.Problem("big", np.eye(nx) + 0.01 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), N, 2.0,
                    rng.standard_normal(nx))
    s = _solver(pkg, big, 4)
    s.set_x_ref_batch(np.zeros((nx, 4)))
    s.set_x0_batch(np.zeros((nx, 4), order="F"))
    _expect_unsupported(pkg, s)
    s.set_x_ref(np.zeros((nx, N)))
    s.solve()
    s.reset()


def test_invalid_arguments_are_refused(pkg):
    import ctypes as C
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    s = _solver(pkg, prob, batch)
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    nx, nu, N = prob.nx, prob.nu, prob.N
    buf = np.zeros(nx * N * batch)
    ptr = buf.ctypes.data_as(pkg._lib.c_double_p)
    for f, rows, cols in ((L.tinympc_set_x_ref_batch, nx, N), (L.tinympc_set_u_ref_batch, nu, N - 1)):
        assert f(s._h, ptr, rows + 1, cols, 0, 4) == E                 # wrong rows
        assert f(s._h, ptr, rows, cols + 1, 0, 4) == E                 # cols neither N (N-1) nor 1
        assert f(s._h, ptr, rows, 1, batch - 2, 4) == E                # range beyond the batch
        assert f(s._h, ptr, rows, 1, -1, 2) == E                       # negative first
        assert f(s._h, ptr, rows, 1, 0, -1) == E                       # negative count
        assert f(s._h, None, rows, 1, 0, 4) == E                       # NULL
    for f, rows in ((L.tinympc_set_x_ref_batch_device, nx), (L.tinympc_set_u_ref_batch_device, nu)):
        assert f(s._h, None, rows, 1, 0, 4) == E
        assert f(s._h, C.c_void_p(buf.ctypes.data), rows, 1, 0, 4) == E  # host memory through the device verb
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_x_ref_batch(np.zeros((nx + 1, 4)))
    assert ei.value.code == E
    # nothing of it switched the handle to per-instance mode
    assert "per-instance-refs" not in s.jit_info()
    s.reset()


def test_kept_across_bounds_async_and_queued_solves(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 300
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=12)
    s = _solver(pkg, prob, batch)
    s.set_x_ref_batch(vx)
    s.set_u_ref_batch(vu)
    x0s = _x0s(prob, batch)
    s.set_x0_batch(x0s)
    # new bounds after the references: the solve uses both
    lo, hi = prob.u_min * 0.8, prob.u_max * 0.8
    s.set_bound_constraints(prob.x_min, prob.x_max, lo, hi)
    bprob = pkg.problems.quadrotor(50)
    bprob.u_min, bprob.u_max = lo, hi
    orcs = {b: _oracle(bprob, X[:, :, b], U[:, :, b]) for b in (0, 150, 299)}
    s.solve()
    _check(s, orcs, x0s, "bounds")
    want = s.get_solution_batch()["controls"]
    # the same solve through solve_async + synchronize, and through solve_queued, from the same (cold) state
    for how in ("async", "queued"):
        s.reset_workspace()
        if how == "async":
            s.solve_async()
            s.synchronize()
        else:
            s.solve_queued()
            assert len(s.collect_kernel_ms()) == 1
        np.testing.assert_array_equal(s.get_solution_batch()["controls"], want, err_msg=how)
    s.reset()

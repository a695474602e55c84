"""Rollout metrics (tinympc_set_rollout_metrics and its verbs; the scored variant of k_plant_step): every slot of a scored rollout equals
the numpy restatement (tests/rollout_metrics_cases.py) of that rollout's own logs bit for bit; the logs, x0 and the ADMM state equal a
rollout without metrics bit for bit; rows accumulate over calls (4 ticks = 2 + 2 = four solve + plant_step ticks); reset, clear, the
device pointer and the refusals.

Shapes: those of tests/test_rollout_gpu.py -- batches 37 and 300 (5 for the layout-M system), 5 ticks, one case per form of the kernel:
16 lanes with operand lengths 8 and 16, tracks with auto-advance (the column min(step, T-1), the held last knot crossed), per-instance
models, the families, 32 and 64 lanes, and the workgroup form (nx + nu > 64). One set of runs per (case, batch) is computed once and
shared by the tests that read it.

Tolerances: none. Every comparison is bit equality -- between two runs of this library, and against the restatement, whose float64
operations are the kernel's, one rounding each, in the documented order."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from rollout_metrics_cases import NAMES, as_rows, restate
from test_rollout_gpu import CASES, PARAMS, SETTINGS, TICKS, TRACK_T, Setup, _assert_logs_equal, _assert_unchanged, _Device, _final, _layout_env, _quad
from test_rollout_gpu import _run as _plain_run
from test_rollout_gpu import _snapshot, _x0s
from test_instance_bounds_gpu import _torch_gpu

pytestmark = pytest.mark.gpu

SETTLE_TOL = 0.05


def _col0(a, rows):
    return np.asarray(a, dtype=np.float64).reshape(rows, -1)[:, 0].copy()


def _weights(prob):
    return np.diag(prob.Q).copy(), np.diag(prob.R).copy()


def _operands(su, ticks, batch):
    """What the solves of a case's handle track and clamp to at knot 0, tick by tick: xr (nx, ticks, batch), ur, and the (lo, hi) pairs."""
    prob = su.prob
    nx, nu = prob.nx, prob.nu
    if su.case.tracks:  # step t (auto-advance 1 from step 0): column min(t, T - 1)
        cols = np.minimum(np.arange(ticks), TRACK_T - 1)
        xr, ur = su.X[:, cols, :], su.U[:, cols, :]
    else:
        x0 = _col0(prob.x_ref, nx) if prob.x_ref is not None else np.zeros(nx)
        u0 = _col0(prob.u_ref, nu) if prob.u_ref is not None else np.zeros(nu)
        xr = np.repeat(np.repeat(x0[:, None, None], ticks, axis=1), batch, axis=2)
        ur = np.repeat(np.repeat(u0[:, None, None], ticks, axis=1), batch, axis=2)
    xb = ub = None
    if prob.has_bounds():
        # (a side the problem leaves open is unbounded: set_bound_constraints fills it with -/+ 1e17, which no state comes near)
        rep = lambda v, n, fill: np.repeat((_col0(v, n) if v is not None else np.full(n, fill))[:, None], batch, axis=1)
        xb = (rep(prob.x_min, nx, -np.inf), rep(prob.x_max, nx, np.inf))
        ub = (rep(prob.u_min, nu, -np.inf), rep(prob.u_max, nu, np.inf))
    return xr, ur, xb, ub


_RUNS = {}


def _run(pkg, name, batch):
    key = (name, batch)
    if key in _RUNS:
        return _RUNS[key]
    su = Setup(pkg, name, batch)
    prob = su.prob
    qx, ru = _weights(prob)
    out = dict(su=su, qx=qx, ru=ru)
    with _layout_env(su.case.layout_env):
        # a: scored, all logs; b: the same again without logs
        a, b = su.handle(), su.handle()
        for h in (a, b):
            h.set_rollout_metrics(settle_tol=SETTLE_TOL)  # (None: the diagonals of Q and R)
        out["zero"] = as_rows(a.rollout_metrics())
        out["logs"] = a.rollout(TICKS, disturbance=su.w)
        out["rows"] = as_rows(a.rollout_metrics())
        out["gpu_ms_nologs"] = b.rollout(TICKS, disturbance=su.w, log=())["gpu_ms"]
        out["rows_nologs"] = as_rows(b.rollout_metrics())
        a.solve()
        out["final"] = _final(a)
        out["steps"] = a.get_ref_step_batch().copy()
        out["rows_after_solve"] = as_rows(a.rollout_metrics())  # (a solve is no step)
        a.reset_rollout_metrics()
        out["rows_reset"] = as_rows(a.rollout_metrics())
        # c: 4 ticks at once; d: 2 + 2; e: four solve + plant_step ticks (tracks: the step moves by hand behind the plant step)
        c, d, e = su.handle(), su.handle(), su.handle(auto_advance=False)
        for h in (c, d, e):
            h.set_rollout_metrics(qx, ru, SETTLE_TOL)
        w4 = np.asfortranarray(su.w[:, :4, :])
        c.rollout(4, disturbance=w4, log=())
        d.rollout(2, disturbance=np.asfortranarray(w4[:, :2, :]), log=("u",))
        d.rollout(2, disturbance=np.asfortranarray(w4[:, 2:, :]), log=())
        for t in range(4):
            e.solve()
            e.plant_step(w4[:, t, :])
            if su.case.tracks:
                e.advance_ref_step(1)
        out["rows4"] = [as_rows(h.rollout_metrics()) for h in (c, d, e)]
        # f: on, then off again: the plain kernel
        f = su.handle()
        f.set_rollout_metrics(qx, ru, SETTLE_TOL)
        f.clear_rollout_metrics()
        out["logs_cleared"] = f.rollout(TICKS, disturbance=su.w)
        with pytest.raises(pkg.TinyMPCError) as ei:
            f.rollout_metrics()
        out["cleared_code"] = ei.value.code
        for h in (a, b, c, d, e, f):
            h.reset()
    _RUNS[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. the rows are the restatement
@pytest.mark.parametrize("name,batch", PARAMS)
def test_every_slot_equals_the_restatement_of_the_rollouts_own_logs(pkg, name, batch):
    run = _run(pkg, name, batch)
    su, logs = run["su"], run["logs"]
    xr, ur, xb, ub = _operands(su, TICKS, batch)
    want = restate(logs["x"], logs["u"], logs["iter"], logs["status"], xr, ur, xb, ub, run["qx"], run["ru"], SETTLE_TOL)
    got = run["rows"]
    print("metrics %s batch %d: cost %.6g .. %.6g, x breach max %.3g, u breach max %.3g, iterations %d .. %d, unconverged %d, settle %s"
          % (name, batch, got[:, 1].min(), got[:, 1].max(), got[:, 2].max(), got[:, 3].max(), got[:, 4].min(), got[:, 4].max(),
             int(got[:, 6].sum()), np.unique(got[:, 7])))
    for i, k in enumerate(NAMES):
        np.testing.assert_array_equal(got[:, i], want[:, i], err_msg=k)
    np.testing.assert_array_equal(got[:, 0], np.full(batch, TICKS))
    assert (got[:, 1] > 0).all() and (got[:, 4] >= TICKS).all()
    np.testing.assert_array_equal(run["zero"], np.zeros((batch, 8)))  # (set: on and reset)
    np.testing.assert_array_equal(run["rows_after_solve"], got)


# ------------------------------------------------------------------------------------------------ 2. the metrics change nothing else
@pytest.mark.parametrize("name,batch", PARAMS)
def test_logs_and_final_state_equal_a_rollout_without_metrics(pkg, name, batch):
    run, plain = _run(pkg, name, batch), _plain_run(pkg, name, batch)
    _assert_logs_equal(plain["logs"], run["logs"])
    for k, v in plain["final"][0].items():  # x0 and the ADMM state: one more solve on both
        np.testing.assert_array_equal(v, run["final"][k], err_msg=k)
    np.testing.assert_array_equal(plain["steps"][0], run["steps"])
    # ... and a handle whose metrics were turned off again runs the plain kernel
    _assert_logs_equal(plain["logs"], run["logs_cleared"])
    assert run["cleared_code"] == pkg._lib.ERR_INVALID_INPUT


# ------------------------------------------------------------------------------------------------ 3. without logs, twice, in pieces, reset
@pytest.mark.parametrize("name,batch", PARAMS)
def test_rows_without_logs_in_pieces_and_after_reset(pkg, name, batch):
    run = _run(pkg, name, batch)
    # log=() on a second handle: the same rows (and two identical runs give identical bits)
    np.testing.assert_array_equal(run["rows"], run["rows_nologs"])
    # 4 ticks = 2 + 2 = four solve + plant_step ticks
    whole, halves, single = run["rows4"]
    np.testing.assert_array_equal(whole, halves)
    np.testing.assert_array_equal(whole, single)
    np.testing.assert_array_equal(whole[:, 0], np.full(batch, 4))
    su, logs = run["su"], run["logs"]
    xr, ur, xb, ub = _operands(su, 4, batch)
    want = restate(logs["x"][:, :5], logs["u"][:, :4], logs["iter"][:4], logs["status"][:4], xr, ur, xb, ub, run["qx"], run["ru"], SETTLE_TOL)
    np.testing.assert_array_equal(whole, want)  # (the first four ticks of the logged run)
    np.testing.assert_array_equal(run["rows_reset"], np.zeros((batch, 8)))


# ------------------------------------------------------------------------------------------------ 4. per-instance goals and boxes
@pytest.mark.parametrize("batch", [37, 300])
def test_per_instance_goals_and_boxes(pkg, batch):
    """Goals and boxes per instance (set_x_ref_batch / set_u_ref_batch / set_bound_constraints_batch): the scored step reads the instance's
    own reference and box. Every second instance's box excludes its x0 in one coordinate; settle_tol is taken from the logged errors of a
    first run so that some instances settle and some do not."""
    P = pkg.problems
    prob = P.quadrotor(20)
    nx, nu = prob.nx, prob.nu
    rng = np.random.default_rng(23)
    x0s = _x0s(prob, batch)
    gx = np.asfortranarray(x0s + rng.uniform(0.0, 1.0, batch)[None, :] * 0.3 * rng.standard_normal((nx, batch)))
    gu = np.asfortranarray(0.02 * rng.standard_normal((nu, batch)))
    xlo, xhi = np.full((nx, batch), -10.0), np.full((nx, batch), 10.0)
    ulo, uhi = np.repeat(prob.u_min[:, None], batch, axis=1), np.repeat(prob.u_max[:, None], batch, axis=1)
    for b in range(0, batch, 2):  # the box ends 0.05 short of x0 in one position coordinate
        c = b % 3
        if b % 4 == 0:
            xlo[c, b] = x0s[c, b] + 0.05
        else:
            xhi[c, b] = x0s[c, b] - 0.05
    qx, ru = rng.uniform(0.5, 2.0, nx), rng.uniform(0.5, 2.0, nu)

    def handle():
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, **SETTINGS)
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        s.set_x_ref_batch(gx)
        s.set_u_ref_batch(gu)
        s.set_bound_constraints_batch(np.asfortranarray(xlo), np.asfortranarray(xhi), np.asfortranarray(ulo), np.asfortranarray(uhi))
        s.set_x0_batch(x0s)
        return s

    first = handle()
    first_logs = first.rollout(TICKS)
    first.reset()
    err = np.abs(first_logs["x"][:, :TICKS, :] - gx[:, None, :]).max(axis=(0, 1))  # every instance's worst |e| over the run
    tol = float(np.median(err))
    s = handle()
    s.set_rollout_metrics(qx, ru, tol)
    logs = s.rollout(TICKS)
    got = as_rows(s.rollout_metrics())
    _assert_logs_equal(first_logs, logs)
    rep = lambda v, n: np.repeat(v[:, None, :], n, axis=1)
    want = restate(logs["x"], logs["u"], logs["iter"], logs["status"], rep(gx, TICKS), rep(gu, TICKS), (xlo, xhi), (ulo, uhi), qx, ru, tol)
    print("goals and boxes, batch %d: settle_tol %.4g; settle steps %s; instances with a breached box %d of %d (worst %.3g)"
          % (batch, tol, np.unique(want[:, 7]), int((want[:, 2] > 0).sum()), batch, want[:, 2].max()))
    for slot in (2, 7):  # both outcomes occur, in the restatement
        assert (want[:, slot] != 0).any() and (want[:, slot] == 0).any(), NAMES[slot]
    assert (want[0::2, 2] > 0.049).all()  # (0.05 up to the rounding of x0 + 0.05 - x0)
    for i, k in enumerate(NAMES):
        np.testing.assert_array_equal(got[:, i], want[:, i], err_msg=k)
    # the shared reference and the shared box would have given other rows: the per-instance operands are what was read
    shared_box = (np.repeat(prob.x_min[:, None], batch, axis=1), np.repeat(prob.x_max[:, None], batch, axis=1))
    other = restate(logs["x"], logs["u"], logs["iter"], logs["status"], np.zeros((nx, TICKS, batch)), np.zeros((nu, TICKS, batch)),
                    shared_box, (ulo, uhi), qx, ru, tol)
    assert (other[:, 1] != want[:, 1]).all() and (other[:, 2] != want[:, 2]).any()
    s.reset()


# ------------------------------------------------------------------------------------------------ 5. the getters
@pytest.mark.parametrize("batch", [37, 300])
def test_device_pointer_matches_the_host_getter(pkg, batch):
    lib, L = pkg.load_library(), pkg._lib
    prob, s = _quad(pkg, batch)
    s.set_rollout_metrics(settle_tol=SETTLE_TOL)
    s.rollout(TICKS, log=())
    m = s.rollout_metrics()
    assert m["steps"].dtype == np.int64 and m["cost"].dtype == np.float64 and m["settle"].dtype == np.int64 and m["cost"].shape == (batch,)
    host = np.zeros((batch, 8))
    assert lib.tinympc_get_rollout_metrics(s._h, host.ctypes.data_as(L.c_double_p)) == 0
    np.testing.assert_array_equal(host, as_rows(m))
    rows = L.c_double_p()
    assert lib.tinympc_get_rollout_metrics_device_ptr(s._h, C.byref(rows)) == 0 and rows
    s.synchronize()
    dev = _Device(pkg)
    np.testing.assert_array_equal(dev.get_raw(C.cast(rows, C.c_void_p), host), host)
    torch = _torch_gpu()
    if torch is not None:
        t = s.rollout_metrics(device=True)
        assert tuple(t.shape) == (batch, 8) and t.dtype == torch.float64 and t.is_cuda
        np.testing.assert_array_equal(t.cpu().numpy(), host)
    # the pointer is the rows: the next steps move what it shows
    s.rollout(2, log=())
    s.synchronize()
    np.testing.assert_array_equal(dev.get_raw(C.cast(rows, C.c_void_p), host)[:, 0], np.full(batch, TICKS + 2))
    s.reset()


# ------------------------------------------------------------------------------------------------ 6. refusals change nothing
def test_refusals_change_nothing(pkg):
    batch = 37
    lib, L = pkg.load_library(), pkg._lib
    prob, s = _quad(pkg, batch)
    _, twin = _quad(pkg, batch)
    nx, nu = prob.nx, prob.nu
    dp = lambda a: a.ctypes.data_as(L.c_double_p)
    qx, ru = np.ones(nx), np.ones(nu)
    host = np.full((batch, 8), -7.0)
    rows = L.c_double_p()
    for h in (s, twin):
        h.solve()
    snap = _snapshot(s)
    E = L.ERR_INVALID_INPUT
    # while the metrics are off: get, reset and device_ptr
    assert lib.tinympc_get_rollout_metrics(s._h, dp(host)) == E
    assert "metrics are off" in L.last_error()
    assert lib.tinympc_reset_rollout_metrics(s._h) == E
    assert lib.tinympc_get_rollout_metrics_device_ptr(s._h, C.byref(rows)) == E
    assert (host == -7.0).all() and not rows
    # NULL weights, weights that are negative or not finite, a settle_tol that is not finite
    bad_q, neg_r, inf_q = qx.copy(), ru.copy(), qx.copy()
    bad_q[3], neg_r[nu - 1], inf_q[0] = np.nan, -1e-3, np.inf
    scores = [None, L.RolloutScore(None, dp(ru), 0.1), L.RolloutScore(dp(qx), None, 0.1), L.RolloutScore(dp(bad_q), dp(ru), 0.1),
              L.RolloutScore(dp(qx), dp(neg_r), 0.1), L.RolloutScore(dp(inf_q), dp(ru), 0.1), L.RolloutScore(dp(qx), dp(ru), np.nan),
              L.RolloutScore(dp(qx), dp(ru), np.inf)]
    for i, sc in enumerate(scores):
        assert lib.tinympc_set_rollout_metrics(s._h, C.byref(sc) if sc is not None else None) == E, i
        assert lib.tinympc_get_rollout_metrics(s._h, dp(host)) == E, i  # (still off)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_rollout_metrics(qx=-qx)
    assert ei.value.code == E
    _assert_unchanged(s, snap, "off")
    # on: a refused re-weighting leaves the weights, the tolerance and the rows as they are
    s.set_rollout_metrics(qx, ru, 0.1)
    twin.set_rollout_metrics(qx, ru, 0.1)
    s.rollout(2, log=())
    twin.rollout(2, log=())
    before = as_rows(s.rollout_metrics())
    for i, sc in enumerate(scores):
        assert lib.tinympc_set_rollout_metrics(s._h, C.byref(sc) if sc is not None else None) == E, i
    assert lib.tinympc_get_rollout_metrics(s._h, None) == E
    assert lib.tinympc_get_rollout_metrics_device_ptr(s._h, None) == E
    np.testing.assert_array_equal(as_rows(s.rollout_metrics()), before)
    s.rollout(2, log=())
    twin.rollout(2, log=())
    np.testing.assert_array_equal(as_rows(s.rollout_metrics()), as_rows(twin.rollout_metrics()))
    # x0 and the ADMM state too: one more solve on the handle and on its twin, which saw none of the refused calls
    s.solve()
    twin.solve()
    a, b = _snapshot(s), _snapshot(twin)
    for k in a[0]:
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    s.reset()
    twin.reset()


def test_single_instance_handles_and_sessions_are_refused(pkg):
    lib, L = pkg.load_library(), pkg._lib
    prob = pkg.problems.cartpole(10, True)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho, **SETTINGS)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x0(prob.x0)
    s.solve()
    before = (s.get_solution(), s.get_stats())
    qx, ru = np.ones(prob.nx), np.ones(prob.nu)
    score = L.RolloutScore(qx.ctypes.data_as(L.c_double_p), ru.ctypes.data_as(L.c_double_p), 0.1)
    host = np.full((1, 8), -7.0)
    rows = L.c_double_p()
    calls = (lambda: lib.tinympc_set_rollout_metrics(s._h, C.byref(score)), lambda: lib.tinympc_reset_rollout_metrics(s._h),
             lambda: lib.tinympc_clear_rollout_metrics(s._h), lambda: lib.tinympc_get_rollout_metrics(s._h, host.ctypes.data_as(L.c_double_p)),
             lambda: lib.tinympc_get_rollout_metrics_device_ptr(s._h, C.byref(rows)))
    for i, call in enumerate(calls):
        assert call() == L.ERR_UNSUPPORTED, i
        assert "batched handles outside a session only" in L.last_error(), i
    after = (s.get_solution(), s.get_stats())
    np.testing.assert_array_equal(before[0]["controls"], after[0]["controls"])
    assert before[1]["iter"] == after[1]["iter"]
    s.session_begin()
    u_in = s.session_step(prob.x0)
    for i, call in enumerate(calls):
        assert call() == L.ERR_UNSUPPORTED, i
    np.testing.assert_array_equal(s.session_step(prob.x0).shape, u_in.shape)  # (the session is still open and answers)
    s.session_end()
    assert (host == -7.0).all() and not rows
    s.reset()

"""Reference tracks (tinympc_set_x_ref_track_batch / _u_ref_track_batch, the step verbs, auto-advance): instance b at step k solves
exactly what it solves after set_x_ref_batch / set_u_ref_batch with columns min(k+i, T-1) of its track -- checked against the oracle
per instance, bit for bit against a twin handle that receives every window by hand (plain, with per-instance bounds, with per-instance
models and rho), across the step verbs, the mode rules, the refusals of per-instance references, single-instance handles (launched
and inside a session) and device input.

Shapes: the smallest that put several instances with different steps into one wavefront and leave a ragged last group -- 16 lanes
per instance (quadrotor, N = 10, 37 instances), 32 (24/8, N = 8, 5 instances), 64 (48/16, N = 6, 3 instances)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O
from test_instance_bounds_gpu import _DeviceArrays
from test_instance_refs_gpu import _wide

pytestmark = pytest.mark.gpu

TOL = 1e-9
SETTINGS = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)

CASES = {  # name -> (problem, batch)
    "quadrotor": (lambda P: P.quadrotor(10), 37),
    "wide32": (lambda P: _wide(P, 24, 8, 8), 5),
    "wide64": (lambda P: _wide(P, 48, 16, 6), 3),
}


def _solver(pkg, prob, batch, settings=SETTINGS):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    return s


def _tracks(prob, batch, Tx, Tu, seed=1):
    """-> X nx x Tx x batch, U nu x Tu x batch: every instance its own, every knot different."""
    rng = np.random.default_rng(seed)
    gx, gu = 0.4 * rng.standard_normal((prob.nx, batch)), 0.05 * rng.standard_normal((prob.nu, batch))
    tx, tu = np.arange(Tx), np.arange(Tu)
    X = gx[:, None, :] * (1.0 + 0.5 * np.sin(0.37 * tx[None, :, None] + np.arange(prob.nx)[:, None, None] + np.arange(batch)[None, None, :]))
    U = gu[:, None, :] * np.cos(0.29 * tu[None, :, None] + np.arange(batch)[None, None, :])
    return np.asfortranarray(X), np.asfortranarray(U)


def _windows(X, U, steps, N):
    """The windows the contract names: X_b[:, min(k+i, Tx-1)], i < N, and U_b[:, min(k+i, Tu-1)], i < N-1."""
    batch = X.shape[2]
    wx = np.zeros((X.shape[0], N, batch), order="F")
    wu = np.zeros((U.shape[0], N - 1, batch), order="F")
    for b in range(batch):
        k = int(steps[b])
        wx[:, :, b] = X[:, np.minimum(k + np.arange(N), X.shape[1] - 1), b]
        wu[:, :, b] = U[:, np.minimum(k + np.arange(N - 1), U.shape[1] - 1), b]
    return wx, wu


def _steps(batch, T, N, seed=0):
    """Per instance from {0, 1, T-N, T-1, T+5}, clipped at 0; neighbours differ (several steps inside one wavefront)."""
    choices = np.maximum(np.array([0, 1, T - N, T - 1, T + 5]), 0)
    return choices[(np.arange(batch) + seed) % 5].astype(np.int32)


def _x0s(prob, batch, scale=1.0, seed=2):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(prob.x0[:, None] * scale + 0.2 * rng.standard_normal((prob.nx, batch)))


def _same(a, b, tag=""):
    sa, sb = a.get_solution_batch(), b.get_solution_batch()
    ta, tb = a.get_stats_batch(), b.get_stats_batch()
    np.testing.assert_array_equal(sa["states"], sb["states"], err_msg=str(tag))
    np.testing.assert_array_equal(sa["controls"], sb["controls"], err_msg=str(tag))
    for k in ta:
        np.testing.assert_array_equal(ta[k], tb[k], err_msg="%s %s" % (tag, k))


def _bits(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["residuals"].copy()


def _cold_solve(s, x0s):
    s.reset_workspace()
    s.set_x0_batch(x0s)
    s.solve()
    return _bits(s)


def _equal_bits(a, b, tag=""):
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q, err_msg=str(tag))


def _torch():
    """The torch legs are extras: everything they check also runs on raw device buffers (_DeviceBuffers), torch or not."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the GPU")
    return torch


class _DeviceBuffers(_DeviceArrays):
    """_DeviceArrays (device memory through the HIP runtime the library itself uses) with int32 buffers and overwriting."""

    def put_ints(self, a):
        h = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(h.nbytes, 4)) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemcpy(p, C.c_void_p(h.ctypes.data), h.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p

    def overwrite(self, p, nbytes):
        """The caller's buffer may be overwritten as soon as a verb has returned."""
        junk = np.full(nbytes, 0x5A, dtype=np.uint8)
        assert self.hip.hipMemcpy(p, C.c_void_p(junk.ctypes.data), nbytes, 1) == 0


# ------------------------------------------------------------------------------------------------------------ 1. oracle per instance
@pytest.mark.parametrize("lengths", ["N-3,N-3", "N,3N", "3N,N", "3N,1", "N-3,3N"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_instance_matches_the_oracle_at_its_own_step(pkg, case, lengths):
    prob, batch = CASES[case][0](pkg.problems), CASES[case][1]
    N = prob.N
    Tx, Tu = ({"N-3": N - 3, "N": N, "3N": 3 * N, "1": 1}[t] for t in lengths.split(","))
    X, U = _tracks(prob, batch, Tx, Tu)
    steps = _steps(batch, Tx, N)
    s = _solver(pkg, prob, batch)
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    s.set_ref_step_batch(steps)
    samples = sorted({0, 1, 2, batch - 1})  # first, last, and neighbours inside one wavefront (their steps differ)
    assert steps[0] != steps[1] and steps[1] != steps[2]
    orcs = {b: O.OraclePort(prob).load_problem(prob, SETTINGS) for b in samples}
    for rnd in range(3):  # a cold start, then two warm ticks after advance_ref_step(1)
        if rnd:
            s.advance_ref_step(1)
        np.testing.assert_array_equal(s.get_ref_step_batch(), steps + rnd)
        wx, wu = _windows(X, U, steps + rnd, N)
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        sol, st = s.get_solution_batch(), s.get_stats_batch()
        for b, orc in orcs.items():
            orc.set_x_ref(wx[:, :, b])
            orc.set_u_ref(wu[:, :, b])
            orc.set_x0(x0s[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (case, lengths, rnd, b)
            assert st["status"][b] == orc.stats()["status"], (case, lengths, rnd, b)
            assert rel_err(sol["states"][:, :, b], orc.solution()[0]) < TOL, (case, lengths, rnd, b)
            assert rel_err(sol["controls"][:, :, b], orc.solution()[1]) < TOL, (case, lengths, rnd, b)
    assert s.launch_info()["layout"] == "A" and "reference-track" in s.jit_info()
    s.reset()


# ------------------------------------------------------------------------------------------- 2. bit-identical to windows sent by hand
def _instance_bounds(prob, batch, seed=3):
    """Per-knot bounds per instance: the problem's box (or +-2 / +-0.3), scaled per instance and per knot."""
    rng = np.random.default_rng(seed)
    nx, nu, N = prob.nx, prob.nu, prob.N
    xlo = prob.x_min if prob.x_min is not None else np.full(nx, -2.0)
    xhi = prob.x_max if prob.x_max is not None else np.full(nx, 2.0)
    ulo = prob.u_min if prob.u_min is not None else np.full(nu, -0.3)
    uhi = prob.u_max if prob.u_max is not None else np.full(nu, 0.3)
    fx, fu = rng.uniform(0.6, 1.0, (1, N, batch)), rng.uniform(0.6, 1.0, (1, N - 1, batch))
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1)[:, None, None]
    return (np.asfortranarray(col(xlo) * fx), np.asfortranarray(col(xhi) * fx), np.asfortranarray(col(ulo) * fu), np.asfortranarray(col(uhi) * fu))


def _instance_models(prob, batch, seed=4):
    rng = np.random.default_rng(seed)
    nx, nu = prob.nx, prob.nu
    A = prob.A[:, :, None] * (1.0 + 0.01 * rng.standard_normal((nx, nx, batch)))
    B = prob.B[:, :, None] * (1.0 + 0.05 * rng.standard_normal((nx, nu, batch)))
    Q = prob.Q[:, :, None] * rng.uniform(0.5, 2.0, (1, 1, batch))
    R = prob.R[:, :, None] * rng.uniform(0.5, 2.0, (1, 1, batch))
    return A, B, Q, R, prob.rho * rng.uniform(0.5, 2.0, batch)


@pytest.mark.parametrize("with_", ["plain", "bounds", "models"])
@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_windows_sent_by_hand(pkg, case, with_):
    prob, batch = CASES[case][0](pkg.problems), CASES[case][1]
    N = prob.N
    X, U = _tracks(prob, batch, 3 * N, N, seed=5)
    steps = _steps(batch, 3 * N, N, seed=1)
    s, twin = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    for h in (s, twin):
        if with_ == "bounds":
            h.set_bound_constraints_batch(*_instance_bounds(prob, batch))
        if with_ == "models":
            A, B, Q, R, rho = _instance_models(prob, batch)
            h.set_model_batch(A, B, Q, R)
            h.set_rho_batch(rho)
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    s.set_ref_step_batch(steps)
    x = _x0s(prob, batch)
    for k in range(8):
        wx, wu = _windows(X, U, steps + k, N)
        twin.set_x_ref_batch(wx)
        twin.set_u_ref_batch(wu)
        u = s.mpc_step(x)
        ut = twin.mpc_step(x)
        np.testing.assert_array_equal(u, ut, err_msg=str(k))
        _same(s, twin, (case, with_, k))
        s.advance_ref_step(1)
        x = np.asfortranarray(prob.A @ x + prob.B @ np.clip(u, -1.0, 1.0))
    info = s.jit_info()
    assert s.launch_info()["layout"] == twin.launch_info()["layout"] == "A"
    assert "reference-track" in info and "per-instance-refs" in info and "reference-track" not in twin.jit_info()
    assert ("per-instance-bounds" in info) == (with_ == "bounds") and ("per-instance-models" in info) == (with_ == "models")
    s.reset()
    twin.reset()


# -------------------------------------------------------------------------------------------------------------------------- 3. steps
def test_step_verbs_advance_and_auto_advance(pkg):
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    N, T = prob.N, 3 * prob.N
    X, U = _tracks(prob, batch, T, T - 4, seed=6)
    s, twin = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    np.testing.assert_array_equal(s.get_ref_step_batch(), np.zeros(batch, dtype=np.int32))  # steps start at 0
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    want = np.zeros(batch, dtype=np.int32)
    s.set_ref_step_batch([3, 1, 4, 1, 5], first=6)  # a sub-range, inside and across wavefronts
    want[6:11] = [3, 1, 4, 1, 5]
    np.testing.assert_array_equal(s.get_ref_step_batch(), want)
    np.testing.assert_array_equal(s.get_ref_step_batch(8, 3), want[8:11])
    s.advance_ref_step(2)
    want += 2
    np.testing.assert_array_equal(s.get_ref_step_batch(), want)
    s.advance_ref_step(-2)
    want -= 2
    np.testing.assert_array_equal(s.get_ref_step_batch(), want)
    with pytest.raises(pkg.TinyMPCError) as ei:  # some step would go below 0: nothing moves
        s.advance_ref_step(-1)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    np.testing.assert_array_equal(s.get_ref_step_batch(), want)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_ref_auto_advance(-1)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    # the advance saturates, it does not wrap
    s.set_ref_step_batch([2**31 - 3], first=batch - 1)
    s.advance_ref_step(7)
    assert s.get_ref_step_batch(batch - 1, 1)[0] == 2**31 - 1 and s.get_ref_step_batch(0, 1)[0] == want[0] + 7
    s.advance_ref_step(-7)
    want[batch - 1] = 2**31 - 1 - 7
    np.testing.assert_array_equal(s.get_ref_step_batch(), want)
    # a step far beyond T gives the bits of step T-1 (here T-1 of the longer track: both halves hold their last knot)
    x0s = _x0s(prob, batch)
    s.set_ref_step_batch(np.full(batch, T - 1, dtype=np.int32))
    at_end = _cold_solve(s, x0s)
    s.set_ref_step_batch(np.full(batch, 2**31 - 1, dtype=np.int32))
    _equal_bits(_cold_solve(s, x0s), at_end, "beyond the end")
    wx, wu = _windows(X, U, np.full(batch, T - 1), N)
    twin.set_x_ref_batch(wx)
    twin.set_u_ref_batch(wu)
    _equal_bits(_cold_solve(twin, x0s), at_end, "the held last knot")
    # auto-advance: the step moves AFTER the tick's solve
    base = _steps(batch, T, N, seed=2)
    s.set_ref_step_batch(base)
    s.set_ref_auto_advance(1)
    for h in (s, twin):
        h.reset_workspace()
    x = x0s
    for k in range(4):
        wx, wu = _windows(X, U, base + k, N)
        twin.set_x_ref_batch(wx)
        twin.set_u_ref_batch(wu)
        u = s.mpc_step(x)
        np.testing.assert_array_equal(u, twin.mpc_step(x), err_msg=str(k))
        _same(s, twin, ("auto", k))
        np.testing.assert_array_equal(s.get_ref_step_batch(), base + k + 1)
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
    s.set_ref_auto_advance(0)
    s.mpc_step(x)
    np.testing.assert_array_equal(s.get_ref_step_batch(), base + 4)
    # reset_workspace (and update_settings) keep tracks and steps
    s.reset_workspace()
    s.update_settings(max_iter=80)
    twin.update_settings(max_iter=80)
    np.testing.assert_array_equal(s.get_ref_step_batch(), base + 4)
    wx, wu = _windows(X, U, base + 4, N)
    twin.set_x_ref_batch(wx)
    twin.set_u_ref_batch(wu)
    _equal_bits(_cold_solve(s, x0s), _cold_solve(twin, x0s), "after reset")
    s.reset()
    twin.reset()


def test_device_steps_from_raw_device_memory(pkg):
    """tinympc_set_ref_step_batch_device on device buffers of the library's own HIP runtime: a sub-range and the whole batch give the
    steps and the bits of host input; a negative entry is refused on the device, steps and solve unchanged."""
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    N, T = prob.N, 2 * prob.N
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    X, U = _tracks(prob, batch, T, T - 2, seed=7)
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    dev = _DeviceBuffers(pkg)
    steps = _steps(batch, T, N, seed=3)
    for q in (h, d):
        q.set_x_ref_track_batch(X)
        q.set_u_ref_track_batch(U)
    x0s = _x0s(prob, batch)
    # a sub-range: inside and across wavefronts, a ragged end
    h.set_ref_step_batch(steps[4:30], first=4)
    p = dev.put_ints(steps[4:30])
    assert L.tinympc_set_ref_step_batch_device(d._h, p, 4, 26) == 0, pkg._lib.last_error()
    dev.overwrite(p, 4 * 26)
    want = np.zeros(batch, dtype=np.int32)
    want[4:30] = steps[4:30]
    np.testing.assert_array_equal(h.get_ref_step_batch(), want)
    np.testing.assert_array_equal(d.get_ref_step_batch(), want)
    _equal_bits(_cold_solve(h, x0s), _cold_solve(d, x0s), "sub-range")
    # the whole batch, steps beyond the end included
    h.set_ref_step_batch(steps)
    p = dev.put_ints(steps)
    assert L.tinympc_set_ref_step_batch_device(d._h, p, 0, batch) == 0, pkg._lib.last_error()
    dev.overwrite(p, 4 * batch)
    np.testing.assert_array_equal(d.get_ref_step_batch(), steps)
    before = _cold_solve(h, x0s)
    _equal_bits(before, _cold_solve(d, x0s), "whole batch")
    # a negative entry anywhere in the range: refused by the kernel's flag, nothing written
    for bad, first in (([3, 0, -1, 7], 9), ([-5], batch - 1), (np.r_[np.zeros(batch - 1, dtype=np.int32), -1], 0)):
        p = dev.put_ints(bad)
        assert L.tinympc_set_ref_step_batch_device(d._h, p, first, len(bad)) == E, (bad, first)
        assert "step" in pkg._lib.last_error()
        np.testing.assert_array_equal(d.get_ref_step_batch(), steps)
        _equal_bits(_cold_solve(d, x0s), before, "after the refused steps")
    assert L.tinympc_set_ref_step_batch_device(d._h, dev.put_ints(steps), batch - 2, 4) == E  # a range beyond the batch
    assert L.tinympc_set_ref_step_batch_device(d._h, None, 0, 4) == E
    np.testing.assert_array_equal(d.get_ref_step_batch(), steps)
    # advancing steps that came from the device
    for q in (h, d):
        q.advance_ref_step(2)
    np.testing.assert_array_equal(d.get_ref_step_batch(), h.get_ref_step_batch())
    _equal_bits(_cold_solve(h, x0s), _cold_solve(d, x0s), "advanced")
    dev.free()
    h.reset()
    d.reset()


def test_tracks_and_steps_from_raw_device_memory_match_host_input(pkg):
    """Tracks (whole batch, then a sub-range) and steps through the _device verbs from raw device buffers, overwritten right after
    each call: the bits of host input over closed-loop ticks."""
    prob, batch = CASES["wide32"][0](pkg.problems), CASES["wide32"][1]
    N, T = prob.N, 3 * prob.N
    L = pkg.load_library()
    X, U = _tracks(prob, batch, T, N - 3, seed=18)
    steps = _steps(batch, T, N, seed=6)
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    dev = _DeviceBuffers(pkg)
    h.set_x_ref_track_batch(X)
    h.set_u_ref_track_batch(U)
    h.set_ref_step_batch(steps)
    px, pu, ps = dev.put(X), dev.put(U), dev.put_ints(steps)
    assert L.tinympc_set_x_ref_track_batch_device(d._h, px, prob.nx, T, 0, batch) == 0, pkg._lib.last_error()
    assert L.tinympc_set_u_ref_track_batch_device(d._h, pu, prob.nu, N - 3, 0, batch) == 0, pkg._lib.last_error()
    assert L.tinympc_set_ref_step_batch_device(d._h, ps, 0, batch) == 0, pkg._lib.last_error()
    dev.overwrite(px, X.nbytes)
    dev.overwrite(pu, U.nbytes)
    dev.overwrite(ps, steps.nbytes)
    x = _x0s(prob, batch)
    for k in range(3):
        np.testing.assert_array_equal(h.mpc_step(x), d.mpc_step(x), err_msg=str(k))
        _same(h, d, k)
        for q in (h, d):
            q.advance_ref_step(1)
    X2, _ = _tracks(prob, batch, T, N - 3, seed=19)
    h.set_x_ref_track_batch(np.asfortranarray(X2[:, :, 1:4]), first=1)
    p2 = dev.put(np.asfortranarray(X2[:, :, 1:4]))
    assert L.tinympc_set_x_ref_track_batch_device(d._h, p2, prob.nx, T, 1, 3) == 0, pkg._lib.last_error()
    dev.overwrite(p2, 8 * prob.nx * T * 3)
    _equal_bits(_cold_solve(h, x), _cold_solve(d, x), "sub-range")
    dev.free()
    h.reset()
    d.reset()


def test_device_steps_match_host_steps(pkg):
    torch = _torch()
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    N, T = prob.N, 2 * prob.N
    X, U = _tracks(prob, batch, T, T, seed=7)
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    steps = _steps(batch, T, N, seed=3)
    for q in (h, d):
        q.set_x_ref_track_batch(X)
        q.set_u_ref_track_batch(U)
    h.set_ref_step_batch(steps[4:30], first=4)
    t = torch.from_numpy(steps[4:30].copy()).cuda()
    d.set_ref_step_batch(t, first=4)
    t.fill_(12345)  # the caller's tensor may be overwritten as soon as the call has returned
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.get_ref_step_batch(), h.get_ref_step_batch())
    x0s = _x0s(prob, batch)
    _equal_bits(_cold_solve(h, x0s), _cold_solve(d, x0s))
    h.reset()
    d.reset()


# --------------------------------------------------------------------------------------------------------------------- 4. mode rules
def test_invalid_calls_change_nothing(pkg):
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    nx, nu, N, T = prob.nx, prob.nu, prob.N, 2 * prob.N
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    X, U = _tracks(prob, batch, T, T, seed=8)
    other, _ = _tracks(prob, batch, T + 3, T, seed=9)
    x0s = _x0s(prob, batch)
    ptr = lambda a: a.ctypes.data_as(pkg._lib.c_double_p)
    # a first call on a sub-range
    s = _solver(pkg, prob, batch)
    before = _cold_solve(s, x0s)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_x_ref_track_batch(np.asfortranarray(X[:, :, 2:9]), first=2)
    assert ei.value.code == E and "whole batch" in str(ei.value)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_u_ref_track_batch(np.asfortranarray(U[:, :, :batch - 1]))
    assert ei.value.code == E
    assert "reference-track" not in s.jit_info() and "per-instance-refs" not in s.jit_info()
    _equal_bits(_cold_solve(s, x0s), before, "first call on a sub-range")
    # ... and with both halves in track mode
    steps = _steps(batch, T, N, seed=4)
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    s.set_ref_step_batch(steps)
    before = _cold_solve(s, x0s)
    assert not np.array_equal(before[1], np.zeros_like(before[1]))
    host_steps = np.full(4, -1, dtype=np.int32)
    bad_calls = {
        "a sub-range with another T": lambda: L.tinympc_set_x_ref_track_batch(s._h, ptr(np.asfortranarray(other[:, :, 3:8])), nx, T + 3, 3, 5),
        "T = 0": lambda: L.tinympc_set_x_ref_track_batch(s._h, ptr(other), nx, 0, 0, batch),
        "T = 0 (u)": lambda: L.tinympc_set_u_ref_track_batch(s._h, ptr(other), nu, 0, 0, batch),
        "wrong rows": lambda: L.tinympc_set_x_ref_track_batch(s._h, ptr(other), nx + 1, T, 0, batch),
        "a range beyond the batch": lambda: L.tinympc_set_x_ref_track_batch(s._h, ptr(other), nx, T, batch - 2, 4),
        "NULL": lambda: L.tinympc_set_x_ref_track_batch(s._h, None, nx, T, 0, batch),
        "a negative step": lambda: L.tinympc_set_ref_step_batch(s._h, host_steps.ctypes.data_as(pkg._lib.c_int_p), 5, 4),
        "steps beyond the batch": lambda: L.tinympc_set_ref_step_batch(s._h, host_steps.ctypes.data_as(pkg._lib.c_int_p), batch - 2, 4),
        "host memory as device tracks": lambda: L.tinympc_set_x_ref_track_batch_device(s._h, C.c_void_p(other.ctypes.data), nx, T, 0, batch),
        "host memory as device tracks (u)": lambda: L.tinympc_set_u_ref_track_batch_device(s._h, C.c_void_p(other.ctypes.data), nu, T, 0, batch),
        "host memory as device steps": lambda: L.tinympc_set_ref_step_batch_device(s._h, C.c_void_p(host_steps.ctypes.data), 5, 4),
        "a sub-range set_x_ref_batch in track mode": lambda: L.tinympc_set_x_ref_batch(s._h, ptr(other), nx, N, 2, 5),
        "a sub-range set_u_ref_batch in track mode": lambda: L.tinympc_set_u_ref_batch(s._h, ptr(other), nu, 1, 0, batch - 1),
    }
    for what, call in bad_calls.items():
        assert call() == E, what
        if "_ref_batch in track mode" in what:
            assert "whole batch" in pkg._lib.last_error(), what
        np.testing.assert_array_equal(s.get_ref_step_batch(), steps, err_msg=what)
        _equal_bits(_cold_solve(s, x0s), before, what)
    assert "reference-track" in s.jit_info()
    s.reset()


def test_negative_device_steps_are_refused_on_the_device(pkg):
    torch = _torch()
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    X, U = _tracks(prob, batch, 2 * prob.N, 5, seed=10)
    s = _solver(pkg, prob, batch)
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    steps = _steps(batch, 2 * prob.N, prob.N)
    s.set_ref_step_batch(steps)
    x0s = _x0s(prob, batch)
    before = _cold_solve(s, x0s)
    bad = torch.from_numpy(np.array([3, 0, -1, 7], dtype=np.int32)).cuda()
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_ref_step_batch(bad, first=9)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    for wrong in (bad.to(torch.int64), bad.reshape(2, 2)):
        with pytest.raises(pkg.TinyMPCError) as ei:
            s.set_ref_step_batch(wrong)
        assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    np.testing.assert_array_equal(s.get_ref_step_batch(), steps)
    _equal_bits(_cold_solve(s, x0s), before)
    s.reset()


def test_leaving_the_mode_and_replacing_tracks(pkg):
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    N, T = prob.N, 2 * prob.N
    X, U = _tracks(prob, batch, T, T, seed=11)
    steps = _steps(batch, T, N, seed=5)
    x0s = _x0s(prob, batch)
    s, never = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    s.set_x_ref_track_batch(X)
    s.set_ref_step_batch(steps)
    info = s.jit_info()
    assert "reference-track" in info and "per-instance-refs" in info and s.launch_info()["layout"] == "A"
    # x in track mode, u shared: the windows of x alone
    wx, wu = _windows(X, U, steps, N)
    never.set_x_ref_batch(wx)
    _equal_bits(_cold_solve(s, x0s), _cold_solve(never, x0s), "x only")
    # a sub-range with the same T replaces those instances' tracks and keeps the steps; a whole-batch call may change T
    X2, _ = _tracks(prob, batch, T, T, seed=12)
    s.set_x_ref_track_batch(np.asfortranarray(X2[:, :, 5:23]), first=5)
    mixed = X.copy()
    mixed[:, :, 5:23] = X2[:, :, 5:23]
    np.testing.assert_array_equal(s.get_ref_step_batch(), steps)
    never.set_x_ref_batch(_windows(mixed, U, steps, N)[0])
    _equal_bits(_cold_solve(s, x0s), _cold_solve(never, x0s), "sub-range replaced")
    for Tn in (T + 7, 3):  # longer (a new store), shorter (the store is reused)
        X3, _ = _tracks(prob, batch, Tn, T, seed=13 + Tn)
        s.set_x_ref_track_batch(X3)
        np.testing.assert_array_equal(s.get_ref_step_batch(), steps)
        never.set_x_ref_batch(_windows(X3, U, steps, N)[0])
        _equal_bits(_cold_solve(s, x0s), _cold_solve(never, x0s), "T = %d" % Tn)
    # a whole-batch set_x_ref_batch returns the half to plain per-instance references
    s.set_u_ref_track_batch(U)
    never.set_u_ref_batch(wu)
    fresh = np.asfortranarray(0.5 * wx)
    for h in (s, never):
        h.set_x_ref_batch(fresh)
    assert "reference-track" in s.jit_info()  # (u is still a track)
    _equal_bits(_cold_solve(s, x0s), _cold_solve(never, x0s), "x back to per-instance references")
    s.set_x_ref_batch(np.asfortranarray(fresh[:, :, 3:6]), first=3)  # ... where sub-ranges are welcome again
    never.set_x_ref_batch(np.asfortranarray(fresh[:, :, 3:6]), first=3)
    for h in (s, never):
        h.set_u_ref_batch(np.asfortranarray(2.0 * wu))
    info = s.jit_info()
    assert "reference-track" not in info and "per-instance-refs" in info
    _equal_bits(_cold_solve(s, x0s), _cold_solve(never, x0s), "u back to per-instance references")
    np.testing.assert_array_equal(s.get_ref_step_batch(), steps)  # the steps stay
    # the shared verbs return a half in track mode to shared references
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    assert "reference-track" in s.jit_info()
    shared_x, shared_u = 0.1 * np.ones((prob.nx, N)), 0.01 * np.ones((prob.nu, N - 1))
    plain = _solver(pkg, prob, batch)
    for h in (s, plain):
        h.set_x_ref(shared_x)
        h.set_u_ref(shared_u)
    info = s.jit_info()
    assert "reference-track" not in info and "per-instance-refs" not in info
    a, b = _cold_solve(s, x0s), _cold_solve(plain, x0s)
    assert s.launch_info()["layout"] == plain.launch_info()["layout"]
    _equal_bits(a, b, "shared again")
    for h in (s, never, plain):
        h.reset()


def test_a_track_of_one_knot_stays_on_layout_a(pkg):
    """Goals per instance run on layout D's goal form at this shape and batch; a T = 1 track holds the same references and does not."""
    prob, batch = pkg.problems.quadrotor(50), 1301
    rng = np.random.default_rng(14)
    gx = 0.4 * rng.standard_normal((prob.nx, batch))
    x0s = _x0s(prob, batch)
    goal, track = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    goal.set_x_ref_batch(gx)
    track.set_x_ref_track_batch(np.asfortranarray(gx[:, None, :]))
    for h in (goal, track):
        h.set_x0_batch(x0s)
        h.solve()
    assert goal.launch_info()["layout"] == "D" and track.launch_info()["layout"] == "A"
    assert "goal" not in track.jit_info() and "reference-track" in track.jit_info()
    np.testing.assert_array_equal(track.get_stats_batch()["status"], goal.get_stats_batch()["status"])
    for h in (goal, track):
        h.reset()


# ----------------------------------------------------------------------------------------------------------------------- 5. refusals
def _expect_unsupported(pkg, call, words="per-instance references"):
    with pytest.raises(pkg.TinyMPCError) as ei:
        call()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    assert words in str(ei.value)


def test_refusals_of_per_instance_references_apply(pkg):
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    X, U = _tracks(prob, batch, 2 * prob.N, 4, seed=15)
    x0s = _x0s(prob, batch)
    s = _solver(pkg, prob, batch)
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    s.set_x0_batch(x0s)
    s.solve()
    good = _bits(s)
    # adaptive rho
    s.update_settings(adaptive_rho=1)
    _expect_unsupported(pkg, s.solve)
    _expect_unsupported(pkg, lambda: s.mpc_step(x0s))
    s.update_settings(adaptive_rho=0)
    _equal_bits(_cold_solve(s, x0s), good, "after adaptive rho")
    # the cone family, then the linear family
    s.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    _expect_unsupported(pkg, s.solve)
    s.update_settings(en_state_soc=0, en_input_soc=0)
    _equal_bits(_cold_solve(s, x0s), good, "after the cones")
    s.set_linear_constraints(np.ones((1, prob.nx)), np.array([50.0]), np.zeros((0, prob.nu)), np.zeros(0))
    _expect_unsupported(pkg, s.solve)
    s.update_settings(en_state_linear=0)
    _equal_bits(_cold_solve(s, x0s), good, "after the linear rows")
    # a session is for single-instance handles
    _expect_unsupported(pkg, s.session_begin, "session")
    _equal_bits(_cold_solve(s, x0s), good, "after session_begin")
    np.testing.assert_array_equal(s.get_ref_step_batch(), np.zeros(batch, dtype=np.int32))
    s.reset()
    # nx + nu > 64: no kernel carries per-instance references
    rng = np.random.default_rng(3)
    nx, nu, N = 60, 8, 6
    big = pkg.problems.Problem("big", np.eye(nx) + 0.01 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), N,
                               2.0, rng.standard_normal(nx))
    s = _solver(pkg, big, 4)
    s.set_x_ref_track_batch(np.zeros((nx, 9, 4)))
    s.set_x0_batch(np.zeros((nx, 4), order="F"))
    _expect_unsupported(pkg, s.solve)
    s.set_x_ref(np.zeros((nx, N)))
    s.solve()
    s.reset()


# ---------------------------------------------------------------------------------------------------------- 6. single-instance handle
@pytest.mark.parametrize("how", ["launched", "session"])
def test_single_instance_track_equals_windows_through_set_x_ref(pkg, how):
    P = pkg.problems
    prob = P.cartpole(10, True)
    N, T = prob.N, 25
    X, U = _tracks(prob, 1, T, T - 3, seed=16)
    a, b = _solver(pkg, prob, 1), _solver(pkg, prob, 1)
    a.set_x_ref_track_batch(X[:, :, 0])  # nx x T
    a.set_u_ref_track_batch(U)           # nu x T x 1
    a.set_ref_step_batch([2])
    assert "reference-track" in a.jit_info() and "per-instance-refs" not in a.jit_info()
    if how == "session":
        for h in (a, b):
            h.session_begin()
    x = prob.x0.copy()
    for k in range(2, 2 + 20):  # ... past the end of both tracks
        assert a.get_ref_step_batch()[0] == k
        wx, wu = _windows(X, U, [k], N)
        b.set_x_ref(wx[:, :, 0])
        b.set_u_ref(wu[:, :, 0])
        if how == "session":
            ua, ub = a.session_step(x), b.session_step(x)
        else:
            ua, ub = a.mpc_step(x)[:, 0], b.mpc_step(x)[:, 0]
        np.testing.assert_array_equal(ua, ub, err_msg=str(k))
        sa, sb = a.get_solution(), b.get_solution()
        np.testing.assert_array_equal(sa["states"], sb["states"], err_msg=str(k))
        np.testing.assert_array_equal(sa["controls"], sb["controls"], err_msg=str(k))
        assert a.get_stats() == b.get_stats(), k
        a.advance_ref_step(1)
        x = prob.A @ x + prob.B @ ua
    if how == "session":
        for h in (a, b):
            h.session_end()
    else:  # auto-advance serves mpc_step of a single-instance handle too
        a.set_ref_auto_advance(2)
        a.mpc_step(x)
        assert a.get_ref_step_batch()[0] == 24
    with pytest.raises(pkg.TinyMPCError) as ei:
        a.advance_ref_step(-1000)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    a.set_x_ref(np.zeros((prob.nx, N)))
    assert "reference-track" in a.jit_info()  # (u is still a track)
    a.set_u_ref(np.zeros((prob.nu, N - 1)))
    assert "reference-track" not in a.jit_info()
    a.reset()
    b.reset()


def test_single_instance_track_with_the_cone_family(pkg):
    """Everything the shared reference verbs work with works with tracks: here the cone family, refused on batched handles."""
    prob = pkg.problems.quadrotor(10)
    X, U = _tracks(prob, 1, 30, 30, seed=17)
    a, b = _solver(pkg, prob, 1), _solver(pkg, prob, 1)
    for h in (a, b):
        h.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    a.set_x_ref_track_batch(X)
    a.set_u_ref_track_batch(U)
    x = prob.x0.copy()
    for k in range(3):
        wx, wu = _windows(X, U, [4 * k], prob.N)
        b.set_x_ref(wx[:, :, 0])
        b.set_u_ref(wu[:, :, 0])
        for h in (a, b):
            h.set_x0(x)
            h.solve()
        np.testing.assert_array_equal(a.get_solution()["controls"], b.get_solution()["controls"], err_msg=str(k))
        a.advance_ref_step(4)
    a.reset()
    b.reset()


# ----------------------------------------------------------------------------------------------------------------- 7. device input
def test_tracks_from_torch_tensors_match_host_input(pkg):
    torch = _torch()
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    N, T = prob.N, 3 * prob.N
    X, U = _tracks(prob, batch, T, N - 3, seed=18)
    steps = _steps(batch, T, N, seed=6)
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    h.set_x_ref_track_batch(X)
    h.set_u_ref_track_batch(U)
    h.set_ref_step_batch(steps)
    tx = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()  # (count, T, nx)
    tu = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
    ts = torch.from_numpy(steps.copy()).cuda()
    d.set_x_ref_track_batch(tx)
    d.set_u_ref_track_batch(tu)
    d.set_ref_step_batch(ts)
    for t in (tx, tu, ts):  # the caller's tensors may be overwritten as soon as the calls have returned
        t.zero_()
    torch.cuda.synchronize()
    x = _x0s(prob, batch)
    for k in range(3):
        np.testing.assert_array_equal(h.mpc_step(x), d.mpc_step(x), err_msg=str(k))
        _same(h, d, k)
        for q in (h, d):
            q.advance_ref_step(1)
    # a sub-range from the device, the same T
    X2, _ = _tracks(prob, batch, T, N - 3, seed=19)
    h.set_x_ref_track_batch(np.asfortranarray(X2[:, :, 7:19]), first=7)
    d.set_x_ref_track_batch(torch.from_numpy(np.ascontiguousarray(X2[:, :, 7:19].T)).cuda(), first=7)
    _equal_bits(_cold_solve(h, x), _cold_solve(d, x), "sub-range")
    # what the library cannot read correctly is refused, not reinterpreted
    for bad in (torch.zeros((batch, T, prob.nx), dtype=torch.float32).cuda(), torch.zeros((prob.nx, T, batch), dtype=torch.float64).cuda(),
                torch.zeros((batch, T), dtype=torch.float64).cuda(), torch.zeros((batch, T, 2 * prob.nx), dtype=torch.float64).cuda()[:, :, ::2]):
        with pytest.raises(pkg.TinyMPCError) as ei:
            d.set_x_ref_track_batch(bad)
        assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    _equal_bits(_cold_solve(h, x), _cold_solve(d, x), "after the refused tensors")
    h.reset()
    d.reset()


def test_tracks_from_another_handles_device_memory(pkg):
    """The _device form on raw device pointers: another handle's device solution (nx x N x batch: tracks of T = N knots)."""
    prob, batch = CASES["quadrotor"][0](pkg.problems), CASES["quadrotor"][1]
    L = pkg.load_library()
    src = _solver(pkg, prob, batch)
    src.set_x0_batch(_x0s(prob, batch, 0.5, seed=4))
    src.solve()
    d_x, d_u = C.c_void_p(), C.c_void_p()
    assert L.tinympc_get_solution_device_ptrs(src._h, C.byref(d_x), C.byref(d_u)) == 0
    sol = src.get_solution_batch()
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    h.set_x_ref_track_batch(sol["states"])
    h.set_u_ref_track_batch(sol["controls"])
    assert L.tinympc_set_x_ref_track_batch_device(d._h, d_x, prob.nx, prob.N, 0, batch) == 0
    assert L.tinympc_set_u_ref_track_batch_device(d._h, d_u, prob.nu, prob.N - 1, 0, batch) == 0
    steps = _steps(batch, prob.N, prob.N, seed=7)
    x0s = _x0s(prob, batch)
    for q in (h, d):
        q.set_ref_step_batch(steps)
    _equal_bits(_cold_solve(h, x0s), _cold_solve(d, x0s))
    for q in (h, d, src):
        q.reset()

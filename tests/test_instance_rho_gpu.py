"""Per-instance ADMM penalty of batched handles (tinympc_set_rho_batch and its _device form): instance b solves what a single-instance
handle set up with (its model, rho_b) would solve -- caches bit-identical to that handle's, every sampled instance against its own
oracle (OraclePort at rho_b), bit for bit against the shared handle where every rho is the shared one; the verb commutes with
tinympc_set_model_batch, survives reset_workspace, reads back through get_rho_batch, and the configurations no kernel carries are
refused, never solved with the shared rho. This file: the verb and layout A; layout D is test_instance_rho_d_gpu.py.

Inputs: rho_b = prob.rho * f_b, f_b log-uniform in [0.5, 4] (seed 11). x0 as the sibling files generate it (`_x0s`), EXCEPT for the
cartpole: from those x0 its input saturates and four of the five sampled instances have the same controls under every rho, so a kernel
that ignored the verb would pass. The cartpole cases use prob.x0 * scale + 0.02 * standard_normal (the sibling files' seed + 3) instead -- the
start scaled as in the sibling files, a tenth of their spread: found on the CPU with the oracle alone; with it every sampled instance differs between
its rho_b and the shared rho (`_guard`, which every oracle test asserts first).
TOL, the sample and the settings are the sibling files'."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, rel_err

import pyoracle as O
from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs, _torch_gpu, _wide
from test_instance_bounds_gpu import _x0s as _x0s_plain
from test_instance_models_gpu import SETTINGS, TOL, _models, _oracle, _same, _sample, _set_models, _solver

pytestmark = pytest.mark.gpu

CASES = {  # name -> (problem, batch)
    "cartpole20": (lambda P: P.cartpole(20, True), 37),
    "wide32": (lambda P: _wide(P, 24, 8, 20), 37),
    "wide64": (lambda P: _wide(P, 48, 16, 12), 21),
    "quadrotor120": (lambda P: P.quadrotor(120), 70),
    "quadrotor50": (lambda P: P.quadrotor(50), 301),
    "quadrotor20": (lambda P: P.quadrotor(20), 37),
}


def _x0s(prob, batch, scale=1.0, seed=2):
    """The sibling files' generator; the cartpole's own (see the module docstring)."""
    if prob.nx == 4:
        rng = np.random.default_rng(seed + 3)
        return np.asfortranarray(prob.x0[:, None] * scale + 0.02 * rng.standard_normal((prob.nx, batch)))
    return _x0s_plain(prob, batch, scale, seed)


def _rhos(prob, batch, seed=11):
    rng = np.random.default_rng(seed)
    return prob.rho * np.exp(rng.uniform(np.log(0.5), np.log(4.0), batch))


def _rho_problem(pb, rho):
    return dataclasses.replace(pb, rho=float(rho))


def _guard(probs_at_rho, probs_shared, x0s, settings=SETTINGS, prepare=None):
    """From the oracle alone: every sampled instance differs between its own rho and the shared rho -- in its iteration count, or in
    states or controls by more than 1e-6 relative --, so that a kernel that ignored the verb cannot pass. -> the number of instances
    that differ in their iteration count."""
    by_iter = 0
    for b in probs_at_rho:
        res = []
        for pb in (probs_at_rho[b], probs_shared[b]):
            orc = _oracle(pb, settings)
            if prepare:
                prepare(orc, b)
            orc.set_x0(x0s[:, b])
            orc.solve()
            res.append((orc.stats()["iter"], orc.solution()[0].copy(), orc.solution()[1].copy()))
        (ia, xa, ua), (ib, xb, ub) = res
        ex, eu = rel_err(xa, xb), rel_err(ua, ub)
        print("guard instance %d: iter %d at its rho, %d at the shared rho; states differ by %.2e, controls by %.2e" % (b, ia, ib, ex, eu))
        assert ia != ib or ex > 1e-6 or eu > 1e-6, b
        by_iter += ia != ib
    return by_iter


def _check(s, orcs, x0s, tag):
    """Iterations and status exact, states and controls within TOL, the four residuals (the dual ones carry rho_b) at rtol 1e-6."""
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, orc in orcs.items():
        orc.set_x0(x0s[:, b])
        orc.solve()
        o = orc.stats()
        ex, eu = rel_err(sol["states"][:, :, b], orc.solution()[0]), rel_err(sol["controls"][:, :, b], orc.solution()[1])
        print("rho %s instance %d: iter %d (oracle %d) status %d (oracle %d) rel_err x %.2e u %.2e residuals %s (oracle %s)"
              % (tag, b, st["iter"][b], o["iter"], st["status"][b], o["status"], ex, eu, st["residuals"][:, b],
                 [o["pri_x"], o["dua_x"], o["pri_u"], o["dua_u"]]))
        assert st["iter"][b] == o["iter"], (tag, b)
        assert st["status"][b] == o["status"], (tag, b)
        assert ex < TOL and eu < TOL, (tag, b, ex, eu)
        np.testing.assert_allclose(st["residuals"][:, b], [o["pri_x"], o["dua_x"], o["pri_u"], o["dua_u"]], rtol=1e-6, atol=1e-10, err_msg=str((tag, b)))


def _bits(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


def _same_bits(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _shared_a(pkg, monkeypatch, prob, batch, settings=SETTINGS):
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    s = _solver(pkg, prob, batch, settings)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    return s


# ---------------------------------------------------------------------------------------------------------------- 1. caches
@pytest.mark.parametrize("case,batch,lo,hi", [("cartpole20", 37, 0, 37), ("wide32", 37, 0, 37), ("wide64", 21, 0, 21), ("wide64", 261, 250, 261)])
def test_caches_equal_single_instance_setups_at_each_rho(pkg, case, batch, lo, hi):
    """cartpole: the rows kernel; nx=24 nu=8: the LDS kernel; nx=48 nu=16: global scratch, 256 instances per launch -- and again with
    first > 0 in a batch above 256 (the index inside a chunk and the absolute instance then differ)."""
    prob = CASES[case][0](pkg.problems)
    rhos = _rhos(prob, batch)
    s = _solver(pkg, prob, batch)
    shared = s.get_cache()
    if lo > 0:  # first the range alone (one launch that starts at instance 250), with values of its own ...
        other = _rhos(prob, batch, seed=13)
        s.set_rho_batch(other[lo:hi], first=lo)
        for b in (lo, hi - 1):
            one = pkg.TinyMPC()
            one.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=float(other[b]), fdyn=prob.fdyn)
            c1, cb = one.get_cache(), s.get_cache_batch(b, 1)
            for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
                np.testing.assert_array_equal(cb[n][:, :, 0], c1[n], err_msg="%s instance %d" % (n, b))
            one.reset()
        np.testing.assert_array_equal(s.get_rho_batch(lo, hi - lo), other[lo:hi])
        np.testing.assert_array_equal(s.get_rho_batch(0, lo), np.full(lo, prob.rho))
    s.set_rho_batch(rhos)  # ... then the whole batch (above 256: two launches, the second starting at instance 256)
    whole = s.get_cache_batch()
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    for b in sorted(set(_sample(batch)) | ({255, 256} if batch > 256 else set())):
        one = pkg.TinyMPC()
        one.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=float(rhos[b]), fdyn=prob.fdyn)
        c1, cb = one.get_cache(), s.get_cache_batch(b, 1)
        for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
            np.testing.assert_array_equal(cb[n][:, :, 0], c1[n], err_msg="%s instance %d" % (n, b))
            np.testing.assert_array_equal(whole[n][:, :, b], c1[n])
            assert not np.array_equal(c1[n], shared[n]), (n, b)  # (rho_b is not the shared rho: another cache)
        assert cb["riccati_iters"][0] == whole["riccati_iters"][b] == c1["riccati_iters"], b
        one.reset()
    np.testing.assert_array_equal(s.get_cache()["Pinf"], shared["Pinf"])  # the single-model verb keeps addressing the shared cache
    s.reset()


# ---------------------------------------------------------------------------------------------------------------- 2. oracle, layout A
@pytest.mark.parametrize("case", ["cartpole20", "wide32", "wide64", "quadrotor120"])
def test_each_instance_matches_the_oracle_at_its_own_rho(pkg, case):
    prob, batch = CASES[case][0](pkg.problems), CASES[case][1]
    rhos = _rhos(prob, batch)
    samples = _sample(batch)
    at_rho = {b: _rho_problem(prob, rhos[b]) for b in samples}
    by_iter = _guard(at_rho, {b: prob for b in samples}, _x0s(prob, batch, 1.0, seed=0))
    if case.startswith("quadrotor"):
        assert by_iter >= 2, by_iter
    s = _solver(pkg, prob, batch)
    s.set_rho_batch(rhos)
    orcs = {b: _oracle(at_rho[b]) for b in samples}
    for rnd in range(3):  # a cold start, then two warm starts
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (case, rnd))
    assert s.launch_info()["layout"] == "A"
    assert "per-instance-models" in s.jit_info(), s.jit_info()
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    s.reset()


# ---------------------------------------------------------------------------------------------------------------- 3. equal rho
@pytest.mark.parametrize("case", ["quadrotor50", "cartpole20", "wide32", "wide64", "quadrotor120"])
def test_the_shared_rho_for_every_instance_changes_no_bit(pkg, monkeypatch, case):
    """set_rho_batch(full(batch, prob.rho)) == a handle that entered the mode with the shared model only == the plain shared handle on
    layout A (what test_instance_models_gpu.py claims for equal models)."""
    from test_instance_models_gpu import _shared_models
    prob, batch = CASES[case][0](pkg.problems), min(CASES[case][1], 300)
    shared = _shared_a(pkg, monkeypatch, prob, batch)
    mode, inst = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    _set_models(mode, _shared_models(prob, batch))
    inst.set_rho_batch(np.full(batch, prob.rho))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, mode, inst):
            h.set_x0_batch(x0s)
            h.solve()
        _same(mode, inst)
        _same(shared, inst)
    assert shared.launch_info()["layout"] == inst.launch_info()["layout"] == "A"
    assert "per-instance-models" in inst.jit_info() and "per-instance-models" not in shared.jit_info()
    ca, cb = mode.get_cache_batch(), inst.get_cache_batch()
    for n in ca:
        np.testing.assert_array_equal(ca[n], cb[n])
    for h in (shared, mode, inst):
        h.reset()


# ---------------------------------------------------------------------------------------------------------------- 4. order and ranges
def test_the_two_verbs_commute(pkg):
    prob, batch = pkg.problems.quadrotor(50), 101
    M, rhos = _models(prob, batch, seed=21, fdyn=True), _rhos(prob, batch, seed=17)  # (seed 17: three sampled instances differ in iterations)
    samples = _sample(batch)
    at_rho = {b: _rho_problem(M.problem(prob, b), rhos[b]) for b in samples}
    x0s = _x0s(prob, batch)
    assert _guard(at_rho, {b: M.problem(prob, b) for b in samples}, x0s) >= 2
    mr, rm = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    _set_models(mr, M)
    mr.set_rho_batch(rhos)
    rm.set_rho_batch(rhos)
    _set_models(rm, M)
    for h in (mr, rm):
        h.set_x0_batch(x0s)
        h.solve()
    _same(mr, rm)
    ca, cb = mr.get_cache_batch(), rm.get_cache_batch()
    for n in ca:
        np.testing.assert_array_equal(ca[n], cb[n])
    _check(mr, {b: _oracle(at_rho[b]) for b in samples}, x0s, "model then rho")
    for b in (0, batch - 1):  # ... and (model_b, rho_b) from scratch
        pb = at_rho[b]
        one = pkg.TinyMPC()
        one.setup(pb.A, pb.B, pb.Q, pb.R, pb.N, rho=pb.rho, fdyn=pb.fdyn)
        c1, cb = one.get_cache(), rm.get_cache_batch(b, 1)
        for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
            np.testing.assert_array_equal(cb[n][:, :, 0], c1[n], err_msg="%s instance %d" % (n, b))
        assert cb["riccati_iters"][0] == c1["riccati_iters"]
        one.reset()
    mr.reset()
    rm.reset()


def test_partial_ranges_second_call_read_back_and_clear(pkg, monkeypatch):
    prob, batch = pkg.problems.quadrotor(50), 200
    rhos, rhos2 = _rhos(prob, batch), _rhos(prob, batch, seed=12)
    s = _solver(pkg, prob, batch)
    np.testing.assert_array_equal(s.get_rho_batch(), np.full(batch, prob.rho))
    s.set_rho_batch(rhos[10:60], first=10)
    expect = np.full(batch, prob.rho)
    expect[10:60] = rhos[10:60]
    np.testing.assert_array_equal(s.get_rho_batch(), expect)
    s.set_rho_batch(rhos2[55:57], first=55)  # a second call moves a sub-range
    expect[55:57] = rhos2[55:57]
    np.testing.assert_array_equal(s.get_rho_batch(), expect)
    np.testing.assert_array_equal(s.get_rho_batch(54, 4), expect[54:58])
    shared = _shared_a(pkg, monkeypatch, prob, batch)
    inside = {b: _oracle(_rho_problem(prob, expect[b])) for b in (10, 30, 54, 55, 56, 57, 59)}
    outside = [b for b in range(batch) if not 10 <= b < 60]
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (s, shared):
            h.set_x0_batch(x0s)
            h.solve()
        _check(s, inside, x0s, ("partial", rnd))
        for x, y in zip(_bits(s), _bits(shared)):
            np.testing.assert_array_equal(x[..., outside], y[..., outside])
    # kept across update_settings and the shared reference / bound verbs
    s.update_settings(max_iter=80)
    s.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    np.testing.assert_array_equal(s.get_rho_batch(), expect)
    assert "per-instance-models" in s.jit_info()
    # clear_model_batch: the shared model and the shared rho again, as a handle that never had the mode
    s.clear_model_batch()
    assert "per-instance-models" not in s.jit_info()
    np.testing.assert_array_equal(s.get_rho_batch(), np.full(batch, prob.rho))
    settings = dict(SETTINGS, max_iter=80)
    ref = _solver(pkg, prob, batch, settings)
    ref.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    x0s = _x0s(prob, batch)
    for h in (s, ref):
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    _same(s, ref)
    assert s.launch_info()["layout"] == ref.launch_info()["layout"]
    for h in (s, shared, ref):
        h.reset()


# ---------------------------------------------------------------------------------------------------------------- 5. reset
def test_reset_workspace_keeps_every_instances_rho(pkg):
    prob, batch = pkg.problems.quadrotor(20), 37
    rhos = _rhos(prob, batch)
    s = _solver(pkg, prob, batch)
    s.set_rho_batch(rhos)
    x0s = _x0s(prob, batch)
    s.set_x0_batch(x0s)
    s.solve()
    first = _bits(s)
    s.reset_workspace()
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    s.set_x0_batch(x0s)
    s.solve()
    _same_bits(first, _bits(s))
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    _check(s, {b: _oracle(_rho_problem(prob, rhos[b])) for b in (0, batch - 1)}, x0s, "after reset")
    s.reset()


# ---------------------------------------------------------------------------------------------------------------- 6. references, bounds
def test_with_per_instance_trajectories_and_bounds_per_knot(pkg):
    prob, batch = pkg.problems.quadrotor(50), 101
    rhos = _rhos(prob, batch)
    (vx, vu), (X, U) = _refs(prob, batch, "trajectory", seed=3)
    verb, full = _bounds(prob, batch, "knot", seed=4)
    samples = _sample(batch)
    box = lambda b: dict(x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
    at_rho = {b: dataclasses.replace(prob, rho=float(rhos[b]), **box(b)) for b in samples}
    at_shared = {b: dataclasses.replace(prob, **box(b)) for b in samples}

    def refs(orc, b):
        orc.set_x_ref(X[:, :, b])
        orc.set_u_ref(U[:, :, b])

    x0s = _x0s(prob, batch)
    # (no iteration-count guard here: under these bounds and trajectories no sampled instance converges within 100 iterations at any rho
    # -- seeds 11..19 tried with the oracle --, so the instances differ in states and controls only)
    _guard(at_rho, at_shared, x0s, prepare=refs)
    s = _solver(pkg, prob, batch)
    s.set_x_ref_batch(vx)
    s.set_rho_batch(rhos)  # (any order)
    s.set_bound_constraints_batch(*verb)
    s.set_u_ref_batch(vu)
    orcs = {}
    for b in samples:
        orcs[b] = _oracle(at_rho[b])
        refs(orcs[b], b)
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=2 + rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, ("refs+bounds", rnd))
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info and "per-instance-models" in info, info
    assert s.launch_info()["layout"] == "A"
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    s.reset()


# ---------------------------------------------------------------------------------------------------------------- 7. closed loop
def test_closed_loop_with_each_instances_own_rho(pkg):
    """Four ticks of mpc_step_batch, every instance advanced by its plant; per-instance oracles warm-started from tick to tick, and bit
    for bit against the three verbs a tick stands for."""
    prob, batch = pkg.problems.quadrotor(50), 64
    settings = dict(max_iter=50, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    rhos = _rhos(prob, batch)
    s, v = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)
    for h in (s, v):
        h.set_rho_batch(rhos)
    samples = _sample(batch)
    orcs = {b: _oracle(_rho_problem(prob, rhos[b]), settings) for b in samples}
    x = _x0s(prob, batch)
    for k in range(4):
        u = s.mpc_step(x)
        v.set_x0_batch(x)
        v.solve()
        np.testing.assert_array_equal(u, v.get_first_controls_batch())
        st = s.get_stats_batch()
        for b, orc in orcs.items():
            orc.set_x0(x[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (k, b)
            assert rel_err(u[:, b], orc.solution()[1][:, 0]) < TOL, (k, b)
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
    assert "per-instance-models" in s.jit_info() and s.launch_info()["layout"] == "A"
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    s.reset()
    v.reset()


# ---------------------------------------------------------------------------------------------------------------- 8. device form
def test_device_input_matches_host_input(pkg):
    prob, batch = pkg.problems.quadrotor(20), 37
    rhos = _rhos(prob, batch)
    x0s = _x0s(prob, batch)
    torch = _torch_gpu()
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    dev = _DeviceArrays(pkg)
    h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    h.set_rho_batch(rhos[5:], first=5)
    assert L.tinympc_set_rho_batch_device(d._h, dev.put(rhos[5:]), 5, batch - 5) == 0
    dev.free()  # (the copy has completed when the verb returns)
    handles = [h, d]
    if torch is not None:
        t = _solver(pkg, prob, batch)
        t.set_rho_batch(torch.from_numpy(rhos[5:].copy()).cuda(), first=5)
        handles.append(t)
    for q in handles:
        q.set_x0_batch(x0s)
        q.solve()
    for q in handles[1:]:
        assert "per-instance-models" in q.jit_info()
        _same(h, q)
        np.testing.assert_array_equal(h.get_rho_batch(), q.get_rho_batch())
        ca, cb = h.get_cache_batch(), q.get_cache_batch()
        for n in ca:
            np.testing.assert_array_equal(ca[n], cb[n])
    # host memory through the device verb is refused; so is device memory that holds a value the verb does not take (validated there)
    s = _solver(pkg, prob, batch)
    buf = np.full(8, 1.0)
    assert L.tinympc_set_rho_batch_device(s._h, C.c_void_p(buf.ctypes.data), 0, 4) == E
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = np.full(4, prob.rho)
        v[2] = bad
        assert L.tinympc_set_rho_batch_device(s._h, dev.put(v), 0, 4) == E, bad
    dev.free()
    if torch is not None:
        for badt in (torch.ones(4, dtype=torch.float32).cuda(), torch.ones((2, 2), dtype=torch.float64).cuda(), torch.ones(8, dtype=torch.float64).cuda()[::2]):
            with pytest.raises(pkg.TinyMPCError) as ei:
                s.set_rho_batch(badt)
            assert ei.value.code == E
    assert "per-instance-models" not in s.jit_info()
    np.testing.assert_array_equal(s.get_rho_batch(), np.full(batch, prob.rho))
    for q in handles + [s]:
        q.reset()


# ---------------------------------------------------------------------------------------------------------------- 9. invalid arguments
def test_invalid_arguments_are_refused_and_change_nothing(pkg):
    prob, batch = pkg.problems.quadrotor(20), 64
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    f = L.tinympc_set_rho_batch
    good = np.full(batch, 1.5 * prob.rho)
    p = good.ctypes.data_as(pkg._lib.c_double_p)

    def bad_calls(s):
        assert f(s._h, None, 0, 4) == E                 # NULL
        assert L.tinympc_set_rho_batch_device(s._h, None, 0, 4) == E
        assert f(s._h, p, 0, 0) == E                    # an empty range
        assert f(s._h, p, 0, -1) == E
        assert f(s._h, p, -1, 2) == E
        assert f(s._h, p, batch - 2, 4) == E            # a range beyond the batch
        for bad in (0.0, -prob.rho, np.nan, np.inf, -np.inf):
            v = good.copy()
            v[batch - 1] = bad                          # (the last value: nothing before it may have been written)
            assert f(s._h, v.ctypes.data_as(pkg._lib.c_double_p), 0, batch) == E, bad
        with pytest.raises(pkg.TinyMPCError) as ei:
            s.set_rho_batch(np.ones((2, 2)))
        assert ei.value.code == E

    x0s = _x0s(prob, batch)
    # on a handle without the mode: nothing of it switched the mode on
    s, ref = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
    bad_calls(s)
    assert "per-instance-models" not in s.jit_info()
    np.testing.assert_array_equal(s.get_rho_batch(), np.full(batch, prob.rho))
    for h in (s, ref):
        h.set_x0_batch(x0s)
        h.solve()
    _same(s, ref)
    # on a handle with the mode: store, caches and solve as they were
    rhos = _rhos(prob, batch)
    s.set_rho_batch(rhos)
    s.solve()
    before, cache = _bits(s), s.get_cache_batch()
    bad_calls(s)
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    after = s.get_cache_batch()
    for n in cache:
        np.testing.assert_array_equal(cache[n], after[n])
    s.reset_workspace()
    ref.reset_workspace()
    s.set_x0_batch(x0s)
    s.solve()
    ref.set_rho_batch(rhos)
    ref.set_x0_batch(x0s)
    ref.solve()
    _same(s, ref)
    assert "per-instance-models" in s.jit_info()
    del before
    s.reset()
    ref.reset()


# ---------------------------------------------------------------------------------------------------------------- 10. refusals
def _expect_unsupported(pkg, call):
    with pytest.raises(pkg.TinyMPCError) as ei:
        call()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    msg = str(ei.value)
    assert "per-instance models" in msg and "per-instance rho (set_rho_batch)" in msg and "tinympc_clear_model_batch" in msg, msg


def test_refusals_and_recovery(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    rhos = _rhos(prob, batch)
    # adaptive rho, set after the verb
    s = _solver(pkg, prob, batch)
    s.set_rho_batch(rhos)
    s.set_x0_batch(_x0s(prob, batch))
    s.solve()
    s.update_settings(adaptive_rho=1)
    _expect_unsupported(pkg, s.solve)
    np.testing.assert_array_equal(s.get_rho_batch(), rhos)
    s.clear_model_batch()  # shared again: the adaptive-rho kernel may run
    s.solve()
    s.reset()
    # cone constraints set after the verb
    s = _solver(pkg, prob, batch)
    s.set_rho_batch(rhos)
    s.set_x0_batch(_x0s(prob, batch))
    s.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    s.update_settings(en_state_soc=1)
    _expect_unsupported(pkg, s.solve)
    s.clear_model_batch()
    s.solve()
    s.reset()
    # nx + nu > 64 (layout M)
    rng = np.random.default_rng(3)
    nx, nu, N = 60, 8, 6
    big = P.Problem("big", np.eye(nx) + 0.01 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), N, 2.0,
                    rng.standard_normal(nx))
    s = _solver(pkg, big, 4)
    s.set_rho_batch(np.array([1.0, 2.0, 3.0, 4.0]))
    s.set_x0_batch(np.zeros((nx, 4), order="F"))
    _expect_unsupported(pkg, s.solve)
    s.clear_model_batch()
    s.solve()
    np.testing.assert_array_equal(s.get_rho_batch(), np.full(4, 2.0))
    s.reset()
    # a session on a single-instance handle
    one = P.quadrotor(20)
    s = _solver(pkg, one, 1)
    s.set_rho_batch(np.array([2.0 * one.rho]))
    _expect_unsupported(pkg, s.session_begin)
    s.set_x0(one.x0)
    s.solve()  # (launched solves carry the instance's rho)
    orc = _oracle(_rho_problem(one, 2.0 * one.rho))
    orc.set_x0(one.x0)
    orc.solve()
    assert s.get_stats()["iter"] == orc.stats()["iter"]
    assert rel_err(s.get_solution()["controls"], orc.solution()[1]) < TOL
    s.clear_model_batch()
    s.reset_workspace()
    s.solve()
    orc = _oracle(one)
    orc.set_x0(one.x0)
    orc.solve()
    assert s.get_stats()["iter"] == orc.stats()["iter"]
    s.reset()


# ---------------------------------------------------------------------------------------------------------------- 11. sharding
def test_two_shards_equal_one_handle(pkg):
    """Two shards as pkg.batch.job_shard cuts them, each handle taking its part of the rho vector: equal to the unsharded handle."""
    prob, n = pkg.problems.quadrotor(50), 202
    rhos, x0s = _rhos(prob, n), _x0s(pkg.problems.quadrotor(50), 202)
    whole = _solver(pkg, prob, n)
    whole.set_rho_batch(rhos)
    whole.set_x0_batch(x0s)
    whole.solve()
    for rank in range(2):
        _, lo, count, _ = pkg.batch.job_shard(rank, 2, global_batch=n)
        hi = lo + count
        part = _solver(pkg, prob, count)
        part.set_rho_batch(rhos[lo:hi])
        part.set_x0_batch(np.asfortranarray(x0s[:, lo:hi]))
        part.solve()
        np.testing.assert_array_equal(part.get_solution_batch()["controls"], whole.get_solution_batch(lo, count)["controls"])
        np.testing.assert_array_equal(part.get_solution_batch()["states"], whole.get_solution_batch(lo, count)["states"])
        np.testing.assert_array_equal(part.get_stats_batch()["iter"], whole.get_stats_batch()["iter"][lo:hi])
        np.testing.assert_array_equal(part.get_cache_batch()["Pinf"], whole.get_cache_batch(lo, count)["Pinf"])
        np.testing.assert_array_equal(part.get_rho_batch(), whole.get_rho_batch(lo, count))
        part.reset()
    whole.reset()


# ---------------------------------------------------------------------------------------------------------------- the example
def test_the_rho_sweep_example_runs(pkg):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rho_sweep.py"), "--count", "16"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "best rho" in out.stdout, out.stdout

"""Per-instance models on layout D (tinympc_set_model_batch on a handle that called tinympc_prepare): the goal kernel with every
wavefront's four operator blocks staged into its own LDS region (IMOD in tinympc_solve_d.hip). Every instance still solves what a
single-instance handle with its own model would -- against the oracle per instance, against the layout A kernel over the whole batch,
bit for bit against the shared-model layout D handle where the models coincide --, and everything the form does not carry (no
prepare(), trajectories, per-knot bounds, wide systems, horizons without a plan, a refused or switched-off specialisation) stays on
layout A and stays correct.

Shapes, the smallest that reach every path: quadrotor N=50 x 773 in the default environment (773 > 768: layout D without a switch; the
compiled-in kernel, one wavefront per SIMD; 193 full wavefronts + one instance: a ragged last wavefront in a partial last workgroup),
and quadrotor N=20 / cartpole N=20 (KT = 8), both with fdyn, x 37 under TINYMPC_LAYOUT=D (run-time specialised, two wavefronts per
SIMD; three workgroups, the last with a one-instance wavefront). Helpers, TOL and the sample are the sibling file's; a seed that put a
sampled instance on a termination edge against the oracle would be changed here and said so (none had to be)."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
from conftest import rel_err

from test_instance_bounds_gpu import _bounds, _refs, _wide, _x0s
from test_instance_models_gpu import SETTINGS, TOL, _check, _models, _oracle, _same, _sample, _set_models, _shared_models, _solver

pytestmark = pytest.mark.gpu

SHAPES = {  # name -> (problem, batch, TINYMPC_LAYOUT at setup, non-zero fdyn?)
    "quadrotor50": (lambda P: P.quadrotor(50), 773, None, False),
    "quadrotor20": (lambda P: P.quadrotor(20), 37, "D", True),
    "cartpole20": (lambda P: P.cartpole(20, True), 37, "D", True),
}


def _handle(pkg, monkeypatch, shape, settings=SETTINGS):
    make, batch, layout, fdyn = SHAPES[shape]
    prob = make(pkg.problems)
    if layout:
        monkeypatch.setenv("TINYMPC_LAYOUT", layout)
    s = _solver(pkg, prob, batch, settings)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    return s, prob, batch, fdyn


def _on_d(s):
    info = s.jit_info()
    assert s.launch_info()["layout"] == "D", (s.launch_info(), info)
    assert "per-instance-models" in info and "refused" not in info, info


def _on_a(s):
    assert s.launch_info()["layout"] == "A", (s.launch_info(), s.jit_info())
    assert "per-instance-models" in s.jit_info(), s.jit_info()


def _each_instance_close(d, a, tag):
    """Iterations and status equal, states and controls within TOL, for EVERY instance of the batch."""
    sd, sa, td, ta = d.get_solution_batch(), a.get_solution_batch(), d.get_stats_batch(), a.get_stats_batch()
    np.testing.assert_array_equal(td["iter"], ta["iter"], err_msg=str(tag))
    np.testing.assert_array_equal(td["status"], ta["status"], err_msg=str(tag))
    for n in ("states", "controls"):
        err = np.max(np.abs(sd[n] - sa[n]), axis=(0, 1)) / np.maximum(np.max(np.abs(sa[n]), axis=(0, 1)), 1e-300)
        print("models D against A %s %s: worst instance %d rel_err %.2e" % (tag, n, int(np.argmax(err)), float(np.max(err))))
        assert np.all(err < TOL), (tag, n, int(np.argmax(err)), float(np.max(err)))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_instance_matches_the_oracle_and_layout_a(pkg, monkeypatch, shape):
    """Tests 1 and 2 of the feature on one pair of handles: the prepared handle (layout D) against per-instance oracles on the sample,
    and against the same models on a handle that never called prepare() (layout A) over the whole batch; cold, then two warm starts."""
    d, prob, batch, fdyn = _handle(pkg, monkeypatch, shape)
    a = _handle(pkg, monkeypatch, shape)[0]
    M = _models(prob, batch, fdyn=fdyn)
    for h in (d, a):
        _set_models(h, M)
    d.prepare()
    _on_d(d)
    # (the quadrotor N=50 kernel is found by the options of its plan: a plan that moved would leave it to the run-time compiler)
    assert ("compiled-in" in d.jit_info()) == (shape == "quadrotor50"), d.jit_info()
    orcs = {b: _oracle(M.problem(prob, b)) for b in _sample(batch)}
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (d, a):
            h.set_x0_batch(x0s)
            h.solve()
        _check(d, orcs, x0s, (shape, rnd))
        _each_instance_close(d, a, (shape, rnd))
    _on_d(d)
    _on_a(a)
    d.reset()
    a.reset()


@pytest.mark.parametrize("shape", ["quadrotor50", "cartpole20"])
def test_equal_models_are_bit_identical_to_the_shared_handle_on_layout_d(pkg, monkeypatch, shape):
    inst, prob, batch, _ = _handle(pkg, monkeypatch, shape)
    shared = _handle(pkg, monkeypatch, shape)[0]
    _set_models(inst, _shared_models(prob, batch))
    inst.prepare()
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, inst):
            h.set_x0_batch(x0s)
            h.solve()
        _same(shared, inst)  # solutions, iterations, status, the four residuals
    _on_d(inst)
    assert shared.launch_info()["layout"] == "D" and "per-instance-models" not in shared.jit_info()
    shared.reset()
    inst.reset()


def test_partial_ranges_second_call_and_clear(pkg, monkeypatch):
    s, prob, batch, _ = _handle(pkg, monkeypatch, "quadrotor50")
    shared = _handle(pkg, monkeypatch, "quadrotor50")[0]
    M, M2 = _models(prob, batch, seed=5), _models(prob, batch, seed=6, fdyn=True)
    _set_models(s, M, 10, 60)
    _set_models(s, M2, 55, 57)  # a second call over a sub-range
    s.prepare()
    inside = {b: _oracle((M2 if 55 <= b < 57 else M).problem(prob, b)) for b in (10, 30, 54, 55, 56, 57, 59)}
    outside = [b for b in range(batch) if not 10 <= b < 60]
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (s, shared):
            h.set_x0_batch(x0s)
            h.solve()
        _check(s, inside, x0s, ("partial", rnd))
        a, b = s.get_solution_batch(), shared.get_solution_batch()
        np.testing.assert_array_equal(a["states"][:, :, outside], b["states"][:, :, outside])
        np.testing.assert_array_equal(a["controls"][:, :, outside], b["controls"][:, :, outside])
        ta, tb = s.get_stats_batch(), shared.get_stats_batch()
        np.testing.assert_array_equal(ta["iter"][outside], tb["iter"][outside])
        np.testing.assert_array_equal(ta["status"][outside], tb["status"][outside])
        np.testing.assert_array_equal(ta["residuals"][:, outside], tb["residuals"][:, outside])
    _on_d(s)
    assert shared.launch_info()["layout"] == "D"
    # clear_model_batch: every instance on the shared model again, as a handle that never had the mode, on the same layout as it
    s.clear_model_batch()
    assert "per-instance-models" not in s.jit_info()
    ref = _handle(pkg, monkeypatch, "quadrotor50")[0]
    x0s = _x0s(prob, batch)
    for h in (s, ref):
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    _same(s, ref)
    assert s.launch_info()["layout"] == ref.launch_info()["layout"] == "D"
    for h in (s, shared, ref):
        h.reset()


@pytest.mark.parametrize("refs,bounds,layout", [("goal", "box", "D"), ("trajectory", "box", "A"), ("goal", "knot", "A")])
def test_combined_with_per_instance_references_and_bounds(pkg, monkeypatch, refs, bounds, layout):
    s, prob, batch, _ = _handle(pkg, monkeypatch, "quadrotor50")
    M = _models(prob, batch, seed=3, fdyn=True)
    (vx, vu), (X, U) = _refs(prob, batch, refs, seed=3)
    verb, full = _bounds(prob, batch, bounds, seed=4)
    s.set_x_ref_batch(vx)
    _set_models(s, M)  # (any order)
    s.prepare()
    s.set_bound_constraints_batch(*verb)
    s.set_u_ref_batch(vu)
    orcs = {}
    for b in _sample(batch):
        pb = dataclasses.replace(M.problem(prob, b), x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
        orcs[b] = _oracle(pb)
        orcs[b].set_x_ref(X[:, :, b])
        orcs[b].set_u_ref(U[:, :, b])
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (refs, bounds, rnd))
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info and "per-instance-models" in info, info
    assert s.launch_info()["layout"] == layout, (s.launch_info(), info)
    assert "refused" not in info, info
    s.reset()


def test_closed_loop_with_each_instances_own_plant(pkg, monkeypatch):
    """Four ticks of mpc_step_batch on layout D, every instance's state advanced by its OWN plant x+ = A_b x + B_b u + fdyn_b; against
    per-instance oracles warm-started from tick to tick, and bit for bit against the three verbs a tick stands for."""
    settings = dict(max_iter=50, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    s, prob, batch, _ = _handle(pkg, monkeypatch, "quadrotor50", settings)
    v = _handle(pkg, monkeypatch, "quadrotor50", settings)[0]
    M = _models(prob, batch, seed=7, fdyn=True)
    for h in (s, v):
        _set_models(h, M)
        h.prepare()
    orcs = {b: _oracle(M.problem(prob, b), settings) for b in _sample(batch)}
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
        x = np.asfortranarray(np.einsum("ijb,jb->ib", M.A, x) + np.einsum("ijb,jb->ib", M.B, u) + M.f)
    _on_d(s)
    _on_d(v)
    s.reset()
    v.reset()


def _solve_and_check(s, prob, M, batch, samples, tag):
    x0s = _x0s(prob, batch)
    s.set_x0_batch(x0s)
    s.solve()
    _check(s, {b: _oracle(M.problem(prob, b)) for b in samples}, x0s, tag)


def test_without_prepare_the_mode_stays_on_layout_a(pkg, monkeypatch):
    s, prob, batch, fdyn = _handle(pkg, monkeypatch, "quadrotor20")
    M = _models(prob, batch, seed=12, fdyn=fdyn)
    _set_models(s, M)
    _solve_and_check(s, prob, M, batch, [0, batch - 1], "no prepare")
    _on_a(s)
    assert "refused" not in s.jit_info()
    s.reset()


def test_with_the_specialiser_switched_off_a_shape_that_is_not_compiled_in_stays_on_layout_a(pkg, monkeypatch):
    s, prob, batch, fdyn = _handle(pkg, monkeypatch, "quadrotor20")
    monkeypatch.setenv("TINYMPC_JIT", "0")
    M = _models(prob, batch, seed=13, fdyn=fdyn)
    _set_models(s, M)
    s.prepare()
    _solve_and_check(s, prob, M, batch, [batch - 1], "TINYMPC_JIT=0")
    _on_a(s)
    assert "refused(TINYMPC_JIT=0)" in s.jit_info(), s.jit_info()
    s.reset()


def test_a_refused_specialisation_leaves_the_mode_on_layout_a_and_says_why(pkg, monkeypatch):
    """TINYMPC_JIT_REG_LIMIT (the specialiser's test hook) lowers the register budget the built kernel is checked against. Cartpole
    N=10: compiled in for the shared model, so the handle is on layout D without the specialiser, and no other test of this process
    builds its model form (a built kernel is remembered per process)."""
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")
    prob, batch = pkg.problems.cartpole(10, True), 37
    s = _solver(pkg, prob, batch)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    assert s.launch_info()["layout"] == "D"
    monkeypatch.setenv("TINYMPC_JIT_REG_LIMIT", "64")
    monkeypatch.setenv("TINYMPC_JIT_QUIET", "1")
    M = _models(prob, batch, seed=14, fdyn=True)
    _set_models(s, M)
    s.prepare()
    _solve_and_check(s, prob, M, batch, [0, batch - 1], "refused")
    _on_a(s)
    info = s.jit_info()
    assert info.startswith("refused(") and "registers, the plan allows 64" in info, info
    s.reset()


@pytest.mark.parametrize("case", ["wide32", "quadrotor120"])
def test_shapes_without_a_model_form_stay_on_layout_a_after_prepare(pkg, case):
    P = pkg.problems
    prob, batch = (_wide(P, 24, 8, 20), 37) if case == "wide32" else (P.quadrotor(120), 70)
    s = _solver(pkg, prob, batch)
    M = _models(prob, batch, seed=15, fdyn=True)
    _set_models(s, M)
    s.prepare()
    _solve_and_check(s, prob, M, batch, [0, batch - 1], case)
    _on_a(s)
    s.reset()


def test_prepare_before_set_model_batch_reaches_layout_d_at_the_first_solve(pkg, monkeypatch):
    first, prob, batch, fdyn = _handle(pkg, monkeypatch, "quadrotor20")
    then = _handle(pkg, monkeypatch, "quadrotor20")[0]
    M = _models(prob, batch, seed=16, fdyn=fdyn)
    first.prepare()
    _set_models(first, M)
    _set_models(then, M)
    then.prepare()
    x0s = _x0s(prob, batch)
    for h in (first, then):
        h.set_x0_batch(x0s)
        h.solve()
        _on_d(h)
    _same(first, then)
    _check(first, {b: _oracle(M.problem(prob, b)) for b in (0, batch - 1)}, x0s, "prepare first")
    first.reset()
    then.reset()

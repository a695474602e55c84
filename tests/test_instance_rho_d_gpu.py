"""Per-instance rho on layout D (tinympc_set_rho_batch on a handle that called tinympc_prepare): the model form of the goal kernel (IMOD
in tinympc_solve_d.hip) stages each of a wavefront's four operator blocks with its own instance's -rho and carries rho as a lane
variable. Every instance still solves what a single-instance handle set up with rho_b would -- against the oracle per instance, against
the layout A kernel over the whole batch, bit for bit against the shared-model layout D handle where every rho is the shared one.

Shapes: those of test_instance_models_d_gpu.py -- quadrotor N=50 x 773 in the default environment (the compiled-in kernel, one wavefront
per SIMD), quadrotor N=20 and cartpole N=20 x 37 under TINYMPC_LAYOUT=D (run-time specialised, two wavefronts per SIMD). For the 773
instances rho cycles through four values with the instance index, so the four 16-lane groups of every wavefront hold four different
values: staging that took block 0's rho for all four blocks would show. The other shapes draw rho_b as test_instance_rho_gpu.py does;
helpers, the cartpole's x0 generator, TOL and the sample are that file's."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from test_instance_bounds_gpu import _bounds, _refs
from test_instance_models_d_gpu import SHAPES, _each_instance_close, _handle, _on_a, _on_d
from test_instance_models_gpu import _models, _oracle, _same, _sample, _set_models, _shared_models
from test_instance_rho_gpu import _check, _guard, _rho_problem, _rhos, _x0s

pytestmark = pytest.mark.gpu

# x prob.rho, by instance index modulo 4: the four lane groups of a wavefront (chosen with the oracle alone among six such cycles: with
# this one three of the five sampled instances differ in their iteration count between their rho and the shared one)
CYCLE = (3.7, 0.6, 2.4, 1.3)


def _shape_rhos(prob, batch, shape):
    if shape == "quadrotor50":
        return prob.rho * np.array(CYCLE)[np.arange(batch) % 4]
    return _rhos(prob, batch)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_each_instance_matches_the_oracle_and_layout_a(pkg, monkeypatch, shape):
    """The prepared handle (layout D) against per-instance oracles on the sample, and against the same handle without prepare() (layout
    A) over the whole batch; cold, then two warm starts."""
    d, prob, batch, _ = _handle(pkg, monkeypatch, shape)
    a = _handle(pkg, monkeypatch, shape)[0]
    rhos = _shape_rhos(prob, batch, shape)
    samples = _sample(batch)
    at_rho = {b: _rho_problem(prob, rhos[b]) for b in samples}
    by_iter = _guard(at_rho, {b: prob for b in samples}, _x0s(prob, batch, 1.0, seed=0))
    if shape.startswith("quadrotor"):
        assert by_iter >= 2, by_iter
    for h in (d, a):
        h.set_rho_batch(rhos)
    d.prepare()
    _on_d(d)
    assert ("compiled-in" in d.jit_info()) == (shape == "quadrotor50"), d.jit_info()
    orcs = {b: _oracle(at_rho[b]) for b in samples}
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (d, a):
            h.set_x0_batch(x0s)
            h.solve()
        _check(d, orcs, x0s, (shape, rnd))
        _each_instance_close(d, a, (shape, rnd))
    _on_d(d)
    _on_a(a)
    np.testing.assert_array_equal(d.get_rho_batch(), rhos)
    d.reset()
    a.reset()


@pytest.mark.parametrize("shape", ["quadrotor50", "cartpole20"])
def test_the_shared_rho_for_every_instance_is_bit_identical_on_layout_d(pkg, monkeypatch, shape):
    """set_rho_batch(full(batch, prob.rho)) == the handle that entered the mode with the shared model only == the shared handle."""
    inst, prob, batch, _ = _handle(pkg, monkeypatch, shape)
    mode = _handle(pkg, monkeypatch, shape)[0]
    shared = _handle(pkg, monkeypatch, shape)[0]
    inst.set_rho_batch(np.full(batch, prob.rho))
    _set_models(mode, _shared_models(prob, batch))
    inst.prepare()
    mode.prepare()
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, mode, inst):
            h.set_x0_batch(x0s)
            h.solve()
        _same(mode, inst)  # solutions, iterations, status, the four residuals
        _same(shared, inst)
    _on_d(inst)
    _on_d(mode)
    assert shared.launch_info()["layout"] == "D" and "per-instance-models" not in shared.jit_info()
    for h in (shared, mode, inst):
        h.reset()


def test_combined_with_models_goals_and_boxes(pkg, monkeypatch):
    s, prob, batch, _ = _handle(pkg, monkeypatch, "quadrotor50")
    M = _models(prob, batch, seed=3, fdyn=True)
    rhos = _shape_rhos(prob, batch, "quadrotor50")
    (vx, vu), (X, U) = _refs(prob, batch, "goal", seed=3)
    verb, full = _bounds(prob, batch, "box", seed=4)
    samples = _sample(batch)
    box = lambda b: dict(x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
    at_rho = {b: dataclasses.replace(M.problem(prob, b), rho=float(rhos[b]), **box(b)) for b in samples}
    at_shared = {b: dataclasses.replace(M.problem(prob, b), **box(b)) for b in samples}

    def refs(orc, b):
        orc.set_x_ref(X[:, :, b])
        orc.set_u_ref(U[:, :, b])

    # (no iteration-count guard: with these goals and boxes no sampled instance converges within 100 iterations at any rho)
    _guard(at_rho, at_shared, _x0s(prob, batch), prepare=refs)
    s.set_x_ref_batch(vx)
    s.set_rho_batch(rhos)  # (any order)
    s.prepare()
    _set_models(s, M)
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
        _check(s, orcs, x0s, ("combined", rnd))
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info, info
    _on_d(s)
    s.reset()


def test_prepare_before_or_after_set_rho_batch_gives_the_same_bits(pkg, monkeypatch):
    first, prob, batch, _ = _handle(pkg, monkeypatch, "quadrotor20")
    then = _handle(pkg, monkeypatch, "quadrotor20")[0]
    rhos = _rhos(prob, batch)
    first.prepare()
    first.set_rho_batch(rhos)
    then.set_rho_batch(rhos)
    then.prepare()
    x0s = _x0s(prob, batch)
    for h in (first, then):
        h.set_x0_batch(x0s)
        h.solve()
        _on_d(h)
    _same(first, then)
    _check(first, {b: _oracle(_rho_problem(prob, rhos[b])) for b in (0, batch - 1)}, x0s, "prepare first")
    first.reset()
    then.reset()

"""Per-instance cone slopes (tinympc_set_cone_slopes_batch) on layout D: a batched handle that called prepare(), before or after the verb,
runs the register-resident throughput kernel in its per-instance families form -- the cone slope is the lane's instance's, read once in
front of the iteration loop -- where the row mode runs it: 16 lanes, N <= 22, references and bounds constant over the horizon, cones
without rounds. Checked against the plain-C oracle per sampled instance at the layout-A file's tolerances: the compiled-in rocket N=10
kernel, a run-time specialised horizon, slopes and per-instance rows together, slopes alone on a handle without any linear row; cones
that share rows stay on layout A and the jit info says why; and a handle that moves A -> D -> A between warm ticks keeps its duals.

problems.rocket() follows a reference TRAJECTORY, which keeps a handle on layout A: these cases hold the reference at the trajectory's
first column (instance_cone_cases.held, as test_instance_lin_d_gpu does) and draw their data at a seed of their own, at which the
oracle alone meets the sample conditions with that reference."""
from __future__ import annotations

import numpy as np
import pytest

import instance_cone_cases as K

pytestmark = pytest.mark.gpu


def _d_solver(pkg, monkeypatch, prob, batch, settings):
    """A handle that runs layout D whatever its batch size."""
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")
    return K.solver(pkg, prob, batch, settings)


def _on(s, layout, cones=True, linear=False):
    info = s.jit_info()
    assert s.launch_info()["layout"] == layout, (s.launch_info(), info)
    assert ("per-instance-cones" in info) == cones and ("per-instance-linear" in info) == linear, info
    if layout == "D":
        assert "refused" not in info, info
    return info


@pytest.mark.parametrize("name,order", [("rocket10-held", "verb first"), ("rocket10-held", "prepare first"), ("rocket20-held", "verb first"),
                                        ("rocket10-held-no-rows", "verb first")])
def test_each_instance_matches_the_oracle_on_layout_d(pkg, monkeypatch, name, order):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, name)
    own, shared, other = K.reference(pkg, name)
    K.assert_sample_conditions(name, settings, own, shared, other)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    if order == "prepare first":  # (the form is then looked for at the first launch of the mode)
        s.prepare()
        s.set_cone_slopes_batch(cx, cu)
    else:
        s.set_cone_slopes_batch(cx, cu)
        _on(s, "A")  # (without prepare(): layout A)
        s.prepare()
        _on(s, "D")
    s.set_x0_batch(x0s)
    s.solve()
    info = _on(s, "D")
    # (the rocket N=10 kernel with one row -- the shared row, or the absent one of a handle without rows -- is found by the options of
    # its plan; the other horizon is left to the run-time compiler)
    assert ("compiled-in" in info) == name.startswith("rocket10"), info
    K.assert_matches(s, own, name + " on D")
    s.reset()


def test_slopes_and_rows_per_instance_together_on_layout_d(pkg, monkeypatch):
    name = "rocket10-held"
    prob, batch, settings, x0s, cx, cu = K.data(pkg, name)
    rng = np.random.default_rng(K.SEED + 1)
    Ax = np.repeat(np.asarray(prob.linear["Alin_x"], dtype=np.float64)[:, :, None], batch, axis=2)
    bx = rng.uniform(0.0, 1.0, (1, batch))  # every instance's own ground plane, -z <= b_b
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_linear_constraints_batch(Ax, bx, None, None)
    s.prepare()
    _on(s, "D", cones=False, linear=True)
    s.set_cone_slopes_batch(cx, cu)  # (another specialisation of the form: looked for at the next launch)
    s.set_x0_batch(x0s)
    s.solve()
    _on(s, "D", cones=True, linear=True)
    expect = {}
    for b in K.sample(batch):
        orc = K.oracle(prob, settings, cx[:, b], cu[:, b])
        orc.set_linear_constraints(Ax[:, :, b], bx[:, b], np.zeros((0, prob.nu)), np.zeros(0))
        orc.update_settings()
        expect[b] = K.run(orc, x0s[:, b])
    K.assert_matches(s, expect, "slopes + rows on D")
    s.reset()


def test_cones_that_share_rows_stay_on_layout_a_and_the_info_says_why(pkg, monkeypatch):
    name = "rocket20-held-two-rounds"
    prob, batch, settings, x0s, cx, cu = K.data(pkg, name)
    own, _, _ = K.reference(pkg, name)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_cone_slopes_batch(cx, cu)
    s.prepare()
    info = _on(s, "A")
    assert "refused(" in info and "rounds" in info, info
    s.set_x0_batch(x0s)
    s.solve()
    _on(s, "A")
    K.assert_matches(s, own, name)
    s.reset()


def test_a_handle_that_moves_between_the_layouts_keeps_its_warm_start(pkg, monkeypatch):
    """Tick 0 on layout A (no prepare() yet), tick 1 on layout D, tick 2 on layout A again (a reference trajectory): the oracle is driven
    through the same three ticks with its workspace kept."""
    prob, batch, settings, x0s, cx, cu = K.data(pkg, "rocket10-held")
    settings = dict(settings, max_iter=40)
    traj = pkg.problems.rocket(10).x_ref
    samples = K.sample(batch)
    s = _d_solver(pkg, monkeypatch, prob, batch, settings)
    s.set_cone_slopes_batch(cx, cu)
    orcs = {b: K.oracle(prob, settings, cx[:, b], cu[:, b]) for b in samples}
    for tick, layout in enumerate("ADA"):
        if tick == 1:
            s.prepare()
        if tick == 2:
            s.set_x_ref(traj)
        x0t = x0s * (1.0 - 0.05 * tick)
        s.mpc_step(x0t)
        _on(s, layout)
        expect = {}
        for b in samples:
            if tick == 2:
                orcs[b].set_x_ref(traj)
            expect[b] = K.run(orcs[b], x0t[:, b])
        K.assert_matches(s, expect, ("tick", tick, layout))
    s.reset()

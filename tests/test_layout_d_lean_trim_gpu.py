"""Layout D's trimmed lean kernels (tinympc_ltrim_d.hip; tinympc_plan.hip: lean_trim_applies) against the three forms they descend from.

The variant changes no arithmetic: a lean round evaluates its priority from a clock value read one block earlier and stores d through a
per-lane address (lanes that must not store write dump rows) instead of a narrowed EXEC. So the four builds of one handle configuration --
TINYMPC_LEAN=0 (plain), TINYMPC_LEAN_START=0 (the lean kernels of tinympc_lean_d.hip), TINYMPC_LEAN_TRIM=0 (tinympc_lstart_d.hip) and
nothing set (the trimmed kernels) -- must return the same bits: states, controls, iteration counts, status and the four residuals of a cold
solve, and of the warm solve that follows it, which starts from everything the cold one wrote back (duals, slack, d, the stale v|z of
converged instances).

What can go wrong is a d store that lands where it must not, or does not land: every compiled-in 16-lane shape (quadrotor N=50: 16 of 64
lanes store; the cartpoles, nx+nu = 5: four lanes store and eleven lanes of every row are idle), the shared-table and the per-instance goal
form, batches of 1 and 5 (a partly filled wavefront: the lanes of absent instances are dump lanes), 64 and 4 x 4 + 1 (a second workgroup),
and settings that give lean runs of every length and parity, the headline's form, and lean runs that follow an iteration in which some
instances converged (their d must stay as it was written back; the others go on). `fdyn` is nonzero on every state row, as in
test_layout_d_lean_start_gpu.py.

The converging setting's tolerances were chosen on the CPU with OraclePort so that, with the x0 scales below, instances converge at the
first or second check (iteration 3 or 6) and others run to max_iter = 12; both facts are asserted here, on the oracle's result where the
oracle can state the case (shared references and bounds) and on the plain kernel's result always -- a case in which they do not hold fails.
A batch of one has one instance, so there the mixture cannot exist and only the equality is checked."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as O

pytestmark = pytest.mark.gpu

WHAT = ("states", "controls", "iterations", "status", "residuals")
BUILDS = {  # name -> (environment, the words jit_info must / must not have)
    "plain": ({"TINYMPC_LEAN": "0"}, (), ("lean", "lds-start", "trim")),
    "lean": ({"TINYMPC_LEAN_START": "0"}, ("lean",), ("lds-start", "trim")),
    "start": ({"TINYMPC_LEAN_TRIM": "0"}, ("lean", "lds-start"), ("trim",)),
    "trim": ({}, ("lean", "lds-start", "trim"), ()),
}
SWITCHES = ("TINYMPC_LEAN", "TINYMPC_LEAN_START", "TINYMPC_LEAN_TRIM")
SHAPES = ("quadrotor50", "cartpole20", "cartpole10")
# tolerances of the converging setting (max_iter 12, a check every third iteration), per shape: see the module's docstring
CONVERGING_TOL = {"quadrotor50": 0.3, "cartpole20": 3.0, "cartpole10": 1.0}
# (max_iter, check_termination, tolerance or None = the shape's converging tolerance)
SETTINGS = [(1, 0, 0.0), (2, 0, 0.0), (3, 0, 0.0), (4, 0, 0.0), (7, 0, 0.0), (7, 1, 0.0), (12, 3, None)]
X0_SCALES = np.array([0.003, 3.0, 0.03, 1.0, 0.3, 0.01, 2.0, 0.1])


def _problem(P, shape):
    prob = P.quadrotor(50) if shape == "quadrotor50" else P.cartpole(20 if shape == "cartpole20" else 10, True)
    prob.fdyn = 0.01 * np.array([(1 + (i % 5)) * (-1.0) ** i for i in range(prob.nx)])  # nonzero on every state row
    return prob


def _x0s(P, prob, shape, batch):
    sc = X0_SCALES[np.arange(batch) % 8] * (1 + 0.01 * np.arange(batch))
    base = P.quadrotor_batch_x0(batch) if shape == "quadrotor50" else np.tile(np.asarray(prob.x0, dtype=float).reshape(-1, 1), (1, batch))
    return np.asfortranarray(base * sc[None, :])


def _goals(prob, batch):
    """One goal and one box per instance (what selects the goal-form kernel), close enough to the shared ones to keep the problem's character."""
    rng = np.random.default_rng(5)
    gx, gu = 0.02 * rng.standard_normal((prob.nx, batch)), 0.005 * rng.standard_normal((prob.nu, batch))
    wx, wu = rng.uniform(0.9, 1.3, (prob.nx, batch)), rng.uniform(0.9, 1.3, (prob.nu, batch))
    xmin, xmax, umin, umax = (b[:, :1] for b in prob.expanded_bounds())  # (the problem's own box; a missing side is +-1e17, as the API fills it)
    return gx, gu, (xmin * wx, xmax * wx, umin * wu, umax * wu)


def _settings(shape, max_iter, ct, tol):
    tol = CONVERGING_TOL[shape] if tol is None else tol
    return dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=max_iter, check_termination=ct)


def _everything(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return sol["states"].copy(), sol["controls"].copy(), st["iter"].copy(), st["status"].copy(), st["residuals"].copy()


def _run(pkg, monkeypatch, shape, form, batch):
    """{build: [(cold solve, warm solve) per setting]}: one handle per build, every setting from a reset workspace."""
    P = pkg.problems
    prob = _problem(P, shape)
    x0s = _x0s(P, prob, shape, batch)
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")  # (small batches would go to the latency layouts)
    monkeypatch.setenv("TINYMPC_REFILL", "0")
    got = {}
    for name, (env, has, has_not) in BUILDS.items():
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **_settings(shape, *SETTINGS[0]))
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if form == "goal":
            gx, gu, box = _goals(prob, batch)
            s.set_x_ref_batch(gx)
            s.set_u_ref_batch(gu)
            s.set_bound_constraints_batch(*box)
        got[name] = []
        for setting in SETTINGS:
            s.update_settings(**_settings(shape, *setting))
            s.reset_workspace()
            s.set_x0_batch(x0s)
            s.solve()
            words = s.jit_info().split()
            assert s.launch_info()["layout"] == "D" and "compiled-in" in words, s.jit_info()
            assert all(w in words for w in has) and not any(w in words for w in has_not), (name, setting, s.jit_info())
            # (a batch of one has no per-instance tables: its goal and box are the shared verbs', and the shared-table kernel runs)
            assert form != "goal" or batch == 1 or "goal" in words, s.jit_info()
            cold = _everything(s)
            s.set_x0_batch(np.asfortranarray(0.9 * x0s))
            s.solve()
            got[name].append((cold, _everything(s)))
        s.reset()
    return got


def _mixed(it, status, max_iter=12):
    it, status = np.asarray(it), np.asarray(status)
    return bool(np.any((status == 1) & (it <= 6)) and np.any(it == max_iter))


@pytest.mark.parametrize("batch", [1, 5, 64, 17])
@pytest.mark.parametrize("form", ["shared", "goal"])
@pytest.mark.parametrize("shape", SHAPES)
def test_four_builds_return_the_same_bits(pkg, monkeypatch, shape, form, batch):
    got = _run(pkg, monkeypatch, shape, form, batch)
    for k, setting in enumerate(SETTINGS):
        for other in ("plain", "lean", "start"):
            for w, solve in enumerate(("cold", "warm")):
                for a, b, what in zip(got[other][k][w], got["trim"][k][w], WHAT):
                    np.testing.assert_array_equal(a, b, err_msg=f"{shape} {form} batch={batch} (max_iter, ct, tol)={setting}: {solve} solve against the {other} kernel: {what}")
        max_iter, ct, tol = setting
        it, status = got["trim"][k][0][2], got["trim"][k][0][3]
        if tol is not None:  # forced iteration counts
            assert np.all(it == max_iter) and np.all(status != 1), (setting, it, status)
        elif batch > 1:
            assert _mixed(got["plain"][k][0][2], got["plain"][k][0][3]), (shape, form, batch, got["plain"][k][0][2], got["plain"][k][0][3])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_converging_tolerances_mix_early_and_late_instances_on_the_oracle(pkg, shape):
    """The CPU side of the converging setting (no kernel runs here; the module is a GPU module because its subject is): with shared
    references and bounds the oracle converges some instances of every batch size used above at the first or second check and runs others
    to max_iter."""
    P = pkg.problems
    prob = _problem(P, shape)
    settings = _settings(shape, 12, 3, None)
    orc = O.OraclePort(prob).load_problem(prob, settings)
    _, _, it, status, _ = orc.solve_batch(_x0s(P, prob, shape, 64))
    for batch in (5, 17, 64):  # (instance i has the same x0 in every batch)
        assert _mixed(it[:batch], status[:batch]), (shape, batch, it[:batch], status[:batch])

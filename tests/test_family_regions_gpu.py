"""Every kernel that carries the cone and half-space families, on inputs that take every outcome of both projections.

The projections are selects on the device, and their arithmetic exists in several separately maintained places: soc_project_element /
halfspace_project_element (tinympc_sweep.h: layouts A, C, D, the wide reduction form of tinympc_fam_red.h, layout M's phase between the
sweeps), project_cone (tinympc_solve_e_common.h: layouts E and F) and the per-instance rows variant k_admm_solve_ifam. The other family
tests reach them through the rocket's nominal landing, where at short horizons the state cone is a no-op, the row is never violated
and no input ever lies in the polar cone. Here each kernel solves the data sets of family_region_cases.py, whose ORACLE census takes
each of the eight outcomes in at least 2 % of its side's projections and mixes outcomes over the knots of one iteration
(test_family_regions_cpu.py asserts the same for the same data without a GPU; each test below asserts it again for exactly what it
compares, on the oracle, before anything runs on the device).

Per case two settings -- 40 forced iterations, and max_iter = 120 with tolerances 2e-3 / 1e-4 -- and per setting two solves: cold, then
from the duals the first left with the states rotated by one instance, so that the warm start lands in another region (a single
instance takes the six states in turn, twice: twelve warm-started solves). Every instance against its state's oracle solution:
iteration counts and statuses identical, states and controls within 1e-9 relative, and the four residuals of the last check within
1e-6 on every kernel (the projection of a solve's last iteration shows in the slack and the residuals, not in the trajectories). Each
kernel is forced the way its own test forces it, at shapes those tests specialise."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import family_region_cases as F

pytestmark = pytest.mark.gpu
TOL = 1e-9
JIT_ORIGINS = ("compiled ", "disk-cache ", "compiled-in ")


def _handle(pkg, prob, settings, batch):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_cone_constraints(**prob.cones)
    s.set_linear_constraints(**prob.linear)
    if prob.x_ref is not None:
        s.set_x_ref(prob.x_ref)
    if prob.u_ref is not None:
        s.set_u_ref(prob.u_ref)
    return s


def _compare(s, expect, tag):
    """Every instance of the handle's last solve against expect[b] (a family_region_cases.Solve): iterations, statuses, trajectories and
    the four residuals of the last check (primal / dual state, primal / dual input). -> the largest relative error of a trajectory."""
    batch = len(expect)
    if batch == 1:  # the single-instance verbs
        one, st1 = s.get_solution(), s.get_stats()
        sol = dict(states=one["states"][:, :, None], controls=one["controls"][:, :, None])
        res = [st1[k] for k in ("primal_residual_state", "dual_residual_state", "primal_residual_input", "dual_residual_input")]
        st = dict(iter=np.array([st1["iter"]]), status=np.array([st1["status"]]), residuals=np.array(res)[:, None])
    else:
        sol, st = s.get_solution_batch(), s.get_stats_batch()
    np.testing.assert_array_equal(st["iter"], np.array([e.iter for e in expect]), err_msg=tag)
    np.testing.assert_array_equal(st["status"], np.array([e.status for e in expect]), err_msg=tag)
    worst = 0.0
    for b, e in enumerate(expect):
        ex, eu = rel_err(sol["states"][:, :, b], e.states), rel_err(sol["controls"][:, :, b], e.controls)
        worst = max(worst, ex, eu)
        assert ex < TOL and eu < TOL, (tag, b, ex, eu)
    er = rel_err(st["residuals"], np.array([e.residuals for e in expect]).T)
    print(tag, "iterations %d..%d, largest relative error %.2e, residuals %.2e" % (st["iter"].min(), st["iter"].max(), worst, er))
    assert er < 1e-6, (tag, er)
    return worst


def _two_solves(s, x0s, per_instance, tag, after_first=None):
    """Cold from x0s, then warm from the rotated states; per_instance[b] = [cold Solve, warm Solve] of instance b."""
    for rnd, xs in enumerate((x0s, F.rotated(x0s))):
        s.set_x0_batch(np.asfortranarray(xs))
        s.solve()
        if rnd == 0 and after_first is not None:
            after_first(s)
        _compare(s, [p[rnd] for p in per_instance], "%s solve %d" % (tag, rnd))


def _rocket_batch(batch):
    """The six states repeated cyclically: instance b starts from state b % 6 and continues, warm, from state (b + 1) % 6."""
    idx = np.arange(batch) % 6
    return np.asfortranarray(F.ROCKET_X0[:, idx]), idx


def _force(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _rocket_case(pkg, monkeypatch, N, kernel, setting, env, check, prepare=False):
    """One kernel (a key of family_region_cases.ROCKET_BATCHED) on rocket(N) x its batch under one setting. env: the variables that force the
    kernel; check(s): its layout / jit_info asserts."""
    _force(monkeypatch, env)
    horizons, batch = F.ROCKET_BATCHED[kernel]
    assert N in horizons
    tag = "%s rocket N=%d x %d %s" % (kernel, N, batch, setting)
    ref = F.rocket_reference(pkg.problems, N, setting)
    x0s, idx = _rocket_batch(batch)
    F.assert_covered(F.flat(ref), tag, F.batch_weights(batch))
    s = _handle(pkg, pkg.problems.rocket(N, with_linear=True), F.SETTINGS[setting], batch)
    if prepare:
        s.prepare()
        check(s)
    # (the second solve's states come from the state index, not from rolling the columns: the ragged last column's successor is column 0)
    for rnd, xs in enumerate((x0s, np.asfortranarray(F.ROCKET_X0[:, (idx + 1) % 6]))):
        s.set_x0_batch(xs)
        s.solve()
        if rnd == 0:
            check(s)
        _compare(s, [ref[i][rnd] for i in idx], "%s solve %d" % (tag, rnd))
    s.reset()


def _rocket_single(pkg, monkeypatch, N, setting, env, check, tag=""):
    """One kernel on ONE instance of rocket(N) through the single-instance verbs. One instance cannot carry six states at once, so it takes
    them in turn: twelve warm-started solves, the six states and then the six again (the census of exactly these twelve is asserted)."""
    _force(monkeypatch, env)
    tag = "%s rocket N=%d x 1 %s" % (tag, N, setting)
    ticks = F.rocket_session_reference(pkg.problems, N, setting)
    F.assert_covered(ticks, tag)
    s = _handle(pkg, pkg.problems.rocket(N, with_linear=True), F.SETTINGS[setting], 1)
    for k, e in enumerate(ticks):
        s.set_x0(F.ROCKET_X0[:, k % 6])
        s.solve()
        if k == 0:
            check(s)
        _compare(s, [e], "%s solve %d" % (tag, k))
    s.reset()


SETTINGS = list(F.SETTINGS)


# ---- layout A: k_admm_solve_fam

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("N", [10, 30])
def test_layout_a(pkg, monkeypatch, N, setting):
    def check(s):
        assert s.launch_info()["layout"] == "A", s.jit_info()
    _rocket_case(pkg, monkeypatch, N, "layout A", setting, {"TINYMPC_LAYOUT": "A"}, check)


# ---- layout C: the latency kernel's families variant, one instance per workgroup

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("batch", [1, 6])
def test_layout_c(pkg, monkeypatch, batch, setting):
    def check(s):
        assert s.launch_info()["layout"] == "C", s.jit_info()
    if batch == 1:
        _rocket_single(pkg, monkeypatch, 20, setting, {"TINYMPC_LAYOUT": "C"}, check, tag="layout C")
    else:
        _rocket_case(pkg, monkeypatch, 20, "layout C", setting, {"TINYMPC_LAYOUT": "C"}, check)


# ---- layout D with the families in registers (test_hip_families.test_families_on_layout_d)

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("N", [10, 20, 28])
def test_layout_d(pkg, monkeypatch, N, setting):
    """TINYMPC_LAYOUT=D holds the families in registers up to N = 22, so N = 10 and 20 run layout D. N = 28 does NOT: as in that test, it
    runs the library's own choice for a large batch, which is layout E's cut form on the 512-register plan (and is labelled so)."""
    def check(s):
        info = s.jit_info()
        if N <= 22:
            assert s.launch_info()["layout"] == "D", info
        else:
            assert s.launch_info()["layout"] == "E" and "uncut" not in info, info
    kernel = "layout D" if N <= 22 else "layout E, cut (the library's choice)"
    _rocket_case(pkg, monkeypatch, N, kernel, setting, {"TINYMPC_JIT": "1", "TINYMPC_LAYOUT": "D" if N <= 22 else None}, check)


# ---- layout E, uncut and cut (test_hip_families.test_families_on_layout_e)

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("N", [10, 44, 100])
def test_layout_e(pkg, monkeypatch, N, setting):
    def check(s):
        info = s.jit_info()
        assert ("uncut" in info) == (N == 10), info
        assert s.launch_info()["layout"] == "E" and info.startswith(JIT_ORIGINS) and "scratch=0" in info, info
    _rocket_case(pkg, monkeypatch, N, "layout E", setting, {"TINYMPC_LAYOUT": "E"}, check, prepare=True)


# ---- layout F: one wavefront (N = 10), chunked (20, 44), compiled in (100) (test_hip_families.test_layout_f_the_specialised_latency_kernel)

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("batch", [1, 7])
@pytest.mark.parametrize("N", [10, 20, 44, 100])
def test_layout_f(pkg, monkeypatch, N, batch, setting):
    """(batch 1: the single-instance verbs -- pinned-host x0, solution and completion stamp; batch 7 = 6 + 1: the batched verbs)"""
    def check(s):
        info = s.jit_info()
        assert s.launch_info()["layout"] == "F", info
        assert info.startswith(JIT_ORIGINS) and "layout=F" in info and "scratch=0" in info, info
    if batch == 1:
        _rocket_single(pkg, monkeypatch, N, setting, {"TINYMPC_LAYOUT": "F"}, check, tag="layout F")
    else:
        _rocket_case(pkg, monkeypatch, N, "layout F", setting, {"TINYMPC_LAYOUT": "F"}, check)


# ---- the resident session on layout F (test_session_gpu.test_session_with_per_tick_references_and_families)

@pytest.mark.parametrize("setting", SETTINGS)
def test_session_on_layout_f(pkg, monkeypatch, setting):
    """Twelve ticks of one resident instance: the six states in turn, then the six again, each tick warm from the one before."""
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    ticks = F.rocket_session_reference(pkg.problems, 10, setting)
    F.assert_covered(ticks, "session rocket N=10 %s" % setting)
    prob = pkg.problems.rocket(10, with_linear=True)
    s = _handle(pkg, prob, F.SETTINGS[setting], 1)
    s.session_begin()
    assert s.launch_info()["layout"] == "F"
    worst = 0.0
    for k, e in enumerate(ticks):
        u0 = s.session_step(F.ROCKET_X0[:, k % 6])
        worst = max(worst, _compare(s, [e], "session rocket N=10 %s tick %d" % (setting, k)))
        np.testing.assert_array_equal(u0, s.get_solution()["controls"][:, 0])
    print("session rocket N=10", setting, "largest relative error %.2e" % worst)
    s.session_end()
    s.reset()


# ---- the per-instance rows variant, k_admm_solve_ifam (test_instance_lin_gpu)

@pytest.mark.parametrize("setting", SETTINGS)
def test_per_instance_rows(pkg, monkeypatch, setting):
    """The rocket's ground-plane row with a b of its own per instance (family_region_cases.ROCKET_ROW_B: above and below the ground, and
    +inf -- a row that is there and never violated)."""
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    N, batch = 10, F.ROCKET_ROWS_BATCH
    ref = F.rocket_rows_reference(pkg.problems, N, setting)
    x0s, idx = _rocket_batch(batch)
    F.assert_covered(F.flat(ref), "per-instance rows rocket N=10 x %d %s" % (batch, setting), F.batch_weights(batch))
    prob = pkg.problems.rocket(N, with_linear=True)
    s = _handle(pkg, prob, F.SETTINGS[setting], batch)
    Ax = np.repeat(np.asarray(prob.linear["Alin_x"], dtype=np.float64)[:, :, None], batch, axis=2)
    bx = F.ROCKET_ROW_B[idx][None, :]
    assert np.isinf(bx).sum() >= 2 and len(set(bx[0, :6])) == 6
    s.set_linear_constraints_batch(Ax, bx, None, None)
    assert s.launch_info()["layout"] == "A" and "per-instance-linear" in s.jit_info()
    for rnd, xs in enumerate((x0s, np.asfortranarray(F.ROCKET_X0[:, (idx + 1) % 6]))):
        s.set_x0_batch(xs)
        s.solve()
        assert s.launch_info()["layout"] == "A" and "per-instance-linear" in s.jit_info()
        _compare(s, [ref[i][rnd] for i in idx], "per-instance rows %s solve %d" % (setting, rnd))
    s.reset()


# ---- layout D's wide kernels: 32 and 64 lanes per instance, tinympc_fam_red.h (test_hip_families.test_families_on_wide_systems)

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("shape", F.WIDE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_wide_systems(pkg, monkeypatch, shape, setting):
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    nx, nu, N, batch = shape
    prob, x0s, ref = F.wide_reference(pkg.problems, nx, nu, N, batch, setting)
    F.assert_covered(F.flat(ref), "wide %s %s" % (shape, setting))
    s = _handle(pkg, prob, F.SETTINGS[setting], batch)

    def check(h):
        assert h.launch_info()["layout"] == "D", h.jit_info()
    _two_solves(s, x0s, ref, "wide %s %s" % (shape, setting), after_first=check)
    s.reset()


# ---- layout M's cone phase between the sweeps (test_large_systems_gpu.test_families_on_large_systems)

@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("shape", F.LARGE_SHAPES, ids=lambda v: "x".join(map(str, v)).replace(" ", "-"))
def test_large_systems(pkg, monkeypatch, shape, setting):
    """One pass over all rows (up to eight linear rows per side) and a pass per row (ten rows), at the smallest shape that test runs them."""
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    monkeypatch.delenv("TINYMPC_M_FAM_FAST", raising=False)
    nx, nu, N, batch, form = shape
    prob, x0s, ref = F.large_reference(pkg.problems, nx, nu, N, batch, form, setting)
    F.assert_covered(F.flat(ref), "large %s %s" % (shape, setting))
    s = _handle(pkg, prob, F.SETTINGS[setting], batch)

    def check(h):
        assert h.launch_info()["layout"] == "M", h.jit_info()
    _two_solves(s, x0s, ref, "large %s %s" % (shape, setting), after_first=check)
    s.reset()

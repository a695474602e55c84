"""Every implementation of the precompute's inverse on systems where its pivot search swaps rows (tests/pivot_swap_cases.py; the
inputs' own conditions are tests/test_pivot_swap_cpu.py): rows_inverse (k_precompute_rows, single and batched), wg_lu_inverse
(k_precompute in LDS and in global scratch, single and batched, and k_lqr behind the class helpers), k_lu_inverse and k_gain_solve
(layout M, nu <= 64 and beyond) -- the row swaps, the permutation, the lane a result row is fetched from and the right-hand side
P e_c, none of which any other system of the suite reaches. Against the oracle at the project's tolerances: caches 1e-10 (rows
against the LDS kernel 1e-11) up to 64 rows, 1e-9 on layout M; solves 1e-9, iteration counts equal. The case (80, 66) is also the
first solve with more than 64 input rows."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import matlab_class_oracle as M
import pivot_swap_cases as S
import pyoracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.layouts("C")]  # (the precompute does not depend on the solve kernel: once, not once per layout)

TOL = 1e-9            # solves (test_hip_parity.py, test_large_systems_gpu.py)
TOL_CACHE = 1e-10     # caches against the oracle, nx+nu <= 64 (test_hip_parity.py)
TOL_CACHE_M = 1e-9    # ... layout M (test_large_systems_gpu.py)
TOL_ROWS_LDS = 1e-11  # k_precompute_rows against k_precompute on the same handle data (test_hip_parity.py)
MATS = ("Kinf", "Pinf", "Quu_inv", "AmBKt")
FDYN_CASES = ("rows6x3", "lds20x6", "global48x16", "large70x14", "gain80x66")  # one per form


@pytest.fixture(autouse=True)
def kernel_layout(request, monkeypatch):
    monkeypatch.setenv("TINYMPC_LAYOUT", request.param)
    return request.param


_memo = {}


def _oracle_cache(pkg, name):
    """The case's cache from the oracle (box problem: the reference's own core where it is built) and its Riccati step count, computed
    once and shared (read-only) by the tests here."""
    if name not in _memo:
        prob = S.problem(pkg.problems, name)
        port = O.OraclePort(prob)
        orc = O.OracleRef(prob) if O.ref_available() else port
        _memo[name] = ({n: orc.get(n) for n in MATS}, port.stats()["riccati_iters"])
    return _memo[name]


def _cache(pkg, prob):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho, fdyn=prob.fdyn)
    c = s.get_cache()
    s.reset()
    return c


@pytest.mark.parametrize("name", list(S.CASES))
def test_cache_of_every_case_matches_the_oracle(pkg, monkeypatch, name):
    nx, nu, form = S.CASES[name]
    prob = S.problem(pkg.problems, name)
    ref, steps = _oracle_cache(pkg, name)
    tol = TOL_CACHE_M if S.layout_m(name) else TOL_CACHE
    monkeypatch.delenv("TINYMPC_PRECOMPUTE", raising=False)
    c = _cache(pkg, prob)
    worst = max(rel_err(c[n], ref[n]) for n in MATS)
    print("pivot-swap cache %-12s (%s): worst rel_err against the oracle %.2e, steps %d (oracle %d)" % (name, form, worst, c["riccati_iters"], steps))
    for n in MATS:
        assert rel_err(c[n], ref[n]) < tol, (name, n)
    assert c["riccati_iters"] == steps
    if form == "rows":  # the same handle data through the one-workgroup LDS kernel
        monkeypatch.setenv("TINYMPC_PRECOMPUTE", "lds")
        l = _cache(pkg, prob)
        monkeypatch.delenv("TINYMPC_PRECOMPUTE")
        worst_l = max(rel_err(l[n], ref[n]) for n in MATS)
        worst_rl = max(rel_err(c[n], l[n]) for n in MATS)
        print("pivot-swap cache %-12s (lds): worst rel_err against the oracle %.2e, rows against lds %.2e" % (name, worst_l, worst_rl))
        for n in MATS:
            assert rel_err(l[n], ref[n]) < tol, (name, n, "lds")
            assert rel_err(c[n], l[n]) < TOL_ROWS_LDS, (name, n, "rows vs lds")
        assert l["riccati_iters"] == steps


@pytest.mark.parametrize("name", FDYN_CASES)
def test_affine_terms_behind_a_swapping_inverse(pkg, monkeypatch, name):
    """fdyn set: the cache against the restatement (the reference's snapshot has no fdyn), and APf / BPf -- computed behind the last
    inverse -- through one short solve from a non-zero state; the rows case also through the LDS kernel."""
    nx, nu, form = S.CASES[name]
    prob = S.problem(pkg.problems, name)
    prob.fdyn = 0.05 * np.random.default_rng(nx + nu).standard_normal(nx)
    settings = dict(max_iter=12, abs_pri_tol=0.0, abs_dua_tol=0.0)
    orc = O.OraclePort(prob).load_problem(prob, settings)
    orc.solve()
    tol = TOL_CACHE_M if S.layout_m(name) else TOL_CACHE
    sols = {}
    for mode in (("rows", "lds") if form == "rows" else (form,)):
        if mode == "lds" and form == "rows":
            monkeypatch.setenv("TINYMPC_PRECOMPUTE", "lds")
        else:
            monkeypatch.delenv("TINYMPC_PRECOMPUTE", raising=False)
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho, fdyn=prob.fdyn)
        c = s.get_cache()
        for n in MATS:
            assert rel_err(c[n], orc.get(n)) < tol, (name, mode, n)
        assert c["riccati_iters"] == orc.stats()["riccati_iters"]
        s.set_x0(prob.x0)
        s.update_settings(**settings)
        s.solve()
        sol = s.get_solution()
        ex, eu = rel_err(sol["states"], orc.solution()[0]), rel_err(sol["controls"], orc.solution()[1])
        print("pivot-swap fdyn %-12s (%s): solve rel_err x %.2e u %.2e" % (name, mode, ex, eu))
        assert s.get_stats()["iter"] == orc.stats()["iter"] == 12
        assert ex < TOL and eu < TOL, (name, mode, ex, eu)
        sols[mode] = sol["controls"]
        s.reset()
    monkeypatch.delenv("TINYMPC_PRECOMPUTE", raising=False)
    if form == "rows":
        assert rel_err(sols["rows"], sols["lds"]) < TOL


@pytest.mark.parametrize("name", list(S.CASES))
def test_solve_on_a_swapping_cache(pkg, name):
    """Batch 5 (layout M: 17, one ragged tile), input clamp active, fifteen forced iterations, against the oracle."""
    ref, _ = _oracle_cache(pkg, name)
    prob, x0s = S.solve_problem(pkg.problems, name, ref["Kinf"])
    batch = x0s.shape[1]
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, **S.SOLVE_SETTINGS)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x0_batch(x0s)
    s.solve()
    if S.layout_m(name):
        assert s.launch_info()["layout"] == "M"  # (80, 66): the first solve with more than 64 input rows
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    orc = O.OraclePort(prob).load_problem(prob, S.SOLVE_SETTINGS)
    ox, ou, oit, ost, _ = orc.solve_batch(x0s)
    ex, eu = rel_err(sol["states"], ox), rel_err(sol["controls"], ou)
    print("pivot-swap solve %-12s layout %s: rel_err x %.2e u %.2e" % (name, s.launch_info()["layout"], ex, eu))
    assert np.isclose(np.abs(ou), prob.u_max[0], rtol=0, atol=1e-12).any()  # the clamp is active
    np.testing.assert_array_equal(st["iter"], oit)
    np.testing.assert_array_equal(st["status"], ost)
    assert ex < TOL and eu < TOL, (name, ex, eu)
    s.reset()


@pytest.mark.parametrize("nx,nu", [(6, 3), (20, 6)])
def test_batched_precompute_with_swapping_and_tame_neighbours(pkg, monkeypatch, nx, nu):
    """set_model_batch on a (6, 3) handle (batched k_precompute_rows) and a (20, 6) handle (k_precompute<true>): odd instances swap in
    every step, even ones never. Each instance against its own oracle and bit-equal to a single-instance setup of its model
    (include/tinympc_hip.h): pivot state -- used, mine, perm[n] -- that leaked between neighbours would break either."""
    monkeypatch.delenv("TINYMPC_LAYOUT")  # (per-instance models: the library's own choice of solve kernel; nothing is solved here)
    monkeypatch.delenv("TINYMPC_PRECOMPUTE", raising=False)
    batch = 9
    base, A, B, Q, R, probs = S.mixed_models(pkg.problems, nx, nu, 6, batch)
    s = pkg.TinyMPC()
    s.setup(base.A, base.B, base.Q, base.R, base.N, batch=batch, rho=base.rho)
    s.set_model_batch(A, B, Q, R)
    whole = s.get_cache_batch()
    worst = 0.0
    for b, pb in enumerate(probs):
        orc = O.OraclePort(pb)
        one = _cache(pkg, pb)
        for n in MATS:
            e = rel_err(whole[n][:, :, b], orc.get(n))
            worst = max(worst, e)
            assert e < TOL_CACHE, (n, b, e)
            np.testing.assert_array_equal(whole[n][:, :, b], one[n], err_msg="%s instance %d" % (n, b))
        assert whole["riccati_iters"][b] == one["riccati_iters"] == orc.stats()["riccati_iters"], b
    print("pivot-swap batched precompute (%d, %d): worst rel_err against the oracles %.2e, steps %s" % (nx, nu, worst, list(whole["riccati_iters"])))
    s.reset()


@pytest.mark.parametrize("name", ["rows6x3", "lds20x6", "global48x16"])
def test_class_helpers_on_swapping_systems(pkg, monkeypatch, name):
    """solve_lqr(rho) and compute_cache_terms() (k_lqr: wg_lu_inverse twice, in LDS and -- (48, 16) -- in global scratch) against the
    class restatement, at the tolerances of test_matlab_class_helpers.py."""
    monkeypatch.delenv("TINYMPC_LAYOUT")
    p = S.problem(pkg.problems, name)
    nx, nu = p.B.shape
    s = pkg.TinyMPC()
    s.setup(p.A, p.B, p.Q, p.R, p.N, rho=p.rho)
    for rho in (p.rho, 3.7 * p.rho):
        got = s.solve_lqr(rho)
        want = M.solve_lqr(p.A, p.B, p.Q, p.R, rho)
        worst = max(rel_err(g, w) for g, w in zip(got, want))
        print("pivot-swap solve_lqr %-12s rho %.2f: worst rel_err %.2e" % (name, rho, worst))
        for g, w in zip(got, want):
            assert rel_err(g, w) < 1e-9
        assert M.dare_residual(p.A, p.B, p.Q + rho * np.eye(nx), p.R + rho * np.eye(nu), got[1]) < 1e-11
    got = s.compute_cache_terms()
    Ko, Po, Qio, Amo, it = M.compute_cache_terms(p.A, p.B, p.Q, p.R, p.rho)
    worst = max(rel_err(g, w) for g, w in zip(got, (Ko, Po, Qio, Amo)))
    print("pivot-swap compute_cache_terms %-12s: worst rel_err %.2e, steps %d (restatement %d)" % (name, worst, s.cache_terms_iters, it))
    assert abs(s.cache_terms_iters - it) <= 1  # the stopping norm sits at 1e-10: one step of slack
    for g, w in zip(got, (Ko, Po, Qio, Amo)):
        assert rel_err(g, w) < 1e-8
    s.reset()

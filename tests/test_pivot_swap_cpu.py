"""The inputs of tests/test_pivot_swap_gpu.py do what they are for (no GPU): conditions on tests/pivot_swap_cases.py, not
measurements. Every case's S = R1 + B'PB swaps rows under partial pivoting in (all but at most one of) its Riccati steps and in the
S of Quu_inv, stays moderately conditioned, and stops its Riccati iteration far from the threshold; the three float64 references
(the numpy restatement, the plain-C oracle, the reference's own core where it is built) agree on these systems to 1e-12 -- the first
pin of the oracle's own swap branch; and the systems the suite had before do not swap at all, which is why these exist."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pivot_swap_cases as S
import pyoracle as O

MATS = ("Kinf", "Pinf", "Quu_inv", "AmBKt")
_memo = {}


def _ref(pkg, name):
    """The numpy restatement of a case, computed once and shared (read-only) by every test here."""
    if name not in _memo:
        _memo[name] = S.riccati(S.problem(pkg.problems, name))
    return _memo[name]


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_case_swaps_is_well_conditioned_and_stops_clear_of_the_threshold(pkg, name):
    r = _ref(pkg, name)
    steps = r["riccati_iters"]
    swapping = sum(1 for pos in r["pivots"] if S.swaps(pos) > 0)
    cond = float(np.linalg.cond(r["S"]))
    stop, before = r["diffs"][-1], r["diffs"][-2]
    print("pivot-swap case %-12s steps %3d, with a swap %3d, final S swaps %d, cond(S) %.3g, stopping difference %.4g (before it %.4g)"
          % (name, steps, swapping, S.swaps(r["final"][0]), cond, stop, before))
    assert 2 <= steps < 1000
    assert swapping >= steps - 1, "at least all but one Riccati step must swap"
    assert S.swaps(r["final"][0]) > 0, "the S of Quu_inv must swap"
    assert cond <= 1e4
    # the step count cannot depend on a summation order: both differences four orders above anything rounding moves
    assert stop < 1e-5 - 1e-8 and before > 1e-5 + 1e-8


def test_shape_of_the_swaps_over_the_table(pkg):
    last_row = two_swaps = False
    for name, (nx, nu, form) in S.CASES.items():
        r = _ref(pkg, name)
        for pos in r["pivots"] + [r["final"][0]]:
            last_row = last_row or bool(np.any(pos[:-1] == nu - 1))   # a column before the last takes the LAST row as its pivot
            two_swaps = two_swaps or (nu >= 3 and S.swaps(pos) >= 2)  # two or more swaps in one factorisation
        if form == "rows":
            # the zero-padded class sees blockdiag(S, I): no real column may take a padding row (rows >= nu) as its pivot, in any step
            nup = S.rows_class(nx, nu)[1]
            prob = S.problem(pkg.problems, name)
            B, R1 = prob.B, np.diag(np.diag(prob.R) + 2.0 * prob.rho)
            Pm, seen = prob.rho * np.eye(nx), 0
            A, Q1 = prob.A, np.diag(np.diag(prob.Q) + 2.0 * prob.rho)
            for _ in range(r["riccati_iters"] + 1):  # (every step's S, and the S of Quu_inv)
                Sp = np.eye(nup)
                Sp[:nu, :nu] = R1 + B.T @ Pm @ B
                pos, src = S.pivots(Sp)
                assert np.all(src[:nu] < nu), (name, src)
                seen += S.swaps(pos[:nu])
                K = np.linalg.solve(Sp[:nu, :nu], B.T @ Pm @ A)
                Pm = Q1 + A.T @ Pm @ (A - B @ K)
            assert seen > 0, name
    assert last_row and two_swaps


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_three_references_agree(pkg, name):
    """OraclePort (lu_inverse of oracle/tinympc_oracle.c, swapping) against numpy / LAPACK: < 1e-12 on all four matrices, equal step
    counts. (The reference's own core is compared in the test below, where it is built.)"""
    prob, r = S.problem(pkg.problems, name), _ref(pkg, name)
    orc = O.OraclePort(prob)
    worst = max(rel_err(orc.get(n), r[n]) for n in MATS)
    print("pivot-swap case %-12s oracle against numpy: worst %.2e, steps %d / %d" % (name, worst, orc.stats()["riccati_iters"], r["riccati_iters"]))
    for n in MATS:
        assert rel_err(orc.get(n), r[n]) < 1e-12, n
    assert orc.stats()["riccati_iters"] == r["riccati_iters"]


@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref/libtinympc_ref.so not built (needs the reference tree)")
@pytest.mark.parametrize("name", list(S.CASES))
def test_the_reference_core_agrees(pkg, name):
    """Eigen's PartialPivLU inside the reference's own tiny_precompute_and_set_cache against numpy and the oracle. (The core does not
    report its step count; one step more or less would move Kinf by ~1e-5, seven orders above the bound.)"""
    prob, r = S.problem(pkg.problems, name), _ref(pkg, name)
    ref, orc = O.OracleRef(prob), O.OraclePort(prob)
    for n in MATS:
        assert rel_err(ref.get(n), r[n]) < 1e-12, n
        assert rel_err(orc.get(n), ref.get(n)) < 1e-12, n


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_short_solve_clamps(pkg, name):
    """The solve the GPU test runs on each cache has its input clamp active, and runs all fifteen iterations."""
    prob, x0s = S.solve_problem(pkg.problems, name, _ref(pkg, name)["Kinf"])
    orc = O.OraclePort(prob).load_problem(prob, S.SOLVE_SETTINGS)
    _, ou, oit, _, _ = orc.solve_batch(x0s)
    assert np.all(oit == S.SOLVE_SETTINGS["max_iter"])
    at_bound = np.isclose(np.abs(ou), prob.u_max[0], rtol=0, atol=1e-12)
    print("pivot-swap case %-12s short solve: %d of %d instances sit on an input bound somewhere" % (name, int(at_bound.any(axis=(0, 1)).sum()), x0s.shape[1]))
    assert at_bound.any(), "the clamp must be active"
    assert not at_bound.all(), "... and not everywhere"


def test_mixed_models_alternate_swapping_and_tame_instances(pkg):
    for nx, nu in ((6, 3), (20, 6)):
        probs = S.mixed_models(pkg.problems, nx, nu, 6, 9)[-1]
        for b, pb in enumerate(probs):
            r = S.riccati(pb)
            swapping = sum(1 for pos in r["pivots"] if S.swaps(pos) > 0)
            assert (swapping >= r["riccati_iters"] - 1 and S.swaps(r["final"][0]) > 0) if b % 2 else (swapping == 0 and S.swaps(r["final"][0]) == 0), (nx, nu, b)
            assert r["diffs"][-1] < 1e-5 - 1e-8 and r["diffs"][-2] > 1e-5 + 1e-8, (nx, nu, b)


@pytest.mark.parametrize("name", ["rows6x3", "lds20x6", "global48x16"])
def test_class_helper_recursions_swap_and_their_reference_is_sound(pkg, name):
    """The class's recursions (rho once, full Q and R, P0 = Q: oracle/matlab_class_oracle.py) on the cases the GPU test runs them on:
    their first and their stationary S swap too, and scipy's DARE solution -- the reference of solve_lqr at 1e-9 -- equals the
    recursion run to stationarity in numpy to 1e-12."""
    import matlab_class_oracle as M
    p = S.problem(pkg.problems, name)
    nx, nu = p.B.shape
    for rho in (p.rho, 3.7 * p.rho):
        K, Pd, C1, C2 = M.solve_lqr(p.A, p.B, p.Q, p.R, rho)
        Qr, Rr = p.Q + rho * np.eye(nx), p.R + rho * np.eye(nu)
        assert S.swaps(S.pivots(Rr + p.B.T @ Qr @ p.B)[0]) > 0 and S.swaps(S.pivots(Rr + p.B.T @ Pd @ p.B)[0]) > 0
        assert np.linalg.cond(Rr + p.B.T @ Pd @ p.B) <= 1e4
        Pi = Qr.copy()
        for _ in range(5000):
            Ki = np.linalg.solve(Rr + p.B.T @ Pi @ p.B, p.B.T @ Pi @ p.A)
            Pn = Qr + p.A.T @ Pi @ (p.A - p.B @ Ki)
            done = np.max(np.abs(Pn - Pi)) < 1e-15 * np.max(np.abs(Pn))
            Pi = Pn
            if done:
                break
        Ki = np.linalg.solve(Rr + p.B.T @ Pi @ p.B, p.B.T @ Pi @ p.A)
        assert rel_err(K, Ki) < 1e-12 and rel_err(Pd, Pi) < 1e-12 and rel_err(C2, (p.A - p.B @ Ki).T) < 1e-12
        assert rel_err(C1, np.linalg.inv(Rr + p.B.T @ Pi @ p.B)) < 1e-12


def test_the_gap_stays_recorded(pkg):
    """The systems the suite had before never swap: the quadrotor, and _system(70, 14) of test_large_systems_gpu.py (restated)."""
    P = pkg.problems
    for prob in (P.quadrotor(20), S.tame_large_system(P, 70, 14, 10, 84)):
        r = S.riccati(prob)
        assert r["riccati_iters"] > 20
        assert sum(S.swaps(pos) for pos in r["pivots"]) == 0 and S.swaps(r["final"][0]) == 0

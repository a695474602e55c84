"""Every cut of a layout D launch into runs of lean rounds (the loop behind the `iteration` lambda of tinympc_solve_d.hip), on every lean
build: plain (TINYMPC_LEAN=0), lean (TINYMPC_LEAN_START=0), start (TINYMPC_LEAN_TRIM=0), trim (TINYMPC_LEAN_SHARE=0), share
(TINYMPC_LEAN_PARK=0) and park (nothing set). (test_layout_d_lean_park_gpu.py's converging setting gives runs of six that end on a check,
test_layout_d_lean_trim_gpu.py's runs of two: the tails behind the last check and the handovers between the builds' kernels are here.)

The settings grid, its classes of cuts and the oracle's conditions are those of tests/lean_run_cases.py, checked without a GPU by
tests/test_lean_run_structure_cpu.py: max_iter below, on and behind every check, so that a launch ends on a check, in a tail run of one to
seven rounds behind dead rows (parked status 1 and it_done < max_iter, then the final write-back with no iteration with residuals between),
or in a single run that is its own tail; four tolerance pairs (none, both, and each alone -- not reachable, and the host's lean_applies must
agree with the kernel's nres about it); a cold solve from reset_workspace and the warm solve behind it. No build changes any arithmetic:
each returns the plain kernel's bits, and the plain kernel's are the oracle's counts, statuses and (to 1e-9) trajectories.

The handover test runs lean_run_cases.SEQUENCE on one handle WITHOUT reset_workspace between its steps: update_settings moves the handle
from the park kernels to the shared ones, to the plain kernel, to a solve of no iteration and back, each reading the G, V, D and stale v|z
that the one before it left.

After every solve the lean words of jit_info are the exact set the build and the setting call for (lean_run_cases.lean_words): a switch that
did nothing fails here. The cartpoles (no LDS slots, no park kernels) run the intervals 7 and 3 against the plain kernel only: their
converging tolerances have marginal verdicts on the oracle."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import lean_run_cases as L
from lean_run_cases import BUILDS, PAIRS, SEQUENCE, WARM
from test_layout_d_lean_trim_gpu import _everything

pytestmark = pytest.mark.gpu

WHAT = ("states", "controls", "iterations", "status", "residuals")
TOL = 1e-9  # states and controls against the oracle (test_slot_refill_gpu.py, test_layout_d_lean_gpu.py)
FORMS = ("shared", "goal")


def _handles(pkg, monkeypatch, shape, form, batch):
    """(build, handle) one after the other, each with its build's switches in the environment while it is in use (the plan reads them at
    every launch)."""
    prob = L.problem(pkg, shape)
    monkeypatch.setenv("TINYMPC_LAYOUT", "D")  # (small batches would go to the latency layouts)
    monkeypatch.setenv("TINYMPC_REFILL", "0")
    for build, (env, _) in BUILDS.items():
        for k in L.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=1,
                check_termination=0)
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        if form == "goal":
            gx, gu, box = L.goals(prob, batch)
            s.set_x_ref_batch(gx)
            s.set_u_ref_batch(gu)
            s.set_bound_constraints_batch(*box)
        yield build, s
        s.reset()


def _solve(s, build, shape, form, batch, x0, max_iter, ct, pri, dua):
    s.set_x0_batch(np.asfortranarray(x0))
    s.solve()
    words = s.jit_info().split()
    where = (build, shape, form, batch, (max_iter, ct, pri, dua), s.jit_info())
    assert s.launch_info()["layout"] == "D", where
    assert max_iter <= 0 or "compiled-in" in words, where
    assert tuple(w for w in L.LEAN_WORDS if w in words) == L.lean_words(build, shape, max_iter, ct, pri, dua), where
    # (a batch of one has no per-instance tables: its goal and box are the shared verbs', and the shared-table kernel runs)
    assert form != "goal" or batch == 1 or max_iter <= 0 or "goal" in words, where
    return _everything(s)


def _grid(pkg, monkeypatch, shape, form, batch, ct):
    """{build: {(max_iter, pair): (cold solve, warm solve)}}: one handle per build, every cell from a reset workspace."""
    prob = L.problem(pkg, shape)
    x0 = L.x0s(pkg, prob, batch, shape)
    got = {}
    for build, s in _handles(pkg, monkeypatch, shape, form, batch):
        got[build] = {}
        for max_iter, _ in L.cells(ct):
            for pair in PAIRS:
                pri, dua = L.pair_tols(pair, L.TOLS[shape])
                s.update_settings(abs_pri_tol=pri, abs_dua_tol=dua, max_iter=max_iter, check_termination=ct)
                s.reset_workspace()
                cold = _solve(s, build, shape, form, batch, x0, max_iter, ct, pri, dua)
                warm = _solve(s, build, shape, form, batch, WARM * x0, max_iter, ct, pri, dua)
                got[build][(max_iter, pair)] = (cold, warm)
    return got


def _assert_builds_equal_plain(got, tag):
    for build in BUILDS:
        if build == "plain":
            continue
        for key, solves in got[build].items():
            for k, solve in enumerate(("cold", "warm")):
                for a, b, what in zip(solves[k], got["plain"][key][k], WHAT):
                    np.testing.assert_array_equal(a, b, err_msg=f"{tag} (max_iter, pair)={key}: {solve} solve of the {build} build against the plain kernel: {what}")


def _assert_one_sided_pairs_are_forced(got, ct):
    """One tolerance zero: nothing converges, and nothing in the arithmetic depends on the other one."""
    for build in BUILDS:
        for (max_iter, pair), solves in got[build].items():
            if pair not in ("pri", "dua"):
                continue
            for k, solve in enumerate(("cold", "warm")):
                where = (build, max_iter, ct, pair, solve)
                assert np.all(solves[k][3] != 1) and np.all(solves[k][2] == max_iter), (where, solves[k][2], solves[k][3])
                for a, b, what in zip(solves[k], got[build][(max_iter, "none")][k], WHAT):
                    np.testing.assert_array_equal(a, b, err_msg=f"{where} against the cell with both tolerances zero: {what}")


def _mixed(it, status, max_iter):
    it, status = np.asarray(it)[:4], np.asarray(status)[:4]
    return bool(np.any((status == 1) & (it < max_iter)) and np.any((status != 1) & (it == max_iter)))


@pytest.fixture(scope="module")
def oracle_grid(pkg):
    """{(max_iter, ct, pair): (cold, warm)} for the pairs the oracle is asked about, batch 9, shared tables; computed once, never changed."""
    prob = L.problem(pkg)
    x0 = L.x0s(pkg, prob, 9)
    orc = L.OracleBatch(prob, 9)
    return {(m, ct, pair): L.oracle_cell(orc, x0, m, ct, *L.pair_tols(pair)) for m, ct in L.GRID for pair in ("both", "none")}


def _assert_matches_oracle(got, want, max_iter, ct, where):
    st, sc, it, status, res = got
    ox, ou, oit, ostatus, ores = want
    print(where, "iterations", it.tolist(), "status", status.tolist(), "rel_err", rel_err(st, ox), rel_err(sc, ou))
    np.testing.assert_array_equal(it, oit, err_msg=f"{where}: iterations")
    np.testing.assert_array_equal(status, ostatus, err_msg=f"{where}: status")
    assert rel_err(st, ox) < TOL, where
    assert rel_err(sc, ou) < TOL, where
    if ct > 0 and max_iter >= ct:  # a check fell inside the launch (every instance reaches the first one)
        np.testing.assert_allclose(res, ores, rtol=1e-6, atol=1e-10, err_msg=f"{where}: residuals")  # (test_large_systems_gpu.py)


@pytest.mark.parametrize("batch,ct", [(b, ct) for b, cts in L.BATCHES.items() for ct in cts])
@pytest.mark.parametrize("form", FORMS)
def test_every_cut_on_every_build_returns_the_plain_kernels_bits(pkg, monkeypatch, oracle_grid, form, batch, ct):
    got = _grid(pkg, monkeypatch, L.SHAPE, form, batch, ct)
    _assert_builds_equal_plain(got, f"{form} batch={batch} ct={ct}")
    _assert_one_sided_pairs_are_forced(got, ct)
    for (max_iter, pair), solves in got["park"].items():
        if pair == "none":
            assert np.all(solves[0][2] == max_iter) and np.all(solves[0][3] != 1), (max_iter, ct, solves[0][2], solves[0][3])
    if form == "shared" and batch == 9:
        for (max_iter, pair), solves in got["park"].items():
            if pair in ("both", "none"):
                for k, solve in enumerate(("cold", "warm")):
                    _assert_matches_oracle(solves[k], oracle_grid[(max_iter, ct, pair)][k], max_iter, ct, f"max_iter={max_iter} ct={ct} {pair} {solve}")
    elif batch > 1 and ct in (7, 8):
        # no oracle for this form or batch: the plain kernel's own counts show a tail behind a check with dead and live rows in one wavefront
        tails = [m for m, _ in L.cells(ct) if m > ct and L.lean_runs(m, ct, *L.pair_tols("both"))[1]]
        for m in tails:
            print(form, batch, ct, m, got["plain"][(m, "both")][0][2].tolist(), got["plain"][(m, "both")][0][3].tolist())
        assert any(_mixed(got["plain"][(m, "both")][0][2], got["plain"][(m, "both")][0][3], m) for m in tails), (form, batch, ct)


@pytest.mark.parametrize("form", FORMS)
def test_handover_between_the_builds_kernels_without_a_reset(pkg, monkeypatch, form):
    batch = 9
    prob = L.problem(pkg)
    x0 = L.x0s(pkg, prob, batch)
    got = {}
    for build, s in _handles(pkg, monkeypatch, L.SHAPE, form, batch):
        got[build] = []
        for max_iter, ct, tol, scale in SEQUENCE:
            s.update_settings(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=max_iter, check_termination=ct)
            got[build].append(_solve(s, build, L.SHAPE, form, batch, scale * x0, max_iter, ct, tol, tol))
    for build in BUILDS:
        for k, step in enumerate(SEQUENCE):
            for a, b, what in zip(got[build][k], got["plain"][k], WHAT):
                np.testing.assert_array_equal(a, b, err_msg=f"{form} step {k} {step}: the {build} build against the plain kernel: {what}")
    if form == "shared":
        want = L.oracle_sequence(L.OracleBatch(prob, batch), x0)
        for k, (max_iter, ct, tol, scale) in enumerate(SEQUENCE):
            if max_iter > 0:  # (what a solve of no iteration returns is compared among the builds only; the step behind it is the oracle's again)
                _assert_matches_oracle(got["park"][k], want[k], max_iter, ct, f"step {k} {SEQUENCE[k]}")
            else:
                print("step", k, "no iteration: iterations", got["park"][k][2].tolist(), "status", got["park"][k][3].tolist(), "states against the oracle's",
                      rel_err(got["park"][k][0], want[k][0]), "controls", rel_err(got["park"][k][1], want[k][1]))


@pytest.mark.parametrize("ct", [7, 3])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ["cartpole20", "cartpole10"])
def test_the_cartpoles_cuts_on_every_build_return_the_plain_kernels_bits(pkg, monkeypatch, shape, form, ct):
    got = _grid(pkg, monkeypatch, shape, form, 9, ct)
    _assert_builds_equal_plain(got, f"{shape} {form} ct={ct}")
    _assert_one_sided_pairs_are_forced(got, ct)

"""Layout D's lean kernels with a slot split of their own inside a run of lean rounds (tinympc_lpark_d.hip; tinympc_plan.hip:
lean_park_applies) against the shared kernels they descend from (TINYMPC_LEAN_PARK=0: tinympc_lshare_d.hip), the trimmed ones
(TINYMPC_LEAN_SHARE=0) and the plain kernel (TINYMPC_LEAN=0).

Inside a run twelve of the 25 LDS slots are register slots: their d comes from LDS at the run's entry, their slack goes back to LDS in the
run's last forward sweep, and what lived in the registers they take is parked in LDS rows the run leaves dead. No arithmetic changes, so
the four builds of one handle configuration must return the same bits -- states, controls, iteration counts, statuses and the four
residuals -- for a cold solve, for the warm solve behind it (which reads back every G, V and D the cold one wrote: a d, a slack or a
parked value left in the wrong place shows there), and for a solve behind `reset_workspace`, which must equal the fresh handle's.

Only the quadrotor N=50 has LDS slots, so the shape is fixed; batches of 1 (a lone instance), 5 (a last wavefront with one live row) and 9
(a full wavefront plus one); the shared-table and the per-instance goal form. Every build runs ALL cases in one fresh child process (the
plan reads its switches from the environment), and the tests compare what the four children wrote.

Settings (max_iter, check_termination, tolerance), with PARK_MIN_RUN = 6 in the plan: forced solves whose single run is 6 (at the
threshold), 7 (just above) and 40 rounds; 5 rounds (below: `park` must be absent from jit_info, the shared kernels run); 0 and 1
iterations (no run, and a run of one); and a converging solve with a check every 7th iteration -- runs of six, several per solve. Its
tolerance, 0.1, was chosen on the CPU with OraclePort so that, with test_layout_d_lean_trim_gpu.py's x0 scales, the first wavefront's
instances leave at different checks: two at iteration 7, one at 14, one never (max_iter = 28) -- rows that stop being live between
runs, with their write-backs pending at a run's entry. That mixture is asserted on the oracle (shared form) and on the plain kernel's
result (both forms)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHAT = ("states", "controls", "iterations", "status", "residuals")
SWITCHES = ("TINYMPC_LEAN", "TINYMPC_LEAN_START", "TINYMPC_LEAN_TRIM", "TINYMPC_LEAN_SHARE", "TINYMPC_LEAN_PARK")
BUILDS = {  # name -> (environment, the words of a lean launch's jit_info)
    "plain": ({"TINYMPC_LEAN": "0"}, ()),
    "trim": ({"TINYMPC_LEAN_SHARE": "0"}, ("lean", "lds-start", "trim")),
    "share": ({"TINYMPC_LEAN_PARK": "0"}, ("lean", "lds-start", "trim", "share")),
    "park": ({}, ("lean", "lds-start", "trim", "share", "park")),
}
LEAN_WORDS = ("lean", "lds-start", "trim", "share", "park")
PARK_MIN_RUN = 6  # (tinympc_plan.hip)
CONVERGING = (28, 7, 0.1)
# (max_iter, check_termination, tolerance); the first one runs on the fresh handle and once more at the end, behind reset_workspace
SETTINGS = [(40, 0, 0.0), (6, 0, 0.0), (7, 0, 0.0), (5, 0, 0.0), CONVERGING, (0, 0, 0.0), (1, 0, 0.0), (40, 0, 0.0)]
FORMS = ("shared", "goal")
BATCHES = (1, 5, 9)


def _first_run(max_iter, ct, tol):
    """Rounds of the launch's first run of lean rounds, as the kernel's loop and the plan form it."""
    if ct > 0 and tol > 0.0:
        return min(ct - 1, max_iter)
    last_check = (max_iter // ct) * ct if ct > 0 else 0
    return last_check - 1 if last_check > 0 else max_iter


def _words(build, setting):
    """The lean words jit_info must have for a setting (all settings here have a check interval other than 1)."""
    max_iter, ct, tol = setting
    if max_iter <= 0:
        return ()
    words = BUILDS[build][1]
    return words if _first_run(*setting) >= PARK_MIN_RUN else tuple(w for w in words if w != "park")


def _child(out_path):
    """Every case on this process's build: {key: array} into an .npz, the jit_info words beside them."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import __graft_entry__ as ge
    from test_layout_d_lean_trim_gpu import _everything, _goals, _problem, _x0s
    pkg = ge.load_package()
    P = pkg.problems
    prob = _problem(P, "quadrotor50")
    out, words = {}, {}
    for form in FORMS:
        for batch in BATCHES:
            x0s = _x0s(P, prob, "quadrotor50", batch)
            s = pkg.TinyMPC()
            mi, ct, tol = SETTINGS[0]
            s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, abs_pri_tol=tol, abs_dua_tol=tol,
                    max_iter=mi, check_termination=ct)
            s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            if form == "goal":
                gx, gu, box = _goals(prob, batch)
                s.set_x_ref_batch(gx)
                s.set_u_ref_batch(gu)
                s.set_bound_constraints_batch(*box)
            for k, (mi, ct, tol) in enumerate(SETTINGS):
                if k > 0:
                    s.update_settings(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=mi, check_termination=ct)
                    s.reset_workspace()
                s.set_x0_batch(x0s)
                s.solve()
                assert s.launch_info()["layout"] == "D", s.launch_info()
                words[f"{form}|{batch}|{k}"] = s.jit_info()
                solves = {"cold": _everything(s)}
                s.set_x0_batch(np.asfortranarray(0.9 * x0s))
                s.solve()
                solves["warm"] = _everything(s)
                s.reset_workspace()
                s.set_x0_batch(x0s)
                s.solve()
                solves["again"] = _everything(s)
                for name, arrays in solves.items():
                    for what, a in zip(WHAT, arrays):
                        out[f"{form}|{batch}|{k}|{name}|{what}"] = a
            s.reset()
    np.savez(out_path, words=np.array(json.dumps(words)), **out)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{build: (arrays, words)}: one child process per build, one after the other."""
    d = tmp_path_factory.mktemp("lean_park")
    got = {}
    for build, (env_add, _) in BUILDS.items():
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(env_add)
        env["TINYMPC_LAYOUT"] = "D"  # (small batches would go to the latency layouts)
        env["TINYMPC_REFILL"] = "0"
        path = os.path.join(str(d), build + ".npz")
        run = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (build, run.stdout[-2000:], run.stderr[-2000:])  # (nothing more is started behind a child that ended badly)
        with np.load(path) as z:
            got[build] = ({k: z[k] for k in z.files if k != "words"}, json.loads(str(z["words"])))
    return got


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", FORMS)
def test_every_build_runs_the_kernels_its_switches_name(results, form, batch):
    for build in BUILDS:
        for k, setting in enumerate(SETTINGS):
            words = results[build][1][f"{form}|{batch}|{k}"].split()
            want = _words(build, setting)
            assert setting[0] <= 0 or "compiled-in" in words, (build, setting, words)
            assert all(w in words for w in want) and not any(w in words for w in LEAN_WORDS if w not in want), (build, setting, words)
            # (a batch of one has no per-instance tables: its goal and box are the shared verbs', and the shared-table kernel runs)
            assert form != "goal" or batch == 1 or "goal" in words, (build, setting, words)
    # the run below the threshold keeps the shared kernels, the one at it does not
    assert _first_run(*SETTINGS[3]) == PARK_MIN_RUN - 1 and _first_run(*SETTINGS[1]) == PARK_MIN_RUN and _first_run(*CONVERGING) == PARK_MIN_RUN
    assert "park" not in results["park"][1][f"{form}|{batch}|3"].split() and "park" in results["park"][1][f"{form}|{batch}|1"].split()


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=[f"iter{m}-ct{c}-tol{t}-{k}" for k, (m, c, t) in enumerate(SETTINGS)])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", FORMS)
def test_the_four_builds_return_the_same_bits(results, form, batch, setting):
    park = results["park"][0]
    for other in ("share", "trim", "plain"):
        for solve in ("cold", "warm", "again"):
            for what in WHAT:
                key = f"{form}|{batch}|{setting}|{solve}|{what}"
                np.testing.assert_array_equal(results[other][0][key], park[key], err_msg=f"{key} (max_iter, ct, tol)={SETTINGS[setting]} against the {other} kernel")
    max_iter, ct, tol = SETTINGS[setting]
    it, status = park[f"{form}|{batch}|{setting}|cold|iterations"], park[f"{form}|{batch}|{setting}|cold|status"]
    if tol == 0.0:  # forced iteration counts
        assert np.all(it == max_iter) and np.all(status != 1), (SETTINGS[setting], it, status)
    elif batch > 1:  # the first wavefront's instances leave at different checks, and one never does
        it, status = results["plain"][0][f"{form}|{batch}|{setting}|cold|iterations"][:4], results["plain"][0][f"{form}|{batch}|{setting}|cold|status"][:4]
        assert len(set(it[status == 1])) >= 2 and np.any((status != 1) & (it == max_iter)), (form, batch, it, status)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", FORMS)
def test_a_solve_behind_reset_workspace_equals_the_fresh_handles(results, form, batch):
    """Within the park build: the solve behind reset_workspace equals the cold one of the same setting, and the first setting, run once
    more behind every other one, returns what the fresh handle returned -- G, V, D and the parked values all came back."""
    park = results["park"][0]
    for k in range(len(SETTINGS)):
        for what in WHAT:
            np.testing.assert_array_equal(park[f"{form}|{batch}|{k}|again|{what}"], park[f"{form}|{batch}|{k}|cold|{what}"], err_msg=f"{form} {batch} {SETTINGS[k]} {what}")
    assert SETTINGS[0] == SETTINGS[-1]
    for solve in ("cold", "warm"):
        for what in WHAT:
            np.testing.assert_array_equal(park[f"{form}|{batch}|{len(SETTINGS) - 1}|{solve}|{what}"], park[f"{form}|{batch}|0|{solve}|{what}"], err_msg=f"{form} {batch} {solve} {what}")


def test_the_converging_tolerance_spreads_the_first_wavefront_over_the_checks_on_the_oracle(pkg):
    """The CPU side of the converging setting (no kernel runs here; the module is a GPU module because its subject is)."""
    import pyoracle as O
    from test_layout_d_lean_trim_gpu import _problem, _x0s
    P = pkg.problems
    prob = _problem(P, "quadrotor50")
    max_iter, ct, tol = CONVERGING
    orc = O.OraclePort(prob).load_problem(prob, dict(abs_pri_tol=tol, abs_dua_tol=tol, max_iter=max_iter, check_termination=ct))
    _, _, it, status, _ = orc.solve_batch(_x0s(P, prob, "quadrotor50", 9))
    it, status = np.asarray(it)[:4], np.asarray(status)[:4]  # (instance i has the same x0 in every batch)
    assert sorted(it) == [7, 7, 14, 28] and sorted(status) == [1, 1, 1, 11], (it, status)


if __name__ == "__main__":
    _child(sys.argv[1])

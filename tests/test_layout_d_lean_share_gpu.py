"""Layout D's lean kernels with d and the slack sharing the register slots (tinympc_lshare_d.hip; tinympc_plan.hip: lean_share_applies)
against the trimmed kernels they descend from (TINYMPC_LEAN_SHARE=0: tinympc_ltrim_d.hip) and the plain kernel (TINYMPC_LEAN=0).

Inside a run of lean rounds the register of a slack slot holds the backward sweep's accumulator [p_s | d_s] and the slack v_s in turn; d_s
of those slots never goes through LDS, except at the entry of a run (LDS -> registers) and in its last round (every d_s stored again). No
arithmetic changes, so the builds of one handle configuration must return the same bits: states, controls, iteration counts, status and
the four residuals of a cold solve, and of the warm solve behind it, which reads back every G, V and D the cold one wrote -- where a d or
a slack left in the wrong place shows.

Every compiled-in 16-lane shape (quadrotor N=50: 24 shared register slots above 25 LDS slots; the cartpoles: every slot is shared and a
shared backward sweep stores no d at all), the shared-table and the per-instance goal form, batches of 1 and 5 (a partly filled
wavefront), 64 and 4 x 4 + 1 (a second workgroup), and settings that give runs of one, two, three and more lean rounds ending in the
final write-back, the headline's form (a run, then the iteration with residuals), checks that cannot end the solve, and runs of two
between checks which some instances leave converged while their wavefront goes on. `fdyn` is nonzero on every state row.

The converging setting is test_layout_d_lean_trim_gpu.py's (its tolerances and x0 scales were chosen on the CPU with OraclePort): on the
plain kernel's result instances converge at the first or second check and others run to max_iter = 12; a case in which that mixture
does not hold fails. A batch of one has one instance, so there only the equality is checked."""
from __future__ import annotations

import numpy as np
import pytest

from test_layout_d_lean_trim_gpu import SHAPES, WHAT, _everything, _goals, _mixed, _problem, _settings, _x0s

pytestmark = pytest.mark.gpu

BUILDS = {  # name -> (environment, the words jit_info must / must not have)
    "plain": ({"TINYMPC_LEAN": "0"}, (), ("lean", "lds-start", "trim", "share")),
    "trim": ({"TINYMPC_LEAN_SHARE": "0"}, ("lean", "lds-start", "trim"), ("share",)),
    "share": ({}, ("lean", "lds-start", "trim", "share"), ()),
}
SWITCHES = ("TINYMPC_LEAN", "TINYMPC_LEAN_START", "TINYMPC_LEAN_TRIM", "TINYMPC_LEAN_SHARE")
# (max_iter, check_termination, tolerance or None = the shape's converging tolerance)
SETTINGS = [(1, 0, 0.0), (2, 0, 0.0), (3, 0, 0.0), (4, 0, 0.0), (7, 0, 0.0), (7, 1, 0.0), (9, 3, 0.0), (12, 3, None)]


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


@pytest.mark.parametrize("batch", [1, 5, 64, 17])
@pytest.mark.parametrize("form", ["shared", "goal"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_shared_kernels_return_the_bits_of_the_trimmed_and_the_plain_ones(pkg, monkeypatch, shape, form, batch):
    got = _run(pkg, monkeypatch, shape, form, batch)
    for k, setting in enumerate(SETTINGS):
        for other in ("trim", "plain"):
            for w, solve in enumerate(("cold", "warm")):
                for a, b, what in zip(got[other][k][w], got["share"][k][w], WHAT):
                    np.testing.assert_array_equal(a, b, err_msg=f"{shape} {form} batch={batch} (max_iter, ct, tol)={setting}: {solve} solve against the {other} kernel: {what}")
        max_iter, ct, tol = setting
        it, status = got["share"][k][0][2], got["share"][k][0][3]
        if tol is not None:  # forced iteration counts
            assert np.all(it == max_iter) and np.all(status != 1), (setting, it, status)
        elif batch > 1:
            assert _mixed(got["plain"][k][0][2], got["plain"][k][0][3]), (shape, form, batch, got["plain"][k][0][2], got["plain"][k][0][3])

"""Resident solves (tinympc_set_resident) and the x0 verbs of a single-instance handle: the session is stepped with the PINNED copy of
x0, launches read the device copy -- every verb that sets x0 must leave both up to date, or a resident solve answers for a stale state
while its launched twin does not (the contract: resident solves are bit-identical to launched ones)."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-9  # the suite's bar against the restatement (tests/test_hip_parity.py)


def _solver(pkg, prob, settings):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho, fdyn=prob.fdyn, **settings)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if prob.x_ref is not None:
        s.set_x_ref(prob.x_ref)
    if prob.u_ref is not None:
        s.set_u_ref(prob.u_ref)
    return s


def test_resident_solves_take_x0_from_every_x0_verb(pkg):
    """A resident solve steps the session with the pinned copy of x0. On a single-instance handle tinympc_set_x0_batch and its _device
    form used to bring only the device copy up to date: set_resident(True), set_x0_batch(x), solve() solved for the x0 of the last set_x0
    (or for zero). Six ticks from different states on cartpole N=20 (its session kernel is compiled in), the verb alternating between
    set_x0, set_x0_batch and the device form: a resident handle and a launched twin agree bit for bit, and both follow the restatement."""
    from test_instance_bounds_gpu import _DeviceArrays  # (device memory through the HIP runtime the library uses: no torch needed)
    P = pkg.problems
    prob = P.cartpole(20, True)
    settings = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40)
    states = [prob.x0 * c + d for c, d in zip((1.0, -0.7, 0.45, -1.2, 0.8, -0.3), np.linspace(-0.05, 0.05, 6))]
    # the restatement first: warm-started ticks whose first controls differ from tick to tick -- a solve for a stale x0 cannot pass
    orc = O.OraclePort(prob).load_problem(prob, settings)
    want = []
    for x in states:
        orc.set_x0(x)
        orc.solve()
        ox, ou = orc.solution()
        want.append((ox.copy(), ou.copy(), orc.stats()["iter"], orc.stats()["status"]))
    for (_, u_prev, _, _), (_, u, _, _) in zip(want, want[1:]):
        assert np.max(np.abs(u[:, 0] - u_prev[:, 0])) > 1e-3 * max(np.max(np.abs(u[:, 0])), np.max(np.abs(u_prev[:, 0])))
    # (the device copies first: an allocation synchronises the device, and would wait for a resident kernel's idle time-out)
    dev = _DeviceArrays(pkg)
    on_device = {k: dev.put(x[:, None]) for k, x in enumerate(states) if k % 3 == 2}
    L = pkg.load_library()
    a, b = _solver(pkg, prob, settings), _solver(pkg, prob, settings)
    a.set_resident(True)
    for k, x in enumerate(states):
        for h in (a, b):
            if k % 3 == 0:
                h.set_x0(x)
            elif k % 3 == 1:
                h.set_x0_batch(np.asfortranarray(x[:, None]))
            else:
                assert L.tinympc_set_x0_batch_device(h._h, on_device[k], 0, 1) == 0
            h.solve()
        if k == 0:
            assert a.launch_info()["layout"] == b.launch_info()["layout"] == "F"
        sa, sb = a.get_solution(), b.get_solution()
        np.testing.assert_array_equal(sa["controls"], sb["controls"], err_msg=f"tick {k}")
        np.testing.assert_array_equal(sa["states"], sb["states"], err_msg=f"tick {k}")
        assert a.get_stats() == b.get_stats(), (k, a.get_stats(), b.get_stats())  # (iterations, status and the four residuals)
        ox, ou, it, status = want[k]
        assert (a.get_stats()["iter"], a.get_stats()["status"]) == (it, status), (k, a.get_stats(), it, status)
        assert rel_err(sa["controls"], ou) < TOL and rel_err(sa["states"], ox) < TOL, k
    a.reset()
    b.reset()
    dev.free()
